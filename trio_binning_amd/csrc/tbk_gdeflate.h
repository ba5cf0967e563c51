// tbk_gdeflate.h — the GPU gzip encoder behind the bin writer (tbk_gdeflate.hip): members in, gzip members out, three jobs deep.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

struct tbk_gdeflate;
struct tbk_gdeflate_member { const char *src; size_t n; int tag; };   // n bytes of text (host memory, ideally pinned); tag: the caller's (the bin)
struct tbk_gdeflate_out { int tag; const char *data; size_t n; };      // one finished gzip member

int tbk_gdeflate_create(int device, tbk_gdeflate **out);
void tbk_gdeflate_destroy(tbk_gdeflate *g);
// Queue a job: the members' text is copied to the device and coded, asynchronously.  The caller then sums each member's CRC-32
// (tbk_gdeflate_set_crc, any time before the job is collected; the device sums them too) and waits for tbk_gdeflate_text_done before it touches the text again.
int tbk_gdeflate_submit(tbk_gdeflate *g, const tbk_gdeflate_member *members, size_t n_members);
// The same with bgzf framing (include/tbk.h "BAM output"): every member (<= 65280 bytes) becomes one bgzf block, its deflate blocks cut at
// the job's cut hints (non-decreasing offsets into the members' bytes laid back to back, none beyond their end; n_hints may be 0).
int tbk_gdeflate_submit_bgzf(tbk_gdeflate *g, const tbk_gdeflate_member *members, size_t n_members, const uint64_t *hints, size_t n_hints);
void tbk_gdeflate_set_crc(tbk_gdeflate *g, size_t member, uint32_t crc);
int tbk_gdeflate_text_done(tbk_gdeflate *g, int back = 0);   // back: how many jobs before the newest
// Move the pipeline on and take the oldest finished job's members (none when nothing is ready and !drain).  The bytes lie in the
// job's pinned buffer and stay valid until the next tbk_gdeflate_submit, which may take over that job's slot and grow (free) the
// buffer; further collects leave them alone.
int tbk_gdeflate_collect(tbk_gdeflate *g, bool drain, std::vector<tbk_gdeflate_out> &out);
int tbk_gdeflate_in_flight(const tbk_gdeflate *g);
void tbk_gdeflate_stats(const tbk_gdeflate *g, uint64_t *text_bytes, uint64_t *member_bytes, uint64_t *blocks, uint64_t *members);

// Bytes of the header of the gzip member at p, whose first `bs` bytes are its own (a bgzf member's BSIZE + 1): the fixed ten, FEXTRA,
// FNAME and FCOMMENT (zero-terminated) and FHCRC (RFC 1952 2.3.1); 0 when they and the 8-byte trailer do not fit in bs.  What the
// host's bgzf parsers and the GPU inflater's take the member's deflate stream to start behind.
inline size_t tbk_gzip_header_len(const uint8_t *p, size_t bs) {
    if (bs < 18) return 0;
    const int flg = p[3];
    size_t h = 10;
    if (flg & 4) h = 12 + (p[10] | ((size_t)p[11] << 8));
    for (int f = 8; f <= 16; f <<= 1)
        if (flg & f) {
            while (h < bs && p[h]) h++;
            if (h >= bs) return 0;
            h++;
        }
    if (flg & 2) h += 2;
    return h + 8 <= bs ? h : 0;
}

// ---- the other direction: bgzf blocks inflated on the device (tbk_gdeflate.hip, second half) -------------------------------------------
struct tbk_ginflate;
struct tbk_ginflate_block { uint64_t in_off; uint32_t in_len, out_len, crc; uint32_t pad_; };   // a raw deflate stream in the window's input; its text's length and CRC-32 (the bgzf trailer's)
constexpr int TBK_GINFLATE_SLOTS = 4;   // one being staged, one on the device, one with the parser, one more (measured at configs[1] scale: 8 -> 3.9, 5 -> 4.2, 4 -> 4.4 Gbases/s: their pinned memory costs more to get and to give back than lending it to the batches saves)
int tbk_ginflate_create(int device, tbk_ginflate **out);
void tbk_ginflate_destroy(tbk_ginflate *g);
uint8_t *tbk_ginflate_input(tbk_ginflate *g, int slot, size_t bytes);
int tbk_ginflate_reserve(tbk_ginflate *g, int slot, size_t in_bytes, size_t n_blocks, size_t out_bytes);
int tbk_ginflate_submit(tbk_ginflate *g, int slot, size_t in_bytes, const tbk_ginflate_block *blocks, size_t n_blocks, size_t head);
int tbk_ginflate_wait(tbk_ginflate *g, int slot, uint8_t **out_base, size_t *text_bytes, uint32_t *bad);
