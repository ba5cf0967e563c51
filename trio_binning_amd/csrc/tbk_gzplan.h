// tbk_gzplan.h — an ordinary (non-bgzf) gzip file inflated chunk-parallel in two passes: the plan, the chain check and the loop
// around them, host only (tbk_gzplan.cpp).  Who decodes the chunks is behind TbkGzBackend: the GPU's marker-mode inflater
// (tbk_gdeflate.hip, gz_inflate_kernel and the passes behind it), or the host's own TbkInflate::run16 standing in for it (tests, and the
// check of what the device did).  The scheme is LineSource::pinflate_loop's (tbk_fastx.cpp), cut for thousands of chunks to a window.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

constexpr uint32_t TBK_GZ_HIST = 32768;      // elements of window in front of every chunk's symbols
constexpr uint16_t TBK_GZ_NOTHING = 0x7FFF;  // a window position before the member's first byte (pinflate_loop's NOTHING)

// A chunk of pass a.  Bits count from the first byte of the window's input.  Its symbols lie at sym_off + TBK_GZ_HIST of the window's
// symbol buffer, the (materialised) window in the TBK_GZ_HIST elements in front of them.
struct TbkGzChunk {
    uint64_t start_bit, stop_bit;   // decode from start_bit (a block header), stop in front of the first block header at or past stop_bit
    uint64_t sym_off;               // elements; a multiple of 8
    uint32_t out_cap;               // symbols of room
    uint32_t window_known;          // 1: the caller has put the real window in front (chunk 0); 0: the decoder writes markers 0x8000 + i
};
enum TbkGzStatus : uint32_t { TBK_GZ_SKIPPED = 0, TBK_GZ_BOUNDARY = 1, TBK_GZ_MEMBER_DONE = 2, TBK_GZ_FAILED = 3, TBK_GZ_NO_ROOM = 4, TBK_GZ_NO_INPUT = 5 };
struct TbkGzResult {
    uint32_t status, n_sym;
    uint64_t end_bit;   // exact: the next block header (BOUNDARY) or the bit behind the final block (MEMBER_DONE)
};

struct TbkGzBackend {
    virtual ~TbkGzBackend() {}
    // pass a: every chunk decoded into 16-bit symbols; window0 = TBK_GZ_HIST elements, chunk 0's real window.  Returns a TBK_* code.
    virtual int decode(const uint8_t *in, size_t in_bytes, const TbkGzChunk *chunks, size_t n, const uint16_t *window0, TbkGzResult *res) = 0;
    // passes b-d over the first n_acc chunks of the last decode(): windows front to back, markers -> bytes (chunk i's at text_off[i]),
    // per-chunk CRC-32, bad[i] != 0 where a resolved value was no byte.  *text stays valid until the next resolve().
    virtual int resolve(size_t n_acc, const TbkGzResult *res, const uint64_t *text_off, uint64_t text_total, uint8_t **text, uint32_t *crc, uint8_t *bad) = 0;
};

struct TbkGzStats { uint64_t windows, guessed, accepted, redecoded, handed_back; double guess_s; uint32_t most_accepted; };

struct TbkGzOptions {
    size_t chunk = (size_t)128 << 10;    // compressed bytes per chunk
    size_t window = (size_t)256 << 20;   // compressed bytes per window
    int threads = 16;                    // for the block-start guesses
    size_t max_symbols = (size_t)3 << 29;   // elements of one window's symbol buffer at the most
    size_t ratio = 6;                    // symbols of room per compressed byte to begin with (a chunk without room doubles it)
};
// TBK_GZIP_CHUNK / TBK_GZIP_WINDOW / TBK_GZIP_RATIO (tests) over the defaults
TbkGzOptions tbk_gz_options_from_env(int threads);

// The next window's chunks: chunk 0 at `start_bit` (exact), the others at the first bit of their span of opt.chunk bytes where a
// dynamic-Huffman block can begin (TbkInflate::open_dynamic_block_at); spans without one merge into the chunk before.  `ratio`: symbols
// of room per compressed byte.  *in_lo / *in_bytes: the stretch of the file the window's input is.
void tbk_gz_plan_window(const uint8_t *data, size_t size, uint64_t start_bit, const TbkGzOptions &opt, size_t window_bytes, size_t ratio,
                        std::vector<TbkGzChunk> &chunks, size_t *in_lo, size_t *in_bytes);
// The induction of pinflate_loop: chunk i counts iff chunk i-1 counted, ended at a boundary and exactly on chunk i's start, and chunk i
// itself decoded to a boundary or its member's end.  0: chunk 0 itself did not.
size_t tbk_gz_chain_accept(const TbkGzChunk *chunks, const TbkGzResult *res, size_t n);

// The whole file through `be`: text handed to `sink` window by window, in order (sink returns false to stop: TBK_ERR_STATE).  Returns
// a TBK_* code; `err` = the host path's message ("inflate: ...").
int tbk_gz_run(TbkGzBackend &be, const uint8_t *data, size_t size, const TbkGzOptions &opt, const std::function<bool(const uint8_t *, size_t, bool)> &sink,
               TbkGzStats *stats, std::string *err);

// TbkInflate::run16 on host threads behind the backend's interface
TbkGzBackend *tbk_gz_host_backend(int threads);

// the GPU behind the same interface (tbk_gdeflate.hip, last part): streams, pinned and device buffers for one window at a time
int tbk_gzinflate_create(int device, TbkGzBackend **out);
void tbk_gzinflate_destroy(TbkGzBackend *g);
int tbk_gzinflate_reserve(TbkGzBackend *g, size_t in_bytes, size_t n_chunks, size_t symbols, size_t text_bytes);
