// tbk_bam.h — unaligned BAM records (PacBio HiFi and ONT uBAM) turned into FASTQ text: the rule of include/tbk.h ("BAM
// input") as code that needs no device.  tbk_bam_header_len finds the end of the header, tbk_bam_index walks the
// block_size chain of a window of records, tbk_bam_measure says how long a record's text is (or why it is refused) and
// tbk_bam_fastq_host writes the text.  Plain C++ without a HIP header, so that tests/native/bam_check.cpp can run it under
// AddressSanitizer and UBSan on the CPU; tbk_bam.hip includes it for the constants and for tbk_bam_measure, which the
// measure kernel runs as it stands (TBK_BAM_HD), so host and device refuse the same records for the same reason.
#ifndef TBK_BAM_H
#define TBK_BAM_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#ifdef __HIPCC__
#define TBK_BAM_HD __host__ __device__
#else
#define TBK_BAM_HD
#endif

#define TBK_BAM_MAX_RECORD_ (1u << 28)      /* = TBK_BAM_MAX_RECORD of include/tbk.h */
#define TBK_BAM_SKIP_DEFAULT_ 0x900u        /* secondary | supplementary: samtools fastq's default */
#define TBK_BAM_NO_BAD (~0ull)

// reasons a record is refused by, in the order they are looked for (tbk_bam_reason has the words)
enum : uint32_t {
    TBK_BAM_OK = 0,
    TBK_BAM_LONG_BLOCK = 1,    // block_size > TBK_BAM_MAX_RECORD (a negative one too)
    TBK_BAM_SHORT_BLOCK = 2,   // block_size < 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq
    TBK_BAM_SHORT_NAME = 3,    // l_read_name < 2
    TBK_BAM_NAME_NUL = 4,      // the name's last byte is not NUL
    TBK_BAM_NAME_BYTE = 5,     // a name byte outside 0x21..0x7E
    TBK_BAM_CUT_OFF = 6,       // the file ends inside the record
};

static inline const char *tbk_bam_reason(uint32_t reason) {
    switch (reason) {
    case TBK_BAM_LONG_BLOCK: return "block_size is larger than TBK_BAM_MAX_RECORD";
    case TBK_BAM_SHORT_BLOCK: return "block_size is too small for the record's name, cigar, bases and qualities";
    case TBK_BAM_SHORT_NAME: return "l_read_name is less than 2";
    case TBK_BAM_NAME_NUL: return "the read name does not end in NUL";
    case TBK_BAM_NAME_BYTE: return "a read name byte outside 0x21..0x7E";
    case TBK_BAM_CUT_OFF: return "the file ends inside the record";
    default: return "refused";
    }
}

TBK_BAM_HD static inline uint32_t tbk_bam_u32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
TBK_BAM_HD static inline uint32_t tbk_bam_u16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// The fields of a record that its text depends on.  Offsets count from the block_size field.
struct TbkBamRec {
    uint32_t block_size, l_read_name, n_cigar_op, flag, l_seq;
    uint32_t seq_at, qual_at;   // where seq and qual begin
    uint32_t has_qual;          // qual[0] != 0xFF
};

// The record at `rec`, whose 4 + block_size bytes are readable and whose block_size is at least 32 (tbk_bam_index hands out
// no other).  Returns the reason it is refused by, or TBK_BAM_OK with its fields and *text_len = the bytes of its text: 0
// for a record that is skipped (flag & skip_flags, or no bases).
TBK_BAM_HD static inline uint32_t tbk_bam_measure(const uint8_t *rec, uint32_t skip_flags, TbkBamRec *r, uint32_t *text_len) {
    r->block_size = tbk_bam_u32(rec);
    r->l_read_name = rec[12];
    r->n_cigar_op = tbk_bam_u16(rec + 16);
    r->flag = tbk_bam_u16(rec + 18);
    r->l_seq = tbk_bam_u32(rec + 20);
    *text_len = 0;
    if (r->block_size > TBK_BAM_MAX_RECORD_) return TBK_BAM_LONG_BLOCK;
    const uint64_t need = 32ull + r->l_read_name + 4ull * r->n_cigar_op + ((uint64_t)r->l_seq + 1) / 2 + r->l_seq;
    if ((uint64_t)r->block_size < need) return TBK_BAM_SHORT_BLOCK;
    if (r->l_read_name < 2) return TBK_BAM_SHORT_NAME;
    const uint8_t *name = rec + 36;
    if (name[r->l_read_name - 1] != 0) return TBK_BAM_NAME_NUL;
    for (uint32_t i = 0; i + 1 < r->l_read_name; i++)
        if (name[i] < 0x21 || name[i] > 0x7E) return TBK_BAM_NAME_BYTE;
    r->seq_at = 36 + r->l_read_name + 4 * r->n_cigar_op;
    r->qual_at = r->seq_at + (r->l_seq + 1) / 2;
    r->has_qual = 0;
    if (r->l_seq == 0 || (r->flag & skip_flags)) return TBK_BAM_OK;
    r->has_qual = rec[r->qual_at] != 0xFF;
    *text_len = r->l_read_name - 1 + (r->has_qual ? 2 * r->l_seq + 6 : r->l_seq + 3);
    return TBK_BAM_OK;
}

// Bytes of the header at the front of `text` (magic, l_text, text, n_ref, the references): *len = 0 while `size` bytes do
// not hold all of it yet.  Returns 0, or -1 when the text cannot be a BAM file's: another magic, or a negative length.
static inline int tbk_bam_header_len(const uint8_t *text, uint64_t size, uint64_t *len) {
    *len = 0;
    if (!size) return 0;
    const uint64_t have = size < 4 ? size : 4;
    if (memcmp(text, "BAM\1", (size_t)have) != 0) return -1;
    if (size < 8) return 0;
    const uint32_t l_text = tbk_bam_u32(text + 4);
    if (l_text > 0x7FFFFFFFu) return -1;
    uint64_t p = 8ull + l_text;
    if (size < p + 4) return 0;
    const uint32_t n_ref = tbk_bam_u32(text + p);
    if (n_ref > 0x7FFFFFFFu) return -1;
    p += 4;
    for (uint32_t i = 0; i < n_ref; i++) {
        if (size < p + 4) return 0;
        const uint32_t l_name = tbk_bam_u32(text + p);
        if (l_name > 0x7FFFFFFFu) return -1;
        p += 8ull + l_name;   // l_name, name, l_ref
    }
    if (size < p) return 0;
    *len = p;
    return 0;
}

// `records` begins at a record boundary.  offsets[0 .. *n) = where the records that lie wholly within `size` bytes begin,
// at most `cap` of them; *consumed = where the first record not handed out begins.  Returns TBK_BAM_OK when the walk ended
// at `size`, at `cap` records or in front of a record that needs more bytes, or the reason why the record at *consumed can
// never be handed out: a block_size above TBK_BAM_MAX_RECORD, or one below the 32 bytes of the fixed part.
static inline uint32_t tbk_bam_index(const uint8_t *records, uint64_t size, uint64_t *offsets, uint64_t cap, uint64_t *n, uint64_t *consumed) {
    uint64_t p = 0, k = 0;
    uint32_t why = TBK_BAM_OK;
    while (k < cap && size - p >= 4) {
        const uint32_t bs = tbk_bam_u32(records + p);
        if (bs > TBK_BAM_MAX_RECORD_) { why = TBK_BAM_LONG_BLOCK; break; }
        if (bs < 32) { why = TBK_BAM_SHORT_BLOCK; break; }
        if (size - p - 4 < bs) break;
        offsets[k++] = p;
        p += 4ull + bs;
    }
    *n = k;
    *consumed = p;
    return why;
}

static const char TBK_BAM_LETTERS[17] = "=ACMGRSVTWYHKDBN";
static const char TBK_BAM_COMPLEMENT[17] = "=TGKCYSBAWRDMHVN";   // of the letter with the same code

// The transcoder in plain C++: the text of records[offsets[i]], i in [0, n), back to back into dst[0 .. cap).  lengths
// (may be NULL) gets every record's text length, 0 for a skipped one.  *text_len = bytes of text - also when cap is too
// small, in which case nothing past cap is written and the caller sizes dst by it; *n_written / *n_skipped count records.
// Returns TBK_BAM_NO_BAD, or (index of the first refused record << 8) | reason; the text in front of it has been written.
static inline uint64_t tbk_bam_fastq_host(const uint8_t *records, const uint64_t *offsets, uint64_t n, uint32_t skip_flags, uint8_t *dst, uint64_t cap,
                                          uint32_t *lengths, uint64_t *text_len, uint64_t *n_written, uint64_t *n_skipped) {
    uint64_t at = 0, written = 0, skipped = 0, bad = TBK_BAM_NO_BAD;
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t *rec = records + offsets[i];
        TbkBamRec r;
        uint32_t len = 0;
        const uint32_t why = tbk_bam_measure(rec, skip_flags, &r, &len);
        if (why != TBK_BAM_OK) { bad = (i << 8) | why; break; }
        if (lengths) lengths[i] = len;
        if (!len) { skipped++; continue; }
        written++;
        if (at + len <= cap) {
            uint8_t *w = dst + at;
            const uint8_t *seq = rec + r.seq_at, *qual = rec + r.qual_at;
            const uint32_t L = r.l_seq;
            const bool rev = (r.flag & 0x10u) != 0;
            *w++ = r.has_qual ? '@' : '>';
            memcpy(w, rec + 36, r.l_read_name - 1);
            w += r.l_read_name - 1;
            *w++ = '\n';
            for (uint32_t j = 0; j < L; j++) {
                const uint32_t s = rev ? L - 1 - j : j;
                const uint32_t code = (seq[s >> 1] >> (4 * (1 - (s & 1)))) & 15u;
                *w++ = (uint8_t)(rev ? TBK_BAM_COMPLEMENT[code] : TBK_BAM_LETTERS[code]);
            }
            *w++ = '\n';
            if (r.has_qual) {
                *w++ = '+';
                *w++ = '\n';
                for (uint32_t j = 0; j < L; j++) {
                    const uint32_t q = qual[rev ? L - 1 - j : j];
                    *w++ = (uint8_t)((q > 93 ? 93 : q) + 33);
                }
                *w++ = '\n';
            }
        }
        at += len;
    }
    *text_len = at;
    if (n_written) *n_written = written;
    if (n_skipped) *n_skipped = skipped;
    return bad;
}

// The same on several threads, a share of the records each, in two calls.  The first (dst == NULL) measures: it cuts the
// shares, fills s and gives *text_len and the counts, or returns the first refused record as tbk_bam_fastq_host does (the
// shares are in file order, so the first share's is the first).  The second writes the text into dst, which holds
// *text_len bytes.
struct TbkBamShares {
    int nt = 1;
    std::vector<uint64_t> len, at, bad, written, skipped;
};
static inline uint64_t tbk_bam_fastq_shares(const uint8_t *records, const uint64_t *offsets, uint64_t n, uint32_t skip_flags, int threads, TbkBamShares &s,
                                            uint8_t *dst, uint64_t *text_len, uint64_t *n_written, uint64_t *n_skipped) {
    if (!dst) {
        const uint64_t most = n / 64 ? n / 64 : 1;   // (a thread is not worth fewer than 64 records)
        s.nt = threads < 1 ? 1 : ((uint64_t)threads > most ? (int)most : threads);
        for (std::vector<uint64_t> *v : {&s.len, &s.at, &s.bad, &s.written, &s.skipped}) v->assign((size_t)s.nt, 0);
    }
    const int nt = s.nt;
    auto share = [&](int t) {
        const uint64_t lo = n * (uint64_t)t / (uint64_t)nt, hi = n * (uint64_t)(t + 1) / (uint64_t)nt;
        uint64_t len = 0;
        const uint64_t bad = tbk_bam_fastq_host(records, offsets + lo, hi - lo, skip_flags, dst ? dst + s.at[(size_t)t] : nullptr, dst ? s.len[(size_t)t] : 0, nullptr, &len,
                                                &s.written[(size_t)t], &s.skipped[(size_t)t]);
        s.bad[(size_t)t] = bad == TBK_BAM_NO_BAD ? bad : bad + (lo << 8);
        if (!dst) s.len[(size_t)t] = len;
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; t++) pool.emplace_back(share, t);
    share(0);
    for (std::thread &th : pool) th.join();
    *text_len = 0; *n_written = 0; *n_skipped = 0;
    for (int t = 0; t < nt; t++) {
        if (s.bad[(size_t)t] != TBK_BAM_NO_BAD) return s.bad[(size_t)t];
        if (!dst) s.at[(size_t)t] = *text_len;
        *text_len += s.len[(size_t)t];
        *n_written += s.written[(size_t)t];
        *n_skipped += s.skipped[(size_t)t];
    }
    return TBK_BAM_NO_BAD;
}

// ---- records kept whole (include/tbk.h "BAM output") -----------------------------------------------------------------------
// Of the records tbk_bam_index handed out and the transcoder accepted: where the WRITTEN ones (not skipped) begin and how long
// they are, block_size field included, in file order - the k-th entry is the record behind the k-th record of the window's text.
struct TbkBamSlice { uint64_t off; uint32_t len; };
static inline void tbk_bam_written(const uint8_t *records, const uint64_t *offsets, uint64_t n, uint32_t skip_flags, std::vector<TbkBamSlice> &out) {
    out.clear();
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t *rec = records + offsets[i];
        const uint32_t l_seq = tbk_bam_u32(rec + 20), flag = tbk_bam_u16(rec + 18);
        if (l_seq == 0 || (flag & skip_flags)) continue;
        out.push_back(TbkBamSlice{offsets[i], 4u + tbk_bam_u32(rec)});
    }
}
// The four places of a whole, accepted record where the kind of its bytes changes - start of seq, of qual, of the tags, the
// record's end - as offsets from `base` (where the record lies in a bin's bytes): the bgzf coder's cut hints.
static inline void tbk_bam_hints(const uint8_t *rec, uint32_t len, uint64_t base, uint64_t out[4]) {
    const uint32_t l_seq = tbk_bam_u32(rec + 20);
    const uint64_t seq_at = 36ull + rec[12] + 4ull * tbk_bam_u16(rec + 16), qual_at = seq_at + ((uint64_t)l_seq + 1) / 2, tags_at = qual_at + l_seq;
    out[0] = base + (seq_at < len ? seq_at : len);
    out[1] = base + (qual_at < len ? qual_at : len);
    out[2] = base + (tags_at < len ? tags_at : len);
    out[3] = base + len;
}

// ---- the device side (tbk_bam.hip): a transcoder that keeps its buffers from window to window ------------------------------
// tbk_bamdev_measure copies a window (records, the offsets tbk_bam_index gave) to the device, measures and scans it: *text_len,
// the counts, *bad = TBK_BAM_NO_BAD or ((first_record + index of the first refused record) << 8 | reason).  tbk_bamdev_write
// then writes the text of that window and brings it home.  The *_device forms take device pointers (d_records readable 16 bytes
// past the window's end, d_text 16-byte aligned) and leave the copies to the caller.
struct tbk_bamdev;
int tbk_bamdev_create(int device, tbk_bamdev **out);
void tbk_bamdev_destroy(tbk_bamdev *b);
int tbk_bamdev_measure(tbk_bamdev *b, const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, uint32_t skip_flags, uint64_t first_record,
                       uint64_t *text_len, uint64_t *n_written, uint64_t *n_skipped, uint64_t *bad);
int tbk_bamdev_write(tbk_bamdev *b, uint8_t *dst);
int tbk_bamdev_measure_device(tbk_bamdev *b, const uint8_t *d_records, const uint64_t *d_offsets, uint64_t n, uint32_t skip_flags, uint64_t first_record,
                              uint64_t *text_len, uint64_t *n_written, uint64_t *n_skipped, uint64_t *bad);
int tbk_bamdev_write_device(tbk_bamdev *b, const uint8_t *d_records, const uint64_t *d_offsets, uint8_t *d_text);
// Timing (tbk_bam_bench_device): the window measured last is written again between two HIP events; *seconds = the kernel's time.
int tbk_bamdev_time_write(tbk_bamdev *b, double *seconds);
#endif /* TBK_BAM_H */
