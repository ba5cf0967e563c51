// tbk_bam_tag.h — BAM records rewritten with their haplotype and counts as tags: the rule of include/tbk.h ("Haplotag
// output") as code that needs no device.  tbk_tag_measure walks a record's aux area field by field and says how long the
// tagged record is, where the at most three fields it loses lie, or why it is refused; tbk_tag_write_host writes the tagged
// record; tbk_bam_haplotag_host does a run of records on several threads.  Plain C++ without a HIP header, so that
// tests/native/bam_tag_check.cpp can run it under AddressSanitizer and UBSan on the CPU; tbk_bam_tag.hip includes it, and its
// measure kernel runs tbk_tag_measure as it stands (TBK_BAM_HD), so host and device refuse the same records for the same reason.
#ifndef TBK_BAM_TAG_H
#define TBK_BAM_TAG_H
#include "tbk_bam.h"

#define TBK_TAG_GROWTH 18u   /* a record grows by at most HP C x (4) + ka I a (7) + kb I b (7) bytes */

// reasons beside tbk_bam.h's (of those a record can give TBK_BAM_LONG_BLOCK and TBK_BAM_SHORT_BLOCK here), in the order a field is
// looked at: its three bytes, its type, its value, and - once the field is known whole - its name
enum : uint32_t {
    TBK_TAG_SHORT_FIELD = 16,   // fewer than 3 bytes left for a field
    TBK_TAG_TYPE = 17,          // unknown type
    TBK_TAG_SUBTYPE = 18,       // unknown B subtype
    TBK_TAG_NEG_COUNT = 19,     // negative B count
    TBK_TAG_PAST_END = 20,      // a value that runs past the record's end
    TBK_TAG_NO_NUL = 21,        // Z / H without a NUL before the end
    TBK_TAG_TWICE_HP = 22,      // a second field named HP,
    TBK_TAG_TWICE_KA = 23,      // ka,
    TBK_TAG_TWICE_KB = 24,      // kb
    TBK_TAG_LONG = 25,          // block_size' > TBK_BAM_MAX_RECORD
};

static inline const char *tbk_tag_reason(uint32_t reason) {
    switch (reason) {
    case TBK_TAG_SHORT_FIELD: return "fewer than 3 bytes are left for a tag field";
    case TBK_TAG_TYPE: return "a tag field of unknown type";
    case TBK_TAG_SUBTYPE: return "a B tag field of unknown subtype";
    case TBK_TAG_NEG_COUNT: return "a B tag field with a negative count";
    case TBK_TAG_PAST_END: return "a tag field's value runs past the record's end";
    case TBK_TAG_NO_NUL: return "a Z or H tag field without a NUL before the record's end";
    case TBK_TAG_TWICE_HP: return "a second tag field named HP";
    case TBK_TAG_TWICE_KA: return "a second tag field named ka";
    case TBK_TAG_TWICE_KB: return "a second tag field named kb";
    case TBK_TAG_LONG: return "the tagged record's block_size is larger than TBK_BAM_MAX_RECORD";
    default: return tbk_bam_reason(reason);
    }
}

// where the fields a record loses lie (offsets from the block_size field, in the record's order) and how long they are; unused
// entries are {0, 0}
struct TbkTagDrops { uint32_t at[3], len[3]; };

// The first NUL of rec[at .. end), or `end`.  Bytes up to the first 8-byte boundary of the address, then aligned words (four
// a trip while 32 bytes are left: an MM string of an ONT read is tens of kilobytes), then the bytes behind the last whole
// word; no byte outside [at, end) is read.
TBK_BAM_HD static inline uint32_t tbk_tag_find_nul(const uint8_t *rec, uint32_t at, uint32_t end) {
    const uint64_t ones = 0x0101010101010101ull, tops = 0x8080808080808080ull;
    while (at < end && ((uintptr_t)(rec + at) & 7u)) { if (!rec[at]) return at; at++; }
    while (end - at >= 32) {
        uint64_t w[4];
        __builtin_memcpy(w, __builtin_assume_aligned(rec + at, 8), 32);
        if ((((w[0] - ones) & ~w[0]) | ((w[1] - ones) & ~w[1]) | ((w[2] - ones) & ~w[2]) | ((w[3] - ones) & ~w[3])) & tops) break;
        at += 32;
    }
    while (end - at >= 8) {
        uint64_t w;
        __builtin_memcpy(&w, __builtin_assume_aligned(rec + at, 8), 8);
        if ((w - ones) & ~w & tops) break;
        at += 8;
    }
    while (at < end && rec[at]) at++;
    return at;
}

// The tags a record gains, in their order: HP C 1 / 2 for bin A / B (none for any other bin), ka I a, kb I b.  Returns their bytes.
TBK_BAM_HD static inline uint32_t tbk_tag_tail(char bin, uint32_t a, uint32_t b, uint8_t out[TBK_TAG_GROWTH]) {
    uint32_t n = 0;
    if (bin == 'A' || bin == 'B') { out[n++] = 'H'; out[n++] = 'P'; out[n++] = 'C'; out[n++] = bin == 'A' ? 1 : 2; }
    out[n++] = 'k'; out[n++] = 'a'; out[n++] = 'I';
    for (int i = 0; i < 4; i++) out[n++] = (uint8_t)(a >> (8 * i));
    out[n++] = 'k'; out[n++] = 'b'; out[n++] = 'I';
    for (int i = 0; i < 4; i++) out[n++] = (uint8_t)(b >> (8 * i));
    return n;
}

// The record at `rec`, whose 4 + block_size bytes are readable and whose block_size is at least 32.  Returns the reason it is
// refused by, or TBK_BAM_OK with *new_len = the bytes of the tagged record (4 + block_size') and *d = the fields it loses.
TBK_BAM_HD static inline uint32_t tbk_tag_measure(const uint8_t *rec, char bin, TbkTagDrops *d, uint32_t *new_len) {
    *new_len = 0;
    for (int k = 0; k < 3; k++) d->at[k] = d->len[k] = 0;
    const uint32_t bs = tbk_bam_u32(rec);
    if (bs > TBK_BAM_MAX_RECORD_) return TBK_BAM_LONG_BLOCK;
    const uint32_t end = 4 + bs, l_seq = tbk_bam_u32(rec + 20);
    const uint64_t aux = 36ull + rec[12] + 4ull * tbk_bam_u16(rec + 16) + ((uint64_t)l_seq + 1) / 2 + l_seq;
    if (aux > end) return TBK_BAM_SHORT_BLOCK;
    uint32_t at = (uint32_t)aux, seen = 0, nd = 0, dropped = 0;
    while (at < end) {
        if (end - at < 3) return TBK_TAG_SHORT_FIELD;
        const uint32_t v = at + 3, room = end - v;
        uint64_t size = 0;
        switch (rec[at + 2]) {
        case 'A': case 'c': case 'C': size = 1; break;
        case 's': case 'S': size = 2; break;
        case 'i': case 'I': case 'f': size = 4; break;
        case 'Z': case 'H': {
            const uint32_t nul = tbk_tag_find_nul(rec, v, end);
            if (nul == end) return TBK_TAG_NO_NUL;
            size = (uint64_t)(nul - v) + 1;
            break;
        }
        case 'B': {
            if (room < 5) return TBK_TAG_PAST_END;
            uint32_t each = 0;
            switch (rec[v]) {
            case 'c': case 'C': each = 1; break;
            case 's': case 'S': each = 2; break;
            case 'i': case 'I': case 'f': each = 4; break;
            default: return TBK_TAG_SUBTYPE;
            }
            const uint32_t count = tbk_bam_u32(rec + v + 1);
            if (count > 0x7FFFFFFFu) return TBK_TAG_NEG_COUNT;
            size = 5 + (uint64_t)count * each;
            break;
        }
        default: return TBK_TAG_TYPE;
        }
        if (size > room) return TBK_TAG_PAST_END;
        const uint32_t next = v + (uint32_t)size;
        const int which = rec[at] == 'H' && rec[at + 1] == 'P' ? 0 : rec[at] == 'k' && rec[at + 1] == 'a' ? 1 : rec[at] == 'k' && rec[at + 1] == 'b' ? 2 : -1;
        if (which >= 0) {
            if (seen & (1u << which)) return TBK_TAG_TWICE_HP + (uint32_t)which;
            seen |= 1u << which;
            d->at[nd] = at; d->len[nd] = next - at; nd++;
            dropped += next - at;
        }
        at = next;
    }
    const uint32_t len = end - dropped + (bin == 'A' || bin == 'B' ? 18u : 14u);
    if (len - 4 > TBK_BAM_MAX_RECORD_) return TBK_TAG_LONG;
    *new_len = len;
    return TBK_BAM_OK;
}

// The tagged record, new_len bytes, as tbk_tag_measure planned it.
static inline void tbk_tag_write_host(const uint8_t *rec, char bin, uint32_t a, uint32_t b, const TbkTagDrops &d, uint32_t new_len, uint8_t *dst) {
    const uint32_t end = 4 + tbk_bam_u32(rec), new_bs = new_len - 4;
    for (int i = 0; i < 4; i++) dst[i] = (uint8_t)(new_bs >> (8 * i));
    uint8_t *w = dst + 4;
    uint32_t from = 4;
    for (int k = 0; k < 3 && d.len[k]; k++) {
        memcpy(w, rec + from, d.at[k] - from);
        w += d.at[k] - from;
        from = d.at[k] + d.len[k];
    }
    memcpy(w, rec + from, end - from);
    w += end - from;
    uint8_t tail[TBK_TAG_GROWTH];
    const uint32_t n = tbk_tag_tail(bin, a, b, tail);
    memcpy(w, tail, n);
}

// records[offsets[i]], i in [0, n), tagged with bins[i] and counts[2 i], counts[2 i + 1], back to back into dst[0 .. cap), on
// `threads` threads: all records are measured (a share each), their places summed, and - when they fit cap - written (a share
// each again).  out_off (n + 1 entries, may be NULL): where each tagged record begins, the total last; *out_len = the total, also
// when cap is too small, in which case nothing is written (*fits = false).  Returns TBK_BAM_NO_BAD, or (index of the first
// refused record << 8) | reason, with nothing written.
static inline uint64_t tbk_bam_haplotag_host(const uint8_t *records, const uint64_t *offsets, uint64_t n, const char *bins, const int32_t *counts, uint8_t *dst,
                                             uint64_t cap, uint64_t *out_off, uint64_t *out_len, bool *fits, int threads) {
    *out_len = 0; *fits = true;
    if (out_off) out_off[0] = 0;
    if (!n) return TBK_BAM_NO_BAD;
    const uint64_t most = n / 64 ? n / 64 : 1;   // (a thread is not worth fewer than 64 records)
    const int nt = threads < 1 ? 1 : ((uint64_t)threads > most ? (int)most : threads);
    std::vector<TbkTagDrops> drops((size_t)n);
    std::vector<uint64_t> own;                    // the records' places when the caller wants none
    if (!out_off) { own.assign((size_t)n + 1, 0); out_off = own.data(); }
    std::vector<uint64_t> bad((size_t)nt, TBK_BAM_NO_BAD);
    auto run = [&](auto &&share) {
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; t++) pool.emplace_back(share, t);
        share(0);
        for (std::thread &th : pool) th.join();
    };
    run([&](int t) {
        const uint64_t lo = n * (uint64_t)t / (uint64_t)nt, hi = n * (uint64_t)(t + 1) / (uint64_t)nt;
        for (uint64_t i = lo; i < hi; i++) {
            uint32_t len = 0;
            const uint32_t why = tbk_tag_measure(records + offsets[i], bins[i], &drops[(size_t)i], &len);
            if (why != TBK_BAM_OK) { bad[(size_t)t] = (i << 8) | why; return; }
            out_off[i + 1] = len;   // (summed below)
        }
    });
    for (int t = 0; t < nt; t++)
        if (bad[(size_t)t] != TBK_BAM_NO_BAD) return bad[(size_t)t];   // (the shares are in order: the first share's is the first)
    for (uint64_t i = 0; i < n; i++) out_off[i + 1] += out_off[i];
    *out_len = out_off[n];
    if (*out_len > cap || !dst) { *fits = false; return TBK_BAM_NO_BAD; }
    run([&](int t) {
        const uint64_t lo = n * (uint64_t)t / (uint64_t)nt, hi = n * (uint64_t)(t + 1) / (uint64_t)nt;
        for (uint64_t i = lo; i < hi; i++)
            tbk_tag_write_host(records + offsets[i], bins[i], (uint32_t)counts[2 * i], (uint32_t)counts[2 * i + 1], drops[(size_t)i], (uint32_t)(out_off[i + 1] - out_off[i]),
                               dst + out_off[i]);
    });
    return TBK_BAM_NO_BAD;
}

// ---- the device side (tbk_bam_tag.hip): a rewriter that keeps its buffers from batch to batch --------------------------------
// tbk_bamtag_run copies a run of records, their offsets, bins and counts to the device, measures, scans and writes the tagged
// records, and brings them home into dst (cap bytes; host memory, pinned or not): *out_len = their bytes (set with
// TBK_ERR_NOMEM too, when cap is short and nothing is written), out_off as above (may be NULL), *bad = TBK_BAM_NO_BAD or
// (index of the first refused record << 8 | reason), with nothing written.
struct tbk_bamtag;
int tbk_bamtag_create(int device, tbk_bamtag **out);
void tbk_bamtag_destroy(tbk_bamtag *t);
int tbk_bamtag_run(tbk_bamtag *t, const uint8_t *records, uint64_t size, const uint64_t *offsets, uint64_t n, const char *bins, const int32_t *counts, uint8_t *dst,
                   uint64_t cap, uint64_t *out_off, uint64_t *out_len, uint64_t *bad);
#endif /* TBK_BAM_TAG_H */
