// bam_tag_check.cpp — the host pieces of the haplotag output (csrc/tbk_bam_tag.h) by themselves, for a run under
// AddressSanitizer and UBSan on the CPU:   bam_tag_check <records.raw> <plan.bin> <out.raw> <threads> <run|alone>
// records.raw: whole BAM records back to back.  plan.bin: per record one byte of bin and two int32 counts (9 bytes).
// run: all records in one call, on <threads> threads.  alone: every record in a call of its own, from a heap block that is
// exactly as long as the record, so that a read past any record's end is caught.  Every output buffer is sized exactly: the
// first call measures (no dst), the second writes into out_len bytes.  out.raw gets the tagged records; stdout gets
// "ok <records> <bytes> <out_off ...>", or "refused <record number> <reason>" with exit status 3.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tbk_bam_tag.h"

static bool slurp(const char *path, std::vector<uint8_t> &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t tmp[65536];
    for (size_t got; (got = fread(tmp, 1, sizeof tmp, f)) > 0;) out.insert(out.end(), tmp, tmp + got);
    fclose(f);
    return true;
}

// one run through the host rewriter with exactly sized buffers; appends the tagged records and their places
static int rewrite(const uint8_t *records, const std::vector<uint64_t> &offsets, const char *bins, const int32_t *counts, int threads, uint64_t first,
                   std::vector<uint8_t> &out, std::vector<uint64_t> &places) {
    const uint64_t n = offsets.size();
    uint64_t len = 0, len2 = 0;
    bool fits = true;
    std::vector<uint64_t> off(n + 1), off2(n + 1);
    uint64_t bad = tbk_bam_haplotag_host(records, offsets.data(), n, bins, counts, nullptr, 0, off.data(), &len, &fits, threads);
    if (bad != TBK_BAM_NO_BAD) {
        printf("refused %llu %s\n", (unsigned long long)(first + (bad >> 8)), tbk_tag_reason((uint32_t)(bad & 0xFF)));
        return 3;
    }
    if (n && (fits || !len)) return 4;           // (no dst: measured only)
    uint8_t *dst = (uint8_t *)malloc(len ? len : 1);
    if (len > 1) {                               // one byte short: nothing may be written, the length must come all the same
        bad = tbk_bam_haplotag_host(records, offsets.data(), n, bins, counts, dst, len - 1, nullptr, &len2, &fits, threads);
        if (bad != TBK_BAM_NO_BAD || fits || len2 != len) { free(dst); return 5; }
    }
    bad = tbk_bam_haplotag_host(records, offsets.data(), n, bins, counts, dst, len, off2.data(), &len2, &fits, threads);
    if (bad != TBK_BAM_NO_BAD || !fits || len2 != len || off2 != off) { free(dst); return 6; }
    const uint64_t base = out.size();
    out.insert(out.end(), dst, dst + len);
    free(dst);
    for (uint64_t i = 0; i < n; i++) places.push_back(base + off[i + 1]);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    std::vector<uint8_t> file, plan;
    if (!slurp(argv[1], file) || !slurp(argv[2], plan)) return 2;
    const int threads = atoi(argv[4]);
    const bool alone = argv[5][0] == 'a';
    std::vector<uint64_t> offsets(file.size() / 36 + 1);
    uint64_t n = 0, consumed = 0;
    if (tbk_bam_index(file.data(), file.size(), offsets.data(), offsets.size(), &n, &consumed) != TBK_BAM_OK || consumed != file.size()) return 2;
    offsets.resize(n);
    if (plan.size() != 9 * n) return 2;
    std::vector<char> bins(n);
    std::vector<int32_t> counts(2 * n);
    for (uint64_t i = 0; i < n; i++) {
        bins[i] = (char)plan[9 * i];
        memcpy(&counts[2 * i], &plan[9 * i + 1], 8);
    }
    std::vector<uint8_t> out;
    std::vector<uint64_t> places(1, 0);
    if (alone) {
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t len = (i + 1 < n ? offsets[i + 1] : file.size()) - offsets[i];
            uint8_t *rec = (uint8_t *)malloc(len);   // exactly the record
            memcpy(rec, file.data() + offsets[i], len);
            const int rc = rewrite(rec, std::vector<uint64_t>(1, 0), &bins[i], &counts[2 * i], 1, i, out, places);
            free(rec);
            if (rc) return rc;
        }
    } else {
        uint8_t *all = (uint8_t *)malloc(file.size() ? file.size() : 1);
        if (!file.empty()) memcpy(all, file.data(), file.size());
        const int rc = rewrite(all, offsets, bins.data(), counts.data(), threads, 0, out, places);
        free(all);
        if (rc) return rc;
    }
    FILE *f = fopen(argv[3], "wb");
    if (!f || (!out.empty() && fwrite(out.data(), 1, out.size(), f) != out.size())) return 2;
    fclose(f);
    printf("ok %llu %llu", (unsigned long long)n, (unsigned long long)out.size());
    for (uint64_t p : places) printf(" %llu", (unsigned long long)p);
    printf("\n");
    return 0;
}
