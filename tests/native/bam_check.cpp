// bam_check.cpp — the host pieces of the BAM input (csrc/tbk_bam.h) by themselves, for a run under AddressSanitizer and
// UBSan on the CPU:   bam_check <uncompressed.bam> <out.fastq> <window> [skip_flags] [index_cap]
// The file is fed in windows of <window> bytes, the way the reader's loop gets its inflated text: what a window leaves
// over (part of the header, part of a record) goes in front of the next.  Every buffer is sized exactly, so that a read
// past a window's end is caught; the threaded form (tbk_bam_fastq_shares, three threads) must agree with the plain one.
// Prints "ok <records written> <records skipped>", or "refused <record number> <reason>" with exit status 3.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tbk_bam.h"

static int refuse(uint64_t record, const char *why) {
    printf("refused %llu %s\n", (unsigned long long)record, why);
    return 3;
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> file;
    uint8_t tmp[4096];
    for (size_t got; (got = fread(tmp, 1, sizeof tmp, f)) > 0;) file.insert(file.end(), tmp, tmp + got);
    fclose(f);
    const size_t window = (size_t)strtoull(argv[3], nullptr, 10);
    const uint32_t skip = argc > 4 ? (uint32_t)strtoul(argv[4], nullptr, 0) : TBK_BAM_SKIP_DEFAULT_;
    const uint64_t index_cap = argc > 5 ? strtoull(argv[5], nullptr, 10) : 1000;
    if (!window || !index_cap) return 2;
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;

    std::vector<uint8_t> left;
    bool in_header = true;
    uint64_t records = 0, written = 0, skipped = 0;
    for (size_t at = 0; at < file.size() || at == 0; at += window) {
        const size_t take = at < file.size() ? (window < file.size() - at ? window : file.size() - at) : 0;
        std::vector<uint8_t> acc(left.size() + take);   // (exactly as long as its bytes)
        if (!left.empty()) memcpy(acc.data(), left.data(), left.size());
        if (take) memcpy(acc.data() + left.size(), file.data() + at, take);
        size_t pos = 0;
        if (in_header) {
            uint64_t len = 0;
            if (tbk_bam_header_len(acc.data(), acc.size(), &len) != 0) return refuse(0, "not a BAM file");
            if (len) { in_header = false; pos = (size_t)len; }
        }
        while (!in_header) {
            std::vector<uint64_t> offsets(index_cap);
            uint64_t n = 0, consumed = 0;
            const uint32_t why = tbk_bam_index(acc.data() + pos, acc.size() - pos, offsets.data(), index_cap, &n, &consumed);
            uint64_t need = 0, w = 0, s = 0;
            uint64_t bad = tbk_bam_fastq_host(acc.data() + pos, offsets.data(), n, skip, nullptr, 0, nullptr, &need, &w, &s);
            if (bad != TBK_BAM_NO_BAD) return refuse(records + (bad >> 8), tbk_bam_reason((uint32_t)(bad & 0xFF)));
            std::vector<uint8_t> text(need);
            std::vector<uint32_t> lengths(n);
            bad = tbk_bam_fastq_host(acc.data() + pos, offsets.data(), n, skip, text.data(), need, lengths.data(), &need, &w, &s);
            if (bad != TBK_BAM_NO_BAD || need != text.size()) return 4;
            uint64_t sum = 0;
            for (uint32_t l : lengths) sum += l;
            if (sum != need) return 4;
            // the threaded form must write the same text and count the same records
            TbkBamShares shares;
            uint64_t need_mt = 0, w_mt = 0, s_mt = 0;
            if (tbk_bam_fastq_shares(acc.data() + pos, offsets.data(), n, skip, 3, shares, nullptr, &need_mt, &w_mt, &s_mt) != TBK_BAM_NO_BAD || need_mt != need) return 5;
            std::vector<uint8_t> text_mt(need);
            if (tbk_bam_fastq_shares(acc.data() + pos, offsets.data(), n, skip, 3, shares, text_mt.data(), &need_mt, &w_mt, &s_mt) != TBK_BAM_NO_BAD) return 5;
            if (text_mt != text || w_mt != w || s_mt != s) return 5;
            if (need && fwrite(text.data(), 1, need, out) != need) return 2;
            records += n; written += w; skipped += s;
            pos += (size_t)consumed;
            if (why != TBK_BAM_OK) return refuse(records, tbk_bam_reason(why));
            if (n < index_cap) break;   // (the walk stopped for want of bytes, not of room)
        }
        left.assign(acc.begin() + (long)pos, acc.end());
        if (at + window >= file.size()) break;
    }
    fclose(out);
    if (in_header) return refuse(0, "the file ends inside the header");
    if (!left.empty()) return refuse(records, tbk_bam_reason(TBK_BAM_CUT_OFF));
    printf("ok %llu %llu\n", (unsigned long long)written, (unsigned long long)skipped);
    return 0;
}
