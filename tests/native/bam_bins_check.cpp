// bam_bins_check.cpp — the host pieces of the BAM bins (include/tbk.h "BAM output") by themselves, for a run under
// AddressSanitizer and UBSan on the CPU:   bam_bins_check <uncompressed.bam> <out.bam> <window> [hints 0|1] [threads]
// Built from this file, csrc/tbk_deflate.cpp and csrc/tbk_crc.cpp (-lz); nothing of it is loaded into Python.
// The file is fed in windows of <window> bytes as bam_check.cpp feeds it; of every window the records are indexed
// (tbk_bam_index), the written ones picked (tbk_bam_written: the record-carrying index of the reader's chunks) and
// appended, whole, to one bin with their four cut hints (tbk_bam_hints) - every buffer sized exactly.  The bin then
// goes through the host bgzf coder (tbk_bgzf_members_threads_), the header through it by itself, and <out.bam> gets
// header blocks, record blocks and the end-of-file marker.  Also coded, and thrown away: the bin without hints, the bin
// under a too small buffer (TBK_ERR_NOMEM must say what is needed) and refused hint lists.
// Prints "ok <records kept> <records skipped> <members> <bytes out>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tbk_bam.h"

extern "C" int tbk_bgzf_members_threads_(const uint8_t *data, uint64_t size, const uint64_t *hints, uint64_t n_hints, uint8_t *dst, uint64_t cap, uint64_t *need,
                                         uint64_t *n_members, int threads);

static bool code(const std::vector<uint8_t> &data, const std::vector<uint64_t> &hints, int threads, std::vector<uint8_t> &out, uint64_t *members) {
    uint64_t need = 0;
    // the size query: no buffer at all, then one byte too few, then exactly enough
    int rc = tbk_bgzf_members_threads_(data.data(), data.size(), hints.data(), hints.size(), nullptr, 0, &need, members, threads);
    if (data.empty()) { out.clear(); return rc == 0 && need == 0 && *members == 0; }
    if (rc != -6 || !need) return false;
    std::vector<uint8_t> small(need - 1);
    uint64_t again = 0;
    if (tbk_bgzf_members_threads_(data.data(), data.size(), hints.data(), hints.size(), small.data(), small.size(), &again, members, threads) != -6 || again != need) return false;
    out.assign(need, 0);
    return tbk_bgzf_members_threads_(data.data(), data.size(), hints.data(), hints.size(), out.data(), out.size(), &again, members, threads) == 0 && again == need;
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
    const bool with_hints = argc > 4 ? atoi(argv[4]) != 0 : true;
    const int threads = argc > 5 ? atoi(argv[5]) : 3;
    if (!window) return 2;

    std::vector<uint8_t> left, header, bin;
    std::vector<uint64_t> hints;
    bool in_header = true;
    uint64_t kept = 0, skipped = 0;
    for (size_t at = 0; at < file.size() || at == 0; at += window) {
        const size_t take = at < file.size() ? (window < file.size() - at ? window : file.size() - at) : 0;
        std::vector<uint8_t> acc(left.size() + take);   // (exactly as long as its bytes)
        if (!left.empty()) memcpy(acc.data(), left.data(), left.size());
        if (take) memcpy(acc.data() + left.size(), file.data() + at, take);
        size_t pos = 0;
        if (in_header) {
            uint64_t len = 0;
            if (tbk_bam_header_len(acc.data(), acc.size(), &len) != 0) return 3;
            if (len) { in_header = false; pos = (size_t)len; header.assign(acc.begin(), acc.begin() + (long)len); }
        }
        while (!in_header) {
            constexpr uint64_t CAP = 7;   // (small: the index fills up in the middle of a window)
            std::vector<uint64_t> offsets(CAP);
            uint64_t n = 0, consumed = 0;
            const uint32_t why = tbk_bam_index(acc.data() + pos, acc.size() - pos, offsets.data(), CAP, &n, &consumed);
            if (why != TBK_BAM_OK) return 3;
            // the chunk's own copy of the records, exactly as long as they are, and its slices
            std::vector<uint8_t> bytes(acc.begin() + (long)pos, acc.begin() + (long)(pos + consumed));
            std::vector<TbkBamSlice> slices;
            tbk_bam_written(bytes.data(), offsets.data(), n, TBK_BAM_SKIP_DEFAULT_, slices);
            uint64_t text = 0, w = 0, s = 0;
            if (tbk_bam_fastq_host(bytes.data(), offsets.data(), n, TBK_BAM_SKIP_DEFAULT_, nullptr, 0, nullptr, &text, &w, &s) != TBK_BAM_NO_BAD) return 3;
            if (w != slices.size() || w + s != n) return 4;   // the written count and the kept count must agree
            for (const TbkBamSlice &sl : slices) {
                if (sl.off + sl.len > bytes.size()) return 4;
                uint64_t h[4];
                tbk_bam_hints(bytes.data() + sl.off, sl.len, bin.size(), h);
                for (int k = 0; k < 4; k++) if (h[k] > bin.size() + sl.len || (k && h[k] < h[k - 1])) return 4;
                if (with_hints) hints.insert(hints.end(), h, h + 4);
                bin.insert(bin.end(), bytes.begin() + (long)sl.off, bytes.begin() + (long)(sl.off + sl.len));
            }
            kept += w; skipped += s;
            pos += (size_t)consumed;
            if (n < CAP) break;
        }
        left.assign(acc.begin() + (long)pos, acc.end());
        if (at + window >= file.size()) break;
    }
    if (in_header || !left.empty()) return 3;

    std::vector<uint8_t> head_blocks, rec_blocks, scratch;
    uint64_t head_members = 0, members = 0, m2 = 0;
    if (!code(header, {}, threads, head_blocks, &head_members)) return 5;
    if (!code(bin, hints, threads, rec_blocks, &members)) return 5;
    if (!code(bin, {}, 1, scratch, &m2) || m2 != members) return 5;            // fixed cuts, one thread
    if (!code({}, {}, threads, scratch, &m2)) return 5;                        // nothing in, nothing out
    // refused hint lists: decreasing, beyond the end
    uint64_t need = 0;
    const uint64_t down[2] = {5, 4}, past[1] = {bin.size() + 1};
    if (bin.size() >= 5 && tbk_bgzf_members_threads_(bin.data(), bin.size(), down, 2, nullptr, 0, &need, &m2, 1) != -1) return 6;
    if (tbk_bgzf_members_threads_(bin.data(), bin.size(), past, 1, nullptr, 0, &need, &m2, 1) != -1) return 6;

    static const unsigned char marker[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    if (fwrite(head_blocks.data(), 1, head_blocks.size(), out) != head_blocks.size()) return 2;
    if (!rec_blocks.empty() && fwrite(rec_blocks.data(), 1, rec_blocks.size(), out) != rec_blocks.size()) return 2;
    if (fwrite(marker, 1, sizeof marker, out) != sizeof marker) return 2;
    fclose(out);
    printf("ok %llu %llu %llu %llu\n", (unsigned long long)kept, (unsigned long long)skipped, (unsigned long long)(head_members + members),
           (unsigned long long)(head_blocks.size() + rec_blocks.size() + sizeof marker));
    return 0;
}
