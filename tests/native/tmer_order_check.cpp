// Checks of the searched t-mer order (csrc/tbk_tmer_order.h) as tbk_common.h uses it, for tests/test_tmer_order.py:
//   table     a function of the canonical 4-mer, low 5 bits zero, one rank per canonical 4-mer
//   rank      tbk_tmer_rank reads the table at t = 4 and the hash at every other t
//   strands   a k-mer and its reverse complement select the same buckets (tbk_bucket_candidates), and tbk_bucket_of picks one of them
// Prints one "ok ..." line per check, or "FAIL ..." and exits 1.
#include <cstdio>
#include <random>
#include <set>
#include "../../trio_binning_amd/csrc/tbk_common.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAIL "); printf(__VA_ARGS__); printf("\n"); fails++; } } while (0)

int main() {
    std::set<uint32_t> ranks;
    int canon = 0;
    for (uint32_t x = 0; x < 256; x++) {
        const uint32_t y = tbk_revcomp32(x, 4);
        CHECK(tbk_tmer4_ranks[x] == tbk_tmer4_ranks[y], "x %u and its reverse complement %u differ", x, y);
        CHECK((tbk_tmer4_ranks[x] & 31u) == 0, "x %u: low bits %u", x, tbk_tmer4_ranks[x] & 31u);
        CHECK(tbk_tmer4_ranks[x] != 0xFFFFFFFFu, "x %u: rank is the empty sentinel", x);
        if (x <= y) { canon++; ranks.insert(tbk_tmer4_ranks[x]); }
    }
    CHECK(canon == 136 && ranks.size() == 136, "%d canonical 4-mers, %zu distinct ranks", canon, ranks.size());
    if (!fails) printf("ok table\n");

    std::mt19937_64 rng(5);
    int n_t4 = 0;
    for (int k = 15; k <= 32; k++)
        for (int w = 2; w <= 8; w++)
            for (int m = 8; m <= 16; m++) {
                TbkMz z = tbk_mz_params(k, w, 1000, m, 1);
                if (z.t == 0) continue;
                for (int span3 = 0; span3 < 2; span3++) {
                    const TbkMz zz = span3 ? tbk_mz_span3(z) : z;
                    const uint32_t tmask = zz.t == 16 ? 0xFFFFFFFFu : ((1u << (2 * zz.t)) - 1u);
                    n_t4 += zz.t == 4;
                    for (int rep = 0; rep < 50; rep++) {
                        const uint64_t key = rng() & (k == 32 ? ~0ull : ((1ull << (2 * k)) - 1));
                        for (int i = 0; i < tbk_mz_positions(zz); i++) {
                            const uint32_t x = (uint32_t)(key >> (2 * (zz.o + i))) & tmask, y = tbk_revcomp32(x, zz.t);
                            const uint32_t want = (zz.t == 4 ? tbk_tmer4_ranks[x] : tbk_mmer_hash(x < y ? x : y)) & ~tbk_mz_tagmask(zz);
                            CHECK(tbk_tmer_rank(key, zz, i) == want, "k %d w %d m %d t %d position %d", k, w, zz.m, zz.t, i);
                        }
                    }
                }
            }
    CHECK(n_t4 > 0, "no span with t = 4");
    if (!fails) printf("ok rank (%d spans with t = 4)\n", n_t4);

    // strand flips: k = 21 at the bench's span (w = 6, m = 16, t = 4) and at the other spans that rank 4-mers
    const int spans[][3] = {{21, 6, 0}, {22, 5, 14}, {19, 4, 12}, {23, 6, 0}};
    for (const auto &s : spans) {
        const int k = s[0];
        const TbkMz z = tbk_mz_span3(tbk_mz_params(k, s[1], 300000000, s[2], 1));
        CHECK(z.t == 4 || k == 23, "k %d: t %d", k, z.t);
        const uint64_t kmask = (1ull << (2 * k)) - 1;
        uint64_t tied = 0;
        for (int rep = 0; rep < 200000; rep++) {
            uint64_t key = rng() & kmask;
            if (rep % 4 == 1) key = (key & ~0xFFFFull) | (0x5555ull * (rng() & 3));   // runs of one base: ties
            if (rep % 4 == 2) { const uint64_t u = rng() & 0xFF; key = u * 0x0101010101ull & kmask; }
            const uint64_t rc = tbk_revcomp_packed(key, k);
            const uint32_t n_buckets = 261131725u;
            uint32_t a[16], b[16];
            const int na = tbk_bucket_candidates(key, z, n_buckets, a), nb = tbk_bucket_candidates(rc, z, n_buckets, b);
            tied += na > 1;
            const std::set<uint32_t> sa(a, a + na), sb(b, b + nb);
            CHECK(na >= 1 && sa == sb, "k %d key %llx: %d and %d candidate buckets", k, (unsigned long long)key, na, nb);
            CHECK(sa.count(tbk_bucket_of(key, z, n_buckets)) && sa.count(tbk_bucket_of(rc, z, n_buckets)), "k %d key %llx: tbk_bucket_of", k, (unsigned long long)key);
            if (fails > 10) return 1;
        }
        CHECK(tied > 0, "k %d: no ties met", k);
        printf("ok strands k %d w %d m %d t %d (%llu tied)\n", k, z.w, z.m, z.t, (unsigned long long)tied);
    }
    return fails ? 1 : 0;
}
