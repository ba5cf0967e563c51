// Searches the order in which mod-sampling ranks the 136 canonical 4-mers (k = 21: w = 6, m = 16, t = 4, 18 t-mer positions:
// tbk_mz_span3) for fewer table lines per window, and writes the winner as csrc/tbk_tmer_order.h.
//
// Any order of the canonical t-mers is a valid sampling rule: the insert side and the probe kernels only have to agree on it, and
// the single-read probe kernel reads a t-mer's rank from a 256-entry table anyway.  The hash order (tbk_mmer_hash) is a random one.
// The search starts from it and hill-climbs: batches of random swaps and moves of ranks, the best improving one kept.
//   objective    the `lanes` metric of tools/sampling_density.cpp: windows cut into lanes of 32, even lanes walk up the forward strand
//                (ties to the lowest position), odd lanes walk down it on the reverse strand (ties to the highest forward position);
//                a lane's first window always fetches unless the neighbouring lane starts on the same bucket; every bucket switch
//                inside a lane is another line.  That is what the probe kernel pays.  `continuous` (one walk up) is reported beside it.
//   training     one random sequence; scores are reported on a held-out random sequence and on haplotype-like sequence (a 40 % GC
//                genome with CpG depletion, two SNP'd copies of it cut into 15 kb reads with 0.1 % substitution errors).  A move
//                is only taken if it keeps the tie rate on a haplotype-like training sequence within --max-tie-rise (relative) of
//                the hash order's: unconstrained, the search ranks AT-rich 4-mers low and real-shaped sequence ties more often.
//   table build  the tie rate (windows whose smallest rank sits at positions that name different m-mers: the insert side stores
//                the key under each of them) and the distinct sampled canonical 16-mers per 1e8 windows (fewer = crowded buckets)
//   g++ -O3 -march=native -std=c++17 -pthread -I trio_binning_amd/csrc -o /tmp/tmer_order_search tools/tmer_order_search.cpp
//   /tmp/tmer_order_search [--iters N] [--seed S] [--train BASES] [--test BASES] [--distinct WINDOWS] [--max-tie-rise-permille P]
//                          [--out HEADER]
// With --out the winning order is written as the header (256 ranks by forward 4-mer code, canonical form folded in, low 5 bits
// zero: the format of the probe kernel's LDS table); the order compiled into tbk_common.h is scored beside it either way, through
// tbk_tmer_rank itself, which checks that the header in the tree is the order this tool found.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>
#include "tbk_common.h"

namespace {

constexpr int K = 21, NT = 18;
constexpr uint32_t N_BUCKETS = 261131725u;  // the bench's 3e8-key table (tools/sampling_density.cpp)
TbkMz g_z;

uint32_t canon4(uint32_t x) { const uint32_t y = tbk_revcomp32(x, 4); return x < y ? x : y; }

std::vector<uint8_t> random_bases(uint64_t n, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::vector<uint8_t> b(n);
    for (auto &x : b) x = (uint8_t)(rng() & 3);
    return b;
}

// A genome of 40 % GC whose C -> G steps are cut to a quarter (CpG depletion), two haplotypes with a SNP every ~1000 bases,
// reads of 15 kb from either haplotype with 0.1 % substitution errors, concatenated.
std::vector<uint8_t> haplotype_like(uint64_t n, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    const uint64_t glen = std::max<uint64_t>(n / 4, 100000);
    std::vector<uint8_t> g(glen);
    const double p[4] = {0.3, 0.2, 0.2, 0.3};  // A C G T
    uint8_t prev = 0;
    for (uint64_t i = 0; i < glen; i++) {
        double q[4] = {p[0], p[1], p[2], p[3]};
        if (prev == 1) { q[2] *= 0.25; }
        const double s = q[0] + q[1] + q[2] + q[3];
        double r = u(rng) * s;
        uint8_t c = 0;
        while (c < 3 && r >= q[c]) { r -= q[c]; c++; }
        g[i] = prev = c;
    }
    std::vector<uint8_t> h[2] = {g, g};
    for (int hp = 0; hp < 2; hp++)
        for (uint64_t i = 0; i < glen; i++)
            if (u(rng) < 0.0005) h[hp][i] = (uint8_t)((h[hp][i] + 1 + (rng() % 3)) & 3);
    std::vector<uint8_t> out;
    out.reserve(n);
    const uint64_t rlen = 15000;
    while (out.size() < n) {
        const auto &src = h[rng() & 1];
        const uint64_t at = rng() % (glen - rlen);
        for (uint64_t i = 0; i < rlen && out.size() < n; i++) {
            uint8_t c = src[at + i];
            if (u(rng) < 0.001) c = (uint8_t)((c + 1 + (rng() % 3)) & 3);
            out.push_back(c);
        }
    }
    return out;
}

// per base position: the forward 4-mer code there (base j in the low bits, as tbk_tmer_rank reads a key) and the bucket of the
// canonical 16-mer that starts there
struct Prepared {
    std::vector<uint8_t> code;
    std::vector<uint32_t> cm, bucket;
    uint64_t n_win = 0;
};

Prepared prepare(const std::vector<uint8_t> &b) {
    Prepared p;
    const uint64_t n = b.size();
    p.n_win = n - K + 1;
    p.code.assign(n, 0);
    p.cm.assign(n, 0);
    p.bucket.assign(n, 0);
    for (uint64_t j = 0; j + 4 <= n; j++) p.code[j] = (uint8_t)(b[j] | b[j + 1] << 2 | b[j + 2] << 4 | b[j + 3] << 6);
    for (uint64_t j = 0; j + 16 <= n; j++) {
        uint32_t x = 0;
        for (int i = 0; i < 16; i++) x |= (uint32_t)b[j + i] << (2 * i);
        const uint32_t y = tbk_revcomp32(x, 16);
        p.cm[j] = x < y ? x : y;
        p.bucket[j] = tbk_reduce(tbk_mmer_hash(p.cm[j]), N_BUCKETS);
    }
    return p;
}

struct Score {
    uint64_t lanes = 0, cont = 0, ties = 0, extra = 0, covered = 0, n_win = 0;
    double lanes_d() const { return covered ? (double)lanes / (double)covered : 0.0; }
    double cont_d() const { return n_win ? (double)cont / (double)n_win : 0.0; }
    double tie_d() const { return n_win ? (double)ties / (double)n_win : 0.0; }
    double extra_d() const { return n_win ? (double)extra / (double)n_win : 0.0; }
};

// rank[x]: the rank of forward 4-mer code x, low 5 bits zero
Score evaluate(const Prepared &p, const uint32_t *rank, bool with_ties) {
    Score s;
    s.n_win = p.n_win;
    const uint64_t n_win = p.n_win;
    std::vector<uint32_t> lo(n_win), hi(n_win);
    std::vector<uint32_t> rk(p.code.size());
    for (size_t j = 0; j < rk.size(); j++) rk[j] = rank[p.code[j]];
    for (uint64_t i = 0; i < n_win; i++) {
        const uint32_t *r = &rk[i];
        uint32_t bl = 0xFFFFFFFFu, bh = 0xFFFFFFFFu;
        for (int q = 0; q < NT; q++) {
            const uint32_t a = r[q] | (uint32_t)q, c = r[q] | (uint32_t)(NT - 1 - q);
            bl = a < bl ? a : bl;
            bh = c < bh ? c : bh;
        }
        const int pl = (int)(bl & 31u), ph = NT - 1 - (int)(bh & 31u);
        lo[i] = p.bucket[i + g_z.o + pl % g_z.w];
        hi[i] = p.bucket[i + g_z.o + ph % g_z.w];
        if (with_ties && pl != ph) {
            const uint32_t best = bl & ~31u;
            unsigned seen = 0;
            for (int q = 0; q < NT; q++) if (r[q] == best) seen |= 1u << (q % g_z.w);
            const int d = __builtin_popcount(seen);
            s.ties += d > 1;
            s.extra += (uint64_t)(d - 1);
        }
    }
    s.cont = 1;
    for (uint64_t i = 1; i < n_win; i++) s.cont += lo[i] != lo[i - 1];
    const uint64_t n_lanes = n_win / 32;
    for (uint64_t L = 0; L < n_lanes; L++) {
        const uint64_t a = 32 * L;
        const bool up = (L & 1) == 0;
        const uint32_t *v = up ? &lo[a] : &hi[a];
        uint64_t sw = 0;
        for (int j = 1; j < 32; j++) sw += v[j] != v[j - 1];
        // even lane L starts at a beside odd lane L - 1's start a - 1: one request when both name one bucket
        const bool first = !(up && L > 0 && lo[a] == hi[a - 1]);
        s.lanes += sw + (first ? 1 : 0);
    }
    s.covered = n_lanes * 32;
    return s;
}

// the same metrics through tbk_tmer_rank / tbk_bucket_candidates themselves (the order compiled into tbk_common.h)
Score evaluate_compiled(const std::vector<uint8_t> &b) {
    Score s;
    const uint64_t n_win = b.size() - K + 1, kmask = (1ull << (2 * K)) - 1;
    s.n_win = n_win;
    std::vector<uint32_t> lo(n_win), hi(n_win);
    uint64_t fwd = 0;
    for (uint64_t i = 0; i < b.size(); i++) {
        fwd = (fwd >> 2) | ((uint64_t)b[i] << (2 * (K - 1)));
        if (i + 1 < (uint64_t)K) continue;
        const uint64_t f = fwd & kmask, w = i + 1 - K;
        uint32_t bl = 0xFFFFFFFFu, bh = 0xFFFFFFFFu;
        for (int q = 0; q < NT; q++) {
            const uint32_t r = tbk_tmer_rank(f, g_z, q);
            bl = std::min(bl, r | (uint32_t)q);
            bh = std::min(bh, r | (uint32_t)(NT - 1 - q));
        }
        lo[w] = tbk_bucket_at(f, g_z, (int)(bl & 31u) % g_z.w, N_BUCKETS);
        hi[w] = tbk_bucket_at(f, g_z, (NT - 1 - (int)(bh & 31u)) % g_z.w, N_BUCKETS);
        uint32_t cand[16];
        const int nc = tbk_bucket_candidates(f, g_z, N_BUCKETS, cand);
        s.ties += nc > 1;
        s.extra += (uint64_t)(nc - 1);
    }
    s.cont = 1;
    for (uint64_t i = 1; i < n_win; i++) s.cont += lo[i] != lo[i - 1];
    const uint64_t n_lanes = n_win / 32;
    for (uint64_t L = 0; L < n_lanes; L++) {
        const uint64_t a = 32 * L;
        const bool up = (L & 1) == 0;
        const uint32_t *v = up ? &lo[a] : &hi[a];
        uint64_t sw = 0;
        for (int j = 1; j < 32; j++) sw += v[j] != v[j - 1];
        s.lanes += sw + (!(up && L > 0 && lo[a] == hi[a - 1]) ? 1 : 0);
    }
    s.covered = n_lanes * 32;
    return s;
}

// distinct sampled canonical 16-mers over `n_win` windows of random sequence (forward walk, ties to the lowest position)
uint64_t distinct_sampled(const uint32_t *rank, uint64_t n_win, uint64_t seed, uint64_t *events) {
    const uint64_t chunk = 1u << 24;
    std::vector<uint32_t> got;
    uint32_t last = 0xFFFFFFFFu;
    *events = 0;
    for (uint64_t done = 0; done < n_win; done += chunk) {
        const uint64_t nw = std::min(chunk, n_win - done);
        const std::vector<uint8_t> b = random_bases(nw + K - 1, seed + done);
        const Prepared p = prepare(b);
        std::vector<uint32_t> rk(p.code.size());
        for (size_t j = 0; j < rk.size(); j++) rk[j] = rank[p.code[j]];
        for (uint64_t i = 0; i < nw; i++) {
            uint32_t bl = 0xFFFFFFFFu;
            for (int q = 0; q < NT; q++) { const uint32_t a = rk[i + q] | (uint32_t)q; bl = a < bl ? a : bl; }
            const uint32_t cm = p.cm[i + g_z.o + (bl & 31u) % g_z.w];
            if (cm != last) { got.push_back(cm); last = cm; ++*events; }
        }
    }
    std::sort(got.begin(), got.end());
    return (uint64_t)(std::unique(got.begin(), got.end()) - got.begin());
}

void ranks_from_perm(const std::vector<uint32_t> &perm, uint32_t *rank) {
    uint32_t pos[256];
    for (size_t i = 0; i < perm.size(); i++) pos[perm[i]] = (uint32_t)i;
    for (uint32_t x = 0; x < 256; x++) rank[x] = pos[canon4(x)] << 5;
}

uint64_t arg_u64(int argc, char **argv, const char *name, uint64_t def) {
    for (int i = 1; i + 1 < argc; i++) if (!strcmp(argv[i], name)) return strtoull(argv[i + 1], nullptr, 10);
    return def;
}
const char *arg_str(int argc, char **argv, const char *name) {
    for (int i = 1; i + 1 < argc; i++) if (!strcmp(argv[i], name)) return argv[i + 1];
    return nullptr;
}

}  // namespace

int main(int argc, char **argv) {
    const uint64_t iters = arg_u64(argc, argv, "--iters", 3000), seed = arg_u64(argc, argv, "--seed", 7);
    const uint64_t n_train = arg_u64(argc, argv, "--train", 1000000), n_test = arg_u64(argc, argv, "--test", 4000000);
    const uint64_t n_distinct = arg_u64(argc, argv, "--distinct", 100000000);
    const char *out = arg_str(argc, argv, "--out");
    g_z = tbk_mz_span3(tbk_mz_params(K, 6, 300000000, 0, 1));
    if (g_z.w != 6 || g_z.m != 16 || g_z.t != 4 || tbk_mz_positions(g_z) != NT || g_z.o != 0) { fprintf(stderr, "unexpected span\n"); return 1; }

    // the hash order: canonical 4-mers sorted by tbk_mmer_hash with the low 5 bits cleared (ties: none among the 136)
    std::vector<uint32_t> perm;
    for (uint32_t x = 0; x < 256; x++) if (canon4(x) == x) perm.push_back(x);
    std::stable_sort(perm.begin(), perm.end(), [](uint32_t a, uint32_t b) { return (tbk_mmer_hash(a) & ~31u) < (tbk_mmer_hash(b) & ~31u); });
    std::vector<uint32_t> hash_perm = perm;
    uint32_t hash_rank[256], rank[256];
    ranks_from_perm(hash_perm, hash_rank);

    const double max_tie_rise = arg_u64(argc, argv, "--max-tie-rise-permille", 20) / 1000.0;
    const Prepared train = prepare(random_bases(n_train, seed)), train_hap = prepare(haplotype_like(n_train, seed + 500));
    const uint64_t tie_cap = (uint64_t)((double)evaluate(train_hap, hash_rank, true).ties * (1.0 + max_tie_rise));
    std::mt19937_64 rng(seed * 0x9E3779B97F4A7C15ull + 1);
    ranks_from_perm(perm, rank);
    uint64_t cur = evaluate(train, rank, false).lanes;
    const uint64_t start = cur;
    const int batch = 16;
    const unsigned n_threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    for (uint64_t it = 0; it < iters; it++) {
        std::vector<std::vector<uint32_t>> cand(batch, perm);
        for (int c = 0; c < batch; c++) {
            const size_t i = rng() % perm.size(), j = rng() % perm.size();
            if (rng() & 1) std::swap(cand[c][i], cand[c][j]);
            else { const uint32_t v = cand[c][i]; cand[c].erase(cand[c].begin() + i); cand[c].insert(cand[c].begin() + j, v); }
        }
        std::vector<uint64_t> sc(batch);
        std::atomic<int> next(0);
        std::vector<std::thread> th;
        for (unsigned t = 0; t < n_threads; t++)
            th.emplace_back([&] {
                uint32_t r[256];
                for (int c; (c = next++) < batch;) {
                    ranks_from_perm(cand[c], r);
                    sc[c] = evaluate(train, r, false).lanes;
                    if (sc[c] < cur && evaluate(train_hap, r, true).ties > tie_cap) sc[c] = ~0ull;
                }
            });
        for (auto &t : th) t.join();
        const int b = (int)(std::min_element(sc.begin(), sc.end()) - sc.begin());
        if (sc[b] < cur) { cur = sc[b]; perm = cand[b]; }
        if (it % 500 == 499) fprintf(stderr, "iter %llu: train lanes %.4f (start %.4f)\n", (unsigned long long)it + 1, (double)cur / (double)train.n_win, (double)start / (double)train.n_win);
    }
    ranks_from_perm(perm, rank);

    const std::vector<uint8_t> test_b = random_bases(n_test, seed + 1000), hap_b = haplotype_like(n_test, seed + 2000);
    const Prepared test = prepare(test_b), hap = prepare(hap_b);
    const Score th_ = evaluate(test, hash_rank, true), tb = evaluate(test, rank, true);
    const Score hh = evaluate(hap, hash_rank, true), hb = evaluate(hap, rank, true);
    const Score trh = evaluate(train, hash_rank, false), trb = evaluate(train, rank, false);
    uint64_t ev_h = 0, ev_b = 0;
    const uint64_t dh = distinct_sampled(hash_rank, n_distinct, seed + 3000, &ev_h), db = distinct_sampled(rank, n_distinct, seed + 3000, &ev_b);
    const Score ch = evaluate_compiled(test_b);
    char line[4][256];
    snprintf(line[0], sizeof line[0], "train %llu random bases: lanes %.4f -> %.4f", (unsigned long long)n_train, trh.lanes_d(), trb.lanes_d());
    snprintf(line[1], sizeof line[1], "held-out %llu random bases: lanes %.4f -> %.4f (%+.2f %%), continuous %.4f -> %.4f, tie rate %.4f -> %.4f",
             (unsigned long long)n_test, th_.lanes_d(), tb.lanes_d(), 100.0 * (tb.lanes_d() / th_.lanes_d() - 1.0), th_.cont_d(), tb.cont_d(), th_.tie_d(), tb.tie_d());
    snprintf(line[2], sizeof line[2], "haplotype-like %llu bases: lanes %.4f -> %.4f (%+.2f %%), continuous %.4f -> %.4f, tie rate %.4f -> %.4f",
             (unsigned long long)n_test, hh.lanes_d(), hb.lanes_d(), 100.0 * (hb.lanes_d() / hh.lanes_d() - 1.0), hh.cont_d(), hb.cont_d(), hh.tie_d(), hb.tie_d());
    snprintf(line[3], sizeof line[3], "distinct sampled 16-mers per %llu windows: %llu -> %llu (%+.2f %%), per bucket switch %.5f -> %.5f", (unsigned long long)n_distinct,
             (unsigned long long)dh, (unsigned long long)db, 100.0 * ((double)db / (double)dh - 1.0), (double)dh / (double)ev_h, (double)db / (double)ev_b);
    printf("hash order -> searched order (seed %llu, %llu iterations of %d candidates)\n", (unsigned long long)seed, (unsigned long long)iters, batch);
    for (auto &l : line) printf("  %s\n", l);
    printf("  compiled-in order (tbk_tmer_rank, tbk_bucket_candidates) on the held-out bases: lanes %.4f, continuous %.4f, tie rate %.4f, extra copies %.4f\n",
           ch.lanes_d(), ch.cont_d(), ch.tie_d(), ch.extra_d());
    if (!out) return 0;
    FILE *f = fopen(out, "w");
    if (!f) { perror(out); return 1; }
    fprintf(f, "// tbk_tmer_order.h - generated by tools/tmer_order_search.cpp (--seed %llu --iters %llu --train %llu --test %llu --max-tie-rise-permille %llu); do not edit.\n",
            (unsigned long long)seed, (unsigned long long)iters, (unsigned long long)n_train, (unsigned long long)n_test, (unsigned long long)(max_tie_rise * 1000.0 + 0.5));
    fprintf(f, "// The order in which mod-sampling ranks the canonical 4-mers (t = 4: k = 21's entry layouts and short keys, tbk_mz_span3),\n");
    fprintf(f, "// searched for fewer bucket switches per window than the hash order tbk_mmer_hash gives them.  Scores, hash order -> this one:\n");
    for (auto &l : line) fprintf(f, "//   %s\n", l);
    fprintf(f, "// tbk_tmer4_ranks[x]: the rank of forward 4-mer code x (base i at bits 2i), equal for x and its reverse complement;\n");
    fprintf(f, "// the low 5 bits are zero (they carry a position tag in the probe kernels).\n");
    fprintf(f, "#pragma once\n#include <stdint.h>\n\nstatic constexpr uint32_t tbk_tmer4_ranks[256] = {\n");
    for (int x = 0; x < 256; x++) fprintf(f, "%s0x%04Xu,%s", x % 12 == 0 ? "    " : "", rank[x], x % 12 == 11 || x == 255 ? "\n" : " ");
    fprintf(f, "};\n");
    fclose(f);
    return 0;
}
