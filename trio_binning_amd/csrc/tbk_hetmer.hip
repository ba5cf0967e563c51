// tbk_hetmer.hip — the het-mer pairs of ONE count database (tbk_kmerdb_hetmers; include/tbk.h has the definitions): for every
// entry with a counter in range, its middle partners - the canonical k-mers that differ from it in the middle base alone -
// are looked up in the database itself.  An entry with exactly one partner in range forms a pair with it; the pair's two
// counters are the coverage of the two alleles of a heterozygous site.  Three lookups per candidate, through a directory over
// the top bits of the rank (tbk_query.hip's, built per call): a partner differs from the entry at bits k - 1 and k of its 2k,
// whether the variant kept its orientation or (mirrored flanks) flipped onto another middle base - up to 3 * 4^((k - 1) / 2)
// ranks away, which is the other end of a small database and some tens of entries in one of 1e8 21-mers; the bounds of the
// entry's tile bound nothing either way.
// Three kernels: the tally (strided over tiles, LDS tallies, one flush per block), and for the pairs themselves a flag kernel
// and a scatter around the shared compaction (tbk_compact.h).  No block waits for another; keys compare as unsigned 64-bit
// numbers; the databases are only read.  Host side: tbk_kmerdb_hetmers in tbk_count.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tbk.h"
#include "tbk_compact.h"
#include "tbk_lookup.h"

// What a lookup reads: the database behind its directory (n >= 1 wherever a kernel runs: a lane whose search is over reads
// entry 0), its k and the candidates' counter range.
struct HetDb {
    TbkDbView view;
    int k;
    uint32_t c_min, c_max;
};

// a partner database as the pairs ask it (het_classes: the question of db_held_in_range): not given = n 0 and NULL arrays, never dereferenced
struct HetPartner {
    const uint64_t *keys;
    const uint8_t *counts;
    uint64_t n;
    uint32_t c_min, c_max;
};

// the reverse complement of a rank, in rank form: the complement's pairs in reverse order; what ~ sets above the 2k bits
// lands below them and is shifted out (lex_rank reverses the pairs of a 64-bit word and drops 64 - 2k bits)
__device__ __forceinline__ uint64_t het_revcomp(uint64_t rank, int k) { return lex_rank(~rank, k); }

// The middle partners of candidate x (k odd, m = (k - 1) / 2: base m sits at bit 2m of the rank, the one position reverse
// complement maps to itself) that are candidates too: their number, 0..3, and - meaningful when that is 1 - the one's
// entry and counter.  The three variants x ^ (d << 2m) are made canonical and treated as a SET: one that is x itself (AAT ->
// ATT = its reverse complement) or equals an earlier one (AAT: ACT and AGT are one k-mer) is dropped before anything is
// searched.  The three are then searched side by side (db_search_group, tbk_lookup.h: no load under a branch); one that never
// began (`live` false: not a candidate; a dropped variant) reads entry 0 like one that is over.  Nothing crosses lanes here: a
// wave may call it with some lanes only (the scatter does).
__device__ __forceinline__ uint32_t het_partners_in_range(const HetDb &db, bool live, uint64_t x, uint32_t &partner, uint32_t &c_partner) {
    const int mid_bit = db.k - 1;  // 2m
    uint64_t want[3];
    uint32_t at[3], c[3];
    bool ok[3], hit[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const uint64_t v = x ^ ((uint64_t)(d + 1) << mid_bit);
        const uint64_t rc = het_revcomp(v, db.k);
        want[d] = v < rc ? v : rc;
        ok[d] = live && want[d] != x;
#pragma unroll
        for (int e = 0; e < d; e++) ok[d] = ok[d] && want[d] != want[e];  // (an earlier variant that was x itself is no partner either)
    }
    db_search_group<3>(db.view, db.k, want, ok, at, hit, c);  // (the directory's shift is <= 62: k is odd, so at most 31)
    uint32_t found = 0;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        if (hit[d] && c[d] >= db.c_min && c[d] <= db.c_max) {
            found++;
            partner = at[d];
            c_partner = c[d];
        }
    }
    return found;
}

// Entry i founds a pair when it is a candidate with exactly one partner in range and is the lower-ranked of the two: every
// pair is found once, from there (the partner then has exactly one partner too, i itself: classes are equivalence classes).
__device__ __forceinline__ bool het_founds_pair(const HetDb &db, uint64_t i, bool in_n, uint32_t &c, uint32_t &partner, uint32_t &c_partner,
                                                uint32_t &found, bool &candidate) {
    c = in_n ? db.view.counts[i] : 0u;
    candidate = in_n && c >= db.c_min && c <= db.c_max;
    const uint64_t x = db.view.keys[in_n ? i : 0];
    partner = 0;
    c_partner = 0;
    found = het_partners_in_range(db, candidate, x, partner, c_partner);
    return candidate && found == 1u && i < partner;
}

// the minor member of a pair has the lower counter, on a tie the lower rank: i < partner, so i is the minor one unless its
// counter is the higher
__device__ __forceinline__ bool het_first_is_minor(uint32_t c, uint32_t c_partner) { return c <= c_partner; }

// The origin classes of a pair's two members - bit 0 set when y holds the key with a counter in y's range, bit 1 the same for
// z - as four lower-bound searches side by side: the founder's key between its tile's bounds in y and in z, the partner's key
// over the whole of y and of z.  Pairs are a few per cent of the entries, so a wave comes here with a lane or two, and what it
// waits for is the chain of dependent loads: one after the other the four searches took 10 ms of a 13 ms call on 1e8 entries
// (profiles/r21); in step they cost what the longest of them costs.  A partner that is not given has n = 0 and
// equal bounds: no load at all.
__device__ __forceinline__ void het_classes(const HetPartner &y, const HetPartner &z, const uint64_t *bound, uint64_t key_i, uint64_t key_p,
                                            uint32_t &cls_i, uint32_t &cls_p) {
    const HetPartner *who[4] = {&y, &z, &y, &z};
    const uint64_t want[4] = {key_i, key_i, key_p, key_p};
    uint64_t lo[4] = {bound[0], bound[2], 0, 0}, hi[4] = {bound[1], bound[3], y.n, z.n};
    for (;;) {
        bool more = false;
#pragma unroll
        for (int s = 0; s < 4; s++) more = more || lo[s] < hi[s];
        if (!more) break;
        uint64_t v[4], mid[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            mid[s] = lo[s] + (hi[s] - lo[s]) / 2;  // (< hi <= n)
            v[s] = lo[s] < hi[s] ? who[s]->keys[mid[s]] : 0;
        }
#pragma unroll
        for (int s = 0; s < 4; s++) {
            if (lo[s] < hi[s]) {
                if (v[s] < want[s]) lo[s] = mid[s] + 1; else hi[s] = mid[s];
            }
        }
    }
    bool held[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {  // (lo is the lower bound: <= the upper end it started from, <= n)
        held[s] = lo[s] < who[s]->n && who[s]->keys[lo[s]] == want[s];
        if (held[s]) {
            const uint32_t c = who[s]->counts[lo[s]];
            held[s] = c >= who[s]->c_min && c <= who[s]->c_max;
        }
    }
    cls_i = (held[0] ? 1u : 0u) | (held[1] ? 2u : 0u);
    cls_p = (held[2] ? 1u : 0u) | (held[3] ? 2u : 0u);
}

// ---- the tally ----------------------------------------------------------------------------------------------------------------
// out: [0] candidates, [1..4] candidates by partners in range 0..3, [5] pairs, [6..21] origin[cls_minor * 4 + cls_major];
// spec: 256 x 256, cell c_minor * 256 + c_major.  Both zeroed by the caller.
// A block strides over tiles of 1024 entries (the comparisons' capped grid) and flushes once, with 64-bit atomics.  The
// candidates by number of partners are counted by ballot into registers - one LDS add per wave, value and kernel, not one per
// lane on four addresses, which a wave-instruction would serialise; pairs are a few per cent of the entries at most, so their
// cells take a plain LDS atomic each: the spectrum's low-counter corner in LDS, as tbk_kmerdb_joint_kernel keeps it and for its
// reason (a pair's counters are the two alleles' coverage, around half the library's), every cell outside it straight to a
// global atomic.  Only pairs ask y and z, four searches per pair, in step (het_classes).
constexpr uint64_t HETMER_GRID = 2048;                      // 256 CUs x the 8 blocks of 4 waves a CU holds
constexpr uint64_t HETMER_MAX_TILES_PER_BLOCK = 1ull << 21;  // x 1024 entries: half of what a 32-bit tally counts
#ifndef TBK_HETMER_CORNER  // (measurement only: other sides)
#define TBK_HETMER_CORNER 64
#endif
constexpr uint32_t HCORNER = TBK_HETMER_CORNER;
static_assert(HCORNER >= 2 && HCORNER <= 128 && (HCORNER & (HCORNER - 1)) == 0, "a power of two whose square of 32-bit words fits in LDS");
constexpr uint32_t HETMER_SUMS = 6 + 16;

__global__ void __launch_bounds__(256)
tbk_hetmer_tally_kernel(HetDb db, HetPartner y, HetPartner z, uint64_t tiles, unsigned long long *__restrict__ out,
                        unsigned long long *__restrict__ spec) {
    __shared__ uint32_t tally[HCORNER * HCORNER];
    __shared__ uint32_t sums[HETMER_SUMS];
    __shared__ uint64_t bound[4];  // y: first, last; z: first, last
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n = db.view.n;
    for (uint32_t i = threadIdx.x; i < HCORNER * HCORNER; i += 256) tally[i] = 0;
    if (threadIdx.x < HETMER_SUMS) sums[threadIdx.x] = 0;
    __syncthreads();
    uint32_t by_partners[4] = {0, 0, 0, 0}, n_pairs = 0;  // (the same in every lane of a wave)
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t first = tile * TBK_DBT_TILE;  // (< n)
        compact_tile_bounds(db.view.keys, n, first, y.keys, y.n, bound, 0);
        compact_tile_bounds(db.view.keys, n, first, z.keys, z.n, bound + 2, 64);
        __syncthreads();
        for (uint32_t r = 0; r < TBK_DBT_TILE / 256; r++) {
            const uint64_t i = first + (uint64_t)r * 256 + threadIdx.x;
            uint32_t c, partner, c_partner, found;
            bool candidate;
            const bool pair = het_founds_pair(db, i, i < n, c, partner, c_partner, found, candidate);
#pragma unroll
            for (uint32_t v = 0; v < 4; v++) by_partners[v] += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(candidate && found == v));
            n_pairs += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(pair));
            if (pair) {
                const bool first_minor = het_first_is_minor(c, c_partner);
                const uint32_t c_minor = first_minor ? c : c_partner, c_major = first_minor ? c_partner : c;
                if (c_minor < HCORNER && c_major < HCORNER)
                    atomicAdd(&tally[c_minor * HCORNER + c_major], 1u);
                else
                    atomicAdd(&spec[c_minor * 256 + c_major], 1ull);
                uint32_t cls_i, cls_p;
                het_classes(y, z, bound, db.view.keys[i], db.view.keys[partner], cls_i, cls_p);
                atomicAdd(&sums[6 + (first_minor ? cls_i * 4 + cls_p : cls_p * 4 + cls_i)], 1u);
            }
        }
        __syncthreads();  // the bounds are read before the next trip writes them
    }
    if (lane == 0) {
        uint32_t candidates = 0;
#pragma unroll
        for (uint32_t v = 0; v < 4; v++) {
            if (by_partners[v]) atomicAdd(&sums[1 + v], by_partners[v]);
            candidates += by_partners[v];
        }
        if (candidates) atomicAdd(&sums[0], candidates);
        if (n_pairs) atomicAdd(&sums[5], n_pairs);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < HCORNER * HCORNER; i += 256) {
        const uint32_t v = tally[i];
        if (v) atomicAdd(&spec[(i / HCORNER) * 256 + i % HCORNER], (unsigned long long)v);
    }
    if (threadIdx.x < HETMER_SUMS && sums[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)sums[threadIdx.x]);
}

// ---- the pairs themselves: flag, (scan,) scatter ---------------------------------------------------------------------------------
// flag: the entries that found a pair, one bit each, one count per tile; one block per tile of 1024 entries
__global__ void __launch_bounds__(256)
tbk_hetmer_flag_kernel(HetDb db, uint64_t *__restrict__ flags, unsigned long long *__restrict__ tile_counts) {
    const uint64_t n = db.view.n;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    __shared__ uint32_t tile_sum;
    const uint64_t tile = blockIdx.x;
    if (threadIdx.x == 0) tile_sum = 0;
    __syncthreads();
    // compact_flag_tile's loop with the predicate called by EVERY lane: the lookup is a wave's common loop, and a lane past n
    // or outside the range goes through it without a load of its own
    uint32_t mine = 0;
    for (uint32_t r = 0; r < TBK_DBT_TILE / 256; r++) {
        const uint32_t word = r * 4 + wave;
        const uint64_t i = tile * TBK_DBT_TILE + (uint64_t)word * 64 + lane;
        uint32_t c, partner, c_partner, found;
        bool candidate;
        const uint64_t mask = __builtin_amdgcn_ballot_w64(het_founds_pair(db, i, i < n, c, partner, c_partner, found, candidate));
        if (lane == 0) flags[tile * TBK_DBT_WORDS + word] = mask;
        mine += (uint32_t)__popcll(mask);
    }
    if (lane == 0 && mine) atomicAdd(&tile_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0) tile_counts[tile] = tile_sum;
}

// scatter: one record per flagged entry, in the entries' order - ascending by the rank of the pair's lower-ranked member.
// The partner is found AGAIN rather than kept from the flag pass (a word per entry would be 32 times the bit the call holds),
// and the flagged entries are dealt to consecutive threads (compact_scatter_tile_dense): pairs are sparse, and a lane per
// entry of the tile would have a wave pay three searches for its 64 entries when one of them is flagged.  The threads of a
// wave that have no entry left still walk the lookup's common loop, without loads of their own.
static_assert(sizeof(tbk_hetmer_pair) == 24, "two ranks, four bytes, four bytes of padding");
__global__ void __launch_bounds__(256)
tbk_hetmer_scatter_kernel(HetDb db, HetPartner y, HetPartner z, const uint64_t *__restrict__ flags, const unsigned long long *__restrict__ tile_offsets,
                          tbk_hetmer_pair *__restrict__ out, uint64_t n_out) {
    __shared__ uint64_t bound[4];  // y: first, last; z: first, last
    const uint64_t n = db.view.n;
    const uint64_t first = (uint64_t)blockIdx.x * TBK_DBT_TILE;  // (< n)
    compact_tile_bounds(db.view.keys, n, first, y.keys, y.n, bound, 0);
    compact_tile_bounds(db.view.keys, n, first, z.keys, z.n, bound + 2, 64);
    compact_scatter_tile_dense(n, flags, tile_offsets, [=](uint64_t i, uint64_t at) {  // (its barriers publish the bounds)
        if (at >= n_out) return;
        uint32_t c, partner, c_partner, found;
        bool candidate;
        if (!het_founds_pair(db, i, true, c, partner, c_partner, found, candidate)) return;  // (flags that are not this database's: nothing written)
        const uint64_t x = db.view.keys[i], px = db.view.keys[partner];
        uint32_t cls_i, cls_p;
        het_classes(y, z, bound, x, px, cls_i, cls_p);
        const bool first_minor = het_first_is_minor(c, c_partner);
        tbk_hetmer_pair rec;
        rec.minor = first_minor ? x : px;
        rec.major = first_minor ? px : x;
        rec.c_minor = (uint8_t)(first_minor ? c : c_partner);
        rec.c_major = (uint8_t)(first_minor ? c_partner : c);
        rec.cls_minor = (uint8_t)(first_minor ? cls_i : cls_p);
        rec.cls_major = (uint8_t)(first_minor ? cls_p : cls_i);
        rec.reserved[0] = rec.reserved[1] = rec.reserved[2] = rec.reserved[3] = 0;
        out[at] = rec;
    });
}

// =======================================================================================
// launchers (called from tbk_count.cpp)
// =======================================================================================
static bool hetmer_args(uint64_t n, int k, int prefix_bits, const TbkHetmerPartner *y, const TbkHetmerPartner *z) {
    return n >= 1 && n <= 0xFFFFFFFFull && k >= 1 && k <= 31 && (k & 1) && prefix_bits >= 0 && prefix_bits <= 2 * k && prefix_bits <= 30 && y && z;
}

static HetPartner hetmer_partner(const TbkHetmerPartner *p) { return HetPartner{p->keys, p->counts, p->n, p->c_min, p->c_max}; }

extern "C" hipError_t tbk_launch_hetmer_tally(const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, int k, const uint32_t *d_dir, int prefix_bits,
                                              uint32_t c_min, uint32_t c_max, const TbkHetmerPartner *y, const TbkHetmerPartner *z,
                                              unsigned long long *d_sums, unsigned long long *d_spec, hipStream_t stream) {
    if (!n) return hipSuccess;
    if (!hetmer_args(n, k, prefix_bits, y, z)) return hipErrorInvalidValue;
    const uint64_t tiles = tbk_kmerdb_table_tiles(n);
    const unsigned grid = tbk_count_entry_grid_(tiles < HETMER_GRID ? tiles : HETMER_GRID);
    if ((tiles + grid - 1) / grid > HETMER_MAX_TILES_PER_BLOCK) return hipErrorInvalidValue;
    const HetDb db{{d_keys, d_counts, d_dir, (uint32_t)n, prefix_bits}, k, c_min, c_max};
    hipLaunchKernelGGL(tbk_hetmer_tally_kernel, dim3(grid), dim3(256), 0, stream, db, hetmer_partner(y), hetmer_partner(z), tiles, d_sums, d_spec);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_hetmer_flag(const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, int k, const uint32_t *d_dir, int prefix_bits,
                                             uint32_t c_min, uint32_t c_max, uint64_t *d_flags, unsigned long long *d_tile_counts, hipStream_t stream) {
    const TbkHetmerPartner none = {nullptr, nullptr, 0, 1, 255};
    if (!n) return hipSuccess;
    if (!hetmer_args(n, k, prefix_bits, &none, &none)) return hipErrorInvalidValue;
    const HetDb db{{d_keys, d_counts, d_dir, (uint32_t)n, prefix_bits}, k, c_min, c_max};
    return compact_launch_tiles(n, stream, tbk_hetmer_flag_kernel, db, d_flags, d_tile_counts);
}

extern "C" hipError_t tbk_launch_hetmer_scatter(const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, int k, const uint32_t *d_dir, int prefix_bits,
                                                uint32_t c_min, uint32_t c_max, const TbkHetmerPartner *y, const TbkHetmerPartner *z,
                                                const uint64_t *d_flags, const unsigned long long *d_tile_offsets, tbk_hetmer_pair *d_out, uint64_t n_out,
                                                hipStream_t stream) {
    if (!n) return hipSuccess;
    if (!hetmer_args(n, k, prefix_bits, y, z)) return hipErrorInvalidValue;
    const HetDb db{{d_keys, d_counts, d_dir, (uint32_t)n, prefix_bits}, k, c_min, c_max};
    return compact_launch_tiles(n, stream, tbk_hetmer_scatter_kernel, db, hetmer_partner(y), hetmer_partner(z), d_flags, d_tile_offsets, d_out, n_out);
}
