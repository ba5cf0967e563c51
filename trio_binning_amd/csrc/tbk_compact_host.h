// tbk_compact_host.h — the stable tile compaction of the count databases as the host sees it: "keep the flagged entries of a
// sorted database, in their order, at their exact number".  Three launches, no block ever waits for another: flag (one bit
// per entry, one count per tile), an exclusive scan of the tile counts (rocPRIM), scatter.  The tile, the buffers the three
// steps share (Compaction) and the one declaration of every launcher; included by the .hip files that define the launchers
// (a signature that drifts is a compile error) and by the .cpp files that call them.  The kernels' side: tbk_compact.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Round r of a block's wave w covers the 64 entries from tile * TILE + (r * 4 + w) * 64 on, and their ballot is flag word
// tile * WORDS + r * 4 + w - so bit j of flag word i belongs to entry 64 i + j.
constexpr uint32_t TBK_DBT_TILE = 1024;                // entries per tile
constexpr uint32_t TBK_DBT_WORDS = TBK_DBT_TILE / 64;  // flag words per tile
static_assert(TBK_DBT_TILE == 4 * 256 && TBK_DBT_TILE % 64 == 0, "a tile is 4 rounds of a 256-thread block and whole 64-bit flag words");

constexpr uint64_t tbk_kmerdb_table_tiles(uint64_t n) { return (n + TBK_DBT_TILE - 1) / TBK_DBT_TILE; }

extern "C" {
// d_tally: 3 + 256 words, d_hist: 256 words; both zeroed by the caller
hipError_t tbk_launch_kmerdb_check(const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, int k, uint32_t floor, unsigned long long *d_tally,
                                   hipStream_t stream);
hipError_t tbk_launch_kmerdb_tally(const uint8_t *d_counts, uint64_t n, unsigned long long *d_hist, hipStream_t stream);

// The flag kernels: d_flags holds TBK_DBT_WORDS words per tile of the first database, d_tile_counts one count per tile.  One
// block per tile, no grid stride.  The arrays of a partner with no entry may be NULL.
hipError_t tbk_launch_kmerdb_flag(const uint64_t *a_keys, const uint8_t *a_counts, uint64_t n_a, const uint64_t *b_keys, uint64_t n_b, uint32_t ci,
                                  uint32_t cx, uint64_t *d_flags, unsigned long long *d_tile_counts, hipStream_t stream);
hipError_t tbk_launch_kmerdb_inherited_flag(const uint64_t *a_keys, const uint8_t *a_counts, uint64_t n_a, const uint64_t *b_keys, uint64_t n_b,
                                            const uint64_t *h_keys, const uint8_t *h_counts, uint64_t n_h, uint32_t ci, uint32_t cx, uint32_t h_ci,
                                            uint32_t h_cx, uint64_t *d_flags, unsigned long long *d_tile_counts, hipStream_t stream);
hipError_t tbk_launch_kmerdb_union_flag(const uint64_t *a_keys, uint64_t n_a, const uint64_t *b_keys, uint64_t n_b, uint64_t *d_flags,
                                        unsigned long long *d_tile_counts, hipStream_t stream);
hipError_t tbk_launch_dump_heads(const uint64_t *d_keys, uint64_t n, uint64_t *d_flags, unsigned long long *d_tile_counts, hipStream_t stream);
hipError_t tbk_launch_dump_select(const uint8_t *d_counts, uint64_t n, uint32_t lo, uint32_t hi, uint64_t *d_flags, unsigned long long *d_tile_counts,
                                  hipStream_t stream);

// d_out[i] = d_in[0] + ... + d_in[i - 1], n elements; the caller passes one element more than it has tiles, so the last is
// the total.  Returns with the stream idle.
hipError_t tbk_launch_kmerdb_scan(const unsigned long long *d_in, unsigned long long *d_out, uint64_t n, hipStream_t stream);

// The scatters: the flagged entries to d_tile_offsets[their tile] + the flagged entries before them in the tile, n_out in
// all - as packed keys, as ranks, as ranks with their counters, as the heads of runs with the runs' saturated sums.
hipError_t tbk_launch_kmerdb_scatter(const uint64_t *a_keys, uint64_t n_a, const uint64_t *d_flags, const unsigned long long *d_tile_offsets, int k,
                                     uint64_t *d_out, uint64_t n_out, hipStream_t stream);
hipError_t tbk_launch_kmerdb_scatter_ranks(const uint64_t *a_keys, uint64_t n_a, const uint64_t *d_flags, const unsigned long long *d_tile_offsets,
                                           uint64_t *d_out, uint64_t n_out, hipStream_t stream);
hipError_t tbk_launch_kmerdb_scatter_pairs(const uint64_t *a_keys, const uint8_t *a_counts, uint64_t n_a, const uint64_t *d_flags,
                                           const unsigned long long *d_tile_offsets, uint64_t *d_out_keys, uint8_t *d_out_counts, uint64_t n_out,
                                           hipStream_t stream);
hipError_t tbk_launch_dump_fold(const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, const uint64_t *d_flags,
                                const unsigned long long *d_tile_offsets, uint64_t *d_out_keys, uint8_t *d_out_counts, uint64_t n_out,
                                hipStream_t stream);
// d_flags and d_tile_offsets are A's (the last offset the number of duplicates); the output holds n_out = n_a + n_b - duplicates
hipError_t tbk_launch_kmerdb_union_scatter(const uint64_t *a_keys, const uint8_t *a_counts, uint64_t n_a, const uint64_t *b_keys,
                                           const uint8_t *b_counts, uint64_t n_b, const uint64_t *d_flags, const unsigned long long *d_tile_offsets,
                                           uint64_t *d_out_keys, uint8_t *d_out_counts, uint64_t n_out, hipStream_t stream);

// The selection into a database (tbk_select.hip, tbk_kmerdb_select): a partner is the arrays of a database, the literal
// counter range it is asked with and what the answer must be - `require` 1: it holds the key in that range, 0: it does not.
// A partner that is not there has n = 0, NULL arrays and require = 0: it never rejects and is never dereferenced.
struct TbkSelectPartner {
    const uint64_t *keys;
    const uint8_t *counts;
    uint64_t n;
    uint32_t c_min, c_max;
    uint32_t require;
};
// flag: the entries of base with a counter in [c_min, c_max] and tbk_rank_gc(key) in [g_min, g_max] that both partners let
// pass, p0 asked before p1
hipError_t tbk_launch_kmerdb_select_flag(const uint64_t *base_keys, const uint8_t *base_counts, uint64_t n, uint32_t c_min, uint32_t c_max,
                                         uint32_t g_min, uint32_t g_max, const TbkSelectPartner *p0, const TbkSelectPartner *p1, uint64_t *d_flags,
                                         unsigned long long *d_tile_counts, hipStream_t stream);
// scatter with a counter made of the base's and the partners' (rule: TBK_SELECT_COUNTER_MIN or _SUM; both partners are REQUIRE
// ones, or not there); the rule that keeps the base's counter is tbk_launch_kmerdb_scatter_pairs
hipError_t tbk_launch_kmerdb_select_scatter(int rule, const uint64_t *base_keys, const uint8_t *base_counts, uint64_t n, const TbkSelectPartner *r0,
                                            const TbkSelectPartner *r1, const uint64_t *d_flags, const unsigned long long *d_tile_offsets,
                                            uint64_t *d_out_keys, uint8_t *d_out_counts, uint64_t n_out, hipStream_t stream);

// The comparisons (tbk_compare.hip) compact nothing: they stride over the tiles of the database they walk and tally.  d_spec
// holds 256 * 256 words (joint: cell cx * 256 + cy) or 4 * 256 (origin: cell class * 256 + c), zeroed by the caller; `keep`
// has bit `class` set for every class that is tallied (15: all four).
hipError_t tbk_launch_kmerdb_joint_spectrum(const uint64_t *x_keys, const uint8_t *x_counts, uint64_t n_x, const uint64_t *y_keys,
                                            const uint8_t *y_counts, uint64_t n_y, unsigned long long *d_spec, hipStream_t stream);
hipError_t tbk_launch_kmerdb_origin_spectrum(const uint64_t *base_keys, const uint8_t *base_counts, uint64_t n, const uint64_t *y_keys,
                                             const uint8_t *y_counts, uint64_t n_y, uint32_t y_min, uint32_t y_max, const uint64_t *z_keys,
                                             const uint8_t *z_counts, uint64_t n_z, uint32_t z_min, uint32_t z_max, uint32_t keep,
                                             unsigned long long *d_spec, hipStream_t stream);
// One database by the G-or-C bases of its keys and by counter: d_spec holds 33 * 256 words (cell gc * 256 + c), zeroed by the
// caller.  layout 0 is the build's choice of what a block keeps in LDS; 1 (the whole matrix) and 2 (the counters below 64)
// name the two for the measurement.
hipError_t tbk_launch_kmerdb_gc_spectrum(const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, int k, int layout, unsigned long long *d_spec,
                                         hipStream_t stream);
// `blocks` under the entry cap of tbk_count_set_grid_caps_ (tbk_count_kernels.hip), for strided launches in other files
unsigned tbk_count_entry_grid_(uint64_t blocks);

// The directory of a sorted database (tbk_query.hip): d_dir takes 2^prefix_bits + 1 32-bit offsets, d_dir[p] the first entry whose
// rank has the top prefix_bits bits >= p.  The query session keeps one; the het-mer call builds one per call.
hipError_t tbk_launch_query_directory(const uint64_t *d_keys, uint64_t n, int k, int prefix_bits, uint32_t *d_dir, hipStream_t stream);

// The het-mer pairs of one database (tbk_hetmer.hip, tbk_kmerdb_hetmers): the database with its directory and the candidates'
// literal counter range; y and z as the pairs ask them - a partner that is not given has n = 0 and NULL arrays and is never
// dereferenced.  Nothing is launched for n = 0.
struct TbkHetmerPartner {
    const uint64_t *keys;
    const uint8_t *counts;
    uint64_t n;
    uint32_t c_min, c_max;
};
struct tbk_hetmer_pair;  // (include/tbk.h)
// d_sums: 22 words - candidates, candidates with 0, 1, 2, 3 partners in range, pairs, origin[16]; d_spec: 256 * 256 words, cell
// c_minor * 256 + c_major; both zeroed by the caller.  Strides over tiles under the entry cap of tbk_count_set_grid_caps_.
hipError_t tbk_launch_hetmer_tally(const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, int k, const uint32_t *d_dir, int prefix_bits,
                                   uint32_t c_min, uint32_t c_max, const TbkHetmerPartner *y, const TbkHetmerPartner *z, unsigned long long *d_sums,
                                   unsigned long long *d_spec, hipStream_t stream);
// flag: the lower-ranked member of every pair; scatter: one record per flagged entry, n_out in all, in the entries' order
hipError_t tbk_launch_hetmer_flag(const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, int k, const uint32_t *d_dir, int prefix_bits,
                                  uint32_t c_min, uint32_t c_max, uint64_t *d_flags, unsigned long long *d_tile_counts, hipStream_t stream);
hipError_t tbk_launch_hetmer_scatter(const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, int k, const uint32_t *d_dir, int prefix_bits,
                                     uint32_t c_min, uint32_t c_max, const TbkHetmerPartner *y, const TbkHetmerPartner *z, const uint64_t *d_flags,
                                     const unsigned long long *d_tile_offsets, tbk_hetmer_pair *d_out, uint64_t n_out, hipStream_t stream);
}

// What a compaction over n entries holds on the device between its flag kernel and its scatter: n / 8 + n / 64 bytes.
struct Compaction {
    uint64_t *d_flags = nullptr;
    unsigned long long *d_tiles = nullptr;  // tiles + 1 counts (the last one 0), then their tiles + 1 offsets (the last one the total)
    uint64_t tiles = 0;
    hipStream_t stream = nullptr;

    Compaction() = default;
    Compaction(const Compaction &) = delete;
    Compaction &operator=(const Compaction &) = delete;
    ~Compaction() { release(); }

    static size_t flag_bytes(uint64_t n) { return (size_t)(tbk_kmerdb_table_tiles(n) * TBK_DBT_WORDS * sizeof(uint64_t)); }
    static size_t tile_bytes(uint64_t n) { return (size_t)(2 * (tbk_kmerdb_table_tiles(n) + 1) * sizeof(unsigned long long)); }
    // device bytes reserve(n) takes (for a caller that accounts for them)
    static size_t bytes(uint64_t n) { return flag_bytes(n) + tile_bytes(n); }
    // n == 0 is no tile: a flag buffer all the same, and the one count the scan then takes
    hipError_t reserve(uint64_t n, hipStream_t s) {
        tiles = tbk_kmerdb_table_tiles(n);
        stream = s;
        hipError_t e = hipMalloc((void **)&d_flags, flag_bytes(n) ? flag_bytes(n) : 16);
        if (e == hipSuccess) e = hipMalloc((void **)&d_tiles, tile_bytes(n));
        if (e == hipSuccess) e = hipMemsetAsync(d_tiles + tiles, 0, sizeof(unsigned long long), stream);
        return e;
    }
    unsigned long long *counts() { return d_tiles; }
    const unsigned long long *offsets() const { return d_tiles + tiles + 1; }
    // after the flag kernel: scans the counts, brings the last offset home and returns with the stream idle
    hipError_t total(unsigned long long *out) {
        hipError_t e = tbk_launch_kmerdb_scan(d_tiles, d_tiles + tiles + 1, tiles + 1, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(out, d_tiles + 2 * tiles + 1, sizeof *out, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        return e;
    }
    void release() {
        if (d_flags) (void)hipFree(d_flags);
        if (d_tiles) (void)hipFree(d_tiles);
        d_flags = nullptr;
        d_tiles = nullptr;
    }
};
