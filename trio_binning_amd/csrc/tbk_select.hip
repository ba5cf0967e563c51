// tbk_select.hip — a selection from count databases that stays a database (tbk_kmerdb_select; include/tbk.h has the rule): the
// entries of `base` with a counter in a range that up to two partners let pass, compacted in base's order with a counter made
// of the base's and the REQUIRE partners'.  The shape of tbk_kmerdb_inherited_flag_kernel and tbk_kmerdb_origin_kernel - a
// tile's bounds in each partner, then a bounded bisection per entry (tbk_compact.h) - with one block of 256 threads per tile
// of 1024 entries of base: no stride, no look-back, no block waiting for another.  Keys compare as unsigned 64-bit numbers
// (k = 32 uses the top bit); the inputs are only read.  Host side: tbk_kmerdb_select in tbk_count.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tbk.h"
#include "tbk_common.h"
#include "tbk_compact.h"
#include "tbk_device.h"

// Does the partner let `key` pass?  "It holds the key with a counter in its range" must be true for a REQUIRE partner and
// false for an EXCLUDE one.  A partner that is not there (n = 0, require = 0) loads nothing and lets everything pass.
__device__ __forceinline__ bool select_passes(const TbkSelectPartner &p, uint64_t lo, uint64_t hi, uint64_t key) {
    return db_held_in_range(p.keys, p.counts, lo, hi, p.n, key, p.c_min, p.c_max) == (p.require != 0u);
}

// ---- flag: one bit per entry of base, one count per tile -------------------------------------------------------------------
// Two threads of wave 0 and two of wave 1 find the tile's bounds in p0 and in p1 side by side; behind the barrier of
// compact_flag_tile every entry tests its own counter first, then the G-or-C bases of its own key (tbk_rank_gc against
// [g_min, g_max]; 0 and 32 never bind) - an entry outside either range loads nothing of a partner - then asks p0, and p1 only for what p0 left (the host puts EXCLUDE partners first: the cheaper rejection).  Equal bounds
// are no load at all.  32 bytes of LDS for the bounds and the tile's sum: occupancy is bounded by registers alone.
__global__ void __launch_bounds__(256)
tbk_kmerdb_select_flag_kernel(const uint64_t *__restrict__ base_keys, const uint8_t *__restrict__ base_counts, uint64_t n, uint32_t c_min,
                              uint32_t c_max, uint32_t g_min, uint32_t g_max, TbkSelectPartner p0, TbkSelectPartner p1,
                              uint64_t *__restrict__ flags, unsigned long long *__restrict__ tile_counts) {
    __shared__ uint64_t bound[4];  // p0: first, last; p1: first, last
    const uint64_t first = (uint64_t)blockIdx.x * TBK_DBT_TILE;  // (< n: one block per tile of base)
    compact_tile_bounds(base_keys, n, first, p0.keys, p0.n, bound, 0);
    compact_tile_bounds(base_keys, n, first, p1.keys, p1.n, bound + 2, 64);
    compact_flag_tile(n, flags, tile_counts, [=](uint64_t i) {
        const uint32_t c = base_counts[i];
        if (c < c_min || c > c_max) return false;
        const uint64_t key = base_keys[i];
        const uint32_t g = tbk_rank_gc(key);
        if (g < g_min || g > g_max) return false;
        return select_passes(p0, bound[0], bound[1], key) && select_passes(p1, bound[2], bound[3], key);
    });
}

// ---- scatter with a made counter: MIN and SUM -------------------------------------------------------------------------------
// The flagged entries go to their places as in every compaction; the counter is the base's joined with the counter each
// REQUIRE partner holds for the key, which the flag pass found but did not keep (a byte per entry would be eight times the
// bit the call may hold beside its output): the tile's bounds in r0 and r1 again, and one more bounded bisection per KEPT
// entry and partner.  A flagged entry is held by every REQUIRE partner; the test stands all the same, so that a partner that
// is not there (n = 0) or flags that do not belong to these partners read nothing out of bounds and add nothing.
// The kept entries are dealt to consecutive threads (compact_scatter_tile_dense): a bisection costs a wave what its slowest
// lane costs, and with compact_scatter_tile's placement - a lane per entry of the tile - a selection that keeps 30 % of the
// entries paid for all of them (profiles/r20: this kernel 1.88 ms that way on 1e8 entries).
template <int RULE>
__device__ __forceinline__ uint32_t select_join(uint32_t c, const TbkSelectPartner &p, uint64_t lo, uint64_t hi, uint64_t key) {
    const uint64_t at = db_lower_bound(p.keys, lo, hi, key);  // (at <= hi <= n)
    if (!(at < p.n && p.keys[at] == key)) return c;
    const uint32_t other = p.counts[at];
    if (RULE == TBK_SELECT_COUNTER_MIN) return other < c ? other : c;
    return c + other;  // (32 bits: at most 3 x 255)
}

template <int RULE>
__global__ void __launch_bounds__(256)
tbk_kmerdb_select_scatter_kernel(const uint64_t *__restrict__ base_keys, const uint8_t *__restrict__ base_counts, uint64_t n, TbkSelectPartner r0,
                                 TbkSelectPartner r1, const uint64_t *__restrict__ flags, const unsigned long long *__restrict__ tile_offsets,
                                 uint64_t *__restrict__ out_keys, uint8_t *__restrict__ out_counts, uint64_t n_out) {
    static_assert(RULE == TBK_SELECT_COUNTER_MIN || RULE == TBK_SELECT_COUNTER_SUM, "the rule that keeps the base's counter is tbk_kmerdb_scatter_pairs");
    __shared__ uint64_t bound[4];  // r0: first, last; r1: first, last
    const uint64_t first = (uint64_t)blockIdx.x * TBK_DBT_TILE;  // (< n)
    compact_tile_bounds(base_keys, n, first, r0.keys, r0.n, bound, 0);
    compact_tile_bounds(base_keys, n, first, r1.keys, r1.n, bound + 2, 64);
#ifdef TBK_SELECT_SPARSE_SCATTER  // (measurement only, VARIANT_SRC=tbk_select tools/build_variant.sh: a lane per entry of the tile)
    compact_scatter_tile(n, flags, tile_offsets, [=](uint64_t i, uint64_t at) {
#else
    compact_scatter_tile_dense(n, flags, tile_offsets, [=](uint64_t i, uint64_t at) {  // (its barriers publish the bounds)
#endif
        if (at >= n_out) return;
        const uint64_t key = base_keys[i];
        uint32_t c = base_counts[i];
        c = select_join<RULE>(c, r0, bound[0], bound[1], key);
        c = select_join<RULE>(c, r1, bound[2], bound[3], key);
        out_keys[at] = key;
        out_counts[at] = (uint8_t)(c < 255u ? c : 255u);
    });
}

// =======================================================================================
// launchers (called from tbk_count.cpp)
// =======================================================================================
extern "C" hipError_t tbk_launch_kmerdb_select_flag(const uint64_t *base_keys, const uint8_t *base_counts, uint64_t n, uint32_t c_min, uint32_t c_max,
                                                    uint32_t g_min, uint32_t g_max, const TbkSelectPartner *p0, const TbkSelectPartner *p1,
                                                    uint64_t *d_flags, unsigned long long *d_tile_counts, hipStream_t stream) {
    return compact_launch_tiles(n, stream, tbk_kmerdb_select_flag_kernel, base_keys, base_counts, n, c_min, c_max, g_min, g_max, *p0, *p1, d_flags,
                                d_tile_counts);
}

extern "C" hipError_t tbk_launch_kmerdb_select_scatter(int rule, const uint64_t *base_keys, const uint8_t *base_counts, uint64_t n,
                                                       const TbkSelectPartner *r0, const TbkSelectPartner *r1, const uint64_t *d_flags,
                                                       const unsigned long long *d_tile_offsets, uint64_t *d_out_keys, uint8_t *d_out_counts,
                                                       uint64_t n_out, hipStream_t stream) {
    if (rule == TBK_SELECT_COUNTER_MIN)
        return compact_launch_tiles(n, stream, tbk_kmerdb_select_scatter_kernel<TBK_SELECT_COUNTER_MIN>, base_keys, base_counts, n, *r0, *r1, d_flags,
                                    d_tile_offsets, d_out_keys, d_out_counts, n_out);
    if (rule == TBK_SELECT_COUNTER_SUM)
        return compact_launch_tiles(n, stream, tbk_kmerdb_select_scatter_kernel<TBK_SELECT_COUNTER_SUM>, base_keys, base_counts, n, *r0, *r1, d_flags,
                                    d_tile_offsets, d_out_keys, d_out_counts, n_out);
    return hipErrorInvalidValue;
}
