// tbk_compare.hip — two or three count databases held against each other (tbk_kmerdb_joint_spectrum,
// tbk_kmerdb_origin_spectrum; include/tbk.h): the joins of tbk_count_kernels.hip - a tile's bounds in the partner, then a
// bounded bisection per entry (tbk_compact.h) - that TALLY what they find instead of compacting it - and the tally of ONE
// database by the GC content of its keys (tbk_kmerdb_gc_spectrum), which joins nothing.  Host side: tbk_count.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbk_common.h"
#include "tbk_compact.h"
#include "tbk_device.h"

// A block of the compaction kernels owns one tile and leaves a count per tile; a block here would leave a histogram per tile,
// and flushing 1024 or more cells costs as much as reading the tile's 1024 entries.  So these kernels STRIDE over tiles (a
// capped grid, tbk_count_entry_grid_), tally in LDS across all their tiles and flush once at the end, with one 64-bit
// atomicAdd per non-zero cell.  An LDS cell is 32 bits: a block may tally at most 2^32 - 1 entries, which the launchers
// check (COMPARE_MAX_TILES_PER_BLOCK).  No block waits for another; keys compare as unsigned 64-bit numbers (k = 32 uses the
// top bit); the databases are only read.
constexpr uint64_t COMPARE_GRID = 2048;                           // 256 CUs x the 8 blocks of 4 waves a CU holds
constexpr uint64_t COMPARE_MAX_TILES_PER_BLOCK = 1ull << 21;      // x 1024 entries: half of what an LDS cell counts

// ---- tbk_kmerdb_origin_spectrum: the entries of `base` by counter and by which of two partners hold them -------------------
// spec[cls * 256 + c] += entries of base with counter c and class cls; bit 0 of cls: y holds the key with a counter in
// [y_min, y_max], bit 1: the same for z.  Two waves find the tile's two pairs of bounds side by side, as the inherited flag
// kernel does; BOTH partners are asked for every entry (the class needs both answers).  `keep`: bit cls set = class cls is
// tallied and flushed - 15 for the call itself; the second launch of the joint spectrum keeps class 0 alone, which then
// lands in spec[c]: the matrix's row 0.
// 4 x 256 32-bit words of LDS (4 KiB) and the bounds: occupancy is bounded by registers and the 32 waves of a CU.  An LDS
// atomic on a real spectrum meets few equal addresses within a wave (a Poisson-like spectrum around 30 spreads a wave's 64
// counters over some 20 cells); a database of one counter serialises them, 64 to a wave-instruction, and is still correct.
__global__ void __launch_bounds__(256)
tbk_kmerdb_origin_kernel(const uint64_t *__restrict__ base_keys, const uint8_t *__restrict__ base_counts, uint64_t n,
                         const uint64_t *__restrict__ y_keys, const uint8_t *__restrict__ y_counts, uint64_t n_y, uint32_t y_min, uint32_t y_max,
                         const uint64_t *__restrict__ z_keys, const uint8_t *__restrict__ z_counts, uint64_t n_z, uint32_t z_min, uint32_t z_max,
                         uint64_t tiles, uint32_t keep, unsigned long long *__restrict__ spec) {
    __shared__ uint32_t tally[4 * 256];
    __shared__ uint64_t bound[4];  // y: first, last; z: first, last
    for (uint32_t i = threadIdx.x; i < 4 * 256; i += 256) tally[i] = 0;
    __syncthreads();
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t first = tile * TBK_DBT_TILE;  // (< n)
        compact_tile_bounds(base_keys, n, first, y_keys, n_y, bound, 0);
        compact_tile_bounds(base_keys, n, first, z_keys, n_z, bound + 2, 64);
        __syncthreads();
        const uint64_t y_lo = bound[0], y_hi = bound[1], z_lo = bound[2], z_hi = bound[3];
        for (uint32_t r = 0; r < TBK_DBT_TILE / 256; r++) {
            const uint64_t i = first + (uint64_t)r * 256 + threadIdx.x;
            if (i >= n) continue;
            const uint64_t key = base_keys[i];
            const uint32_t cls = (db_held_in_range(y_keys, y_counts, y_lo, y_hi, n_y, key, y_min, y_max) ? 1u : 0u) |
                                 (db_held_in_range(z_keys, z_counts, z_lo, z_hi, n_z, key, z_min, z_max) ? 2u : 0u);
            if ((keep >> cls) & 1u) atomicAdd(&tally[cls * 256 + base_counts[i]], 1u);
        }
        __syncthreads();  // the bounds are read before the next trip writes them; after the last trip the tally is whole
    }
    for (uint32_t i = threadIdx.x; i < 4 * 256; i += 256) {
        const uint32_t v = tally[i];
        if (v) atomicAdd(&spec[i], (unsigned long long)v);
    }
}

// ---- tbk_kmerdb_joint_spectrum, the launch over x: every entry of x to the cell (cx, cy), cy = 0 where y lacks the key -----
// The matrix has 65 536 cells, 256 KiB as 32-bit words: more than a CU's LDS.  A block keeps the low-counter corner
// [0, CORNER) x [0, CORNER) in LDS - a sequenced library's spectrum lives around its coverage, and what lies far above it is
// repeats, a small share of the distinct k-mers - and sends every cell outside it straight to a 64-bit global atomicAdd.
// CORNER is a power of two up to 128 (64 KiB of LDS).  It is 64, from measurement (profiles/r19: 2e7 entries a
// side, a spectrum around 30x with 2 % of the counters spread over 64..255): this launch takes 0.37 ms with a corner of 64,
// 0.95 ms with 128 - 64 KiB of LDS leave a CU two blocks instead of eight, which costs more than the repeats' global atomics
// do - and 8 to 15 ms with 32, which leaves the upper half of such a spectrum to global atomics on a few dozen addresses.
// 16 KiB cost no occupancy: nine blocks would fit a CU's LDS, its 32 waves hold eight.
#ifndef TBK_JOINT_CORNER  // (measurement only, tools/build_variant.sh with VARIANT_SRC=tbk_compare: the other sides tried)
#define TBK_JOINT_CORNER 64
#endif
constexpr uint32_t CORNER = TBK_JOINT_CORNER;
static_assert(CORNER >= 2 && CORNER <= 128 && (CORNER & (CORNER - 1)) == 0, "a power of two whose square of 32-bit words fits in LDS");

__global__ void __launch_bounds__(256)
tbk_kmerdb_joint_kernel(const uint64_t *__restrict__ x_keys, const uint8_t *__restrict__ x_counts, uint64_t n_x,
                        const uint64_t *__restrict__ y_keys, const uint8_t *__restrict__ y_counts, uint64_t n_y, uint64_t tiles,
                        unsigned long long *__restrict__ spec) {
    __shared__ uint32_t tally[CORNER * CORNER];
    __shared__ uint64_t bound[2];
    for (uint32_t i = threadIdx.x; i < CORNER * CORNER; i += 256) tally[i] = 0;
    __syncthreads();
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t first = tile * TBK_DBT_TILE;  // (< n_x)
        compact_tile_bounds(x_keys, n_x, first, y_keys, n_y, bound, 0);
        __syncthreads();
        const uint64_t y_lo = bound[0], y_hi = bound[1];
        for (uint32_t r = 0; r < TBK_DBT_TILE / 256; r++) {
            const uint64_t i = first + (uint64_t)r * 256 + threadIdx.x;
            if (i >= n_x) continue;
            const uint64_t key = x_keys[i];
            const uint32_t cx = x_counts[i];
            const uint64_t at = db_lower_bound(y_keys, y_lo, y_hi, key);  // (at <= y_hi <= n_y)
            const uint32_t cy = at < n_y && y_keys[at] == key ? y_counts[at] : 0u;
            if (cx < CORNER && cy < CORNER)
                atomicAdd(&tally[cx * CORNER + cy], 1u);
            else
                atomicAdd(&spec[cx * 256 + cy], 1ull);
        }
        __syncthreads();  // the bounds are read before the next trip writes them; after the last trip the tally is whole
    }
    for (uint32_t i = threadIdx.x; i < CORNER * CORNER; i += 256) {
        const uint32_t v = tally[i];
        if (v) atomicAdd(&spec[(i / CORNER) * 256 + i % CORNER], (unsigned long long)v);
    }
}

// ---- tbk_kmerdb_gc_spectrum: the entries of one database by the G-or-C bases of the key and by counter ----------------------
// spec[g * 256 + c] += entries with tbk_rank_gc(key) == g and counter c.  No partner, no bounds, no bisection: a tile is read
// and tallied, and the loop holds no barrier.  The matrix has k + 1 rows of 256 cells, 22 KiB of 32-bit words at k = 21 and
// 33 KiB at k = 32 - between the 16 KiB that cost the joint kernel no occupancy and the 64 KiB that cost it most of it - so
// the kernel is written for both answers and the launcher takes the one measured faster (GC_LAYOUT):
//   COLS = 256  the whole matrix in LDS, `rows` x 256 words of dynamic LDS: a CU holds 7 blocks at k = 21 and 4 at k = 32;
//   COLS = 64   the counters below 64 in LDS (8.25 KiB at k = 32: no occupancy lost) and the repeats' counters straight to
//               global atomics, as the joint kernel does with what lies outside its corner.
// The whole matrix it is (profiles/r25; r19's spectrum with 2 % of the counters over 64..255): on 2e7 entries, warm
// in the Infinity Cache, 0.052 ms against 0.084 ms at k = 21 and 0.055 against 0.080 at k = 32; on 1e8 entries, from HBM, 0.162
// against 0.345 ms.  28 or 16 waves a CU are enough for a kernel that only streams and tallies, and the repeats' global
// atomics cost the corner more than its spare LDS is worth.
// The grid is GC_GRID = 1024 blocks, not the 2048 of the other two kernels: every block zeroes and flushes a matrix of its own,
// some 1e3 non-zero cells, so half the blocks are half of that work.  Same runs, whole matrix, k = 21, in 2048 / 1024 / 512 /
// 256 blocks: 0.065 / 0.052 / 0.048 / 0.065 ms on 2e7 entries, 0.177 / 0.162 / 0.225 / 0.378 ms on 1e8 - two blocks a CU are
// too few waves once the loads come from HBM; 1024 is at or near the best of both.
// A row above `rows` cannot be met in a database the loader has checked (no bits above 2k); such an entry would go to the
// global matrix, which always has its 33 rows, and never past the block's LDS.
constexpr uint32_t GC_ROWS = 33;
#ifndef TBK_GC_LAYOUT  // 1: the whole matrix in LDS, 2: the corner; the other one is reached by tools/measure_gc.py
#define TBK_GC_LAYOUT 1
#endif
constexpr int GC_LAYOUT = TBK_GC_LAYOUT;
constexpr uint32_t GC_CORNER_COLS = 64;
constexpr uint64_t GC_GRID = 1024;  // 256 CUs x 4 blocks of 4 waves
// (measurement hook, not in tbk.h: tools/measure_gc.py times the launch under other grids in one process; 0 = GC_GRID, the
// state at load.  A plain global read at every launch, as the caps of tbk_count_set_grid_caps_ are, which still apply.)
static uint32_t g_gc_grid = 0;
extern "C" int tbk_kmerdb_gc_set_grid_(uint32_t blocks) {
    if (blocks > 65536) return 1;
    g_gc_grid = blocks;
    return 0;
}

template <uint32_t COLS>
__global__ void __launch_bounds__(256)
tbk_kmerdb_gc_kernel(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ counts, uint64_t n, uint64_t tiles, uint32_t rows,
                     unsigned long long *__restrict__ spec) {
    static_assert(COLS == 256 || COLS == GC_CORNER_COLS, "the whole row or the corner's part of it");
    extern __shared__ uint32_t gc_tally[];  // rows x COLS
    const uint32_t cells = rows * COLS;
    for (uint32_t i = threadIdx.x; i < cells; i += 256) gc_tally[i] = 0;
    __syncthreads();
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t first = tile * TBK_DBT_TILE;  // (< n)
        uint64_t key[TBK_DBT_TILE / 256];
        uint32_t c[TBK_DBT_TILE / 256];
#pragma unroll
        for (uint32_t r = 0; r < TBK_DBT_TILE / 256; r++) {  // the tile's loads first, all in flight together
            const uint64_t i = first + (uint64_t)r * 256 + threadIdx.x;
            key[r] = i < n ? keys[i] : 0;
            c[r] = i < n ? counts[i] : 0;
        }
#pragma unroll
        for (uint32_t r = 0; r < TBK_DBT_TILE / 256; r++) {
            if (first + (uint64_t)r * 256 + threadIdx.x >= n) continue;
            const uint32_t g = tbk_rank_gc(key[r]);  // (<= 32)
            if (g < rows && c[r] < COLS)
                atomicAdd(&gc_tally[g * COLS + c[r]], 1u);
            else
                atomicAdd(&spec[g * 256 + c[r]], 1ull);
        }
    }
    __syncthreads();  // the tally is whole
    for (uint32_t i = threadIdx.x; i < cells; i += 256) {
        const uint32_t v = gc_tally[i];
        if (v) atomicAdd(&spec[(i / COLS) * 256 + i % COLS], (unsigned long long)v);
    }
}

// the grid of a launch that strides over `tiles` tiles: capped, through the test hook's cap, and never so small that a block's
// 32-bit cells could wrap
static bool compare_grid(uint64_t tiles, unsigned *grid, uint64_t most = COMPARE_GRID) {
    *grid = tbk_count_entry_grid_(tiles < most ? tiles : most);
    return (tiles + *grid - 1) / *grid <= COMPARE_MAX_TILES_PER_BLOCK;
}

// d_spec: 4 * 256 words, zeroed by the caller.  The arrays of a database with no entry may be NULL.
extern "C" hipError_t tbk_launch_kmerdb_origin_spectrum(const uint64_t *base_keys, const uint8_t *base_counts, uint64_t n, const uint64_t *y_keys,
                                                        const uint8_t *y_counts, uint64_t n_y, uint32_t y_min, uint32_t y_max, const uint64_t *z_keys,
                                                        const uint8_t *z_counts, uint64_t n_z, uint32_t z_min, uint32_t z_max, uint32_t keep,
                                                        unsigned long long *d_spec, hipStream_t stream) {
    const uint64_t tiles = tbk_kmerdb_table_tiles(n);
    if (!tiles) return hipSuccess;
    unsigned grid = 0;
    if (!compare_grid(tiles, &grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tbk_kmerdb_origin_kernel, dim3(grid), dim3(256), 0, stream, base_keys, base_counts, n, y_keys, y_counts, n_y, y_min, y_max, z_keys,
                       z_counts, n_z, z_min, z_max, tiles, keep, d_spec);
    return hipGetLastError();
}

// d_spec: 256 * 256 words, zeroed by the caller.  Two launches: x against y into the cells (cx, cy or 0); then y against x,
// the origin kernel keeping the class "x lacks it" alone, whose row is the matrix's row 0: the cells (0, cy).
extern "C" hipError_t tbk_launch_kmerdb_joint_spectrum(const uint64_t *x_keys, const uint8_t *x_counts, uint64_t n_x, const uint64_t *y_keys,
                                                       const uint8_t *y_counts, uint64_t n_y, unsigned long long *d_spec, hipStream_t stream) {
    const uint64_t tiles = tbk_kmerdb_table_tiles(n_x);
    if (tiles) {
        unsigned grid = 0;
        if (!compare_grid(tiles, &grid)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(tbk_kmerdb_joint_kernel, dim3(grid), dim3(256), 0, stream, x_keys, x_counts, n_x, y_keys, y_counts, n_y, tiles, d_spec);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return tbk_launch_kmerdb_origin_spectrum(y_keys, y_counts, n_y, x_keys, x_counts, n_x, 1, 255, nullptr, nullptr, 0, 1, 255, 1u, d_spec, stream);
}

// d_spec: 33 * 256 words, zeroed by the caller.  layout 0: the build's (GC_LAYOUT); 1: the whole matrix in LDS; 2: the corner
// (1 and 2 by name are for tools/measure_gc.py, which times both in one process).
extern "C" hipError_t tbk_launch_kmerdb_gc_spectrum(const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, int k, int layout,
                                                    unsigned long long *d_spec, hipStream_t stream) {
    if (k < 1 || (uint32_t)k + 1 > GC_ROWS || layout < 0 || layout > 2) return hipErrorInvalidValue;
    const uint64_t tiles = tbk_kmerdb_table_tiles(n);
    if (!tiles) return hipSuccess;
    unsigned grid = 0;
    if (!compare_grid(tiles, &grid, g_gc_grid ? g_gc_grid : GC_GRID)) return hipErrorInvalidValue;
    const uint32_t rows = (uint32_t)k + 1;  // (<= GC_ROWS)
    if ((layout ? layout : GC_LAYOUT) == 1)
        hipLaunchKernelGGL(tbk_kmerdb_gc_kernel<256>, dim3(grid), dim3(256), rows * 256 * sizeof(uint32_t), stream, d_keys, d_counts, n, tiles, rows, d_spec);
    else
        hipLaunchKernelGGL(tbk_kmerdb_gc_kernel<GC_CORNER_COLS>, dim3(grid), dim3(256), rows * GC_CORNER_COLS * sizeof(uint32_t), stream, d_keys, d_counts,
                           n, tiles, rows, d_spec);
    return hipGetLastError();
}
