// tbk_compact.h — the kernels' side of the tile compaction (tbk_compact_host.h has the tile, the buffers and the launchers):
// the flag loop, the scatter's prologue and placement, the bounds of a tile in a second database and the questions an entry
// asks there, each written once for tbk_count_kernels.hip, tbk_dump.hip, tbk_compare.hip and tbk_select.hip.  Every helper is for a block of 256 threads that owns tile blockIdx.x, inlines
// into its kernel and takes what varies as a lambda.
#pragma once
#include "tbk_compact_host.h"
#include "tbk_device.h"

// The counter test of every selection between databases: 2 or more (a full database also holds the k-mers seen once) and in [ci, cx].
__device__ __forceinline__ bool db_counter_selected(uint32_t c, uint32_t ci, uint32_t cx) { return c >= 2u && c >= ci && c <= cx; }

// Is key not among keys[0 .. n), which ascend, when its lower bound there lies in [lo, hi]?  (0 and n always do.)
__device__ __forceinline__ bool db_absent(const uint64_t *__restrict__ keys, uint64_t lo, uint64_t hi, uint64_t n, uint64_t key) {
    const uint64_t at = db_lower_bound(keys, lo, hi, key);  // (at <= hi <= n)
    return !(at < n && keys[at] == key);
}

// Does the partner hold `key` with a counter in [c_min, c_max], taken literally?  lo .. hi: the tile's bounds there
// (tbk_compare.hip, tbk_select.hip).
__device__ __forceinline__ bool db_held_in_range(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ counts, uint64_t lo, uint64_t hi,
                                                 uint64_t n, uint64_t key, uint32_t c_min, uint32_t c_max) {
    const uint64_t at = db_lower_bound(keys, lo, hi, key);  // (at <= hi <= n)
    if (!(at < n && keys[at] == key)) return false;
    const uint32_t c = counts[at];
    return c >= c_min && c <= c_max;
}

// flag: entry i < n of the tile is kept when pred(i), which is called for no other i.  flags takes the tile's TBK_DBT_WORDS
// ballots, tile_counts[tile] their bits: every wave adds its four rounds up and then to one LDS word.  The one barrier
// before the loop also publishes what the block wrote to LDS before the call (compact_tile_bounds).
template <typename Pred>
__device__ __forceinline__ void compact_flag_tile(uint64_t n, uint64_t *__restrict__ flags, unsigned long long *__restrict__ tile_counts, Pred pred) {
    __shared__ uint32_t tile_sum;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t tile = blockIdx.x;
    if (threadIdx.x == 0) tile_sum = 0;
    __syncthreads();
    uint32_t mine = 0;  // (the same in every lane of a wave)
    for (uint32_t r = 0; r < TBK_DBT_TILE / 256; r++) {
        const uint32_t word = r * 4 + wave;
        const uint64_t i = tile * TBK_DBT_TILE + (uint64_t)word * 64 + lane;
        const uint64_t mask = __builtin_amdgcn_ballot_w64(i < n && pred(i));
        if (lane == 0) flags[tile * TBK_DBT_WORDS + word] = mask;
        mine += (uint32_t)__popcll(mask);
    }
    if (lane == 0 && mine) atomicAdd(&tile_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0) tile_counts[tile] = tile_sum;
}

// A's keys ascend within the tile that starts at entry `first` (< n_a), so every entry's lower bound among `keys` lies
// between those of the tile's first and last entry: threads t0 and t0 + 1 find these two by bisection over all n and leave
// them in the LDS words bound[0] and bound[1], to be read behind the block's next barrier.  An entry then bisects between
// its tile's two bounds only - about log2(tile * n / n_a) dependent loads, on lines the block shares; equal bounds mean
// that nothing of `keys` lies inside the tile's span, and the search is no load at all.
__device__ __forceinline__ void compact_tile_bounds(const uint64_t *__restrict__ a_keys, uint64_t n_a, uint64_t first, const uint64_t *__restrict__ keys,
                                                    uint64_t n, uint64_t *bound, uint32_t t0) {
    const uint32_t t = threadIdx.x - t0;
    if (t < 2) {
        const uint64_t last = (n_a - first < TBK_DBT_TILE ? n_a : first + TBK_DBT_TILE) - 1;
        bound[t] = db_lower_bound(keys, 0, n, a_keys[t ? last : first]);
    }
}

// The tile's flag words and, per word, the flagged entries of the tile below it.
struct CompactWords {
    uint64_t mask[TBK_DBT_WORDS];
    uint32_t before[TBK_DBT_WORDS];
};

// Threads t0 .. t0 + TBK_DBT_WORDS - 1 load the words into w (LDS); two barriers, after which every thread may read w and
// whatever else the block wrote to LDS before the call.
__device__ __forceinline__ void compact_load_words(CompactWords &w, const uint64_t *__restrict__ flags, uint32_t t0) {
    const uint32_t t = threadIdx.x - t0;
    if (t < TBK_DBT_WORDS) w.mask[t] = flags[(uint64_t)blockIdx.x * TBK_DBT_WORDS + t];
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t i = 0; i < TBK_DBT_WORDS; i++) {
            w.before[i] = sum;
            sum += (uint32_t)__popcll(w.mask[i]);
        }
    }
    __syncthreads();
}

// the flagged entries before lane's in its word: what a flagged entry adds to its tile's offset and its word's `before`
__device__ __forceinline__ uint32_t compact_below(uint64_t mask, uint32_t lane) { return (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)); }

// scatter: place(i, at) for every flagged entry i < n of the tile, at = tile_offsets[tile] + the flagged entries before it in the tile
template <typename Place>
__device__ __forceinline__ void compact_scatter_tile(uint64_t n, const uint64_t *__restrict__ flags, const unsigned long long *__restrict__ tile_offsets,
                                                     Place place) {
    __shared__ CompactWords w;
    compact_load_words(w, flags, 0);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t tile = blockIdx.x;
    const uint64_t base = tile_offsets[tile];
    for (uint32_t r = 0; r < TBK_DBT_TILE / 256; r++) {
        const uint32_t word = r * 4 + wave;
        const uint64_t mask = w.mask[word];
        const uint64_t i = tile * TBK_DBT_TILE + (uint64_t)word * 64 + lane;
        if (((mask >> lane) & 1ull) && i < n) place(i, base + w.before[word] + compact_below(mask, lane));
    }
}

// the place of the r-th set bit of mask, counted from bit 0 (r < popcount(mask)): six halvings
__device__ __forceinline__ uint32_t compact_nth_bit(uint64_t mask, uint32_t r) {
    uint32_t at = 0;
    for (uint32_t width = 32; width; width >>= 1) {
        const uint32_t below = (uint32_t)__popcll(mask & ((1ull << width) - 1ull));
        if (r >= below) {
            r -= below;
            mask >>= width;
            at += width;
        }
    }
    return at;
}

// The same scatter with the flagged entries dealt to consecutive threads: thread t takes the t-th, t + 256-th, ... flagged
// entry of the tile, so a wave whose `place` is expensive (a bisection per entry) works with all its lanes however few
// entries of the tile are flagged - in compact_scatter_tile a wave pays for its 64 entries when one of them is.  The entry is
// found from the word table: the word whose `before` covers the place, then the bit within it.
template <typename Place>
__device__ __forceinline__ void compact_scatter_tile_dense(uint64_t n, const uint64_t *__restrict__ flags,
                                                           const unsigned long long *__restrict__ tile_offsets, Place place) {
    __shared__ CompactWords w;
    compact_load_words(w, flags, 0);
    const uint64_t tile = blockIdx.x;
    const uint64_t base = tile_offsets[tile];
    const uint32_t total = w.before[TBK_DBT_WORDS - 1] + (uint32_t)__popcll(w.mask[TBK_DBT_WORDS - 1]);  // (<= TBK_DBT_TILE)
    for (uint32_t j = threadIdx.x; j < total; j += 256) {
        uint32_t word = 0;
        for (uint32_t step = TBK_DBT_WORDS / 2; step; step >>= 1)  // the last word whose `before` is <= j: it holds the j-th flagged entry
            if (w.before[word + step] <= j) word += step;
        const uint64_t i = tile * TBK_DBT_TILE + (uint64_t)word * 64 + compact_nth_bit(w.mask[word], j - w.before[word]);
        if (i < n) place(i, base + j);
    }
}

// One block of 256 threads per tile of n entries, no grid stride; nothing to launch for no entry.
template <typename Kernel, typename... Args>
static hipError_t compact_launch_tiles(uint64_t n, hipStream_t stream, Kernel kernel, Args... args) {
    const uint64_t tiles = tbk_kmerdb_table_tiles(n);
    if (!tiles) return hipSuccess;
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(256), 0, stream, args...);
    return hipGetLastError();
}
