// tbk_query.hip — the MI355X kernels of a database query: how often did the reads see each k-mer of a sequence?
// A directory over the top bits of the database's ranks, the per-window lookup (one counter per window start, the
// histogram, the seen bits, the copies), the per-sequence totals and the per-entry tallies.  Host side: tbk_count.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/tbk.h"
#include "tbk_common.h"
#include "tbk_compact_host.h"  // (the one declaration of tbk_launch_query_directory)
#include "tbk_lookup.h"

// The directory of a TbkDbView (tbk_lookup_host.h).  One thread per prefix bisects the whole database once (db_lower_bound): 2^prefix_bits + 1 offsets, no atomic, no scan.
__global__ void __launch_bounds__(256)
tbk_query_directory_kernel(const uint64_t *__restrict__ keys, uint32_t n, int k, int prefix_bits, uint32_t *__restrict__ dir) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, top = 1ull << prefix_bits;
    if (p > top) return;
    if (p == top) { dir[p] = n; return; }
    const uint64_t first = prefix_bits ? p << (2 * k - prefix_bits) : 0;  // the least rank of prefix p
    dir[p] = (uint32_t)db_lower_bound(keys, 0, n, first);
}

// One wave per pass of TBK_PASS window starts of the separated stream: staging, roll and the grouped search are lookup_pass's
// (tbk_lookup.h).  Per window: bit j of the lane's clean word and of its found word (c >= min_count), indexed by stream
// position like the tracker's bitmaps; the wave's histogram of c in LDS, flushed once per block; the entry's seen bit and,
// with COPIES, its 32-bit copy counter (the host keeps a session below 2^32 window starts); with BYTES, c at the window's
// stream position.  A window over a separator or past `total` is not clean and stays 0 everywhere.
template <bool BYTES, bool COPIES>
__global__ void __launch_bounds__(64)
tbk_query_lookup_kernel(const uint8_t *__restrict__ sep, uint64_t total, uint64_t n_passes, int k, TbkDbView db, uint32_t min_count,
                        uint32_t *__restrict__ clean_bits, uint32_t *__restrict__ found_bits, uint8_t *__restrict__ bytes,
                        unsigned long long *__restrict__ hist, uint32_t *__restrict__ seen, uint32_t *__restrict__ copies) {
    __shared__ uint64_t stage[TBK_CHUNKS + 2];
    __shared__ uint32_t tally[256];
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t i = lane; i < 256; i += 64) tally[i] = 0;
    for (uint64_t pass = blockIdx.x; pass < n_passes; pass += gridDim.x) {
        const uint64_t p_lane = pass * TBK_PASS + (uint64_t)lane * TBK_WPL;
        uint32_t word_clean = 0, word_found = 0;
        lookup_pass(stage, sep, total, pass, k, db, [&](int j0, const LookupGroup &w) {
            uint32_t word = 0;
#pragma unroll
            for (int g = 0; g < TBK_GROUP; g++) {
                const uint32_t cg = w.c[g];
                if (w.ok[g]) {
                    word_clean |= 1u << (j0 + g);
                    atomicAdd(&tally[cg], 1u);
                }
                if (cg >= min_count) word_found |= 1u << (j0 + g);  // (min_count >= 2: never an absent window)
                if (cg) {
                    atomicOr(&seen[w.at[g] >> 5], 1u << (w.at[g] & 31u));
                    if (COPIES) atomicAdd(&copies[w.at[g]], 1u);
                }
                word |= cg << (8 * g);
            }
            if (BYTES) *reinterpret_cast<uint32_t *>(bytes + p_lane + j0) = word;
        });
        clean_bits[pass * 64 + lane] = word_clean;
        found_bits[pass * 64 + lane] = word_found;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (uint32_t i = lane; i < 256; i += 64) {
        const uint32_t v = tally[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
}
static_assert(TBK_GROUP == 4, "a group's counters are one 32-bit store");

// Sequence r lies at stream positions offsets[r] + r .. offsets[r + 1] + r: its clean and its found windows are the set
// bits of the two bitmaps in that range (its last k - 1 window starts hold the separator and are clear).  One wave per
// sequence; the edge words are masked.  totals: n_reads x 2, clean then found.
__global__ void __launch_bounds__(256)
tbk_query_totals_kernel(const uint32_t *__restrict__ clean_bits, const uint32_t *__restrict__ found_bits, const uint64_t *__restrict__ offsets,
                        uint64_t n_reads, unsigned long long *__restrict__ totals) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_reads; r += waves) {
        const uint64_t a = offsets[r] + r, b = offsets[r + 1] + r;  // [a, b)
        unsigned long long clean = 0, found = 0;
        if (b > a) {
            const uint64_t w_first = a >> 5, w_last = (b - 1) >> 5;
            for (uint64_t w = w_first + lane; w <= w_last; w += 64) {
                const uint32_t mask = range_word_mask(w, w_first, w_last, a, b);
                clean += (uint32_t)__popc(clean_bits[w] & mask);
                found += (uint32_t)__popc(found_bits[w] & mask);
            }
        }
        for (int d = 32; d > 0; d >>= 1) {
            clean += __shfl_xor(clean, d);
            found += __shfl_xor(found, d);
        }
        if (lane == 0) {
            totals[2 * r] = clean;
            totals[2 * r + 1] = found;
        }
    }
}

// The counters in the batch's own coordinates: byte offsets[r] + w is window w of read r, stream position offsets[r] + r + w.
__global__ void __launch_bounds__(256)
tbk_query_counts_kernel(const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ offsets, uint64_t n_reads, uint8_t *__restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_reads; r += waves) {
        const uint64_t lo = offsets[r], hi = offsets[r + 1];
        for (uint64_t i = lo + lane; i < hi; i += 64) counts[i] = bytes[i + r];
    }
}

// ---- per-entry tallies: one block per tile of 1024 entries at a time, its sums in LDS, one flush per block -----------
constexpr uint32_t TBK_Q_TILE = 1024;

// out[0]: entries with a counter in [ci, cx] whose seen bit is set; out[1]: entries with a counter in [ci, cx]
__global__ void __launch_bounds__(256)
tbk_query_completeness_kernel(const uint8_t *__restrict__ counts, const uint32_t *__restrict__ seen, uint32_t n, uint32_t ci, uint32_t cx,
                              unsigned long long *__restrict__ out) {
    __shared__ uint32_t sums[2];
    const uint32_t lane = threadIdx.x & 63u;
    if (threadIdx.x < 2) sums[threadIdx.x] = 0;
    __syncthreads();
    uint32_t n_seen = 0, n_solid = 0;  // (the same in every lane of a wave; n < 2^32)
    const uint32_t tiles = (uint32_t)(((uint64_t)n + TBK_Q_TILE - 1) / TBK_Q_TILE);
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        for (uint32_t r = 0; r < TBK_Q_TILE / 256; r++) {
            const uint64_t i = (uint64_t)tile * TBK_Q_TILE + r * 256 + threadIdx.x;
            bool solid = false, both = false;
            if (i < n) {
                const uint32_t c = counts[i];
                solid = c >= ci && c <= cx;
                both = solid && ((seen[i >> 5] >> (i & 31u)) & 1u);
            }
            n_solid += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(solid));
            n_seen += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(both));
        }
    }
    if (lane == 0) {
        if (n_seen) atomicAdd(&sums[0], n_seen);
        if (n_solid) atomicAdd(&sums[1], n_solid);
    }
    __syncthreads();
    if (threadIdx.x < 2 && sums[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)sums[threadIdx.x]);
}

// spec[min(copies, 5)][counter] over every entry: 6 x 256
__global__ void __launch_bounds__(256)
tbk_query_spectrum_kernel(const uint8_t *__restrict__ counts, const uint32_t *__restrict__ copies, uint32_t n, unsigned long long *__restrict__ spec) {
    __shared__ uint32_t cell[6 * 256];
    for (uint32_t i = threadIdx.x; i < 6 * 256; i += 256) cell[i] = 0;
    __syncthreads();
    const uint32_t tiles = (uint32_t)(((uint64_t)n + TBK_Q_TILE - 1) / TBK_Q_TILE);
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        for (uint32_t r = 0; r < TBK_Q_TILE / 256; r++) {
            const uint64_t i = (uint64_t)tile * TBK_Q_TILE + r * 256 + threadIdx.x;
            if (i < n) {
                const uint32_t m = copies[i];
                atomicAdd(&cell[(m < 5u ? m : 5u) * 256 + counts[i]], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 6 * 256; i += 256)
        if (cell[i]) atomicAdd(&spec[i], (unsigned long long)cell[i]);
}

// =======================================================================================
// launchers (called from tbk_count.cpp)
// =======================================================================================
// d_dir: 2^prefix_bits + 1 offsets
extern "C" hipError_t tbk_launch_query_directory(const uint64_t *d_keys, uint64_t n, int k, int prefix_bits, uint32_t *d_dir, hipStream_t stream) {
    if (k < 1 || k > 32 || prefix_bits < 0 || prefix_bits > 2 * k || prefix_bits > 30 || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint64_t blocks = ((1ull << prefix_bits) + 1 + 255) / 256;
    hipLaunchKernelGGL(tbk_query_directory_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_keys, (uint32_t)n, k, prefix_bits, d_dir);
    return hipGetLastError();
}

// (what the arguments of this and the following launchers hold: tbk_lookup_host.h)
extern "C" hipError_t tbk_launch_query_lookup(const uint8_t *d_sep, uint64_t total, uint64_t n_passes, int k, TbkDbView db, uint32_t min_count,
                                              uint32_t *d_clean, uint32_t *d_found, uint8_t *d_bytes, unsigned long long *d_hist, uint32_t *d_seen,
                                              uint32_t *d_copies, uint64_t wave_slots, hipStream_t stream) {
    if (!n_passes) return hipSuccess;
    if (!tbk_db_view_ok(db, k)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_passes, wave_slots))), block(64);
#define TBK_QUERY_LAUNCH(B, C) hipLaunchKernelGGL((tbk_query_lookup_kernel<B, C>), grid, block, 0, stream, d_sep, total, n_passes, k, db, min_count, d_clean, d_found, d_bytes, d_hist, d_seen, d_copies)
    if (d_bytes && d_copies) TBK_QUERY_LAUNCH(true, true);
    else if (d_bytes) TBK_QUERY_LAUNCH(true, false);
    else if (d_copies) TBK_QUERY_LAUNCH(false, true);
    else TBK_QUERY_LAUNCH(false, false);
#undef TBK_QUERY_LAUNCH
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_query_totals(const uint32_t *d_clean, const uint32_t *d_found, const uint64_t *d_offsets, uint64_t n_reads,
                                              unsigned long long *d_totals, uint64_t wave_slots, hipStream_t stream) {
    if (!n_reads) return hipSuccess;
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((n_reads + 3) / 4, wave_slots));
    hipLaunchKernelGGL(tbk_query_totals_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_clean, d_found, d_offsets, n_reads, d_totals);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_query_counts(const uint8_t *d_bytes, const uint64_t *d_offsets, uint64_t n_reads, uint8_t *d_counts,
                                              uint64_t wave_slots, hipStream_t stream) {
    if (!n_reads) return hipSuccess;
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((n_reads + 3) / 4, wave_slots));
    hipLaunchKernelGGL(tbk_query_counts_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_bytes, d_offsets, n_reads, d_counts);
    return hipGetLastError();
}

static unsigned query_tile_blocks(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + TBK_Q_TILE - 1) / TBK_Q_TILE, 2048)); }

extern "C" hipError_t tbk_launch_query_completeness(const uint8_t *d_counts, const uint32_t *d_seen, uint64_t n, uint32_t ci, uint32_t cx,
                                                    unsigned long long *d_out, hipStream_t stream) {
    if (!n) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tbk_query_completeness_kernel, dim3(query_tile_blocks(n)), dim3(256), 0, stream, d_counts, d_seen, (uint32_t)n, ci, cx, d_out);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_query_spectrum(const uint8_t *d_counts, const uint32_t *d_copies, uint64_t n, unsigned long long *d_spec,
                                                hipStream_t stream) {
    if (!n) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tbk_query_spectrum_kernel, dim3(query_tile_blocks(n)), dim3(256), 0, stream, d_counts, d_copies, (uint32_t)n, d_spec);
    return hipGetLastError();
}
