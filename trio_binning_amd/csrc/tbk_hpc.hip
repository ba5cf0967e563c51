// tbk_hpc.hip — the MI355X kernels of homopolymer compression: every run of equal bases of a read written once, before
// k-mers are cut.  The shape of tbk_kmerdb_unique_table and the hit tracker's compactions: one bit per base for the read
// starts, one bit per base for `keep` and a count per tile, an exclusive scan of the tile counts (one block), a scatter
// that knows where its tile starts, and one thread per read that turns offsets[r] into its rank among the kept bits.
// Every launch reads only what an earlier launch finished: no block waits for another.  Host side: tbk_hpc_host.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tbk.h"
#include "tbk_common.h"

constexpr uint32_t TBK_HPC_TILE = 4096;                 // bases per tile: 256 lanes x one 16-byte vector
constexpr uint32_t TBK_HPC_WORDS = TBK_HPC_TILE / 64;  // 64-bit keep words per tile

// f of the contract, four bytes at a time: bit 5 cleared in the bytes that are ASCII letters (A-Z after the clearing,
// bit 7 clear), every other byte as it is.
__device__ __forceinline__ uint32_t hpc_fold4(uint32_t w) {
    const uint32_t u = w & 0x5F5F5F5Fu;                                         // bits 5 and 7 away: 7-bit values, sums cannot carry across bytes
    const uint32_t ge = (u + 0x3F3F3F3Fu) & 0x80808080u;                        // u >= 0x41
    const uint32_t gt = (u + 0x25252525u) & 0x80808080u;                        // u >= 0x5B
    const uint32_t letter = ge & ~gt & ~w & 0x80808080u;
    return w & ~(letter >> 2);
}

// 0x1 per byte of d that is not zero, gathered into four bits (pack4's test, tbk_device.h)
__device__ __forceinline__ uint32_t hpc_nonzero4(uint32_t d) {
    uint32_t nz = (((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u;
    nz >>= 7;
    return (nz | (nz >> 7) | (nz >> 14) | (nz >> 21)) & 0xFu;
}

// the 16 bytes from pos on; bytes at or past `total` read as 0.  pos is a multiple of 16 and the base 16-byte aligned.
__device__ __forceinline__ uint4 hpc_load16(const uint8_t *__restrict__ bases, uint64_t pos, uint64_t total) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (pos + 16 <= total) {
        v = *reinterpret_cast<const uint4 *>(bases + pos);
    } else if (pos < total) {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t i = 0; i < 16; i++)
            if (pos + i < total) w[i >> 2] |= (uint32_t)bases[pos + i] << (8 * (i & 3));
        v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return v;
}

// One thread per offset: read r starts at offsets[r]; the start is a bit of the starts bitmap (zeroed by the caller) unless
// it lies at `total` - a trailing empty read - or beyond, which never touches the bitmap.  Empty reads share their
// successor's start.  The offsets are checked on the way (a batch that is already on the device has been checked by
// nobody): offsets[0] == 0, ascending, offsets[n_reads] == total, else *bad is set and the host refuses the batch.
__global__ void __launch_bounds__(256)
tbk_hpc_starts_kernel(const uint64_t *__restrict__ offsets, uint64_t n_reads, uint64_t total, uint32_t *__restrict__ starts,
                      unsigned long long *__restrict__ bad) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n_reads) return;
    const uint64_t p = offsets[r];
    bool wrong = r == 0 ? p != 0 : false;
    if (r == n_reads) wrong = wrong || p != total;
    else wrong = wrong || offsets[r + 1] < p;
    if (wrong) atomicOr(bad, 1ull);
    if (r < n_reads && p < total) atomicOr(&starts[p >> 5], 1u << (p & 31u));
}

// One block per tile, a lane per 16-byte vector.  keep bit i: position 0, a read start, or f(b[i]) != f(b[i - 1]); the
// byte before a lane's vector is the last (folded) byte of the lane below, or one extra load at the edge of a wave.
// Positions at or past `total` are clear.  keep16[pos / 16] gets the lane's 16 bits, tile_counts[tile] the tile's sum.
__global__ void __launch_bounds__(256)
tbk_hpc_keep_kernel(const uint8_t *__restrict__ bases, uint64_t total, int fold_case, const uint32_t *__restrict__ starts,
                    uint16_t *__restrict__ keep16, unsigned long long *__restrict__ tile_counts) {
    __shared__ uint32_t wave_sum[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t pos = (uint64_t)blockIdx.x * TBK_HPC_TILE + (uint64_t)threadIdx.x * 16;
    uint4 v = hpc_load16(bases, pos, total);
    if (fold_case) { v.x = hpc_fold4(v.x); v.y = hpc_fold4(v.y); v.z = hpc_fold4(v.z); v.w = hpc_fold4(v.w); }
    uint32_t before = __shfl_up(v.w >> 24, 1);
    if (lane == 0) {
        before = 0;
        if (pos > 0 && pos < total) {
            before = bases[pos - 1];
            if (fold_case) before = hpc_fold4(before);
        }
    }
    uint32_t keep = hpc_nonzero4(v.x ^ ((v.x << 8) | before)) | (hpc_nonzero4(v.y ^ ((v.y << 8) | (v.x >> 24))) << 4) |
                    (hpc_nonzero4(v.z ^ ((v.z << 8) | (v.y >> 24))) << 8) | (hpc_nonzero4(v.w ^ ((v.w << 8) | (v.z >> 24))) << 12);
    if (pos < total) keep |= (starts[pos >> 5] >> (pos & 16u)) & 0xFFFFu;
    if (pos == 0) keep |= 1u;
    const uint64_t left = pos < total ? total - pos : 0;  // positions of this vector inside the batch
    if (left < 16) keep &= (1u << left) - 1u;
    keep16[pos >> 4] = (uint16_t)keep;
    uint32_t sum = (uint32_t)__popc(keep);
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    if (lane == 0) wave_sum[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

// Exclusive scan of n tile counts by ONE block of 1024 threads, 8192 counts a round: a thread sums its eight, the sums
// are scanned across the wave by shuffles and across the sixteen waves through LDS, and the round's total is carried
// into the next.  A batch of 256 Mbases has 65537 counts: nine rounds.  out[n - 1] is the total when in[n - 1] is 0.
constexpr uint32_t TBK_HPC_SCAN_PER = 8;
__global__ void __launch_bounds__(1024)
tbk_hpc_scan_kernel(const unsigned long long *__restrict__ in, unsigned long long *__restrict__ out, uint64_t n) {
    __shared__ unsigned long long wave_total[16];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < n; base += 1024 * TBK_HPC_SCAN_PER) {
        const uint64_t i0 = base + (uint64_t)threadIdx.x * TBK_HPC_SCAN_PER;
        unsigned long long x[TBK_HPC_SCAN_PER], mine = 0;
#pragma unroll
        for (uint32_t j = 0; j < TBK_HPC_SCAN_PER; j++) {
            x[j] = i0 + j < n ? in[i0 + j] : 0;
            mine += x[j];
        }
        unsigned long long upto = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long below = __shfl_up(upto, d);
            if (lane >= (uint32_t)d) upto += below;
        }
        if (lane == 63) wave_total[wave] = upto;
        __syncthreads();
        unsigned long long at = carry + upto - mine, round_total = 0;
        for (uint32_t w = 0; w < 16; w++) {
            if (w < wave) at += wave_total[w];
            round_total += wave_total[w];
        }
#pragma unroll
        for (uint32_t j = 0; j < TBK_HPC_SCAN_PER; j++) {
            if (i0 + j < n) out[i0 + j] = at;
            at += x[j];
        }
        carry += round_total;
        __syncthreads();
    }
}

// The kept bytes of a tile, verbatim, to out[tile_offsets[tile] ...].  A lane's place in the tile is a prefix sum of the
// lanes' counts; the bytes are gathered in LDS at the alignment they will have in `out`, so that the tile leaves as
// aligned 16-byte vectors except at its two ragged ends, which go byte by byte (a neighbouring tile owns the rest of
// those vectors).
__global__ void __launch_bounds__(256)
tbk_hpc_scatter_kernel(const uint8_t *__restrict__ bases, uint64_t total, const uint16_t *__restrict__ keep16,
                       const unsigned long long *__restrict__ tile_offsets, uint8_t *__restrict__ out, uint64_t total_out) {
    __shared__ __attribute__((aligned(16))) uint8_t staged[TBK_HPC_TILE + 16];
    __shared__ uint32_t wave_sum[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t pos = (uint64_t)blockIdx.x * TBK_HPC_TILE + (uint64_t)threadIdx.x * 16;
    const uint4 v = hpc_load16(bases, pos, total);
    const uint32_t keep = keep16[pos >> 4];
    const uint32_t mine = (uint32_t)__popc(keep);
    uint32_t upto = mine;  // inclusive prefix sum over the lanes of the wave
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t below = __shfl_up(upto, d);
        if (lane >= (uint32_t)d) upto += below;
    }
    if (lane == 63) wave_sum[wave] = upto;
    __syncthreads();
    uint32_t at = upto - mine;
    for (uint32_t w = 0; w < wave; w++) at += wave_sum[w];
    const uint32_t count = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    const uint64_t first = tile_offsets[blockIdx.x];
    const uint32_t skew = (uint32_t)(first & 15u);
    at += skew;
    const uint32_t word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t j = 0; j < 16; j++)
        if ((keep >> j) & 1u) staged[at++] = (uint8_t)(word[j >> 2] >> (8 * (j & 3)));
    __syncthreads();
    if (first + count > total_out) return;  // (never: the total is the scan's own)
    uint8_t *dst = out + (first - skew);    // 16-byte aligned
    const uint32_t end = skew + count;
    for (uint32_t c = threadIdx.x * 16; c < end; c += 256 * 16) {
        if (c >= skew && c + 16 <= end) {
            *reinterpret_cast<uint4 *>(dst + c) = *reinterpret_cast<const uint4 *>(staged + c);
        } else {
            for (uint32_t i = c < skew ? skew : c; i < c + 16 && i < end; i++) dst[i] = staged[i];
        }
    }
}

// One thread per offset: the new offsets[r] is the number of kept positions before the old one - the scanned count of
// its tile plus the bits of the tile's keep words below it.  An old offset past `total` (a refused batch) is read as `total`.
__global__ void __launch_bounds__(256)
tbk_hpc_offsets_kernel(const uint64_t *__restrict__ offsets, uint64_t n_reads, uint64_t total, const uint64_t *__restrict__ keep64,
                       const unsigned long long *__restrict__ tile_offsets, uint64_t *__restrict__ out_offsets) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n_reads) return;
    uint64_t p = offsets[r];
    if (p > total) p = total;
    const uint64_t tile = p / TBK_HPC_TILE;
    const uint32_t in_tile = (uint32_t)(p % TBK_HPC_TILE);
    uint64_t rank = tile_offsets[tile];  // (p == total on a tile boundary: the entry behind the last tile, the total)
    const uint64_t *words = keep64 + tile * TBK_HPC_WORDS;
    for (uint32_t w = 0; w < in_tile / 64; w++) rank += (uint64_t)__popcll(words[w]);
    if (in_tile & 63u) rank += (uint64_t)__popcll(words[in_tile / 64] & ((1ull << (in_tile & 63u)) - 1ull));
    out_offsets[r] = rank;
}

// ---- the map read backwards: compressed position -> input position (lift), compressed bytes -> input bytes (expand) ----

// The position of set bit number r (from 0) of w, r < popcount(w): the half that holds it, five times over.
__device__ __forceinline__ uint32_t hpc_select64(uint64_t w, uint32_t r) {
    uint32_t x = (uint32_t)w, at = 0;
    uint32_t c = (uint32_t)__popc(x);
    if (r >= c) { r -= c; at = 32; x = (uint32_t)(w >> 32); }
#pragma unroll
    for (uint32_t half = 16; half > 0; half >>= 1) {
        c = (uint32_t)__popc(x & ((1u << half) - 1u));
        if (r >= c) { r -= c; at += half; x >>= half; }
    }
    return at;
}

// out[i] = the input position of kept byte positions[i]: the position of set keep bit number positions[i].  A position at
// (or past: the host refuses those) the compressed total gives `total`.  A lane bisects the tiles + 1 tile offsets for the
// LAST tile whose offset is not above its position - an empty tile has its successor's offset, and a homopolymer longer
// than a tile leaves such tiles - which is then a tile that holds the bit.  The wave serves its lanes' positions in
// turn: the 64 lanes load the tile's 64 keep words as one 512-byte read, popcount, scan the counts across the wave and
// ballot for the word; the owner selects the bit.  No atomics; nothing waits for another wave.
__global__ void __launch_bounds__(256)
tbk_hpc_lift_kernel(const uint64_t *__restrict__ positions, uint64_t n, const uint64_t *__restrict__ keep64,
                    const unsigned long long *__restrict__ tile_offsets, uint64_t tiles, uint64_t total, uint64_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long tile = 0;
    uint32_t rank = 0;  // of the bit among its tile's
    bool inside = false;
    if (i < n) {
        const uint64_t j = positions[i];
        if (j >= tile_offsets[tiles]) {
            out[i] = total;
        } else {
            uint64_t lo = 0, hi = tiles;  // tile_offsets[lo] <= j < tile_offsets[hi]
            while (hi - lo > 1) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (tile_offsets[mid] <= j) lo = mid; else hi = mid;
            }
            tile = lo;
            rank = (uint32_t)(j - tile_offsets[lo]);
            inside = true;
        }
    }
    uint64_t todo = __builtin_amdgcn_ballot_w64(inside);
    while (todo) {  // (the same in every lane)
        const uint32_t owner = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
        todo &= todo - 1ull;
        const unsigned long long t = __shfl(tile, (int)owner);
        const uint32_t r = __shfl(rank, (int)owner);
        const unsigned long long word = keep64[t * TBK_HPC_WORDS + lane];
        const uint32_t mine = (uint32_t)__popcll(word);
        uint32_t upto = mine;  // inclusive prefix sum over the words of the tile
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t below = __shfl_up(upto, d);
            if (lane >= (uint32_t)d) upto += below;
        }
        const uint64_t reached = __builtin_amdgcn_ballot_w64(upto > r);
        if (!reached) continue;  // (never: the rank is below the tile's count)
        const uint32_t w = (uint32_t)__ffsll((unsigned long long)reached) - 1u;
        const unsigned long long the_word = __shfl(word, (int)w);
        const uint32_t before = __shfl(upto - mine, (int)w);
        if (lane == owner) out[i] = t * TBK_HPC_TILE + (uint64_t)w * 64 + hpc_select64(the_word, r - before);
    }
}

// tbk_hpc_scatter_kernel run backwards, for one value per kept byte: input position p gets values[its rank among the
// kept bits] if its keep bit is set and 0 if not.  One block per tile of the input, a lane per 16-byte vector; the
// lane's first rank is the tile's offset plus the prefix sum of the keep popcounts below it.  One aligned 16-byte
// store per lane, byte by byte where `total` cuts the vector.
__global__ void __launch_bounds__(256)
tbk_hpc_expand_kernel(const uint8_t *__restrict__ values, uint64_t total_c, const uint16_t *__restrict__ keep16,
                      const unsigned long long *__restrict__ tile_offsets, uint64_t total, uint8_t *__restrict__ out) {
    __shared__ uint32_t wave_sum[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t pos = (uint64_t)blockIdx.x * TBK_HPC_TILE + (uint64_t)threadIdx.x * 16;
    const uint32_t keep = keep16[pos >> 4];
    const uint32_t mine = (uint32_t)__popc(keep);
    uint32_t upto = mine;  // inclusive prefix sum over the lanes of the wave
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t below = __shfl_up(upto, d);
        if (lane >= (uint32_t)d) upto += below;
    }
    if (lane == 63) wave_sum[wave] = upto;
    __syncthreads();
    uint64_t at = tile_offsets[blockIdx.x] + (upto - mine);
    for (uint32_t w = 0; w < wave; w++) at += wave_sum[w];
    uint32_t word[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < 16; j++)
        if ((keep >> j) & 1u) {
            if (at < total_c) word[j >> 2] |= (uint32_t)values[at] << (8 * (j & 3));
            at++;
        }
    if (pos + 16 <= total) {
        *reinterpret_cast<uint4 *>(out + pos) = make_uint4(word[0], word[1], word[2], word[3]);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 16; i++)
            if (pos + i < total) out[pos + i] = (uint8_t)(word[i >> 2] >> (8 * (i & 3)));
    }
}

// =======================================================================================
// launchers (called from tbk_hpc_host.cpp)
// =======================================================================================
extern "C" uint32_t tbk_hpc_tile(void) { return TBK_HPC_TILE; }
extern "C" uint64_t tbk_hpc_tiles(uint64_t total) { return (total + TBK_HPC_TILE - 1) / TBK_HPC_TILE; }

// d_starts: tiles * TBK_HPC_TILE / 8 bytes; d_keep the same; d_tile_counts and d_tile_offsets: tiles + 1 entries each
// (the last count is 0, so the last offset is the total); d_bad: one word.  d_out must hold the input's `total` bytes
// rounded up to 16; d_out_offsets n_reads + 1 entries.  Everything is queued on `stream`; nothing is waited for.
extern "C" hipError_t tbk_launch_hpc_mark(const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t total, int fold_case,
                                          uint32_t *d_starts, uint64_t *d_keep, unsigned long long *d_tile_counts,
                                          unsigned long long *d_tile_offsets, unsigned long long *d_bad,
                                          hipStream_t stream) {
    const uint64_t tiles = tbk_hpc_tiles(total), read_blocks = (n_reads + 1 + 255) / 256;
    if (!tiles || tiles > 0x7FFFFFFFull || read_blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_starts, 0, tiles * (TBK_HPC_TILE / 8), stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_tile_counts + tiles, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tbk_hpc_starts_kernel, dim3((unsigned)read_blocks), dim3(256), 0, stream, d_offsets, n_reads, total, d_starts, d_bad);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(tbk_hpc_keep_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, d_bases, total, fold_case, d_starts,
                       reinterpret_cast<uint16_t *>(d_keep), d_tile_counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(tbk_hpc_scan_kernel, dim3(1), dim3(1024), 0, stream, d_tile_counts, d_tile_offsets, tiles + 1);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_hpc_move(const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t total, const uint64_t *d_keep,
                                          const unsigned long long *d_tile_offsets, uint8_t *d_out, uint64_t total_out, uint64_t *d_out_offsets,
                                          hipStream_t stream) {
    const uint64_t tiles = tbk_hpc_tiles(total), read_blocks = (n_reads + 1 + 255) / 256;
    if (!tiles || tiles > 0x7FFFFFFFull || read_blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tbk_hpc_scatter_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, d_bases, total, reinterpret_cast<const uint16_t *>(d_keep),
                       d_tile_offsets, d_out, total_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tbk_hpc_offsets_kernel, dim3((unsigned)read_blocks), dim3(256), 0, stream, d_offsets, n_reads, total, d_keep, d_tile_offsets,
                       d_out_offsets);
    return hipGetLastError();
}

// d_keep, d_tile_offsets: what tbk_launch_hpc_mark left for an input of `total` bases.  n positions in, n out.
extern "C" hipError_t tbk_launch_hpc_lift(const uint64_t *d_positions, uint64_t n, const uint64_t *d_keep, const unsigned long long *d_tile_offsets,
                                          uint64_t total, uint64_t *d_out, hipStream_t stream) {
    const uint64_t tiles = tbk_hpc_tiles(total), blocks = (n + 255) / 256;
    if (!n) return hipSuccess;
    if (!tiles || tiles > 0x7FFFFFFFull || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tbk_hpc_lift_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_positions, n, d_keep, d_tile_offsets, tiles, total, d_out);
    return hipGetLastError();
}

// d_values: total_c bytes; d_out: 16-byte aligned, `total` bytes rounded up to 16
extern "C" hipError_t tbk_launch_hpc_expand(const uint8_t *d_values, uint64_t total_c, const uint64_t *d_keep, const unsigned long long *d_tile_offsets,
                                            uint64_t total, uint8_t *d_out, hipStream_t stream) {
    const uint64_t tiles = tbk_hpc_tiles(total);
    if (!tiles || tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tbk_hpc_expand_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, d_values, total_c, reinterpret_cast<const uint16_t *>(d_keep),
                       d_tile_offsets, total, d_out);
    return hipGetLastError();
}
