// tbk_depth.hip — the MI355X kernels of a query session's copy-number track (tbk_kmerdb_query_track): a second pass over
// sequences that were added, which reads the reads' counter c and the session's copy counter a of every window back
// along the sequence and reduces them per bin of W window starts.  Two kernels: the lookup pass leaves bitmaps and two
// bytes per stream position, the bin pass reduces them to one tbk_depth_bin per bin.  Neither writes any state of the
// session.  Host side: tbk_count.cpp; the rule: include/tbk.h, "copy-number track".
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/tbk.h"
#include "tbk_common.h"
#include "tbk_lookup.h"

// What the lookup pass leaves for the bin pass.  The bitmaps hold one bit per stream position, 64 words per pass, like the
// query's: clean, present (c >= 1), saturated (c == 255) and the two verdicts.  c and min(a, 255) are one byte per stream
// position each, TBK_PASS per pass, 0 for a window that is absent or not clean.
struct TbkDepthMarks {
    uint32_t *clean, *present, *saturated, *collapsed, *expanded;
    uint8_t *c, *a;
};

// One wave per pass of TBK_PASS window starts of the separated stream: staging, roll and the grouped search are lookup_pass's
// (tbk_lookup.h).  The session's copy counter a of an entry (copies, beside the view's counters) is read as the search reads
// the counter: for all of a group's windows before any is used, a miss reading entry 0.  Nothing of the session is written:
// no atomic, no histogram.
// The verdicts are drawn here, where the full 32-bit a is at hand, in 64-bit integers: for a present window with
// c < 255, collapsed is 2c > (2a + 1) peak and expanded is a >= 1 and 2c < (2a - 1) peak.  The host passes
// min(peak, 509): 2c <= 508, so every peak above 508 answers as 509 does, and (2a + 1) 509 < 2^42 cannot wrap.
__global__ void __launch_bounds__(64)
tbk_depth_lookup_kernel(const uint8_t *__restrict__ sep, uint64_t total, uint64_t n_passes, int k, TbkDbView db, const uint32_t *__restrict__ copies,
                        uint32_t peak, TbkDepthMarks out) {
    __shared__ uint64_t stage[TBK_CHUNKS + 2];
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t pass = blockIdx.x; pass < n_passes; pass += gridDim.x) {
        const uint64_t p_lane = pass * TBK_PASS + (uint64_t)lane * TBK_WPL;
        uint32_t w_clean = 0, w_present = 0, w_saturated = 0, w_collapsed = 0, w_expanded = 0;
        lookup_pass(stage, sep, total, pass, k, db, [&](int j0, const LookupGroup &w) {
            uint32_t a[TBK_GROUP];
#pragma unroll
            for (int g = 0; g < TBK_GROUP; g++) a[g] = copies[w.hit[g] ? w.at[g] : 0];
            uint32_t word_c = 0, word_a = 0;
#pragma unroll
            for (int g = 0; g < TBK_GROUP; g++) {
                const uint32_t cg = w.c[g], bit = 1u << (j0 + g);
                const uint64_t twice_c = 2ull * cg, twice_a = 2ull * a[g];
                const bool verdict = cg != 0 && cg < 255u;
                if (w.ok[g]) w_clean |= bit;
                if (cg) w_present |= bit;
                if (cg == 255u) w_saturated |= bit;
                if (verdict && twice_c > (twice_a + 1ull) * peak) w_collapsed |= bit;
                if (verdict && a[g] >= 1u && twice_c < (twice_a - 1ull) * peak) w_expanded |= bit;
                word_c |= cg << (8 * g);
                word_a |= (cg ? (a[g] < 255u ? a[g] : 255u) : 0u) << (8 * g);
            }
            *reinterpret_cast<uint32_t *>(out.c + p_lane + j0) = word_c;
            *reinterpret_cast<uint32_t *>(out.a + p_lane + j0) = word_a;
        });
        out.clean[pass * 64 + lane] = w_clean;
        out.present[pass * 64 + lane] = w_present;
        out.saturated[pass * 64 + lane] = w_saturated;
        out.collapsed[pass * 64 + lane] = w_collapsed;
        out.expanded[pass * 64 + lane] = w_expanded;
    }
}
static_assert(TBK_GROUP == 4, "a group's bytes are one 32-bit store");

// the lower median of a 256-row histogram of m >= 1 values, lane l holding the sum of rows 4 l .. 4 l + 3 in `mine`: an
// inclusive wave scan of the lanes' sums finds the lane whose rows hold sorted value (m - 1) / 2, and that lane walks its four rows
__device__ __forceinline__ uint32_t depth_lower_median(const uint32_t *__restrict__ rows, uint32_t mine, uint32_t m, uint32_t lane) {
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= (uint32_t)d) incl += up;
    }
    const uint32_t target = (m - 1u) / 2u;  // 0-based among the sorted values
    const unsigned long long past = __builtin_amdgcn_ballot_w64(incl > target);  // (lane 63 holds m > target: never empty)
    const uint32_t owner = (uint32_t)__builtin_ctzll(past);
    uint32_t run = incl - mine, value = 4u * lane + 3u;  // run: the values before this lane's rows
    bool found = false;
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {  // the first of the four rows whose running sum passes the target
        run += rows[4u * lane + i];
        if (!found && run > target) { value = 4u * lane + i; found = true; }
    }
    return __shfl(value, (int)owner);
}

// One wave per bin, striding over the bins by the grid.  Bin g belongs to the sequence r with prefix[r] <= g < prefix[r + 1]
// (prefix: the host's running sum of bins per sequence, n_reads + 1 entries; a sequence without bins repeats its
// neighbour's value), as its bin b = g - prefix[r]: the window starts [bW, min((b + 1) W, nw)) of r, which lie at stream
// positions offsets[r] + r + w.  The five counts are popcounts over the lookup pass's bitmaps with masked edge words; the
// two histograms, of c and of min(a, 255) over the present windows, are built in LDS from the two byte arrays, read as
// aligned 32-bit words with the bytes outside the bin dropped, and cleared again for the next bin.  Lanes 0..5 store the
// bin's six words: one 24-byte store.
__global__ void __launch_bounds__(64)
tbk_depth_bin_kernel(TbkDepthMarks in, const uint64_t *__restrict__ offsets, const uint64_t *__restrict__ prefix, uint64_t n_reads,
                     uint64_t n_bins, int k, uint32_t window, uint32_t *__restrict__ bins) {
    __shared__ uint32_t hist_c[256], hist_a[256];
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t g = blockIdx.x; g < n_bins; g += gridDim.x) {
        for (uint32_t i = lane; i < 256; i += 64) hist_c[i] = hist_a[i] = 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        uint64_t lo = 0, hi = n_reads;  // the last r in [0, n_reads) with prefix[r] <= g (prefix[0] = 0 <= g < n_bins = prefix[n_reads])
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (prefix[mid] <= g) lo = mid; else hi = mid;
        }
        const uint64_t r = lo, b = g - prefix[r];
        const uint64_t first = offsets[r] + r, nw = offsets[r + 1] - offsets[r] - (uint64_t)k + 1;  // (the sequence has a bin: nw >= 1)
        const uint64_t p0 = first + b * window, p1 = first + std::min<uint64_t>((b + 1) * window, nw);  // [p0, p1), p1 > p0
        uint32_t n_clean = 0, n_present = 0, n_saturated = 0, n_collapsed = 0, n_expanded = 0;
        const uint64_t w_first = p0 >> 5, w_last = (p1 - 1) >> 5;
#pragma unroll 1
        for (uint64_t w = w_first + lane; w <= w_last; w += 64) {
            const uint32_t mask = range_word_mask(w, w_first, w_last, p0, p1);
            n_clean += (uint32_t)__popc(in.clean[w] & mask);
            n_present += (uint32_t)__popc(in.present[w] & mask);
            n_saturated += (uint32_t)__popc(in.saturated[w] & mask);
            n_collapsed += (uint32_t)__popc(in.collapsed[w] & mask);
            n_expanded += (uint32_t)__popc(in.expanded[w] & mask);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            n_clean += __shfl_xor(n_clean, d);
            n_present += __shfl_xor(n_present, d);
            n_saturated += __shfl_xor(n_saturated, d);
            n_collapsed += __shfl_xor(n_collapsed, d);
            n_expanded += __shfl_xor(n_expanded, d);
        }
        uint32_t depth = 0, copies = 0;
        if (n_present) {  // (the same in every lane)
            const uint64_t q_first = p0 >> 2, q_last = (p1 - 1) >> 2;
#pragma unroll 1
            for (uint64_t q = q_first + lane; q <= q_last; q += 64) {
                uint32_t wc = reinterpret_cast<const uint32_t *>(in.c)[q], wa = reinterpret_cast<const uint32_t *>(in.a)[q];
                uint32_t mask = 0xFFFFFFFFu;
                if (q == q_first) mask &= 0xFFFFFFFFu << (8u * (uint32_t)(p0 & 3u));
                if (q == q_last) mask &= 0xFFFFFFFFu >> (8u * (3u - (uint32_t)((p1 - 1) & 3u)));
                wc &= mask;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t cv = (wc >> (8 * i)) & 255u;
                    if (cv) {
                        atomicAdd(&hist_c[cv], 1u);
                        atomicAdd(&hist_a[(wa >> (8 * i)) & 255u], 1u);
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            const uint32_t sum_c = hist_c[4 * lane] + hist_c[4 * lane + 1] + hist_c[4 * lane + 2] + hist_c[4 * lane + 3];
            const uint32_t sum_a = hist_a[4 * lane] + hist_a[4 * lane + 1] + hist_a[4 * lane + 2] + hist_a[4 * lane + 3];
            depth = depth_lower_median(hist_c, sum_c, n_present, lane);
            copies = depth_lower_median(hist_a, sum_a, n_present, lane);
        }
        const uint32_t word = lane == 0 ? n_clean : lane == 1 ? n_clean - n_present : lane == 2 ? n_saturated : lane == 3 ? n_collapsed
                              : lane == 4 ? n_expanded : (depth | (copies << 8));
        if (lane < 6) bins[g * 6 + lane] = word;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the medians' reads of the rows, before the next bin clears them)
    }
}
static_assert(sizeof(tbk_depth_bin) == 24, "a bin is six 32-bit words: five counts, then depth, copies and two zero bytes");

// =======================================================================================
// launchers (called from tbk_count.cpp; what the arguments hold: tbk_lookup_host.h)
// =======================================================================================
extern "C" hipError_t tbk_launch_depth_lookup(const uint8_t *d_sep, uint64_t total, uint64_t n_passes, int k, TbkDbView db, const uint32_t *d_copies,
                                              uint32_t peak, uint32_t *d_clean, uint32_t *d_present, uint32_t *d_saturated, uint32_t *d_collapsed,
                                              uint32_t *d_expanded, uint8_t *d_c, uint8_t *d_a, uint64_t wave_slots, hipStream_t stream) {
    if (!n_passes) return hipSuccess;
    if (!tbk_db_view_ok(db, k) || peak < 1 || peak > 509) return hipErrorInvalidValue;
    const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_passes, wave_slots))), block(64);
    const TbkDepthMarks out{d_clean, d_present, d_saturated, d_collapsed, d_expanded, d_c, d_a};
    hipLaunchKernelGGL(tbk_depth_lookup_kernel, grid, block, 0, stream, d_sep, total, n_passes, k, db, d_copies, peak, out);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_depth_bins(uint32_t *d_clean, uint32_t *d_present, uint32_t *d_saturated, uint32_t *d_collapsed, uint32_t *d_expanded,
                                            uint8_t *d_c, uint8_t *d_a, const uint64_t *d_offsets, const uint64_t *d_prefix, uint64_t n_reads,
                                            uint64_t n_bins, int k, uint32_t window, tbk_depth_bin *d_bins, uint64_t wave_slots, hipStream_t stream) {
    if (!n_bins) return hipSuccess;
    if (!n_reads || !window || k < 1 || k > 32) return hipErrorInvalidValue;
    const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_bins, wave_slots))), block(64);
    const TbkDepthMarks in{d_clean, d_present, d_saturated, d_collapsed, d_expanded, d_c, d_a};
    hipLaunchKernelGGL(tbk_depth_bin_kernel, grid, block, 0, stream, in, d_offsets, d_prefix, n_reads, n_bins, k, window,
                       reinterpret_cast<uint32_t *>(d_bins));
    return hipGetLastError();
}
