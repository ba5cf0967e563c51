// tbk_screen.hip — the MI355X kernels of a query session's read evidence (tbk_kmerdb_query_evidence): per sequence of a batch,
// how many of its windows the database holds with a counter in a range, and how much of the sequence those windows cover.
// Two kernels: the lookup pass leaves the clean and the held bitmap, the evidence kernel reduces both to one record per
// sequence.  Neither writes any state of the session.  Host side: tbk_count.cpp; the rule: include/tbk.h, "read evidence".
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/tbk.h"
#include "tbk_common.h"
#include "tbk_lookup.h"

// One wave per pass of TBK_PASS window starts of the separated stream: staging, roll and the grouped search are lookup_pass's
// (tbk_lookup.h).  What is left is one bit per stream position in each of two bitmaps, 64 words per pass: clean, and
// held - clean with c_lo <= c <= c_hi (c_lo > c_hi: nothing is held).  No atomic, nothing of the session written.
__global__ void __launch_bounds__(64)
tbk_screen_lookup_kernel(const uint8_t *__restrict__ sep, uint64_t total, uint64_t n_passes, int k, TbkDbView db, uint32_t c_lo, uint32_t c_hi,
                         uint32_t *__restrict__ clean, uint32_t *__restrict__ held) {
    __shared__ uint64_t stage[TBK_CHUNKS + 2];
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t pass = blockIdx.x; pass < n_passes; pass += gridDim.x) {
        uint32_t w_clean = 0, w_held = 0;
        lookup_pass(stage, sep, total, pass, k, db, [&](int j0, const LookupGroup &w) {
#pragma unroll
            for (int g = 0; g < TBK_GROUP; g++) {
                const uint32_t bit = 1u << (j0 + g);
                if (w.ok[g]) w_clean |= bit;
                if (w.ok[g] && w.c[g] >= c_lo && w.c[g] <= c_hi) w_held |= bit;
            }
        });
        clean[pass * 64 + lane] = w_clean;
        held[pass * 64 + lane] = w_held;
    }
}

// ---- the evidence: one record per sequence from the two bitmaps ----------------------------------------------------------------
// The covered positions of a stretch of positions as a segment of a segmented max-run: the run of covered positions it begins
// with, the one it ends with, its longest, and whether all of it is covered (then the three are its length).
struct ScreenRuns {
    uint32_t lead, trail, best, full;
};

// a, then b: the stretch of a lies below b's.  Not commutative; ScreenRuns{0, 0, 0, 1}, the empty stretch, is neutral on both sides.
__device__ __forceinline__ ScreenRuns screen_join(const ScreenRuns &a, const ScreenRuns &b) {
    ScreenRuns out;
    out.best = std::max(std::max(a.best, b.best), a.trail + b.lead);
    out.lead = a.full ? a.lead + b.lead : a.lead;
    out.trail = b.full ? a.trail + b.trail : b.trail;
    out.full = a.full & b.full;
    return out;
}

// Sequence r lies at stream positions [a, b) = [offsets[r] + r, offsets[r + 1] + r), as tbk_query_totals_kernel reads it: its
// clean and its held windows are the set bits of the two bitmaps there, and the edge words are masked (range_word_mask).
// The COVERED bitmap is the held one dilated by k - 1 positions upward: k <= 32, so a 32-bit word needs only its predecessor as
// halo, and the dilation is floor(log2 k) + 1 shift-and-ors of the two words side by side in one 64-bit register.  A held window starts at L - k
// at most, so the dilation ends at the sequence's last base, b - 1: the covered words need no mask of their own and the word
// behind the last one holds nothing of this sequence (include/tbk.h says so).  covered is a popcount, stretches counts the
// 0-to-1 edges - the bit below a word is covered when any of the top k bits of the held predecessor is set - and longest is a
// segmented max-run over the words IN WORD ORDER: a word's (lead, trail, best, full) are joined across the lanes by a tree
// in which the lower lane is always the left operand, and a trip's result is joined behind the trips before it.
// One wave per sequence, four to a block, striding over the sequences by the grid.  A long read (15 kb: 470 words) fills
// the lanes for eight trips; a read of a handful of words leaves most lanes idle for its one trip, which then costs what
// tbk_query_totals_kernel costs beside the same lookup - two offsets, three words per lane and the shuffles.  Sharing a
// wave among short reads would take a search for each word's sequence and a join segmented by sequence as well, to save
// time in a kernel that reads three bits per position behind a lookup pass that bisects a bucket for every one: the whole
// wave it is.
__global__ void __launch_bounds__(256)
tbk_screen_evidence_kernel(const uint32_t *__restrict__ clean_bits, const uint32_t *__restrict__ held_bits, const uint64_t *__restrict__ offsets,
                           uint64_t n_reads, int k, unsigned long long *__restrict__ records) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_reads; r += waves) {
        const uint64_t a = offsets[r] + r, b = offsets[r + 1] + r;  // [a, b)
        unsigned long long clean = 0, held = 0, covered = 0, stretches = 0;
        unsigned long long trail = 0, best = 0;  // the words of the trips so far, joined: the run they end with and their longest
        if (b > a) {  // (the same in every lane)
            const uint64_t w_first = a >> 5, w_last = (b - 1) >> 5;
            for (uint64_t w0 = w_first; w0 <= w_last; w0 += 64) {
                const uint64_t w = w0 + lane;
                const bool mine = w <= w_last, halo = mine && w > w_first;
                const uint64_t at = mine ? w : w_last, below = halo ? w - 1 : w_first;  // (no load under a branch: an idle lane reads a word of the sequence)
                const uint32_t mask = mine ? range_word_mask(w, w_first, w_last, a, b) : 0u;
                const uint32_t mask_below = halo ? range_word_mask(below, w_first, w_last, a, b) : 0u;
                const uint32_t c = clean_bits[at] & mask, h = held_bits[at] & mask, hb = held_bits[below] & mask_below;
                const uint32_t cov = covered_word(h, hb, k);  // (tbk_lookup.h: the ladder of shift-and-ors)
                const uint32_t under = (k == 32 ? hb : hb >> (32 - k)) != 0;  // position 32 w - 1 is covered
                clean += (uint32_t)__popc(c);
                held += (uint32_t)__popc(h);
                covered += (uint32_t)__popc(cov);
                stretches += (uint32_t)__popc(cov & ~((cov << 1) | under));
                ScreenRuns runs;
                runs.full = mine ? cov == 0xFFFFFFFFu : 1u;  // (an idle lane: cov is 0, the empty stretch)
                runs.lead = ~cov ? (uint32_t)__ffs((int)~cov) - 1u : 32u;  // the ones below the lowest zero
                runs.trail = (uint32_t)__clz((int)~cov);                   // the ones above the highest zero (32 when there is none)
                uint32_t longest = 0;
                for (uint32_t y = cov; y; y &= y << 1) longest++;  // the longest run of ones of a word: at most 32 steps
                runs.best = longest;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {  // lane l joins the lanes l .. l + 2 d - 1 in order; lane 0 ends with all 64
                    ScreenRuns up;
                    up.lead = __shfl_down(runs.lead, d);
                    up.trail = __shfl_down(runs.trail, d);
                    up.best = __shfl_down(runs.best, d);
                    up.full = __shfl_down(runs.full, d);
                    runs = screen_join(runs, up);
                }
                // behind the trips so far (lane 0's is the wave's; a trip holds 2048 positions, the sequence as many as 64 bits count)
                best = std::max(std::max(best, (unsigned long long)runs.best), trail + runs.lead);
                trail = runs.full ? trail + runs.trail : runs.trail;
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            clean += __shfl_xor(clean, d);
            held += __shfl_xor(held, d);
            covered += __shfl_xor(covered, d);
            stretches += __shfl_xor(stretches, d);
        }
        if (lane == 0) {
            records[5 * r] = clean;
            records[5 * r + 1] = held;
            records[5 * r + 2] = covered;
            records[5 * r + 3] = best;
            records[5 * r + 4] = stretches;
        }
    }
}
static_assert(sizeof(tbk_read_evidence) == 40, "a record is five 64-bit words: clean, held, covered, longest, stretches");

// =======================================================================================
// launchers (called from tbk_count.cpp)
// =======================================================================================
// (what the arguments hold: tbk_lookup_host.h)
extern "C" hipError_t tbk_launch_screen_lookup(const uint8_t *d_sep, uint64_t total, uint64_t n_passes, int k, TbkDbView db, uint32_t c_lo, uint32_t c_hi,
                                               uint32_t *d_clean, uint32_t *d_held, uint64_t wave_slots, hipStream_t stream) {
    if (!n_passes) return hipSuccess;
    if (!tbk_db_view_ok(db, k) || c_lo < 1 || c_lo > 255 || c_hi > 255) return hipErrorInvalidValue;
    const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_passes, wave_slots))), block(64);
    hipLaunchKernelGGL(tbk_screen_lookup_kernel, grid, block, 0, stream, d_sep, total, n_passes, k, db, c_lo, c_hi, d_clean, d_held);
    return hipGetLastError();
}

// Four sequences to a block: the grid-stride loop takes a second trip from 4 wave_slots + 1 sequences on.
extern "C" hipError_t tbk_launch_screen_evidence(const uint32_t *d_clean, const uint32_t *d_held, const uint64_t *d_offsets, uint64_t n_reads, int k,
                                                 tbk_read_evidence *d_records, uint64_t wave_slots, hipStream_t stream) {
    if (!n_reads) return hipSuccess;
    if (k < 1 || k > 32) return hipErrorInvalidValue;
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((n_reads + 3) / 4, wave_slots));
    hipLaunchKernelGGL(tbk_screen_evidence_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_clean, d_held, d_offsets, n_reads, k,
                       reinterpret_cast<unsigned long long *>(d_records));
    return hipGetLastError();
}
