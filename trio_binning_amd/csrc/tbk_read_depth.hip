// tbk_read_depth.hip — the MI355X kernels of a query session's read depth (tbk_kmerdb_query_read_depth): per sequence of a batch,
// a five-number summary of the counters the database holds for its windows.  Two kernels: the lookup pass leaves the clean
// bitmap and one depth byte per stream position, the per-read kernel reduces both to one record per sequence.  Neither writes
// any state of the session.  Host side: tbk_count.cpp; the rule: include/tbk.h, "read depth".
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/tbk.h"
#include "tbk_common.h"
#include "tbk_lookup.h"

// One wave per pass of TBK_PASS window starts of the separated stream: staging, roll and the grouped search are lookup_pass's
// (tbk_lookup.h).  What is left per stream position is one bit of the clean bitmap, 64 words per pass, and one byte: the depth
// d - the counter c when the window is clean and c >= m, else 0 - a group's four as one 32-bit store, as
// tbk_depth_lookup_kernel stores its counters.  Every byte of every pass is written.  No atomic, nothing of the session written.
__global__ void __launch_bounds__(64)
tbk_read_depth_lookup_kernel(const uint8_t *__restrict__ sep, uint64_t total, uint64_t n_passes, int k, TbkDbView db, uint32_t m,
                             uint32_t *__restrict__ clean, uint8_t *__restrict__ depth) {
    __shared__ uint64_t stage[TBK_CHUNKS + 2];
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t pass = blockIdx.x; pass < n_passes; pass += gridDim.x) {
        const uint64_t p_lane = pass * TBK_PASS + (uint64_t)lane * TBK_WPL;
        uint32_t w_clean = 0;
        lookup_pass(stage, sep, total, pass, k, db, [&](int j0, const LookupGroup &w) {
            uint32_t word = 0;
#pragma unroll
            for (int g = 0; g < TBK_GROUP; g++) {
                if (w.ok[g]) w_clean |= 1u << (j0 + g);
                word |= (w.c[g] >= m ? w.c[g] : 0u) << (8 * g);  // (c is 0 for a window that is not clean: m >= 1)
            }
            *reinterpret_cast<uint32_t *>(depth + p_lane + j0) = word;
        });
        clean[pass * 64 + lane] = w_clean;
    }
}
static_assert(TBK_GROUP == 4, "a group's bytes are one 32-bit store");

// ---- the per-read summary ------------------------------------------------------------------------------------------------------------
// A wave's 256-row histogram of the depths d >= 1 of one sequence, read off once: lane l holds rows 4 l .. 4 l + 3 in row[], their
// sum in `mine` and the inclusive wave scan of the sums in `incl` (lane 63: all the present windows).
struct DepthRows {
    uint32_t row[4], mine, incl;
};

__device__ __forceinline__ DepthRows depth_rows_scan(const uint32_t *__restrict__ rows, uint32_t lane) {
    DepthRows h;
#pragma unroll
    for (int i = 0; i < 4; i++) h.row[i] = rows[4u * lane + i];
    h.mine = h.row[0] + h.row[1] + h.row[2] + h.row[3];
    h.incl = h.mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(h.incl, d);
        if (lane >= (uint32_t)d) h.incl += up;
    }
    return h;
}

// depth_lower_median (tbk_depth.hip) for a given 0-based rank and a row-0 count from outside: sorted value `rank` of the multiset
// that holds `zeros` zeros and the rows' values, rank < zeros + present.  The zeros come first; behind them the scan finds the
// lane whose rows hold the value, and that lane walks its four rows.  The scan is shared by every rank asked of one sequence.
__device__ __forceinline__ uint32_t depth_value_at_rank(const DepthRows &h, uint32_t zeros, uint64_t rank, uint32_t lane) {
    if (rank < zeros) return 0;  // (the same in every lane)
    const uint32_t target = (uint32_t)(rank - zeros);  // 0-based among the present values: below lane 63's incl
    const unsigned long long past = __builtin_amdgcn_ballot_w64(h.incl > target);
    const uint32_t owner = past ? (uint32_t)__builtin_ctzll(past) : 63u;
    uint32_t run = h.incl - h.mine, value = 4u * lane + 3u;  // run: the values before this lane's rows
    bool found = false;
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {  // the first of the four rows whose running sum passes the target
        run += h.row[i];
        if (!found && run > target) { value = 4u * lane + i; found = true; }
    }
    return __shfl(value, (int)owner);
}

// Sequence r lies at stream positions [a, b) = [offsets[r] + r, offsets[r + 1] + r), as tbk_screen_evidence_kernel reads it.
// clean is a popcount over the clean bitmap with masked edge words (range_word_mask).  The depth bytes of [a, b) are read as
// aligned 32-bit words with the bytes outside [a, b) dropped, as tbk_depth_bin_kernel reads a bin's - a sequence starts at any of
// the four byte alignments - and every d >= 1 is counted in the wave's own 256 rows of LDS; the positions of [a, b) that are no
// clean window, the last k - 1 among them, hold 0 and are not counted.  Row 0 is never written: the depth-0 windows are
// clean - present.  The rows are read off once per sequence (depth_rows_scan): the five ranks floor(j (clean - 1) / 4) and the
// present windows' lower median come from the one scan, saturated is row 255, and sum - in 64 bits - is the rows weighted by
// their values.  lowest and highest are ranks 0 and clean - 1, which are the bottom non-empty row, counting row 0, and the top one.
// Each lane clears the rows it read for the wave's next sequence.  Lanes 0..9 store the record's ten 32-bit words.
// One wave per sequence, four to a block, striding over the sequences by the grid, as the evidence kernel does.
// TBK_READ_DEPTH_COMBINE (measurement only, tools/build_variant.sh): equal values are combined before the LDS add - the equal
// bytes of a lane's word are added once with their multiplicity, and a trip whose 64 words are all the same is added by lane 0
// alone.  profiles/r28 has what it is worth.
__global__ void __launch_bounds__(256)
tbk_read_depth_kernel(const uint32_t *__restrict__ clean_bits, const uint8_t *__restrict__ depth, const uint64_t *__restrict__ offsets,
                      uint64_t n_reads, uint32_t *__restrict__ records) {
    __shared__ uint32_t rows_of_block[4][256];
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t *rows = rows_of_block[threadIdx.x >> 6];
    const uint32_t *__restrict__ words = reinterpret_cast<const uint32_t *>(depth);
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
#pragma unroll
    for (int i = 0; i < 4; i++) rows[4u * lane + i] = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_reads; r += waves) {
        const uint64_t a = offsets[r] + r, b = offsets[r + 1] + r;  // [a, b)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the rows are clear before the adds)
        unsigned long long clean = 0;
        if (b > a) {  // (the same in every lane)
            const uint64_t w_first = a >> 5, w_last = (b - 1) >> 5;
            for (uint64_t w0 = w_first; w0 <= w_last; w0 += 64) {
                const uint64_t w = w0 + lane;
                const bool mine = w <= w_last;
                const uint64_t at = mine ? w : w_last;  // (no load under a branch: an idle lane reads a word of the sequence)
                const uint32_t mask = mine ? range_word_mask(w, w_first, w_last, a, b) : 0u;
                clean += (uint32_t)__popc(clean_bits[at] & mask);
            }
            const uint64_t q_first = a >> 2, q_last = (b - 1) >> 2;
            for (uint64_t q0 = q_first; q0 <= q_last; q0 += 64) {
                const uint64_t q = q0 + lane;
                const bool mine = q <= q_last;
                uint32_t mask = mine ? 0xFFFFFFFFu : 0u;
                if (q == q_first) mask &= 0xFFFFFFFFu << (8u * (uint32_t)(a & 3u));
                if (q == q_last) mask &= 0xFFFFFFFFu >> (8u * (3u - (uint32_t)((b - 1) & 3u)));
                const uint32_t word = words[mine ? q : q_last] & mask;
#ifdef TBK_READ_DEPTH_COMBINE
                const bool same = __builtin_amdgcn_ballot_w64(word != (uint32_t)__builtin_amdgcn_readfirstlane((int)word)) == 0;
                const bool adder = !same || lane == 0;  // (all 64 words the same: lane 0 adds for the wave)
                const uint32_t scale = same ? 64u : 1u;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t v = (word >> (8 * i)) & 255u;
                    uint32_t times = 0;
                    bool first = true;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const bool equal = ((word >> (8 * j)) & 255u) == v;
                        times += equal;
                        if (j < i && equal) first = false;
                    }
                    if (v && first && adder) atomicAdd(&rows[v], times * scale);
                }
#else
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t v = (word >> (8 * i)) & 255u;
                    if (v) atomicAdd(&rows[v], 1u);
                }
#endif
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) clean += __shfl_xor(clean, d);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the adds before the rows are read)
        const DepthRows h = depth_rows_scan(rows, lane);
#pragma unroll
        for (int i = 0; i < 4; i++) rows[4u * lane + i] = 0;  // (this lane's reads of them are done: clear for the next sequence)
        const uint32_t present = (uint32_t)__shfl(h.incl, 63);
        const uint32_t saturated = (uint32_t)__shfl(h.row[3], 63);
        unsigned long long sum = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) sum += (unsigned long long)h.row[i] * (4u * lane + i);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        uint32_t five = 0, rest = 0;  // lowest, q1, median, q3 | highest, present_median, pad
        if (clean) {  // (the same in every lane; clean < 2^32: the host refuses a longer sequence)
            const uint32_t zeros = (uint32_t)clean - present;
            const uint64_t top = clean - 1;
#pragma unroll
            for (uint64_t j = 0; j < 4; j++) five |= depth_value_at_rank(h, zeros, j * top / 4, lane) << (8 * j);
            rest = depth_value_at_rank(h, zeros, top, lane);
            if (present) rest |= depth_value_at_rank(h, zeros, (uint64_t)zeros + (present - 1u) / 2u, lane) << 8;
        }
        const uint32_t word = lane == 0 ? (uint32_t)clean : lane == 1 ? (uint32_t)(clean >> 32) : lane == 2 ? present : lane == 4 ? saturated
                              : lane == 6 ? (uint32_t)sum : lane == 7 ? (uint32_t)(sum >> 32) : lane == 8 ? five : lane == 9 ? rest : 0u;
        if (lane < 10) records[10 * r + lane] = word;
    }
}
static_assert(sizeof(tbk_read_depth) == 40, "a record is ten 32-bit words: clean, present, saturated and sum in two each, then the six bytes and two of pad");

// =======================================================================================
// launchers (called from tbk_count.cpp; what the arguments hold: tbk_lookup_host.h)
// =======================================================================================
extern "C" hipError_t tbk_launch_read_depth_lookup(const uint8_t *d_sep, uint64_t total, uint64_t n_passes, int k, TbkDbView db, uint32_t m,
                                                   uint32_t *d_clean, uint8_t *d_depth, uint64_t wave_slots, hipStream_t stream) {
    if (!n_passes) return hipSuccess;
    if (!tbk_db_view_ok(db, k) || m < 1 || m > 255) return hipErrorInvalidValue;
    const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_passes, wave_slots))), block(64);
    hipLaunchKernelGGL(tbk_read_depth_lookup_kernel, grid, block, 0, stream, d_sep, total, n_passes, k, db, m, d_clean, d_depth);
    return hipGetLastError();
}

// Four sequences to a block: the grid-stride loop takes a second trip from 4 wave_slots + 1 sequences on.
extern "C" hipError_t tbk_launch_read_depth(const uint32_t *d_clean, const uint8_t *d_depth, const uint64_t *d_offsets, uint64_t n_reads,
                                            tbk_read_depth *d_records, uint64_t wave_slots, hipStream_t stream) {
    if (!n_reads) return hipSuccess;
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((n_reads + 3) / 4, wave_slots));
    hipLaunchKernelGGL(tbk_read_depth_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_clean, d_depth, d_offsets, n_reads,
                       reinterpret_cast<uint32_t *>(d_records));
    return hipGetLastError();
}
