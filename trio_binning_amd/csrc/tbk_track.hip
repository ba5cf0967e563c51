// tbk_track.hip — the MI355X kernels of the hit tracker: WHERE along a read its haplotype k-mers lie.
// The classifier keeps two numbers per read; these kernels keep the positions: one bit per window start and
// haplotype (marking), then the raw runs of consecutive same-haplotype markers (runs).  Host side: tbk_host.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/tbk.h"
#include "tbk_common.h"
#include "tbk_lookup.h"

// tbk_separate_kernel (tbk_count_kernels.hip) with the upper-casing as a switch: every read is followed by one 'N',
// so no window spans two reads and validity is the not-ACGT mask alone.  With ignore_case, clearing bit 5 turns
// exactly a c g t into A C G T among the bytes that were not ACGT before (no other byte has an ACGT byte 0x20 below
// it); without it a lower-case base stays what pack4 calls bad.  One wave per read.
__global__ void __launch_bounds__(256)
tbk_track_separate_kernel(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ offsets, uint64_t n_reads, int ignore_case,
                          uint8_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint8_t keep = ignore_case ? 0xDFu : 0xFFu;
    for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_reads; r += waves) {
        const uint64_t lo = offsets[r], hi = offsets[r + 1];
        uint8_t *dst = out + lo + r;
        for (uint64_t i = lo + lane; i < hi; i += 64) dst[i - lo] = bases[i] & keep;
        if (lane == 0) dst[hi - lo] = 'N';
    }
}

// Membership in a list's standalone table (tbk_host.cpp: table_hash): tbk_lookup_slow for the one form such a table
// has - 64-byte lines of 8 slots, the bucket a hash of the whole key, a purely linear probe sequence, no guests -
// with the line fetched as four 16-byte loads in flight at once.  A miss stops at the first line no key went past
// (slot 6 <= slot 7, tbk_common.h).
__device__ __forceinline__ bool track_lookup(const uint64_t *__restrict__ slots, uint32_t n_buckets, uint64_t key) {
    if (key >= TBK_NOKEY) return false;
    uint32_t b = tbk_reduce(tbk_mix32(key), n_buckets);
    for (uint32_t walked = 0; walked <= n_buckets; walked++) {
        const ulonglong2 *v = reinterpret_cast<const ulonglong2 *>(slots + (uint64_t)b * TBK_SLOTS_PER_BUCKET);
        const ulonglong2 v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];
        if (v0.x == key || v0.y == key || v1.x == key || v1.y == key || v2.x == key || v2.y == key || v3.x == key || v3.y == key) return true;
        if (!(v3.x > v3.y)) return false;
        b = b + 1 == n_buckets ? 0 : b + 1;
    }
    return false;
}

// One wave per pass of TBK_PASS window starts of the separated stream, staged and rolled by LaneWindows (tbk_lookup.h):
// lane l holds the 64 bases from P0 + 32 l on and rolls its 32 windows out of registers.  A clean window asks A's table,
// and B's only if A missed (count_kmers_in_read, c/kmers.c:291-294): two dependent random lines at the most.
// The lane's answers are one word of A-bits and one of B-bits - bit j = the window at P0 + 32 l + j - so the two
// bitmaps are indexed by stream position, a wave writes 256 contiguous bytes of each, and windows over a separator
// or past `total` are clear because the 'N' (or the zero load_chunk reads past the end) is in them.  pass_count gets
// the markers of the pass: the tile counts of the compaction that follows.
__global__ void __launch_bounds__(64)
tbk_track_mark_kernel(const uint8_t *__restrict__ sep, uint64_t total, uint64_t n_passes, int k, const uint64_t *__restrict__ slots_a,
                      uint32_t buckets_a, const uint64_t *__restrict__ slots_b, uint32_t buckets_b, uint32_t *__restrict__ bits_a,
                      uint32_t *__restrict__ bits_b, unsigned long long *__restrict__ pass_count) {
    __shared__ uint64_t stage[TBK_CHUNKS + 2];
    const uint32_t lane = threadIdx.x & 63u;
    LaneWindows win(k);
    for (uint64_t pass = blockIdx.x; pass < n_passes; pass += gridDim.x) {
        const uint64_t P0 = pass * TBK_PASS;
        win.load(stage, sep, P0, total, lane);
        uint32_t word_a = 0, word_b = 0;
#pragma unroll 2
        for (int j = 0; j < TBK_WPL; j++) {
            const uint64_t key = win.key();
            if (win.clean(P0 + (uint64_t)lane * TBK_WPL + (uint64_t)j, total)) {
                if (track_lookup(slots_a, buckets_a, key)) word_a |= 1u << j;
                else if (track_lookup(slots_b, buckets_b, key)) word_b |= 1u << j;
            }
            win.roll();
        }
        bits_a[pass * 64 + lane] = word_a;
        bits_b[pass * 64 + lane] = word_b;
        uint32_t sum = (uint32_t)__popc(word_a | word_b);
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        if (lane == 0) pass_count[pass] = sum;
    }
}

// marks in the batch's own coordinates: byte offsets[r] + w is window w of read r, stream position offsets[r] + r + w.
// One wave per read, like the separation; the bytes of a read's last k - 1 window starts come out 0 with the rest.
__global__ void __launch_bounds__(256)
tbk_track_marks_kernel(const uint32_t *__restrict__ bits_a, const uint32_t *__restrict__ bits_b, const uint64_t *__restrict__ offsets,
                       uint64_t n_reads, uint8_t *__restrict__ marks) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_reads; r += waves) {
        const uint64_t lo = offsets[r], hi = offsets[r + 1];
        for (uint64_t i = lo + lane; i < hi; i += 64) {
            const uint64_t p = i + r;
            const uint32_t a = (bits_a[p >> 5] >> (p & 31u)) & 1u, b = (bits_b[p >> 5] >> (p & 31u)) & 1u;
            marks[i] = (uint8_t)(a | (b << 1));
        }
    }
}

// ---- runs: compact the markers, flag the run heads, compact the heads, close the runs ---------------------------------
// The shape of tbk_kmerdb_unique_table twice over: counts per tile, an exclusive scan of the tile counts (rocPRIM,
// tbk_launch_kmerdb_scan), a scatter that knows where its tile starts.  Every launch is one block per tile (or one
// thread per element) and reads only what an earlier launch finished: no block waits for another.

// A marker: (stream position << 1) | haplotype.  Tile = one pass, counted by the marking kernel; a block's four
// waves take four passes, a lane its own word of each bitmap, and the lanes' places are a prefix sum across the wave.
__global__ void __launch_bounds__(256)
tbk_track_markers_kernel(const uint32_t *__restrict__ bits_a, const uint32_t *__restrict__ bits_b, uint64_t n_passes,
                         const unsigned long long *__restrict__ pass_offsets, uint64_t *__restrict__ markers, uint64_t n_markers) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t pass = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pass >= n_passes) return;
    const uint32_t b = bits_b[pass * 64 + lane];
    uint32_t any = bits_a[pass * 64 + lane] | b;
    const uint32_t mine = (uint32_t)__popc(any);
    uint32_t upto = mine;  // inclusive prefix sum over the lanes
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = __shfl_up(upto, d);
        if (lane >= (uint32_t)d) upto += v;
    }
    uint64_t at = pass_offsets[pass] + (upto - mine);
    const uint64_t p_lane = pass * TBK_PASS + (uint64_t)lane * TBK_WPL;
    while (any) {
        const uint32_t j = (uint32_t)__ffs(any) - 1u;
        if (at < n_markers) markers[at] = ((p_lane + j) << 1) | ((b >> j) & 1u);
        at++;
        any &= any - 1u;
    }
}

constexpr uint32_t TBK_TRK_TILE = 1024;               // markers per tile of the run stage: 4 rounds of a 256-thread block
constexpr uint32_t TBK_TRK_WORDS = TBK_TRK_TILE / 64;  // flag words per tile

// Marker i starts a run if it is the first, if its haplotype is not the previous marker's, or if it lies in another
// read.  A lane takes its predecessor's marker and read from the lane below; lane 0 of a round bisects for marker
// i - 1 itself.  Bit j of flag word w: marker 64 w + j is a head.
__global__ void __launch_bounds__(256)
tbk_track_heads_kernel(const uint64_t *__restrict__ markers, uint64_t n_markers, const uint64_t *__restrict__ offsets, uint64_t n_reads,
                       uint64_t *__restrict__ flags, unsigned long long *__restrict__ tile_counts) {
    __shared__ uint32_t tile_sum;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t tile = blockIdx.x;
    if (threadIdx.x == 0) tile_sum = 0;
    __syncthreads();
    uint32_t mine = 0;  // (the same in every lane of a wave)
    for (uint32_t r = 0; r < TBK_TRK_TILE / 256; r++) {
        const uint32_t word = r * 4 + wave;
        const uint64_t i = tile * TBK_TRK_TILE + (uint64_t)word * 64 + lane;
        unsigned long long m = 0, read = 0;
        if (i < n_markers) {
            m = markers[i];
            read = read_of_position(offsets, n_reads, m >> 1);
        }
        unsigned long long pm = __shfl_up(m, 1), pread = __shfl_up(read, 1);
        bool head = false;
        if (i < n_markers) {
            if (lane == 0 && i > 0) {
                pm = markers[i - 1];
                pread = read_of_position(offsets, n_reads, pm >> 1);
            }
            head = i == 0 || ((pm ^ m) & 1ull) || pread != read;
        }
        const uint64_t mask = __builtin_amdgcn_ballot_w64(head);
        if (lane == 0) flags[tile * TBK_TRK_WORDS + word] = mask;
        mine += (uint32_t)__popcll(mask);
    }
    if (lane == 0 && mine) atomicAdd(&tile_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0) tile_counts[tile] = tile_sum;
}

// Head marker i becomes run tile_offsets[its tile] + the heads before it in the tile: read, first window and
// haplotype are the head's; head_index keeps i so that the next launch can close the run.
__global__ void __launch_bounds__(256)
tbk_track_runs_kernel(const uint64_t *__restrict__ markers, uint64_t n_markers, const uint64_t *__restrict__ offsets, uint64_t n_reads,
                      const uint64_t *__restrict__ flags, const unsigned long long *__restrict__ tile_offsets, tbk_hit_run *__restrict__ runs,
                      uint64_t *__restrict__ head_index, uint64_t n_runs) {
    __shared__ uint64_t word_mask[TBK_TRK_WORDS];
    __shared__ uint32_t word_before[TBK_TRK_WORDS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t tile = blockIdx.x;
    if (threadIdx.x < TBK_TRK_WORDS) word_mask[threadIdx.x] = flags[tile * TBK_TRK_WORDS + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < TBK_TRK_WORDS; w++) {
            word_before[w] = sum;
            sum += (uint32_t)__popcll(word_mask[w]);
        }
    }
    __syncthreads();
    const uint64_t base = tile_offsets[tile];
    for (uint32_t r = 0; r < TBK_TRK_TILE / 256; r++) {
        const uint32_t word = r * 4 + wave;
        const uint64_t mask = word_mask[word];
        const uint64_t i = tile * TBK_TRK_TILE + (uint64_t)word * 64 + lane;
        if (((mask >> lane) & 1ull) && i < n_markers) {
            const uint64_t at = base + word_before[word] + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (at < n_runs) {
                const uint64_t m = markers[i], p = m >> 1;
                const uint64_t read = read_of_position(offsets, n_reads, p);
                tbk_hit_run run;
                run.read = read;
                run.first = p - (offsets[read] + read);
                run.last = run.first;
                run.markers = 0;
                run.hap = (uint32_t)(m & 1ull);
                runs[at] = run;
                head_index[at] = i;
            }
        }
    }
}

// Run j ends at the marker before the next run's head (the last run at the last marker).  The per-read totals are
// the runs' marker counts added up: one atomic per run, from the markers themselves and not from a second probe.
__global__ void __launch_bounds__(256)
tbk_track_close_kernel(const uint64_t *__restrict__ markers, uint64_t n_markers, const uint64_t *__restrict__ offsets,
                       const uint64_t *__restrict__ head_index, tbk_hit_run *__restrict__ runs, uint64_t n_runs, int32_t *__restrict__ counts) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_runs) return;
    const uint64_t end = j + 1 < n_runs ? head_index[j + 1] : n_markers;  // one past the run's last marker
    const uint64_t read = runs[j].read;
    const uint32_t n = (uint32_t)(end - head_index[j]);
    runs[j].last = (markers[end - 1] >> 1) - (offsets[read] + read);
    runs[j].markers = n;
    if (counts) atomicAdd(&counts[2 * read + runs[j].hap], (int32_t)n);
}

// ---- runs found in homopolymer-compressed space, in the coordinates of the batch as given ----------------------------
// The runs above are those of the compressed batch (offsets coff).  The three endpoints of run j as positions of the
// compressed stream - the first byte of its first and of its last marker's window, and the end of that last window -
// go to positions[3 j ..]; tbk_hpc_lift_kernel (tbk_hpc.hip) turns them into positions of the batch as given.  The
// window's end is at most coff[read + 1], which lifts to the next read's start: the read's length.
__global__ void __launch_bounds__(256)
tbk_track_endpoints_kernel(const tbk_hit_run *__restrict__ runs, uint64_t n_runs, const uint64_t *__restrict__ coff, int k,
                           uint64_t *__restrict__ positions) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_runs) return;
    const uint64_t base = coff[runs[j].read];
    positions[3 * j] = base + runs[j].first;
    positions[3 * j + 1] = base + runs[j].last;
    positions[3 * j + 2] = base + runs[j].last + (uint64_t)k;
}

// Run j with its lifted endpoints, relative to its read as given (offsets: the batch's own).
__global__ void __launch_bounds__(256)
tbk_track_lifted_kernel(const tbk_hit_run *__restrict__ runs, uint64_t n_runs, const uint64_t *__restrict__ offsets,
                        const uint64_t *__restrict__ lifted_at, tbk_hit_run_lifted *__restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_runs) return;
    const tbk_hit_run run = runs[j];
    const uint64_t start = offsets[run.read];
    tbk_hit_run_lifted up;
    up.read = run.read;
    up.first = lifted_at[3 * j] - start;
    up.last = lifted_at[3 * j + 1] - start;
    up.end = lifted_at[3 * j + 2] - start;
    up.markers = run.markers;
    up.hap = run.hap;
    out[j] = up;
}

// =======================================================================================
// launchers (called from tbk_host.cpp)
// =======================================================================================
extern "C" uint64_t tbk_track_tiles(uint64_t n_markers) { return (n_markers + TBK_TRK_TILE - 1) / TBK_TRK_TILE; }
extern "C" uint64_t tbk_track_flag_words(uint64_t n_markers) { return tbk_track_tiles(n_markers) * TBK_TRK_WORDS; }

// d_sep: offsets[n_reads] + n_reads bytes.  wave_slots: how many waves the device holds at once (grid-stride over the reads)
extern "C" hipError_t tbk_launch_track_separate(const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, int ignore_case,
                                                uint8_t *d_sep, uint64_t wave_slots, hipStream_t stream) {
    if (!n_reads) return hipSuccess;
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((n_reads + 3) / 4, wave_slots));
    hipLaunchKernelGGL(tbk_track_separate_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_bases, d_offsets, n_reads, ignore_case, d_sep);
    return hipGetLastError();
}

// bitmaps: 64 words per pass each; d_pass_count: one per pass (tbk_probe_passes(total) passes)
extern "C" hipError_t tbk_launch_track_mark(const uint8_t *d_sep, uint64_t total, uint64_t n_passes, int k, const uint64_t *slots_a,
                                            uint32_t buckets_a, const uint64_t *slots_b, uint32_t buckets_b, uint32_t *d_bits_a,
                                            uint32_t *d_bits_b, unsigned long long *d_pass_count, uint64_t wave_slots, hipStream_t stream) {
    if (!n_passes) return hipSuccess;
    if (k < 1 || k > 32 || !buckets_a || !buckets_b) return hipErrorInvalidValue;
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>(n_passes, wave_slots));
    hipLaunchKernelGGL(tbk_track_mark_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, d_sep, total, n_passes, k, slots_a, buckets_a, slots_b,
                       buckets_b, d_bits_a, d_bits_b, d_pass_count);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_track_marks(const uint32_t *d_bits_a, const uint32_t *d_bits_b, const uint64_t *d_offsets, uint64_t n_reads,
                                             uint8_t *d_marks, uint64_t wave_slots, hipStream_t stream) {
    if (!n_reads) return hipSuccess;
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((n_reads + 3) / 4, wave_slots));
    hipLaunchKernelGGL(tbk_track_marks_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_bits_a, d_bits_b, d_offsets, n_reads, d_marks);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_track_markers(const uint32_t *d_bits_a, const uint32_t *d_bits_b, uint64_t n_passes,
                                               const unsigned long long *d_pass_offsets, uint64_t *d_markers, uint64_t n_markers, hipStream_t stream) {
    if (!n_passes || !n_markers) return hipSuccess;
    const uint64_t blocks = (n_passes + 3) / 4;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tbk_track_markers_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_bits_a, d_bits_b, n_passes, d_pass_offsets, d_markers,
                       n_markers);
    return hipGetLastError();
}

// d_flags: tbk_track_flag_words(n_markers) words; d_tile_counts: one per tile
extern "C" hipError_t tbk_launch_track_heads(const uint64_t *d_markers, uint64_t n_markers, const uint64_t *d_offsets, uint64_t n_reads,
                                             uint64_t *d_flags, unsigned long long *d_tile_counts, hipStream_t stream) {
    const uint64_t tiles = tbk_track_tiles(n_markers);
    if (!tiles) return hipSuccess;
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tbk_track_heads_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, d_markers, n_markers, d_offsets, n_reads, d_flags,
                       d_tile_counts);
    return hipGetLastError();
}

// the heads scattered into d_runs (n_runs of them) and closed; d_counts (n_reads x 2, zeroed by the caller) may be NULL
extern "C" hipError_t tbk_launch_track_runs(const uint64_t *d_markers, uint64_t n_markers, const uint64_t *d_offsets, uint64_t n_reads,
                                            const uint64_t *d_flags, const unsigned long long *d_tile_offsets, tbk_hit_run *d_runs,
                                            uint64_t *d_head_index, uint64_t n_runs, int32_t *d_counts, hipStream_t stream) {
    const uint64_t tiles = tbk_track_tiles(n_markers);
    if (!tiles || !n_runs) return hipSuccess;
    const uint64_t close_blocks = (n_runs + 255) / 256;
    if (tiles > 0x7FFFFFFFull || close_blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tbk_track_runs_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, d_markers, n_markers, d_offsets, n_reads, d_flags,
                       d_tile_offsets, d_runs, d_head_index, n_runs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tbk_track_close_kernel, dim3((unsigned)close_blocks), dim3(256), 0, stream, d_markers, n_markers, d_offsets, d_head_index,
                       d_runs, n_runs, d_counts);
    return hipGetLastError();
}

// d_positions: 3 * n_runs stream positions of the compressed batch (offsets d_coff)
extern "C" hipError_t tbk_launch_track_endpoints(const tbk_hit_run *d_runs, uint64_t n_runs, const uint64_t *d_coff, int k, uint64_t *d_positions,
                                                 hipStream_t stream) {
    const uint64_t blocks = (n_runs + 255) / 256;
    if (!n_runs) return hipSuccess;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tbk_track_endpoints_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_runs, n_runs, d_coff, k, d_positions);
    return hipGetLastError();
}

// d_offsets: of the batch as given; d_lifted_at: the 3 * n_runs positions after the lift
extern "C" hipError_t tbk_launch_track_lifted(const tbk_hit_run *d_runs, uint64_t n_runs, const uint64_t *d_offsets, const uint64_t *d_lifted_at,
                                              tbk_hit_run_lifted *d_out, hipStream_t stream) {
    const uint64_t blocks = (n_runs + 255) / 256;
    if (!n_runs) return hipSuccess;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tbk_track_lifted_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_runs, n_runs, d_offsets, d_lifted_at, d_out);
    return hipGetLastError();
}
