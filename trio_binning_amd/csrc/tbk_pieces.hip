// tbk_pieces.hip — the MI355X kernels of a query session's read pieces (tbk_kmerdb_query_pieces): the maximal runs of covered
// - or of uncovered - positions of every sequence of a batch, as an ordered list of intervals.  The lookup pass and the
// evidence kernel are tbk_screen.hip's; what is here turns the held bitmap into the side bitmap, compacts the runs' starts
// and ends into records (tbk_compact.h) and filters the records by length and by "the longest of its read".  Every kernel works
// over the stream's bitmap words or over the list, never a wave per sequence, so a batch of short reads leaves no lane idle.
// None writes any state of the session.  Host side: tbk_count.cpp; the rule: include/tbk.h, "read pieces".
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/tbk.h"
#include "tbk_common.h"
#include "tbk_compact.h"
#include "tbk_lookup.h"

static_assert(sizeof(tbk_read_piece) == 24, "a record is three 64-bit words: read, first, end");

// The kernels that stride over words, sequences or records: one-wave blocks, as many as the device holds waves at most - a
// second trip of their loops from 64 wave_slots + 1 items on.
static unsigned pieces_grid(uint64_t n, uint64_t wave_slots) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>((n + 63) / 64, wave_slots), 0x7FFFFFFFull));
}

// ---- the side bitmap --------------------------------------------------------------------------------------------------------------
// The separator behind sequence r lies at stream position offsets[r + 1] + r: one bit each into the zeroed words, so that the
// uncovered side can leave them out and no piece joins two sequences.  Neighbouring short reads share a word: a vector atomic.
__global__ void __launch_bounds__(64)
tbk_pieces_separators_kernel(const uint64_t *__restrict__ offsets, uint64_t n_reads, uint32_t *__restrict__ side) {
    const uint64_t step = (uint64_t)gridDim.x * 64;
    for (uint64_t r = (uint64_t)blockIdx.x * 64 + threadIdx.x; r < n_reads; r += step) {
        const uint64_t p = offsets[r + 1] + r;
        atomicOr(&side[p >> 5], 1u << (p & 31u));
    }
}

// Word w of the side bitmap from the held words w and w - 1 (covered_word, tbk_lookup.h).  The covered side is the covered
// word as it is: coverage ends at a sequence's last base (include/tbk.h, "read evidence").  The uncovered side is its
// complement without the separators - the word holds them on entry - and without the positions from `total` on.
__global__ void __launch_bounds__(64)
tbk_pieces_side_kernel(const uint32_t *__restrict__ held, uint64_t n_words, uint64_t total, int k, int uncovered, uint32_t *__restrict__ side) {
    const uint64_t step = (uint64_t)gridDim.x * 64;
    for (uint64_t w = (uint64_t)blockIdx.x * 64 + threadIdx.x; w < n_words; w += step) {
        const uint32_t cov = covered_word(held[w], held[w ? w - 1 : 0] & (w ? 0xFFFFFFFFu : 0u), k);
        uint32_t out = cov;
        if (uncovered) {
            const uint64_t p0 = w * 32;
            const uint32_t inside = total <= p0 ? 0u : total - p0 >= 32 ? 0xFFFFFFFFu : (1u << (uint32_t)(total - p0)) - 1u;
            out = ~cov & ~side[w] & inside;
        }
        side[w] = out;
    }
}

// ---- the runs: flag the starts and the last positions, scan (the host), scatter them into records ----------------------------------
// Bit p of the side bitmap, read as 64-bit words, is stream position p.  A separator is on neither side, so a run of bits lies
// inside one sequence, and the i-th start and the i-th last position in stream order are the same run's.
__device__ __forceinline__ bool pieces_bit(const uint64_t *__restrict__ bits, uint64_t p) { return (bits[p >> 6] >> (p & 63u)) & 1ull; }

// n = 2048 positions per pass
template <bool END>
__global__ void __launch_bounds__(256)
tbk_pieces_flag_kernel(const uint64_t *__restrict__ side, uint64_t n, uint64_t *__restrict__ flags, unsigned long long *__restrict__ tile_counts) {
    compact_flag_tile(n, flags, tile_counts, [&](uint64_t p) {
        if (!pieces_bit(side, p)) return false;
        return END ? !(p + 1 < n && pieces_bit(side, p + 1)) : !(p && pieces_bit(side, p - 1));
    });
}

// the i-th last position p: record i ends at stream position p + 1, until the starts bring it into its read's coordinates
__global__ void __launch_bounds__(256)
tbk_pieces_ends_kernel(uint64_t n, const uint64_t *__restrict__ flags, const unsigned long long *__restrict__ tile_offsets, uint64_t *__restrict__ records,
                       uint64_t n_records) {
    compact_scatter_tile(n, flags, tile_offsets, [&](uint64_t p, uint64_t at) {
        if (at < n_records) records[3 * at + 2] = p + 1;
    });
}

// The i-th start p becomes record i, so the records are ordered by (read, first).  The starts are dealt to consecutive threads:
// each bisects for its read (read_of_position, tbk_lookup.h).
__global__ void __launch_bounds__(256)
tbk_pieces_starts_kernel(uint64_t n, const uint64_t *__restrict__ offsets, uint64_t n_reads, const uint64_t *__restrict__ flags,
                         const unsigned long long *__restrict__ tile_offsets, uint64_t *__restrict__ records, uint64_t n_records) {
    compact_scatter_tile_dense(n, flags, tile_offsets, [&](uint64_t p, uint64_t at) {
        if (at >= n_records) return;
        const uint64_t read = read_of_position(offsets, n_reads, p);
        const uint64_t base = offsets[read] + read;
        records[3 * at] = read;
        records[3 * at + 1] = p - base;
        records[3 * at + 2] -= base;
    });
}

// ---- min_length and the longest of a read ------------------------------------------------------------------------------------------
// A piece's key orders a read's pieces by length and, among equals, by the smaller first: no sequence has 2^32 bases (the host
// refuses it), so both halves fit, and a piece's key is never 0.
__device__ __forceinline__ unsigned long long pieces_key(uint64_t first, uint64_t end) { return ((end - first) << 32) | (0xFFFFFFFFull - first); }

// keys[read] = the largest key among the read's pieces of min_length or more; the words are zeroed by the host
__global__ void __launch_bounds__(64)
tbk_pieces_best_kernel(const uint64_t *__restrict__ records, uint64_t n_records, uint64_t min_length, unsigned long long *__restrict__ keys) {
    const uint64_t step = (uint64_t)gridDim.x * 64;
    for (uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x; i < n_records; i += step) {
        const uint64_t read = records[3 * i], first = records[3 * i + 1], end = records[3 * i + 2];
        if (end - first >= min_length) atomicMax(&keys[read], pieces_key(first, end));
    }
}

__global__ void __launch_bounds__(256)
tbk_pieces_keep_flag_kernel(const uint64_t *__restrict__ records, uint64_t n_records, uint64_t min_length, const unsigned long long *__restrict__ keys,
                            uint64_t *__restrict__ flags, unsigned long long *__restrict__ tile_counts) {
    compact_flag_tile(n_records, flags, tile_counts, [&](uint64_t i) {
        const uint64_t read = records[3 * i], first = records[3 * i + 1], end = records[3 * i + 2];
        if (end - first < min_length) return false;
        return !keys || keys[read] == pieces_key(first, end);
    });
}

__global__ void __launch_bounds__(256)
tbk_pieces_keep_kernel(const uint64_t *__restrict__ records, uint64_t n_records, const uint64_t *__restrict__ flags,
                       const unsigned long long *__restrict__ tile_offsets, uint64_t *__restrict__ out, uint64_t n_out) {
    compact_scatter_tile(n_records, flags, tile_offsets, [&](uint64_t i, uint64_t at) {
        if (at >= n_out) return;
        out[3 * at] = records[3 * i];
        out[3 * at + 1] = records[3 * i + 1];
        out[3 * at + 2] = records[3 * i + 2];
    });
}

// =======================================================================================
// launchers (called from tbk_count.cpp; what the arguments hold: tbk_lookup_host.h)
// =======================================================================================
extern "C" hipError_t tbk_launch_pieces_side(const uint32_t *d_held, const uint64_t *d_offsets, uint64_t n_reads, uint64_t total, uint64_t n_passes, int k,
                                             int uncovered, uint32_t *d_side, uint64_t wave_slots, hipStream_t stream) {
    if (!n_passes) return hipSuccess;
    if (k < 1 || k > 32 || total > n_passes * TBK_PASS) return hipErrorInvalidValue;
    if (uncovered && n_reads) {
        hipLaunchKernelGGL(tbk_pieces_separators_kernel, dim3(pieces_grid(n_reads, wave_slots)), dim3(64), 0, stream, d_offsets, n_reads, d_side);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const uint64_t n_words = n_passes * 64;
    hipLaunchKernelGGL(tbk_pieces_side_kernel, dim3(pieces_grid(n_words, wave_slots)), dim3(64), 0, stream, d_held, n_words, total, k, uncovered, d_side);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_pieces_flag(const uint32_t *d_side, uint64_t n_passes, int end, uint64_t *d_flags, unsigned long long *d_tile_counts,
                                             hipStream_t stream) {
    const uint64_t n = n_passes * TBK_PASS;
    const uint64_t *side = reinterpret_cast<const uint64_t *>(d_side);
    return end ? compact_launch_tiles(n, stream, tbk_pieces_flag_kernel<true>, side, n, d_flags, d_tile_counts)
               : compact_launch_tiles(n, stream, tbk_pieces_flag_kernel<false>, side, n, d_flags, d_tile_counts);
}

extern "C" hipError_t tbk_launch_pieces_ends(uint64_t n_passes, const uint64_t *d_flags, const unsigned long long *d_tile_offsets, tbk_read_piece *d_pieces,
                                             uint64_t n_pieces, hipStream_t stream) {
    if (!n_pieces) return hipSuccess;
    return compact_launch_tiles(n_passes * TBK_PASS, stream, tbk_pieces_ends_kernel, n_passes * TBK_PASS, d_flags, d_tile_offsets,
                                reinterpret_cast<uint64_t *>(d_pieces), n_pieces);
}

extern "C" hipError_t tbk_launch_pieces_starts(uint64_t n_passes, const uint64_t *d_offsets, uint64_t n_reads, const uint64_t *d_flags,
                                               const unsigned long long *d_tile_offsets, tbk_read_piece *d_pieces, uint64_t n_pieces,
                                               hipStream_t stream) {
    if (!n_pieces) return hipSuccess;
    if (!n_reads) return hipErrorInvalidValue;
    return compact_launch_tiles(n_passes * TBK_PASS, stream, tbk_pieces_starts_kernel, n_passes * TBK_PASS, d_offsets, n_reads, d_flags, d_tile_offsets,
                                reinterpret_cast<uint64_t *>(d_pieces), n_pieces);
}

extern "C" hipError_t tbk_launch_pieces_best(const tbk_read_piece *d_pieces, uint64_t n_pieces, uint64_t min_length, unsigned long long *d_keys,
                                             uint64_t wave_slots, hipStream_t stream) {
    if (!n_pieces) return hipSuccess;
    hipLaunchKernelGGL(tbk_pieces_best_kernel, dim3(pieces_grid(n_pieces, wave_slots)), dim3(64), 0, stream, reinterpret_cast<const uint64_t *>(d_pieces),
                       n_pieces, min_length, d_keys);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_pieces_keep_flag(const tbk_read_piece *d_pieces, uint64_t n_pieces, uint64_t min_length, const unsigned long long *d_keys,
                                                  uint64_t *d_flags, unsigned long long *d_tile_counts, hipStream_t stream) {
    return compact_launch_tiles(n_pieces, stream, tbk_pieces_keep_flag_kernel, reinterpret_cast<const uint64_t *>(d_pieces), n_pieces, min_length, d_keys,
                                d_flags, d_tile_counts);
}

extern "C" hipError_t tbk_launch_pieces_keep(const tbk_read_piece *d_pieces, uint64_t n_pieces, const uint64_t *d_flags,
                                             const unsigned long long *d_tile_offsets, tbk_read_piece *d_out, uint64_t n_out, hipStream_t stream) {
    if (!n_out) return hipSuccess;
    return compact_launch_tiles(n_pieces, stream, tbk_pieces_keep_kernel, reinterpret_cast<const uint64_t *>(d_pieces), n_pieces, d_flags, d_tile_offsets,
                                reinterpret_cast<uint64_t *>(d_out), n_out);
}
