// tbk_dump.hip — counted k-mer dumps (`kmc_dump`, `meryl print`, `jellyfish dump -c`: one `KMER<sep>COUNT` line per
// k-mer) turned into the rank/counter pairs of a count database on the GPU, and the selection behind the way back.
//
// The text comes in windows that begin at a line start and end behind a newline (or at the end of a file); the host
// side (tbk_dump_host.cpp) cuts and stages them.  Lines vary in length, so nothing can index them: per window
//   1. tbk_dump_lines_kernel   one block per tile of 4096 bytes, a lane per 16-byte vector: one bit per byte that is a
//                              newline (64 words a tile) and the tile's newline count;
//   2. the exclusive scan of the tile counts (tbk_launch_kmerdb_scan);
//   3. tbk_dump_parse_kernel   a line starts at byte 0 of the window and behind every newline, and its number within
//                              the window is the number of newlines before it: the tile's scanned count plus the
//                              popcounts below the byte.  The lane that holds a line start parses that line from memory
//                              and writes keys[base + number], counts[base + number].  Line starts are never stored.
// A line that breaks the rule (include/tbk.h has it) writes nothing and lowers one 64-bit word to (its global line index
// << 8 | reason) with a vector atomicMin: the smallest index wins, whichever window or tile it lies in.
// After the last window the pairs are checked by tbk_kmerdb_check_kernel; only when they do not ascend strictly are they
// sorted (tbk_launch_sort_u64_u8) and folded here: tbk_dump_flag_kernel<0> flags the first entry of every run of equal keys
// in the layout of tbk_compact.h (bit j of word i is entry 64 i + j, a count per tile of TBK_DBT_TILE), the scan gives
// every tile its place and tbk_dump_fold_kernel writes each head with the saturating sum of its run.
// No block waits for another; the only atomics are the bad-line minimum and block-local counts in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbk_compact.h"

constexpr uint32_t TBK_DUMP_TILE = 4096;                  // bytes per tile: 256 lanes x 16
constexpr uint32_t TBK_DUMP_WORDS = TBK_DUMP_TILE / 64;   // newline words per tile
constexpr uint32_t TBK_DUMP_DIGITS = 32;                  // most digits a counter may have
constexpr uint32_t TBK_DUMP_SLACK = 35;                   // a line is at most k + 35 bytes, its newline not counted

// reasons a line is refused by (tbk_dump_host.cpp has the words; tests/dump_ref.py restates the order they are found in)
enum : uint32_t {
    TBK_DUMP_OK = 0,
    TBK_DUMP_TOO_LONG = 1,
    TBK_DUMP_EMPTY = 2,
    TBK_DUMP_SHORT_KMER = 3,
    TBK_DUMP_NOT_ACGT = 4,
    TBK_DUMP_NO_COUNTER = 5,
    TBK_DUMP_LONG_KMER = 6,
    TBK_DUMP_NO_SEPARATOR = 7,
    TBK_DUMP_EMPTY_COUNTER = 8,
    TBK_DUMP_NOT_DIGITS = 9,
    TBK_DUMP_TOO_MANY_DIGITS = 10,
    TBK_DUMP_ZERO = 11,
    TBK_DUMP_NOT_COMPRESSED = 12,
};

__global__ void __launch_bounds__(256)
tbk_dump_lines_kernel(const uint8_t *__restrict__ text, uint64_t len, uint64_t *__restrict__ nl_bits, unsigned long long *__restrict__ tile_counts) {
    __shared__ uint32_t wave_count[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t tile = blockIdx.x;
    const uint64_t p = tile * TBK_DUMP_TILE + (uint64_t)threadIdx.x * 16;
    uint32_t m = 0;
    if (p < len) {  // (the buffer is readable to the end of its last tile)
        const uint4 v = *reinterpret_cast<const uint4 *>(text + p);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const uint32_t valid = len - p >= 16 ? 16u : (uint32_t)(len - p);
        for (uint32_t j = 0; j < 16; j++)
            if (j < valid && ((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) == (uint32_t)'\n') m |= 1u << j;
    }
    // four lanes make one 64-bit word: byte b of the tile is bit b & 63 of word b >> 6
    const uint64_t m1 = __shfl_down(m, 1), m2 = __shfl_down(m, 2), m3 = __shfl_down(m, 3);
    if ((lane & 3u) == 0) nl_bits[tile * TBK_DUMP_WORDS + (threadIdx.x >> 2)] = (uint64_t)m | (m1 << 16) | (m2 << 32) | (m3 << 48);
    uint32_t c = (uint32_t)__popc(m);
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if (lane == 0) wave_count[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_counts[tile] = (unsigned long long)wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
}

__device__ __forceinline__ uint32_t dump_base_code(uint32_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }

// The line that starts at text[pos] (pos < len).  Returns the reason it is refused by, or TBK_DUMP_OK with its canonical
// k-mer's rank and its counter, saturated at 255.  Reads no byte at or behind len, and at most k + 36 bytes.
__device__ uint32_t dump_parse_line(const uint8_t *__restrict__ text, uint64_t len, uint64_t pos, uint32_t k, int compressed, uint64_t *key,
                                    uint32_t *count) {
    const uint8_t *p = text + pos;
    const uint64_t room = len - pos;
    const uint32_t span = room < (uint64_t)(k + TBK_DUMP_SLACK + 1) ? (uint32_t)room : k + TBK_DUMP_SLACK + 1;
    uint32_t L = 0;  // the line's bytes without its newline; the text's last line may have none
    while (L < span && p[L] != '\n') L++;
    if (L == span && (uint64_t)span < room) return TBK_DUMP_TOO_LONG;
    if (L > k + TBK_DUMP_SLACK) return TBK_DUMP_TOO_LONG;
    if (L == 0) return TBK_DUMP_EMPTY;
    uint64_t fwd = 0, rc = 0;
    uint32_t last = 4;
    bool runs = false;
    const uint32_t nb = L < k ? L : k;
    for (uint32_t i = 0; i < nb; i++) {
        const uint32_t c = p[i];
        const uint32_t code = dump_base_code(c);
        if (code > 3u) return (c == '\t' || c == ' ') ? TBK_DUMP_SHORT_KMER : TBK_DUMP_NOT_ACGT;
        runs = runs || code == last;
        last = code;
        fwd = (fwd << 2) | code;
        rc = (rc >> 2) | ((uint64_t)(3u - code) << (2 * (k - 1)));
    }
    if (L < k) return TBK_DUMP_SHORT_KMER;
    if (L == k) return TBK_DUMP_NO_COUNTER;
    const uint32_t sep = p[k];
    if (sep != '\t' && sep != ' ') return dump_base_code(sep) <= 3u ? TBK_DUMP_LONG_KMER : TBK_DUMP_NO_SEPARATOR;
    const uint32_t digits = L - k - 1;
    if (digits == 0) return TBK_DUMP_EMPTY_COUNTER;
    uint32_t v = 0;
    for (uint32_t i = 0; i < digits; i++) {
        const uint32_t d = (uint32_t)p[k + 1 + i] - (uint32_t)'0';
        if (d > 9u) return TBK_DUMP_NOT_DIGITS;
        v = v * 10u + d;
        if (v > 1000u) v = 1000u;  // (saturated: anything above 255 is 255)
    }
    if (digits > TBK_DUMP_DIGITS) return TBK_DUMP_TOO_MANY_DIGITS;
    if (v == 0) return TBK_DUMP_ZERO;
    if (compressed && runs) return TBK_DUMP_NOT_COMPRESSED;
    *key = fwd < rc ? fwd : rc;  // (unsigned: k = 32 uses bit 63)
    *count = v > 255u ? 255u : v;
    return TBK_DUMP_OK;
}

// tile_offsets: the scanned newline counts of the window's tiles.  base: lines before this window, over all windows - the
// global index of its first line and the place of that line's pair.  capacity: pairs the arrays hold.
__global__ void __launch_bounds__(256)
tbk_dump_parse_kernel(const uint8_t *__restrict__ text, uint64_t len, const uint64_t *__restrict__ nl_bits,
                      const unsigned long long *__restrict__ tile_offsets, uint32_t k, int compressed, uint64_t base, uint64_t capacity,
                      uint64_t *__restrict__ keys, uint8_t *__restrict__ counts, unsigned long long *__restrict__ bad) {
    __shared__ uint64_t word[TBK_DUMP_WORDS + 1];  // word[1 + i]: the tile's newline word i; word[0]: the word before the tile
    __shared__ uint32_t before[TBK_DUMP_WORDS];    // newlines of the tile below word i
    const uint64_t tile = blockIdx.x;
    if (threadIdx.x < TBK_DUMP_WORDS) word[1 + threadIdx.x] = nl_bits[tile * TBK_DUMP_WORDS + threadIdx.x];
    if (threadIdx.x == TBK_DUMP_WORDS) word[0] = tile ? nl_bits[tile * TBK_DUMP_WORDS - 1] : 1ull << 63;  // (byte 0 of a window starts a line)
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < TBK_DUMP_WORDS; w++) {
            before[w] = sum;
            sum += (uint32_t)__popcll(word[1 + w]);
        }
    }
    __syncthreads();
    const uint32_t q = threadIdx.x * 16, wi = q >> 6, shift = q & 63u;
    const uint64_t p0 = tile * TBK_DUMP_TILE + q;
    if (p0 >= len) return;
    const uint64_t nl = word[1 + wi];
    const uint32_t prev = shift ? (uint32_t)(nl >> (shift - 1)) & 1u : (uint32_t)(word[wi] >> 63);
    uint32_t starts = ((((uint32_t)(nl >> shift) & 0xFFFFu) << 1) | prev) & 0xFFFFu;  // bit j: byte p0 + j follows a newline
    const uint64_t tile_base = base + tile_offsets[tile] + before[wi];
    while (starts) {
        const uint32_t j = (uint32_t)__builtin_ctz(starts);
        starts &= starts - 1;
        const uint64_t pos = p0 + j;
        if (pos >= len) break;  // (the window's last newline starts no line)
        const uint64_t line = tile_base + (uint64_t)__popcll(nl & ((1ull << (shift + j)) - 1ull));
        uint64_t key = 0;
        uint32_t count = 0;
        const uint32_t reason = dump_parse_line(text, len, pos, k, compressed, &key, &count);
        if (reason != TBK_DUMP_OK) {
            atomicMin(bad, (unsigned long long)((line << 8) | reason));
        } else if (line < capacity) {
            keys[line] = key;
            counts[line] = (uint8_t)count;
        }
    }
}

// ---- flags over entries: the tile compaction of tbk_compact.h ---------------------------------------------------------------
// MODE 0: entry i is the head of a run of equal keys.  MODE 1: its counter lies in [lo, hi].
template <int MODE>
__global__ void __launch_bounds__(256)
tbk_dump_flag_kernel(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ counts, uint64_t n, uint32_t lo, uint32_t hi,
                     uint64_t *__restrict__ flags, unsigned long long *__restrict__ tile_counts) {
    compact_flag_tile(n, flags, tile_counts, [=](uint64_t i) {
        if (MODE == 0) return i == 0 || keys[i] != keys[i - 1];
        const uint32_t c = counts[i];
        return c >= lo && c <= hi;
    });
}

// Every head to its place with min(255, sum of its run's counters): the head's lane walks forward and stops at 255, and
// every counter is at least 1, so a run costs at most 255 steps however long it is.
__global__ void __launch_bounds__(256)
tbk_dump_fold_kernel(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ counts, uint64_t n, const uint64_t *__restrict__ flags,
                     const unsigned long long *__restrict__ tile_offsets, uint64_t *__restrict__ out_keys, uint8_t *__restrict__ out_counts,
                     uint64_t n_out) {
    compact_scatter_tile(n, flags, tile_offsets, [=](uint64_t i, uint64_t at) {
        const uint64_t key = keys[i];
        uint32_t sum = counts[i];
        for (uint64_t j = i + 1; sum < 255u && j < n && keys[j] == key; j++) sum += counts[j];
        if (at < n_out) {
            out_keys[at] = key;
            out_counts[at] = (uint8_t)(sum > 255u ? 255u : sum);
        }
    });
}

// =======================================================================================
// launchers (called from tbk_dump_host.cpp)
// =======================================================================================
extern "C" uint32_t tbk_dump_tile(void) { return TBK_DUMP_TILE; }

// d_text readable to the end of the last tile; d_nl_bits: 64 words per tile; d_tile_counts: one per tile
extern "C" hipError_t tbk_launch_dump_lines(const uint8_t *d_text, uint64_t len, uint64_t *d_nl_bits, unsigned long long *d_tile_counts, hipStream_t stream) {
    const uint64_t tiles = (len + TBK_DUMP_TILE - 1) / TBK_DUMP_TILE;
    if (!tiles) return hipSuccess;
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tbk_dump_lines_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, d_text, len, d_nl_bits, d_tile_counts);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_dump_parse(const uint8_t *d_text, uint64_t len, const uint64_t *d_nl_bits, const unsigned long long *d_tile_offsets, int k,
                                            int compressed, uint64_t base, uint64_t capacity, uint64_t *d_keys, uint8_t *d_counts,
                                            unsigned long long *d_bad, hipStream_t stream) {
    const uint64_t tiles = (len + TBK_DUMP_TILE - 1) / TBK_DUMP_TILE;
    if (!tiles) return hipSuccess;
    if (tiles > 0x7FFFFFFFull || k < 1 || k > 32) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tbk_dump_parse_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, d_text, len, d_nl_bits, d_tile_offsets, (uint32_t)k, compressed, base,
                       capacity, d_keys, d_counts, d_bad);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_dump_heads(const uint64_t *d_keys, uint64_t n, uint64_t *d_flags, unsigned long long *d_tile_counts, hipStream_t stream) {
    return compact_launch_tiles(n, stream, tbk_dump_flag_kernel<0>, d_keys, (const uint8_t *)nullptr, n, 0u, 0u, d_flags, d_tile_counts);
}

extern "C" hipError_t tbk_launch_dump_select(const uint8_t *d_counts, uint64_t n, uint32_t lo, uint32_t hi, uint64_t *d_flags,
                                             unsigned long long *d_tile_counts, hipStream_t stream) {
    return compact_launch_tiles(n, stream, tbk_dump_flag_kernel<1>, (const uint64_t *)nullptr, d_counts, n, lo, hi, d_flags, d_tile_counts);
}

extern "C" hipError_t tbk_launch_dump_fold(const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, const uint64_t *d_flags,
                                           const unsigned long long *d_tile_offsets, uint64_t *d_out_keys, uint8_t *d_out_counts, uint64_t n_out,
                                           hipStream_t stream) {
    if (!n_out) return hipSuccess;
    return compact_launch_tiles(n, stream, tbk_dump_fold_kernel, d_keys, d_counts, n, d_flags, d_tile_offsets, d_out_keys, d_out_counts, n_out);
}
