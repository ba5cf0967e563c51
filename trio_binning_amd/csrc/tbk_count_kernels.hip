// tbk_count_kernels.hip — the MI355X kernels of the find-unique-kmers step: k-mer counting
// into a table in HBM, its histogram, the A-minus-B selection.  Host side: tbk_count.cpp.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>

#include <type_traits>

#include "tbk_common.h"
#include "tbk_compact.h"
#include "tbk_device.h"

// =======================================================================================
// k-mer counting (the find-unique-kmers step)
// =======================================================================================
// The reference shells out to KMC (find_unique_kmers.py:62-233): count canonical k-mers of a read
// set, keep those seen at least twice (kmc's default -ci2), cap counters at 255 (-cs255), take a
// histogram, subtract the other parent's database and dump the k-mers whose counter lies between
// two cut-offs.  Here the database is a table in HBM: 64-byte lines of 8 keys with a parallel
// array of 32-bit counters, bucket chosen like the classifier's (minimizer of the k-mer, so the
// consecutive windows of a read update the same line while it sits in L2), probe sequence
// tbk_next_bucket.

// (test hook, not in tbk.h: caps on the grids of this file's strided launches, so that a small input takes the later trips of
// their loops.  stream_blocks holds the launches that stride over reads, chunks or passes - separate, retain, both count
// launches - and entry_blocks those that stride over table slots, database entries or a database's tiles (tbk_compare.hip,
// through tbk_count_entry_grid_); 0 = no cap, the state at load.  The
// tile-per-block launches of tbk_compact.h and the rocPRIM scan and sorts take no cap.  Plain globals, read at every launch of
// the process: for a single-threaded test that puts (0, 0) back.)
static uint32_t g_stream_blocks = 0, g_entry_blocks = 0;
extern "C" int tbk_count_set_grid_caps_(uint32_t stream_blocks, uint32_t entry_blocks) {
    g_stream_blocks = stream_blocks;
    g_entry_blocks = entry_blocks;
    return 0;
}
static inline unsigned stream_grid(uint64_t blocks) { return (unsigned)(g_stream_blocks && blocks > g_stream_blocks ? g_stream_blocks : blocks); }
static inline unsigned entry_grid(uint64_t blocks) { return (unsigned)(g_entry_blocks && blocks > g_entry_blocks ? g_entry_blocks : blocks); }
// (the same cap for the launches of tbk_compare.hip, which stride over a database's tiles)
extern "C" unsigned tbk_count_entry_grid_(uint64_t blocks) { return entry_grid(blocks); }

// Copy reads that lie back to back into a stream where every read is followed by one 'N', upper-
// casing on the way (KMC counts lower-case bases like upper-case ones): a window can then never
// span two reads and validity is the not-ACGT mask alone.  One wave per read.
__global__ void __launch_bounds__(256)
tbk_separate_kernel(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ offsets, uint64_t n_reads,
                    uint8_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_reads; r += waves) {
        const uint64_t lo = offsets[r], hi = offsets[r + 1];
        uint8_t *dst = out + lo + r;
        for (uint64_t i = lo + lane; i < hi; i += 64) dst[i - lo] = bases[i] & 0xDFu;
        if (lane == 0) dst[hi - lo] = 'N';
    }
}

// Pass mode keeps every batch on the device in the form the counting kernel stages: one 64-bit word per 16
// bases of the separated stream, 32 bits of 2-bit codes and the 16-bit not-ACGT mask above them (load_chunk's
// value; 0.5 bytes per base).  A batch takes whole words: the positions of its last word past its end carry the
// bad bit (load_chunk reads them as 0), so no window spans two batches.
__global__ void __launch_bounds__(256)
tbk_retain_kernel(const uint8_t *__restrict__ sep, uint64_t total, uint64_t *__restrict__ store, uint64_t n_chunks) {
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks; c += (uint64_t)gridDim.x * blockDim.x)
        store[c] = load_chunk(sep, c * 16, total);
}

// The class a pass-mode launch counts: windows whose canonical k-mer has tbk_class_of(key, n_classes) == cls.
struct TbkClassSel {
    uint32_t n_classes, cls;
};

// bucket b = one 128-byte line: 8 keys (TBK_EMPTY = free), then their 8 32-bit counters, then 32
// spare bytes - keys and counters of a bucket arrive with one HBM line and the increments of a run
// of windows land in a line that already sits in L2
constexpr int TBK_COUNT_LINE = 16;  // uint64 words per bucket line
struct TbkCountView {
    uint64_t *lines;    // n_buckets * 16 words
    uint32_t n_buckets;
    TbkMz mz;
    __device__ __forceinline__ unsigned long long *keys(uint32_t b) const { return (unsigned long long *)(lines + (uint64_t)b * TBK_COUNT_LINE); }
    __device__ __forceinline__ uint32_t *counts(uint32_t b) const { return (uint32_t *)(lines + (uint64_t)b * TBK_COUNT_LINE + TBK_SLOTS_PER_BUCKET); }
};

// A probe sequence longer than this means the table is as good as full (the host grows the table
// long before: tbk_count.cpp); giving up keeps a mis-sized table from turning into an endless walk.
constexpr uint32_t TBK_COUNT_MAX_WALK = 1u << 12;

// find or claim the key's slot along its probe sequence, from bucket b on, and add `n` occurrences;
// `claimed` counts the slots newly taken
__device__ __forceinline__ bool count_from(const TbkCountView &t, uint64_t key, uint32_t b, bool at_home, uint32_t n, uint32_t &claimed) {
    for (uint32_t walked = 0; walked <= t.n_buckets && walked < TBK_COUNT_MAX_WALK; walked++) {
        unsigned long long *line = t.keys(b);
        for (int s = 0; s < TBK_SLOTS_PER_BUCKET; s++) {
            unsigned long long cur = __hip_atomic_load(&line[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == TBK_EMPTY) {
                cur = atomicCAS(&line[s], (unsigned long long)TBK_EMPTY, (unsigned long long)key);
                if (cur == TBK_EMPTY) { cur = key; claimed++; }
            }
            if (cur == key) { atomicAdd(&t.counts(b)[s], n); return true; }
        }
        b = tbk_next_bucket(key, t.mz, t.n_buckets, b, at_home && walked == 0);
    }
    return false;
}

// One wave per pass of 2048 window starts of the separated stream, staged and rolled like the probe
// kernel's; every clean window counts its canonical k-mer.  A lane keeps the 8 keys of the bucket
// of its previous window in registers: consecutive windows mostly share their minimizer, so the
// line is fetched once per run and a window costs its compares and one fire-and-forget atomic add.
// The copy may be stale - other lanes insert meanwhile - but only in one direction: a slot seen
// occupied never changes, and a slot seen free is claimed with a compare-and-swap that returns what
// is really there.
//
// Pass mode (tbk_count.cpp) instantiates the kernel with a TbkClassSel as one more argument: `bases` is then the
// retained store of a batch (tbk_retain_kernel; `total` = 16 x its words), staged with plain 8-byte loads, and a
// clean window counts only if its k-mer belongs to the class.  The plain instantiations have no such argument.
template <int W, bool M64, typename... Sel>
__global__ void __launch_bounds__(64)
tbk_count_kernel(const uint8_t *__restrict__ bases, uint64_t total, uint64_t first_pass, uint64_t n_passes, int k, TbkCountView t,
                 int *__restrict__ failed, unsigned long long *__restrict__ used, Sel... sel) {
    static_assert(sizeof...(Sel) == 0 || (sizeof...(Sel) == 1 && (std::is_same<Sel, TbkClassSel>::value && ...)), "at most one class selector");
    constexpr bool PACKED = sizeof...(Sel) == 1;
    __shared__ uint64_t stage[TBK_CHUNKS + 2];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t kmask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1ull);
    const uint32_t badk = k == 32 ? 0xFFFFFFFFu : ((1u << k) - 1u);
    using win_t = typename std::conditional<M64, uint64_t, uint32_t>::type;
    const int m = t.mz.m, o = t.mz.o;
    const uint64_t mmask = m >= 32 ? ~0ull : ((1ull << (2 * m)) - 1ull);
    auto mmer_order = [&](uint64_t fwd64, uint64_t rc64, uint32_t fsh, uint32_t bsh) -> win_t {
        if (M64) {
            const uint64_t x = (fwd64 >> fsh) & mmask, y = (rc64 >> bsh) & mmask;
            return (win_t)tbk_mmer_hash64(x < y ? x : y);
        }
        const uint32_t x = (uint32_t)(fwd64 >> fsh) & (uint32_t)mmask, y = (uint32_t)(rc64 >> bsh) & (uint32_t)mmask;
        return (win_t)tbk_mmer_hash(x < y ? x : y);
    };
    for (uint64_t pass = first_pass + blockIdx.x; pass < first_pass + n_passes; pass += gridDim.x) {
        const uint64_t P0 = pass * TBK_PASS;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if constexpr (PACKED) {
            const uint64_t *store = reinterpret_cast<const uint64_t *>(bases);
            const uint64_t c0 = P0 / 16, n_chunks = total / 16;  // words past the store read as sixteen not-ACGT bases
            auto word = [&](uint64_t c) -> uint64_t { return c < n_chunks ? store[c] : 0xFFFFull << 32; };
            stage[lane] = word(c0 + lane);
            stage[64 + lane] = word(c0 + 64 + lane);
            if (lane < 2) stage[128 + lane] = word(c0 + 128 + lane);
        } else {
            stage[lane] = load_chunk(bases, P0 + (uint64_t)lane * 16, total);
            stage[64 + lane] = load_chunk(bases, P0 + (uint64_t)(64 + lane) * 16, total);
            if (lane < 2) stage[128 + lane] = load_chunk(bases, P0 + (uint64_t)(128 + lane) * 16, total);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const uint64_t e0 = stage[2 * lane], e1 = stage[2 * lane + 1], e2 = stage[2 * lane + 2], e3 = stage[2 * lane + 3];
        uint32_t s0 = (uint32_t)e0, s1 = (uint32_t)e1, s2 = (uint32_t)e2, s3 = (uint32_t)e3;
        const unsigned __int128 R128 = (unsigned __int128)rev_pairs(~s3) | ((unsigned __int128)rev_pairs(~s2) << 32) |
                                       ((unsigned __int128)rev_pairs(~s1) << 64) | ((unsigned __int128)rev_pairs(~s0) << 96);
        const unsigned __int128 Rs = R128 >> (64 - 2 * k);
        uint32_t t0 = (uint32_t)Rs, t1 = (uint32_t)(Rs >> 32), t2 = (uint32_t)(Rs >> 64), t3 = (uint32_t)(Rs >> 96);
        uint32_t bad_lo = (uint32_t)(e0 >> 32) | ((uint32_t)(e1 >> 32) << 16);
        uint32_t bad_hi = (uint32_t)(e2 >> 32) | ((uint32_t)(e3 >> 32) << 16);
        // minimizer state: the hashes of the span's W m-mers (see probe_pass)
        win_t win[W > 0 ? W : 1];
        uint32_t fsh_new = 0, bsh_new = 0;
        if (W > 0) {
            const uint64_t fs = ((uint64_t)s1 << 32) | s0, bs = ((uint64_t)t3 << 32) | t2;
            win[0] = (win_t)~0ull;
#pragma unroll
            for (int i = 0; i + 1 < W; i++) win[i + 1] = mmer_order(fs, bs, (uint32_t)(2 * (o + i)), (uint32_t)(2 * (o + W - 1 - i)));
            fsh_new = (uint32_t)(2 * (o + W - 1));
            bsh_new = (uint32_t)(2 * o);
        }
        uint64_t held[TBK_SLOTS_PER_BUCKET];  // keys of bucket held_bk as last seen
#pragma unroll
        for (int s = 0; s < TBK_SLOTS_PER_BUCKET; s++) held[s] = 0;
        uint32_t held_bk = 0xFFFFFFFFu;
        uint32_t claimed = 0;  // slots this lane took for new k-mers
        uint32_t adds = 0;     // 64-bit atomic adds this lane issued (bench.py prices the kernel against the chip's rate for THOSE)
        bool full = false;
        // The adds of consecutive windows are merged where they can be: a bucket's eight 32-bit counters
        // are four 64-bit words, the k-mers of a run of windows were inserted one after the other - so
        // they mostly sit in neighbouring slots - and one 64-bit add of (1 | 1 << 32) counts both
        // halves of a word (a counter would have to pass 2^32 to carry into its neighbour: the host keeps
        // every counter below that, tbk_count_clamp_kernel; readers cap at 255).  The lane keeps the adds to the four words of ONE bucket pending and sends them when
        // a window counts in another bucket: the kernel runs at the rate the chip executes atomic adds,
        // so fewer adds is the lever.
        uint32_t pend_bk = 0xFFFFFFFFu;
        unsigned long long pend[4] = {0, 0, 0, 0};
        auto flush = [&]() {
            if (pend_bk == 0xFFFFFFFFu) return;
            unsigned long long *words = reinterpret_cast<unsigned long long *>(t.counts(pend_bk));
#pragma unroll
            for (int w = 0; w < 4; w++)
                if (pend[w]) { atomicAdd(&words[w], pend[w]); pend[w] = 0; adds++; }
        };
#pragma unroll 2
        for (int j = 0; j < TBK_WPL; j++) {
            const uint64_t fwd = ((uint64_t)s0 | ((uint64_t)s1 << 32)) & kmask;
            const uint64_t rc = ((uint64_t)t2 | ((uint64_t)t3 << 32)) & kmask;
            const uint64_t key = fwd < rc ? fwd : rc;
            bool ok = (bad_lo & badk) == 0 && P0 + (uint64_t)lane * TBK_WPL + (uint64_t)j + (uint64_t)k <= total;
            if constexpr (PACKED) {
                const TbkClassSel cs = (sel, ...);
                ok = ok && tbk_class_of(key, cs.n_classes) == cs.cls;
            }
            uint32_t hsel;
            if (W > 0) {
#pragma unroll
                for (int i = 0; i + 1 < W; i++) win[i] = win[i + 1];
                win[W - 1] = mmer_order(((uint64_t)s1 << 32) | s0, ((uint64_t)t3 << 32) | t2, fsh_new, bsh_new);
                win_t best = win[0];
#pragma unroll
                for (int i = 1; i < W; i++) best = win[i] < best ? win[i] : best;
                hsel = M64 ? (uint32_t)best : tbk_scramble((uint32_t)best);
            } else {
                hsel = tbk_mix32(key);
            }
            if (ok) {
                // home bucket first, then along the probe sequence; every bucket visited is fetched with
                // four 16-byte loads in flight at once and scanned in registers
                uint32_t b = tbk_reduce(hsel, t.n_buckets);
                bool done = false;
                for (uint32_t walked = 0; !done && walked < TBK_COUNT_MAX_WALK; walked++) {
                    unsigned long long *line = t.keys(b);
                    if (b != held_bk) {
                        const ulonglong2 *v = reinterpret_cast<const ulonglong2 *>(line);
                        const ulonglong2 v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];
                        held[0] = v0.x; held[1] = v0.y; held[2] = v1.x; held[3] = v1.y;
                        held[4] = v2.x; held[5] = v2.y; held[6] = v3.x; held[7] = v3.y;
                        held_bk = b;
                    }
#pragma unroll
                    for (int s = 0; s < TBK_SLOTS_PER_BUCKET; s++) {
                        if (done) continue;
                        if (held[s] == TBK_EMPTY) {
                            const unsigned long long old = atomicCAS(&line[s], (unsigned long long)TBK_EMPTY, (unsigned long long)key);
                            held[s] = old == TBK_EMPTY ? key : old;
                            claimed += old == TBK_EMPTY ? 1u : 0u;
                        }
                        if (held[s] == key) {
                            if (b != pend_bk) { flush(); pend_bk = b; }
                            pend[s >> 1] += 1ull << (32 * (s & 1));
                            done = true;
                        }
                    }
                    if (!done) b = tbk_next_bucket(key, t.mz, t.n_buckets, b, walked == 0);
                }
                if (!done) full = true;
            }
            s0 = (s0 >> 2) | (s1 << 30); s1 = (s1 >> 2) | (s2 << 30); s2 = (s2 >> 2) | (s3 << 30); s3 >>= 2;
            t3 = (t3 << 2) | (t2 >> 30); t2 = (t2 << 2) | (t1 >> 30); t1 = (t1 << 2) | (t0 >> 30); t0 <<= 2;
            bad_lo = (bad_lo >> 1) | (bad_hi << 31); bad_hi >>= 1;
        }
        flush();
        if (full) atomicExch(failed, 1);
        // slots taken by this wave: one atomic per pass
        uint32_t sum = claimed;
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        if (lane == 0 && sum) atomicAdd(used, (unsigned long long)sum);
        uint32_t asum = adds;
        for (int d = 32; d > 0; d >>= 1) asum += __shfl_xor(asum, d);
        if (lane == 0 && asum) atomicAdd(used + 1 + (pass & 1023u), (unsigned long long)asum);  // (1024 tallies: every pass adding to ONE word cost 3 ms per launch - the chip's rate for atomics on one address)
    }
}

// Counters are 32 bits wide and neighbours share a 64-bit word that the counting kernel adds to in one piece: a counter
// that passed 2^32 would carry into its neighbour.  Readers cap at 255, so a counter may stop anywhere above that: the host
// runs this pass before the window starts added since the last one could take any counter from 2^31 to 2^32 - every
// counter above 2^31 is set back to 2^31 (saturation, not a carry).
__global__ void __launch_bounds__(256)
tbk_count_clamp_kernel(TbkCountView t) {
    const uint64_t n = (uint64_t)t.n_buckets * TBK_SLOTS_PER_BUCKET;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t *c = &t.counts((uint32_t)(i / TBK_SLOTS_PER_BUCKET))[i % TBK_SLOTS_PER_BUCKET];
        if (*c > 0x80000000u) *c = 0x80000000u;
    }
}

extern "C" hipError_t tbk_launch_count_clamp(uint64_t *d_lines, uint32_t n_buckets, TbkMz mz, hipStream_t stream) {
    hipLaunchKernelGGL(tbk_count_clamp_kernel, dim3(entry_grid(4096)), dim3(256), 0, stream, TbkCountView{d_lines, n_buckets, mz});
    return hipGetLastError();
}

// Move every (key, counter) of an old table into a new, larger one (the host grows the table when
// the next batch could fill it).
__global__ void __launch_bounds__(256)
tbk_count_rehash_kernel(TbkCountView from, TbkCountView to, int *__restrict__ failed) {
    const uint64_t n_slots = (uint64_t)from.n_buckets * TBK_SLOTS_PER_BUCKET;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += step) {
        const uint32_t b = (uint32_t)(i >> 3), s = (uint32_t)(i & 7);
        const uint64_t key = from.keys(b)[s];
        if (key == TBK_EMPTY) continue;
        uint32_t claimed = 0;
        if (!count_from(to, key, tbk_bucket_of(key, to.mz, to.n_buckets), true, from.counts(b)[s], claimed)) atomicExch(failed, 1);
    }
}

// hist[c] = k-mers whose counter, capped at 255, equals c (c = 1..255); hist[0] = occupied slots
__global__ void __launch_bounds__(256)
tbk_count_histogram_kernel(TbkCountView t, unsigned long long *__restrict__ hist) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t n_slots = (uint64_t)t.n_buckets * TBK_SLOTS_PER_BUCKET;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += step) {
        const uint32_t b = (uint32_t)(i >> 3), s = (uint32_t)(i & 7);
        if (t.keys(b)[s] == TBK_EMPTY) continue;
        const uint32_t raw = t.counts(b)[s], c = raw < 255u ? raw : 255u;
        atomicAdd(&h[c], 1u);
        atomicAdd(&h[0], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// counter of `key` in a counting table (0 if absent).  Keys are never removed and take the first
// free slot along their probe sequence, so a line with a free slot ends the search.
__device__ __forceinline__ uint32_t count_lookup(const TbkCountView &t, uint64_t key) {
    uint32_t b = tbk_bucket_of(key, t.mz, t.n_buckets);
    for (uint32_t walked = 0; walked <= t.n_buckets && walked < TBK_COUNT_MAX_WALK; walked++) {
        const unsigned long long *line = t.keys(b);
        for (int s = 0; s < TBK_SLOTS_PER_BUCKET; s++) {
            const uint64_t cur = line[s];
            if (cur == key) return t.counts(b)[s];
            if (cur == TBK_EMPTY) return 0;
        }
        b = tbk_next_bucket(key, t.mz, t.n_buckets, b, walked == 0);
    }
    return 0;
}

// kmc_tools simple A B kmers_subtract + kmc_dump -ci -cx: the k-mers of database A (counter >= 2)
// that database B does not hold (its counter < 2) and whose counter, capped at 255, lies in
// [ci, cx].  Each is appended as its lexicographic rank (base 0 in the top bits), ready to sort.
__global__ void __launch_bounds__(256)
tbk_count_unique_kernel(TbkCountView a, TbkCountView b, int k, uint32_t ci, uint32_t cx, uint64_t *__restrict__ out,
                        uint64_t capacity, unsigned long long *__restrict__ n_out) {
    const uint64_t n_slots = (uint64_t)a.n_buckets * TBK_SLOTS_PER_BUCKET;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    // whole waves iterate together: the append below is a wave operation
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; i0 < n_slots; i0 += step) {
        const uint64_t i = i0 + lane;
        bool emit = false;
        uint64_t key = 0;
        if (i < n_slots) {
            key = a.keys((uint32_t)(i >> 3))[i & 7];
            if (key != TBK_EMPTY) {
                const uint32_t raw = a.counts((uint32_t)(i >> 3))[i & 7], c = raw < 255u ? raw : 255u;
                emit = raw >= 2u && c >= ci && c <= cx && count_lookup(b, key) < 2u;
            }
        }
        const uint64_t mask = __builtin_amdgcn_ballot_w64(emit);
        if (mask) {
            unsigned long long base = 0;
            const int leader = __builtin_ctzll(mask);
            if ((int)lane == leader) base = atomicAdd(n_out, (unsigned long long)__popcll(mask));
            base = __shfl(base, leader);
            if (emit) {
                const uint64_t at = base + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (at < capacity) {
                    const uint64_t lex = ((uint64_t)rev_pairs((uint32_t)key) << 32) | (uint64_t)rev_pairs((uint32_t)(key >> 32));
                    out[at] = lex >> (64 - 2 * k);
                }
            }
        }
    }
}

// ---- pass mode: the database a class leaves behind ---------------------------------------------------
// After a class has been counted, its table is distilled: every k-mer seen at least twice (kmc's -ci2) is
// appended to the class's database as (key, counter capped at 255) - 9 bytes - and every slot goes back to
// free, ready for the next class.  The k-mers seen once are dropped here; the histogram (taken just before,
// tbk_count_histogram_kernel) has counted them.  floor = 1 (tbk_counter_options.keep_singletons) keeps them too.
// Appends are per wave, as in tbk_count_unique_kernel.
__global__ void __launch_bounds__(256)
tbk_count_distil_kernel(TbkCountView t, uint32_t floor, uint64_t *__restrict__ db_keys, uint8_t *__restrict__ db_counts, uint64_t capacity,
                        unsigned long long *__restrict__ n_out) {
    const uint64_t n_slots = (uint64_t)t.n_buckets * TBK_SLOTS_PER_BUCKET;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; i0 < n_slots; i0 += step) {
        const uint64_t i = i0 + lane;
        bool emit = false;
        uint64_t key = 0;
        uint32_t raw = 0;
        if (i < n_slots) {
            unsigned long long *kp = &t.keys((uint32_t)(i >> 3))[i & 7];
            key = *kp;
            if (key != TBK_EMPTY) {
                uint32_t *cp = &t.counts((uint32_t)(i >> 3))[i & 7];
                raw = *cp;
                emit = raw >= floor;
                *kp = TBK_EMPTY;
                *cp = 0;
            }
        }
        const uint64_t mask = __builtin_amdgcn_ballot_w64(emit);
        if (mask) {
            unsigned long long base = 0;
            const int leader = __builtin_ctzll(mask);
            if ((int)lane == leader) base = atomicAdd(n_out, (unsigned long long)__popcll(mask));
            base = __shfl(base, leader);
            if (emit) {
                const uint64_t at = base + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (at < capacity) {
                    db_keys[at] = key;
                    db_counts[at] = (uint8_t)(raw < 255u ? raw : 255u);
                }
            }
        }
    }
}

// kmers_subtract + kmc_dump on the databases of ONE class (a k-mer's class depends on the k-mer alone, so the
// other parent holds it in the same class or not at all): the keys of A whose counter lies in [ci, cx] and that
// are not among B's, which arrive sorted; appended as lexicographic ranks like tbk_count_unique_kernel's.
__global__ void __launch_bounds__(256)
tbk_db_unique_kernel(const uint64_t *__restrict__ a_keys, const uint8_t *__restrict__ a_counts, uint64_t n_a,
                     const uint64_t *__restrict__ b_sorted, uint64_t n_b, int k, uint32_t ci, uint32_t cx,
                     uint64_t *__restrict__ out, uint64_t capacity, unsigned long long *__restrict__ n_out) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; i0 < n_a; i0 += step) {
        const uint64_t i = i0 + lane;
        bool emit = false;
        uint64_t key = 0;
        if (i < n_a) {
            key = a_keys[i];
            const uint32_t c = a_counts[i];
            emit = db_counter_selected(c, ci, cx) && db_absent(b_sorted, 0, n_b, n_b, key);
        }
        const uint64_t mask = __builtin_amdgcn_ballot_w64(emit);
        if (mask) {
            unsigned long long base = 0;
            const int leader = __builtin_ctzll(mask);
            if ((int)lane == leader) base = atomicAdd(n_out, (unsigned long long)__popcll(mask));
            base = __shfl(base, leader);
            if (emit) {
                const uint64_t at = base + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (at < capacity) {
                    const uint64_t lex = ((uint64_t)rev_pairs((uint32_t)key) << 32) | (uint64_t)rev_pairs((uint32_t)(key >> 32));
                    out[at] = lex >> (64 - 2 * k);
                }
            }
        }
    }
}

// ---- count databases (tbk_kmerdb): what a counter leaves behind, as an object of its own ---------------
// A database is n (lexicographic rank, counter 2..255) pairs in ascending order of the rank - the form kmc_dump
// prints and write_list takes.  The kernels below make one from a counter, check one that came from a file
// and subtract two.

// (lex_rank, the lexicographic rank of a key in the table's form: tbk_device.h)
// A live one-pass table to (rank, capped counter) pairs: tbk_count_distil_kernel without its stores to the
// table, which is only read.  Appends are per wave; the order is the sort's business.
__global__ void __launch_bounds__(256)
tbk_count_export_kernel(TbkCountView t, int k, uint32_t floor, uint64_t *__restrict__ out_keys, uint8_t *__restrict__ out_counts, uint64_t capacity,
                        unsigned long long *__restrict__ n_out) {
    const uint64_t n_slots = (uint64_t)t.n_buckets * TBK_SLOTS_PER_BUCKET;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; i0 < n_slots; i0 += step) {
        const uint64_t i = i0 + lane;
        bool emit = false;
        uint64_t key = 0;
        uint32_t raw = 0;
        if (i < n_slots) {
            key = t.keys((uint32_t)(i >> 3))[i & 7];
            if (key != TBK_EMPTY) {
                raw = t.counts((uint32_t)(i >> 3))[i & 7];
                emit = raw >= floor;  // (2, or 1: a full database keeps the k-mers seen once)
            }
        }
        const uint64_t mask = __builtin_amdgcn_ballot_w64(emit);
        if (mask) {
            unsigned long long base = 0;
            const int leader = __builtin_ctzll(mask);
            if ((int)lane == leader) base = atomicAdd(n_out, (unsigned long long)__popcll(mask));
            base = __shfl(base, leader);
            if (emit) {
                const uint64_t at = base + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (at < capacity) {
                    out_keys[at] = lex_rank(key, k);
                    out_counts[at] = (uint8_t)(raw < 255u ? raw : 255u);
                }
            }
        }
    }
}

// The database of one class (keys in the table's form) to ranks, copied to its place among the other classes'.
__global__ void __launch_bounds__(256)
tbk_db_rank_kernel(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ counts, uint64_t n, int k,
                   uint64_t *__restrict__ out_keys, uint8_t *__restrict__ out_counts) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        out_keys[i] = lex_rank(keys[i], k);
        out_counts[i] = counts[i];
    }
}

// One pass over a database that came from a file, before anything indexes by its content.  tally[0]: places where
// key[i] >= key[i + 1] (every element reads its right neighbour from memory, so the pairs that straddle a wave, a
// block or a grid stride are compared like any other); tally[1]: keys with a bit of high_mask (the bits above
// 2k; 0 for k = 32); tally[2]: counters below the database's floor (2, or 1 for a full one); tally[3 + c]: counters equal to c.
__global__ void __launch_bounds__(256)
tbk_kmerdb_check_kernel(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ counts, uint64_t n, uint64_t high_mask, uint32_t floor,
                        unsigned long long *__restrict__ tally) {
    __shared__ unsigned int h[256];
    __shared__ unsigned int bad[3];
    h[threadIdx.x] = 0;
    if (threadIdx.x < 3) bad[threadIdx.x] = 0;
    __syncthreads();
    uint32_t disorder = 0, high = 0, low = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[i];
        const uint32_t c = counts[i];
        if (i + 1 < n && key >= keys[i + 1]) disorder++;
        if (key & high_mask) high++;
        if (c < floor) low++;
        atomicAdd(&h[c], 1u);
    }
    if (disorder) atomicAdd(&bad[0], disorder);
    if (high) atomicAdd(&bad[1], high);
    if (low) atomicAdd(&bad[2], low);
    __syncthreads();
    if (threadIdx.x < 3 && bad[threadIdx.x]) atomicAdd(&tally[threadIdx.x], (unsigned long long)bad[threadIdx.x]);
    if (h[threadIdx.x]) atomicAdd(&tally[3 + threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// kmers_subtract + kmc_dump between two databases: the ranks of A whose counter lies in [ci, cx] and that are not
// among B's ascending ranks (bisection, as in tbk_db_unique_kernel); appended per wave, sorted by the host after.
__global__ void __launch_bounds__(256)
tbk_kmerdb_unique_kernel(const uint64_t *__restrict__ a_keys, const uint8_t *__restrict__ a_counts, uint64_t n_a,
                         const uint64_t *__restrict__ b_keys, uint64_t n_b, uint32_t ci, uint32_t cx,
                         uint64_t *__restrict__ out, uint64_t capacity, unsigned long long *__restrict__ n_out) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; i0 < n_a; i0 += step) {
        const uint64_t i = i0 + lane;
        bool emit = false;
        uint64_t key = 0;
        if (i < n_a) {
            key = a_keys[i];
            const uint32_t c = a_counts[i];
            emit = db_counter_selected(c, ci, cx) && db_absent(b_keys, 0, n_b, n_b, key);
        }
        const uint64_t mask = __builtin_amdgcn_ballot_w64(emit);
        if (mask) {
            unsigned long long base = 0;
            const int leader = __builtin_ctzll(mask);
            if ((int)lane == leader) base = atomicAdd(n_out, (unsigned long long)__popcll(mask));
            base = __shfl(base, leader);
            if (emit) {
                const uint64_t at = base + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (at < capacity) out[at] = key;
            }
        }
    }
}

// ---- the same subtraction, left in HBM as a k-mer list (tbk_kmerdb_unique_table) -------------------------------
// A's ranks ascend, so the selected ones in their places ARE the dump's order: a stable compaction, no sort and no
// buffer the size of the upper bound.  Flag, scan, scatter over tiles of TBK_DBT_TILE entries: tbk_compact.h.

// Selection of tbk_kmerdb_unique_kernel, kept as bits.
__global__ void __launch_bounds__(256)
tbk_kmerdb_flag_kernel(const uint64_t *__restrict__ a_keys, const uint8_t *__restrict__ a_counts, uint64_t n_a,
                       const uint64_t *__restrict__ b_keys, uint64_t n_b, uint32_t ci, uint32_t cx,
                       uint64_t *__restrict__ flags, unsigned long long *__restrict__ tile_counts) {
    compact_flag_tile(n_a, flags, tile_counts, [=](uint64_t i) {
        return db_counter_selected(a_counts[i], ci, cx) && db_absent(b_keys, 0, n_b, n_b, a_keys[i]);
    });
}

// The flagged entries of A in their places, as `write(i, at)` stores them: the packed key for a table (key_of_rank), the
// rank as it is for a list that goes to a file (write_list takes ranks), the rank and its counter for a database.
template <typename Write>
__global__ void __launch_bounds__(256)
tbk_kmerdb_scatter_kernel(uint64_t n_a, const uint64_t *__restrict__ flags, const unsigned long long *__restrict__ tile_offsets, uint64_t n_out,
                          Write write) {
    compact_scatter_tile(n_a, flags, tile_offsets, [=](uint64_t i, uint64_t at) {
        if (at < n_out) write(i, at);
    });
}

struct ScatterKey {
    const uint64_t *__restrict__ a_keys;
    int k;
    uint64_t *__restrict__ out;
    __device__ void operator()(uint64_t i, uint64_t at) const { out[at] = key_of_rank(a_keys[i], k); }
};
struct ScatterRank {
    const uint64_t *__restrict__ a_keys;
    uint64_t *__restrict__ out;
    __device__ void operator()(uint64_t i, uint64_t at) const { out[at] = a_keys[i]; }
};
struct ScatterPair {
    const uint64_t *__restrict__ a_keys;
    const uint8_t *__restrict__ a_counts;
    uint64_t *__restrict__ out_keys;
    uint8_t *__restrict__ out_counts;
    __device__ void operator()(uint64_t i, uint64_t at) const {
        out_keys[at] = a_keys[i];
        out_counts[at] = a_counts[i];
    }
};

// ---- three databases: the k-mers of A that B lacks and the child holds (tbk_kmerdb_inherited) -------------------
// The flags and tile counts of tbk_kmerdb_flag_kernel for the three-way selection: counter of A in [ci, cx], not among
// B's ranks, among the child's with a counter in [hi_ci, hi_cx] there.  Every entry bisects between the bounds of its tile
// in B and in the child (compact_tile_bounds; two waves find the two pairs side by side).  B first; the child only for
// what B left.
__global__ void __launch_bounds__(256)
tbk_kmerdb_inherited_flag_kernel(const uint64_t *__restrict__ a_keys, const uint8_t *__restrict__ a_counts, uint64_t n_a,
                                 const uint64_t *__restrict__ b_keys, uint64_t n_b, const uint64_t *__restrict__ h_keys,
                                 const uint8_t *__restrict__ h_counts, uint64_t n_h, uint32_t ci, uint32_t cx, uint32_t h_ci, uint32_t h_cx,
                                 uint64_t *__restrict__ flags, unsigned long long *__restrict__ tile_counts) {
    __shared__ uint64_t bound[4];  // B: first, last; child: first, last
#ifdef TBK_INHERITED_FULL_DEPTH  // (measurement only, tools/build_variant.sh: every entry bisects the whole partner)
    if (threadIdx.x < 4) bound[threadIdx.x] = (threadIdx.x & 1u) ? ((threadIdx.x & 2u) ? n_h : n_b) : 0;
#else
    const uint64_t first = (uint64_t)blockIdx.x * TBK_DBT_TILE;  // (< n_a: one block per tile of A)
    compact_tile_bounds(a_keys, n_a, first, b_keys, n_b, bound, 0);
    compact_tile_bounds(a_keys, n_a, first, h_keys, n_h, bound + 2, 64);
#endif
    compact_flag_tile(n_a, flags, tile_counts, [=](uint64_t i) {
        const uint64_t key = a_keys[i];
        if (!db_counter_selected(a_counts[i], ci, cx) || !db_absent(b_keys, bound[0], bound[1], n_b, key)) return false;
        const uint64_t at = db_lower_bound(h_keys, bound[2], bound[3], key);
        return at < n_h && h_keys[at] == key && db_counter_selected(h_counts[at], h_ci, h_cx);
    });
}

// ---- a class database without its once-seen k-mers: B's side of tbk_counter_unique for a counter that keeps them --------
// tbk_db_unique_kernel tests membership in B by key alone; a class database made with floor 1 also holds the k-mers
// seen once, which B "does not hold" in kmc's sense.  Their keys are left out here, before the sort.
__global__ void __launch_bounds__(256)
tbk_db_solid_keys_kernel(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ counts, uint64_t n, uint64_t *__restrict__ out,
                         uint64_t capacity, unsigned long long *__restrict__ n_out) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; i0 < n; i0 += step) {
        const uint64_t i = i0 + lane;
        const bool emit = i < n && counts[i] >= 2u;
        const uint64_t mask = __builtin_amdgcn_ballot_w64(emit);
        if (mask) {
            unsigned long long base = 0;
            const int leader = __builtin_ctzll(mask);
            if ((int)lane == leader) base = atomicAdd(n_out, (unsigned long long)__popcll(mask));
            base = __shfl(base, leader);
            if (emit) {
                const uint64_t at = base + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (at < capacity) out[at] = keys[i];
            }
        }
    }
}

// ---- tbk_kmerdb_union: two full databases to the database of both read sets -----------------------------------------------
// The RANK-BASED shape.  Both inputs ascend and hold no key twice, so the place of an entry in the union is its own
// index plus its lower bound in the other database, less the keys both hold (the duplicates) that stand before it; no
// sort, no concatenation.  Three steps, separate launches, no block waiting for another:
//   1. flag: one block per tile of TBK_DBT_TILE entries of A.  Every entry finds its lower bound in B, between the
//      bounds of its tile's first and last entry (compact_tile_bounds); a duplicate is an entry whose
//      key B holds at that place - B's key is read from memory wherever it lies, whatever tile of B that is.  One bit
//      per entry of A and a count per tile of A;
//   2. the exclusive scan of the tile counts (tbk_launch_kmerdb_scan);
//   3. scatter, one launch per input.  A's entry i goes to i + lower bound in B - duplicates of A before i, and a
//      duplicate carries min(255, ca + cb), added in 32 bits.  B's entry j asks A in the same way: held by A (again
//      read from A's memory at its lower bound there), it writes nothing - A's copy has written both; otherwise it
//      goes to j + lower bound in A - duplicates of A before that lower bound, which the flag words and tile offsets
//      of A give (the 16 flag words of a tile are one 128-byte line).
// Keys are compared as unsigned 64-bit numbers: at k = 32 a rank uses the top bit.  The bisection is repeated in step
// 3 and not kept: 8 bytes per entry would be more than the bit per entry the call may hold beside its output.
// 256 threads and no LDS to speak of (two bounds, a word table): occupancy is bounded by registers alone; a tile of
// 1024 keeps the per-tile state at 16 bytes per 9 KiB of input and the tile's span in B small enough that the
// bisection's lines are shared by the block.
__global__ void __launch_bounds__(256)
tbk_kmerdb_union_flag_kernel(const uint64_t *__restrict__ a_keys, uint64_t n_a, const uint64_t *__restrict__ b_keys, uint64_t n_b,
                             uint64_t *__restrict__ flags, unsigned long long *__restrict__ tile_counts) {
    __shared__ uint64_t bound[2];
    compact_tile_bounds(a_keys, n_a, (uint64_t)blockIdx.x * TBK_DBT_TILE, b_keys, n_b, bound, 0);
    compact_flag_tile(n_a, flags, tile_counts, [=](uint64_t i) { return !db_absent(b_keys, bound[0], bound[1], n_b, a_keys[i]); });
}

// Every entry of A, flagged or not: the prologue of compact_scatter_tile and a loop of its own.
__global__ void __launch_bounds__(256)
tbk_kmerdb_union_scatter_a_kernel(const uint64_t *__restrict__ a_keys, const uint8_t *__restrict__ a_counts, uint64_t n_a,
                                  const uint64_t *__restrict__ b_keys, const uint8_t *__restrict__ b_counts, uint64_t n_b,
                                  const uint64_t *__restrict__ flags, const unsigned long long *__restrict__ tile_offsets,
                                  uint64_t *__restrict__ out_keys, uint8_t *__restrict__ out_counts, uint64_t n_out) {
    __shared__ uint64_t bound[2];
    __shared__ CompactWords w;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t tile = blockIdx.x;
    const uint64_t first = tile * TBK_DBT_TILE;
    compact_tile_bounds(a_keys, n_a, first, b_keys, n_b, bound, 0);
    compact_load_words(w, flags, 64);  // (another wave than the bisections')
    const uint64_t b_lo = bound[0], b_hi = bound[1];
    const uint64_t dups_before_tile = tile_offsets[tile];
    for (uint32_t r = 0; r < TBK_DBT_TILE / 256; r++) {
        const uint32_t word = r * 4 + wave;
        const uint64_t mask = w.mask[word];
        const uint64_t i = first + (uint64_t)word * 64 + lane;
        if (i < n_a) {
            const uint64_t key = a_keys[i];
            const uint64_t rank = db_lower_bound(b_keys, b_lo, b_hi, key);
            const uint64_t dups = dups_before_tile + w.before[word] + compact_below(mask, lane);
            uint32_t c = a_counts[i];
            if (((mask >> lane) & 1ull) && rank < n_b) c += b_counts[rank];  // (32-bit sum of two bytes)
            const uint64_t at = i + rank - dups;
            if (at < n_out) {
                out_keys[at] = key;
                out_counts[at] = (uint8_t)(c < 255u ? c : 255u);
            }
        }
    }
}

// One block per tile of B; flags and tile_offsets are A's.
__global__ void __launch_bounds__(256)
tbk_kmerdb_union_scatter_b_kernel(const uint64_t *__restrict__ b_keys, const uint8_t *__restrict__ b_counts, uint64_t n_b,
                                  const uint64_t *__restrict__ a_keys, uint64_t n_a, const uint64_t *__restrict__ flags,
                                  const unsigned long long *__restrict__ tile_offsets, uint64_t *__restrict__ out_keys,
                                  uint8_t *__restrict__ out_counts, uint64_t n_out) {
    __shared__ uint64_t bound[2];
    const uint64_t first = (uint64_t)blockIdx.x * TBK_DBT_TILE;  // (< n_b)
    compact_tile_bounds(b_keys, n_b, first, a_keys, n_a, bound, 0);
    __syncthreads();
    const uint64_t a_lo = bound[0], a_hi = bound[1];
    for (uint32_t r = 0; r < TBK_DBT_TILE / 256; r++) {
        const uint64_t j = first + (uint64_t)r * 256 + threadIdx.x;
        if (j >= n_b) continue;
        const uint64_t key = b_keys[j];
        const uint64_t rank = db_lower_bound(a_keys, a_lo, a_hi, key);  // (<= a_hi <= n_a)
        if (rank < n_a && a_keys[rank] == key) continue;  // A's copy carries both counters
        // duplicates of A before entry `rank` of A: its tile's offset and the flag bits of the tile below it.  rank == n_a
        // on a tile edge reads offset [tiles] (the total) and no flag word.
        const uint64_t a_tile = rank / TBK_DBT_TILE;
        const uint32_t in_tile = (uint32_t)(rank % TBK_DBT_TILE), whole = in_tile >> 6, bits = in_tile & 63u;
        uint64_t dups = tile_offsets[a_tile];
        for (uint32_t w = 0; w < whole; w++) dups += (uint64_t)__popcll(flags[a_tile * TBK_DBT_WORDS + w]);
        if (bits) dups += (uint64_t)__popcll(flags[a_tile * TBK_DBT_WORDS + whole] & ((1ull << bits) - 1ull));
        const uint64_t at = j + rank - dups;
        if (at < n_out) {
            out_keys[at] = key;
            out_counts[at] = b_counts[j];
        }
    }
}

// hist[c] += counters equal to c (hist: 256 words, zeroed by the caller): the histogram of a database made on the device
__global__ void __launch_bounds__(256)
tbk_kmerdb_tally_kernel(const uint8_t *__restrict__ counts, uint64_t n, unsigned long long *__restrict__ hist) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) atomicAdd(&h[counts[i]], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// =======================================================================================
// launchers (called from tbk_count.cpp)
// =======================================================================================
extern "C" hipError_t tbk_launch_separate(const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint8_t *d_out,
                                          hipStream_t stream) {
    if (!n_reads) return hipSuccess;
    uint64_t blocks = (n_reads + 3) / 4;
    if (blocks > 262144) blocks = 262144;
    hipLaunchKernelGGL(tbk_separate_kernel, dim3(stream_grid(blocks)), dim3(256), 0, stream, d_bases, d_offsets, n_reads, d_out);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_count_rehash(uint64_t *from_lines, uint32_t from_buckets, TbkMz from_mz, uint64_t *to_lines,
                                              uint32_t to_buckets, TbkMz to_mz, int *d_failed, hipStream_t stream) {
    hipLaunchKernelGGL(tbk_count_rehash_kernel, dim3(entry_grid(8192)), dim3(256), 0, stream, TbkCountView{from_lines, from_buckets, from_mz},
                       TbkCountView{to_lines, to_buckets, to_mz}, d_failed);
    return hipGetLastError();
}

// passes [first_pass, first_pass + n_passes) of the separated stream (tbk_probe_passes(total) in all)
extern "C" hipError_t tbk_launch_count(const uint8_t *d_sep, uint64_t total, uint64_t first_pass, uint64_t n_passes, int k,
                                       uint64_t *d_lines, uint32_t n_buckets, TbkMz mz, int *d_failed, unsigned long long *d_used,
                                       hipStream_t stream) {
    if (total < (uint64_t)k || !n_passes) return hipSuccess;
    const uint64_t blocks = stream_grid(n_passes < TBK_COUNT_GRID_BLOCKS ? n_passes : TBK_COUNT_GRID_BLOCKS);
    const TbkCountView view{d_lines, n_buckets, mz};
    const dim3 grid((unsigned)blocks), block(64);
    const bool m64 = mz.m > 16;
#define TBK_COUNT_LAUNCH(N) case N: if (m64) hipLaunchKernelGGL((tbk_count_kernel<N, true>), grid, block, 0, stream, d_sep, total, first_pass, n_passes, k, view, d_failed, d_used); \
                                    else hipLaunchKernelGGL((tbk_count_kernel<N, false>), grid, block, 0, stream, d_sep, total, first_pass, n_passes, k, view, d_failed, d_used); break;
    switch (mz.t > 0 ? -1 : mz.w) {
        case 0: hipLaunchKernelGGL((tbk_count_kernel<0, false>), grid, block, 0, stream, d_sep, total, first_pass, n_passes, k, view, d_failed, d_used); break;
        TBK_COUNT_LAUNCH(1) TBK_COUNT_LAUNCH(2) TBK_COUNT_LAUNCH(3) TBK_COUNT_LAUNCH(4)
        TBK_COUNT_LAUNCH(5) TBK_COUNT_LAUNCH(6) TBK_COUNT_LAUNCH(7) TBK_COUNT_LAUNCH(8)
        default: return hipErrorInvalidValue;
    }
#undef TBK_COUNT_LAUNCH
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_count_histogram(uint64_t *d_lines, uint32_t n_buckets, TbkMz mz, unsigned long long *d_hist,
                                                 hipStream_t stream) {
    hipLaunchKernelGGL(tbk_count_histogram_kernel, dim3(entry_grid(4096)), dim3(256), 0, stream, TbkCountView{d_lines, n_buckets, mz}, d_hist);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_count_unique(uint64_t *a_lines, uint32_t a_buckets, TbkMz a_mz, uint64_t *b_lines, uint32_t b_buckets,
                                              TbkMz b_mz, int k, uint32_t ci, uint32_t cx, uint64_t *d_out, uint64_t capacity,
                                              unsigned long long *d_n, hipStream_t stream) {
    hipLaunchKernelGGL(tbk_count_unique_kernel, dim3(entry_grid(8192)), dim3(256), 0, stream, TbkCountView{a_lines, a_buckets, a_mz},
                       TbkCountView{b_lines, b_buckets, b_mz}, k, ci, cx, d_out, capacity, d_n);
    return hipGetLastError();
}

// ---- pass mode ------------------------------------------------------------------------------------------
extern "C" hipError_t tbk_launch_retain(const uint8_t *d_sep, uint64_t total, uint64_t *d_store, uint64_t n_chunks, hipStream_t stream) {
    if (!n_chunks) return hipSuccess;
    const uint64_t blocks = (n_chunks + 255) / 256;
    hipLaunchKernelGGL(tbk_retain_kernel, dim3(stream_grid(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream, d_sep, total, d_store, n_chunks);
    return hipGetLastError();
}

// tbk_launch_count for one class of a retained batch of n_chunks words
extern "C" hipError_t tbk_launch_count_class(const uint64_t *d_store, uint64_t n_chunks, uint64_t first_pass, uint64_t n_passes, int k,
                                             uint64_t *d_lines, uint32_t n_buckets, TbkMz mz, int *d_failed, unsigned long long *d_used,
                                             uint32_t n_classes, uint32_t cls, hipStream_t stream) {
    const uint64_t total = n_chunks * 16;
    if (total < (uint64_t)k || !n_passes) return hipSuccess;
    if (!n_classes || cls >= n_classes) return hipErrorInvalidValue;
    const uint64_t blocks = stream_grid(n_passes < TBK_COUNT_GRID_BLOCKS ? n_passes : TBK_COUNT_GRID_BLOCKS);
    const TbkCountView view{d_lines, n_buckets, mz};
    const TbkClassSel sel{n_classes, cls};
    const uint8_t *d_bases = reinterpret_cast<const uint8_t *>(d_store);
    const dim3 grid((unsigned)blocks), block(64);
    const bool m64 = mz.m > 16;
#define TBK_COUNT_LAUNCH(N) case N: if (m64) hipLaunchKernelGGL((tbk_count_kernel<N, true, TbkClassSel>), grid, block, 0, stream, d_bases, total, first_pass, n_passes, k, view, d_failed, d_used, sel); \
                                    else hipLaunchKernelGGL((tbk_count_kernel<N, false, TbkClassSel>), grid, block, 0, stream, d_bases, total, first_pass, n_passes, k, view, d_failed, d_used, sel); break;
    switch (mz.t > 0 ? -1 : mz.w) {
        case 0: hipLaunchKernelGGL((tbk_count_kernel<0, false, TbkClassSel>), grid, block, 0, stream, d_bases, total, first_pass, n_passes, k, view, d_failed, d_used, sel); break;
        TBK_COUNT_LAUNCH(1) TBK_COUNT_LAUNCH(2) TBK_COUNT_LAUNCH(3) TBK_COUNT_LAUNCH(4)
        TBK_COUNT_LAUNCH(5) TBK_COUNT_LAUNCH(6) TBK_COUNT_LAUNCH(7) TBK_COUNT_LAUNCH(8)
        default: return hipErrorInvalidValue;
    }
#undef TBK_COUNT_LAUNCH
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_count_distil(uint64_t *d_lines, uint32_t n_buckets, TbkMz mz, uint32_t floor, uint64_t *d_keys, uint8_t *d_counts,
                                              uint64_t capacity, unsigned long long *d_n, hipStream_t stream) {
    if (floor < 1 || floor > 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tbk_count_distil_kernel, dim3(entry_grid(4096)), dim3(256), 0, stream, TbkCountView{d_lines, n_buckets, mz}, floor, d_keys, d_counts, capacity, d_n);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_db_unique(const uint64_t *a_keys, const uint8_t *a_counts, uint64_t n_a, const uint64_t *b_sorted, uint64_t n_b,
                                           int k, uint32_t ci, uint32_t cx, uint64_t *d_out, uint64_t capacity, unsigned long long *d_n,
                                           hipStream_t stream) {
    if (!n_a) return hipSuccess;
    const uint64_t blocks = (n_a + 255) / 256;
    hipLaunchKernelGGL(tbk_db_unique_kernel, dim3(entry_grid(blocks < 8192 ? blocks : 8192)), dim3(256), 0, stream, a_keys, a_counts, n_a, b_sorted, n_b,
                       k, ci, cx, d_out, capacity, d_n);
    return hipGetLastError();
}

// ---- count databases ------------------------------------------------------------------------------------
extern "C" hipError_t tbk_launch_count_export(uint64_t *d_lines, uint32_t n_buckets, TbkMz mz, int k, uint32_t floor, uint64_t *d_keys, uint8_t *d_counts,
                                              uint64_t capacity, unsigned long long *d_n, hipStream_t stream) {
    if (floor < 1 || floor > 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tbk_count_export_kernel, dim3(entry_grid(4096)), dim3(256), 0, stream, TbkCountView{d_lines, n_buckets, mz}, k, floor, d_keys, d_counts, capacity, d_n);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_db_rank(const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, int k, uint64_t *d_out_keys,
                                         uint8_t *d_out_counts, hipStream_t stream) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(tbk_db_rank_kernel, dim3(entry_grid(blocks < 8192 ? blocks : 8192)), dim3(256), 0, stream, d_keys, d_counts, n, k, d_out_keys, d_out_counts);
    return hipGetLastError();
}

// d_tally: 3 + 256 words, zeroed by the caller
extern "C" hipError_t tbk_launch_kmerdb_check(const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, int k, uint32_t floor,
                                              unsigned long long *d_tally, hipStream_t stream) {
    if (!n) return hipSuccess;
    if (floor < 1 || floor > 2) return hipErrorInvalidValue;
    const uint64_t high_mask = k >= 32 ? 0ull : ~0ull << (2 * k);
    const uint64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(tbk_kmerdb_check_kernel, dim3(entry_grid(blocks < 1024 ? blocks : 1024)), dim3(256), 0, stream, d_keys, d_counts, n, high_mask, floor, d_tally);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_kmerdb_unique(const uint64_t *a_keys, const uint8_t *a_counts, uint64_t n_a, const uint64_t *b_keys, uint64_t n_b,
                                               uint32_t ci, uint32_t cx, uint64_t *d_out, uint64_t capacity, unsigned long long *d_n,
                                               hipStream_t stream) {
    if (!n_a) return hipSuccess;
    const uint64_t blocks = (n_a + 255) / 256;
    hipLaunchKernelGGL(tbk_kmerdb_unique_kernel, dim3(entry_grid(blocks < 8192 ? blocks : 8192)), dim3(256), 0, stream, a_keys, a_counts, n_a, b_keys, n_b,
                       ci, cx, d_out, capacity, d_n);
    return hipGetLastError();
}

// ---- tbk_kmerdb_unique_table: flag, scan, scatter (the buffers: tbk_compact_host.h) ----------------------------------
extern "C" hipError_t tbk_launch_kmerdb_flag(const uint64_t *a_keys, const uint8_t *a_counts, uint64_t n_a, const uint64_t *b_keys, uint64_t n_b,
                                             uint32_t ci, uint32_t cx, uint64_t *d_flags, unsigned long long *d_tile_counts, hipStream_t stream) {
    return compact_launch_tiles(n_a, stream, tbk_kmerdb_flag_kernel, a_keys, a_counts, n_a, b_keys, n_b, ci, cx, d_flags, d_tile_counts);
}

// d_out[i] = d_in[0] + ... + d_in[i - 1], n elements; the caller passes one element more than it has tiles, so the last is the total
extern "C" hipError_t tbk_launch_kmerdb_scan(const unsigned long long *d_in, unsigned long long *d_out, uint64_t n, hipStream_t stream) {
    if (!n) return hipSuccess;
    size_t tmp_bytes = 0;
    void *d_tmp = nullptr;
    hipError_t e = rocprim::exclusive_scan(nullptr, tmp_bytes, d_in, d_out, 0ull, (size_t)n, rocprim::plus<unsigned long long>(), stream);
    if (e != hipSuccess) return e;
    e = hipMalloc(&d_tmp, tmp_bytes ? tmp_bytes : 16);
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(d_tmp, tmp_bytes, d_in, d_out, 0ull, (size_t)n, rocprim::plus<unsigned long long>(), stream);
    const hipError_t e2 = hipStreamSynchronize(stream);
    (void)hipFree(d_tmp);
    return e != hipSuccess ? e : e2;
}

template <typename Write>
static hipError_t launch_scatter(uint64_t n_a, const uint64_t *d_flags, const unsigned long long *d_tile_offsets, uint64_t n_out, hipStream_t stream,
                                 Write write) {
    if (!n_out) return hipSuccess;
    return compact_launch_tiles(n_a, stream, tbk_kmerdb_scatter_kernel<Write>, n_a, d_flags, d_tile_offsets, n_out, write);
}

extern "C" hipError_t tbk_launch_kmerdb_scatter(const uint64_t *a_keys, uint64_t n_a, const uint64_t *d_flags, const unsigned long long *d_tile_offsets,
                                                int k, uint64_t *d_out, uint64_t n_out, hipStream_t stream) {
    if (n_a && n_out && (k < 1 || k > 32)) return hipErrorInvalidValue;
    return launch_scatter(n_a, d_flags, d_tile_offsets, n_out, stream, ScatterKey{a_keys, k, d_out});
}

// ---- tbk_kmerdb_inherited: its own flag kernel, then the scan above and one of the two scatters ------------------
extern "C" hipError_t tbk_launch_kmerdb_inherited_flag(const uint64_t *a_keys, const uint8_t *a_counts, uint64_t n_a, const uint64_t *b_keys,
                                                       uint64_t n_b, const uint64_t *h_keys, const uint8_t *h_counts, uint64_t n_h, uint32_t ci,
                                                       uint32_t cx, uint32_t h_ci, uint32_t h_cx, uint64_t *d_flags,
                                                       unsigned long long *d_tile_counts, hipStream_t stream) {
    return compact_launch_tiles(n_a, stream, tbk_kmerdb_inherited_flag_kernel, a_keys, a_counts, n_a, b_keys, n_b, h_keys, h_counts, n_h, ci, cx, h_ci, h_cx,
                        d_flags, d_tile_counts);
}

extern "C" hipError_t tbk_launch_kmerdb_scatter_ranks(const uint64_t *a_keys, uint64_t n_a, const uint64_t *d_flags,
                                                      const unsigned long long *d_tile_offsets, uint64_t *d_out, uint64_t n_out, hipStream_t stream) {
    return launch_scatter(n_a, d_flags, d_tile_offsets, n_out, stream, ScatterRank{a_keys, d_out});
}

// ---- keep_singletons: B's class keys without the once-seen ones ------------------------------------------------------
extern "C" hipError_t tbk_launch_db_solid_keys(const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, uint64_t *d_out, uint64_t capacity,
                                               unsigned long long *d_n, hipStream_t stream) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(tbk_db_solid_keys_kernel, dim3(entry_grid(blocks < 8192 ? blocks : 8192)), dim3(256), 0, stream, d_keys, d_counts, n, d_out, capacity, d_n);
    return hipGetLastError();
}

// ---- tbk_kmerdb_solid: tbk_launch_kmerdb_flag (no B, 2..255), the scan, then this ------------------------------------------
extern "C" hipError_t tbk_launch_kmerdb_scatter_pairs(const uint64_t *a_keys, const uint8_t *a_counts, uint64_t n_a, const uint64_t *d_flags,
                                                      const unsigned long long *d_tile_offsets, uint64_t *d_out_keys, uint8_t *d_out_counts,
                                                      uint64_t n_out, hipStream_t stream) {
    return launch_scatter(n_a, d_flags, d_tile_offsets, n_out, stream, ScatterPair{a_keys, a_counts, d_out_keys, d_out_counts});
}

// ---- tbk_kmerdb_union: flag A against B, the scan above, scatter A, scatter B, tally --------------------------------------
extern "C" hipError_t tbk_launch_kmerdb_union_flag(const uint64_t *a_keys, uint64_t n_a, const uint64_t *b_keys, uint64_t n_b, uint64_t *d_flags,
                                                   unsigned long long *d_tile_counts, hipStream_t stream) {
    return compact_launch_tiles(n_a, stream, tbk_kmerdb_union_flag_kernel, a_keys, n_a, b_keys, n_b, d_flags, d_tile_counts);
}

extern "C" hipError_t tbk_launch_kmerdb_union_scatter(const uint64_t *a_keys, const uint8_t *a_counts, uint64_t n_a, const uint64_t *b_keys,
                                                      const uint8_t *b_counts, uint64_t n_b, const uint64_t *d_flags,
                                                      const unsigned long long *d_tile_offsets, uint64_t *d_out_keys, uint8_t *d_out_counts,
                                                      uint64_t n_out, hipStream_t stream) {
    if (!n_out) return hipSuccess;
    if (tbk_kmerdb_table_tiles(n_a) > 0x7FFFFFFFull || tbk_kmerdb_table_tiles(n_b) > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const hipError_t e = compact_launch_tiles(n_a, stream, tbk_kmerdb_union_scatter_a_kernel, a_keys, a_counts, n_a, b_keys, b_counts, n_b, d_flags,
                                      d_tile_offsets, d_out_keys, d_out_counts, n_out);
    if (e != hipSuccess) return e;
    return compact_launch_tiles(n_b, stream, tbk_kmerdb_union_scatter_b_kernel, b_keys, b_counts, n_b, a_keys, n_a, d_flags, d_tile_offsets, d_out_keys,
                        d_out_counts, n_out);
}

// d_hist: 256 words, zeroed by the caller
extern "C" hipError_t tbk_launch_kmerdb_tally(const uint8_t *d_counts, uint64_t n, unsigned long long *d_hist, hipStream_t stream) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(tbk_kmerdb_tally_kernel, dim3(entry_grid(blocks < 1024 ? blocks : 1024)), dim3(256), 0, stream, d_counts, n, d_hist);
    return hipGetLastError();
}
