// tbk_lookup.h — the one window lookup of the count-database query kernels (tbk_query.hip, tbk_depth.hip, tbk_repair.hip,
// tbk_screen.hip, tbk_read_depth.hip, tbk_pieces.hip; the het-mer partners of tbk_hetmer.hip; the staging and the roll also in tbk_track.hip).  Three parts, each
// written once here: a wave's windows (LaneWindows), the grouped search of a sorted database behind its directory
// (db_search_group), and the body of the loop over passes that joins the two (lookup_pass).  The kernels keep their
// accumulators, what they do with a group's answers, and their stores.  The host's side: tbk_lookup_host.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbk_device.h"
#include "tbk_lookup_host.h"

// ---- a wave's windows ------------------------------------------------------------------------------------------------------------
// One wave takes a pass of TBK_PASS window starts of the separated stream (every sequence followed by one 'N', so no clean
// window spans two sequences) from stream position P0 on.  The pass is STAGED: its 128 chunks of 16 bases and two chunks of
// halo are packed into LDS (2-bit codes below, not-ACGT mask above, tbk_device.h), between two wavefront fences - the first
// keeps the reads of the pass before from the writes, the second the writes from the reads.  Lane l then takes chunks
// 2 l .. 2 l + 3, the 64 bases from P0 + 32 l on, into registers: the codes as s0..s3, their reverse complement, aligned so that
// the window's is in t2:t3, as t0..t3, and the mask as bad_lo:bad_hi.  The window at the lane's current position is then read
// off the low 2k bits of s0:s1 and of t2:t3 and the low k bits of bad_lo, and ROLLING by one base is a shift of each register
// group: 32 windows per lane without another load.  A byte at or past `total` reads as not ACGT, so a window past the end of
// the stream is never clean through its bases; a window that would only begin before `total` is ruled out by position.
struct LaneWindows {
    uint64_t kmask;  // the low 2k bits
    uint32_t badk;   // the low k bits
    int k;
    uint32_t s0, s1, s2, s3, t0, t1, t2, t3, bad_lo, bad_hi;

    __device__ __forceinline__ explicit LaneWindows(int k_)
        : kmask(k_ == 32 ? ~0ull : ((1ull << (2 * k_)) - 1ull)), badk(k_ == 32 ? 0xFFFFFFFFu : ((1u << k_) - 1u)), k(k_) {}

    // stage: the caller's __shared__ uint64_t[TBK_CHUNKS + 2]; called by all 64 lanes of the wave that owns it
    __device__ __forceinline__ void load(uint64_t *stage, const uint8_t *__restrict__ sep, uint64_t P0, uint64_t total, uint32_t lane) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        stage[lane] = load_chunk(sep, P0 + (uint64_t)lane * 16, total);
        stage[64 + lane] = load_chunk(sep, P0 + (uint64_t)(64 + lane) * 16, total);
        if (lane < 2) stage[128 + lane] = load_chunk(sep, P0 + (uint64_t)(128 + lane) * 16, total);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const uint64_t e0 = stage[2 * lane], e1 = stage[2 * lane + 1], e2 = stage[2 * lane + 2], e3 = stage[2 * lane + 3];
        s0 = (uint32_t)e0; s1 = (uint32_t)e1; s2 = (uint32_t)e2; s3 = (uint32_t)e3;
        const unsigned __int128 R128 = (unsigned __int128)rev_pairs(~s3) | ((unsigned __int128)rev_pairs(~s2) << 32) |
                                       ((unsigned __int128)rev_pairs(~s1) << 64) | ((unsigned __int128)rev_pairs(~s0) << 96);
        const unsigned __int128 Rs = R128 >> (64 - 2 * k);
        t0 = (uint32_t)Rs; t1 = (uint32_t)(Rs >> 32); t2 = (uint32_t)(Rs >> 64); t3 = (uint32_t)(Rs >> 96);
        bad_lo = (uint32_t)(e0 >> 32) | ((uint32_t)(e1 >> 32) << 16);
        bad_hi = (uint32_t)(e2 >> 32) | ((uint32_t)(e3 >> 32) << 16);
    }
    // the current window's canonical k-mer, min(forward, reverse complement), in the table's form (base i at bits 2i)
    __device__ __forceinline__ uint64_t key() const {
        const uint64_t fwd = ((uint64_t)s0 | ((uint64_t)s1 << 32)) & kmask;
        const uint64_t rc = ((uint64_t)t2 | ((uint64_t)t3 << 32)) & kmask;
        return fwd < rc ? fwd : rc;
    }
    // clean: k bases, all ACGT, all before `total`; p is the window's stream position
    __device__ __forceinline__ bool clean(uint64_t p, uint64_t total) const { return (bad_lo & badk) == 0 && p + (uint64_t)k <= total; }
    __device__ __forceinline__ void roll() {
        s0 = (s0 >> 2) | (s1 << 30); s1 = (s1 >> 2) | (s2 << 30); s2 = (s2 >> 2) | (s3 << 30); s3 >>= 2;
        t3 = (t3 << 2) | (t2 >> 30); t2 = (t2 << 2) | (t1 >> 30); t1 = (t1 << 2) | (t0 >> 30); t0 <<= 2;
        bad_lo = (bad_lo >> 1) | (bad_hi << 31); bad_hi >>= 1;
    }
};

// ---- the group search ------------------------------------------------------------------------------------------------------------
// G ranks of 2k bits are looked up in a sorted database side by side.  The searches are independent, so each step is issued
// for all of them before any answer is used: the two directory offsets that bound a rank's bucket, then one key per bisection
// step of the bucket, then the counter.  NO LOAD IS UNDER A BRANCH: a search that is over, or never began (ok[g] false), reads
// entry 0 again - the host gives an empty database one entry of padding - and the loop goes round until the last search of
// the group is over.  Out: hit[g]; at[g], the entry when hit[g]; c[g], its counter, 0 on a miss.
// UNIFORM asks the whole wave whether to go round again, one ballot per step: for a caller whose lanes all come here together
// and that wants the loop's branch scalar (tbk_repair_kernel, one search per lane).  Without it nothing crosses lanes, and a
// wave may come here with some lanes only.
// TBK_LOOKUP_NO_DIRECTORY (measurement only, tools/build_variant.sh, which gives its flags to one source file): every search
// bisects the whole database.
template <int G, bool UNIFORM = false>
__device__ __forceinline__ void db_search_group(const TbkDbView &db, int k, const uint64_t (&rank)[G], const bool (&ok)[G], uint32_t (&at)[G],
                                                bool (&hit)[G], uint32_t (&c)[G]) {
    uint32_t lo[G], hi[G];
    bool found[G];  // (the loop's own, handed out at the end: with the caller's hit[] written in the loop the flags become lane
                    // masks merged by scalar instructions every step, and the het-mer tally takes 30 % longer - profiles/r27)
#ifdef TBK_LOOKUP_NO_DIRECTORY
#pragma unroll
    for (int g = 0; g < G; g++) { lo[g] = 0; hi[g] = ok[g] ? db.n : 0; found[g] = false; }
#else
    const int shift = 2 * k - db.prefix_bits;  // (64 only when prefix_bits is 0: not used then)
#pragma unroll
    for (int g = 0; g < G; g++) {
        const uint64_t p = ok[g] && db.prefix_bits ? rank[g] >> shift : 0;
        lo[g] = db.dir[p];
        hi[g] = db.dir[p + 1];
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
        if (!ok[g]) hi[g] = lo[g];
        found[g] = false;
    }
#endif
    for (;;) {
        bool more = false;
#pragma unroll
        for (int g = 0; g < G; g++) more = more || lo[g] < hi[g];
        if (UNIFORM) more = __builtin_amdgcn_ballot_w64(more) != 0;
        if (!more) break;
        uint64_t v[G];
        uint32_t mid[G];
#pragma unroll
        for (int g = 0; g < G; g++) {
            mid[g] = lo[g] + (hi[g] - lo[g]) / 2;  // (< hi <= n)
            v[g] = db.keys[lo[g] < hi[g] ? mid[g] : 0];
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            if (lo[g] < hi[g]) {
                if (v[g] == rank[g]) { found[g] = true; lo[g] = hi[g] = mid[g]; }
                else if (v[g] < rank[g]) lo[g] = mid[g] + 1;
                else hi[g] = mid[g];
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++) c[g] = db.counts[found[g] ? lo[g] : 0];
#pragma unroll
    for (int g = 0; g < G; g++) {
        at[g] = lo[g];
        hit[g] = found[g];
        c[g] = found[g] ? c[g] : 0;
    }
}

// ---- a pass of a lookup kernel ---------------------------------------------------------------------------------------------------
constexpr int TBK_GROUP = 4;  // windows of a lane whose searches are in flight together (their counter bytes are one 32-bit word)
static_assert(TBK_WPL % TBK_GROUP == 0, "a lane's windows are whole groups");

// a group of a lane's windows, looked up: ok - the window is clean - and db_search_group's answers
struct LookupGroup {
    bool ok[TBK_GROUP], hit[TBK_GROUP];
    uint32_t at[TBK_GROUP], c[TBK_GROUP];
};

// The body of a lookup kernel's loop over passes, called by the 64 lanes of a one-wave block: the pass is staged, and each
// lane rolls its 32 windows out of registers TBK_GROUP at a time.  A clean window's canonical k-mer is the counter's -
// min(forward, reverse complement) in the table's form, which is the lexicographic minimum - brought into rank form
// (lex_rank); a window over a separator or past `total` is not clean and searches nothing.  For every group
//     sink(j0, w)
// gets the group's first window j0 and the LookupGroup w: window g of it is bit j0 + g of the lane's word of a bitmap indexed
// by stream position, and lies at pass * TBK_PASS + lane * TBK_WPL + j0 + g.
template <typename Sink>
__device__ __forceinline__ void lookup_pass(uint64_t *stage, const uint8_t *__restrict__ sep, uint64_t total, uint64_t pass, int k, const TbkDbView &db,
                                            Sink &&sink) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t P0 = pass * TBK_PASS, p_lane = P0 + (uint64_t)lane * TBK_WPL;
    LaneWindows win(k);
    win.load(stage, sep, P0, total, lane);
#pragma unroll 1
    for (int j0 = 0; j0 < TBK_WPL; j0 += TBK_GROUP) {
        uint64_t rank[TBK_GROUP];
        LookupGroup w;
#pragma unroll
        for (int g = 0; g < TBK_GROUP; g++) {
            rank[g] = lex_rank(win.key(), k);
            w.ok[g] = win.clean(p_lane + (uint64_t)(j0 + g), total);
            win.roll();
        }
        db_search_group<TBK_GROUP>(db, k, rank, w.ok, w.at, w.hit, w.c);
        sink(j0, w);
    }
}

// ---- positions and bitmaps of the separated stream -------------------------------------------------------------------------------
// The read of stream position p (never a separator's): the last r with offsets[r] + r <= p - the separators before read r are
// r, and offsets[r] + r rises strictly, so empty reads are stepped over.
__device__ __forceinline__ uint64_t read_of_position(const uint64_t *__restrict__ offsets, uint64_t n_reads, uint64_t p) {
    uint64_t lo = 0, hi = n_reads;  // first r with offsets[r] + r > p
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] + mid <= p) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// The bits of 32-bit word w of a bitmap that lie in the positions [a, b), b > a, whose first and last words are w_first = a >> 5
// and w_last = (b - 1) >> 5: all of an inner word (and of a word outside the range: the caller keeps to it), the edge words masked.
__device__ __forceinline__ uint32_t range_word_mask(uint64_t w, uint64_t w_first, uint64_t w_last, uint64_t a, uint64_t b) {
    uint32_t mask = 0xFFFFFFFFu;
    if (w == w_first) mask &= 0xFFFFFFFFu << (a & 31u);
    if (w == w_last) mask &= 0xFFFFFFFFu >> (31u - (uint32_t)((b - 1) & 31u));
    return mask;
}

// The COVERED word of bitmap word w from the held words w (h) and w - 1 (hb; 0 for word 0): the held bits dilated by k - 1
// positions upward.  k <= 32, so a 32-bit word needs only its predecessor as halo, and the dilation is floor(log2 k) + 1
// shift-and-ors of the two words side by side in one 64-bit register.  (tbk_screen.hip, tbk_pieces.hip)
__device__ __forceinline__ uint32_t covered_word(uint32_t h, uint32_t hb, int k) {
    uint64_t x = ((uint64_t)h << 32) | hb;  // shifts 0 .. n - 1 of the held bits so far; n doubles up to k
    int n = 1;
    while (2 * n <= k) { x |= x << n; n *= 2; }
    x |= x << (k - n);  // (k - n < n)
    return (uint32_t)(x >> 32);
}
