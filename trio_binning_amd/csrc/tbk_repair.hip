// tbk_repair.hip — the MI355X kernels of a query session's repair candidates (tbk_kmerdb_query_repairs): for every maximal
// stretch of broken windows of a batch, the one-base edits that make every window over the edited position a k-mer the
// database holds.  Four kernels: the lookup pass leaves the clean and the broken bitmap, the heads of the stretches are
// flagged and compacted into records (tbk_compact.h), and the repair kernel tries the candidates of every stretch.  None
// writes any state of the session.  Host side: tbk_count.cpp; the rule: include/tbk.h, "repair candidates".
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/tbk.h"
#include "tbk_common.h"
#include "tbk_compact.h"
#include "tbk_lookup.h"

// One wave per pass of TBK_PASS window starts of the separated stream: staging, roll and the grouped search are lookup_pass's
// (tbk_lookup.h).  What is left is one bit per stream position in each of two bitmaps, 64 words per pass: clean, and
// broken - clean with c < m.  No atomic, nothing of the session written.
__global__ void __launch_bounds__(64)
tbk_repair_lookup_kernel(const uint8_t *__restrict__ sep, uint64_t total, uint64_t n_passes, int k, TbkDbView db, uint32_t m,
                         uint32_t *__restrict__ clean, uint32_t *__restrict__ broken) {
    __shared__ uint64_t stage[TBK_CHUNKS + 2];
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t pass = blockIdx.x; pass < n_passes; pass += gridDim.x) {
        uint32_t w_clean = 0, w_broken = 0;
        lookup_pass(stage, sep, total, pass, k, db, [&](int j0, const LookupGroup &w) {
#pragma unroll
            for (int g = 0; g < TBK_GROUP; g++) {
                const uint32_t bit = 1u << (j0 + g);
                if (w.ok[g]) w_clean |= bit;
                if (w.ok[g] && w.c[g] < m) w_broken |= bit;
            }
        });
        clean[pass * 64 + lane] = w_clean;
        broken[pass * 64 + lane] = w_broken;
    }
}

// ---- the stretches: flag the heads, scan (the host), scatter them into records ------------------------------------------------
// Bit p of the broken bitmap, read as 64-bit words, is stream position p.  The separator behind every sequence is never clean,
// so a run of broken bits lies inside one sequence.
__device__ __forceinline__ bool repair_bit(const uint64_t *__restrict__ bits, uint64_t p) { return (bits[p >> 6] >> (p & 63u)) & 1ull; }

// A broken position whose predecessor is not broken is a stretch's head; n = 2048 positions per pass.
__global__ void __launch_bounds__(256)
tbk_repair_heads_kernel(const uint64_t *__restrict__ broken, uint64_t n, uint64_t *__restrict__ flags, unsigned long long *__restrict__ tile_counts) {
    compact_flag_tile(n, flags, tile_counts, [&](uint64_t p) { return repair_bit(broken, p) && !(p && repair_bit(broken, p - 1)); });
}

// Head p becomes record tile_offsets[its tile] + the heads before it in the tile, so the records are ordered by (read, first).
// The heads are dealt to consecutive threads (each bisects for its read and walks the bitmap to the stretch's end).  The
// record takes read, first = f and windows = r; the repair kernel fills in the rest.
__global__ void __launch_bounds__(256)
tbk_repair_stretches_kernel(const uint64_t *__restrict__ broken, uint64_t n, const uint64_t *__restrict__ offsets, uint64_t n_reads,
                            const uint64_t *__restrict__ flags, const unsigned long long *__restrict__ tile_offsets, uint64_t *__restrict__ records,
                            uint64_t n_records) {
    compact_scatter_tile_dense(n, flags, tile_offsets, [&](uint64_t p, uint64_t at) {
        if (at >= n_records) return;
        uint64_t word = p >> 6;
        uint64_t open = ~broken[word] & (~0ull << (p & 63u));  // the positions from p on that are not broken
        while (!open && (word + 1) * 64 < n) open = ~broken[++word];
        const uint64_t end = open ? word * 64 + (uint64_t)__builtin_ctzll(open) : n;  // one past the stretch's last window
        const uint64_t read = read_of_position(offsets, n_reads, p);
        const uint64_t r = end - p;
        records[5 * at] = read;
        records[5 * at + 1] = p - (offsets[read] + read);
        records[5 * at + 2] = 0;
        records[5 * at + 3] = r > 0xFFFFFFFFull ? 0xFFFFFFFFull : r;  // (the host refuses a sequence of 2^32 or more window starts)
        records[5 * at + 4] = 0;
    });
}

// ---- the repair kernel ---------------------------------------------------------------------------------------------------------
constexpr uint32_t TBK_R_CANDS = 256;  // candidates of a stretch: at most 8 k - 4 = 252

// the bits of x spread to the even places of 64
__device__ __forceinline__ uint64_t repair_spread(uint32_t x) {
    uint64_t v = x;
    v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
    v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
    v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}

// One wave per stretch, striding over the stretches by the grid.  With f, l, r of the record and np = k - r + 1 shared
// positions P = [l, f + k - 1], candidate number
//     3 i + j            is SUB(l + i, the j-th of the three other bases),   i < np, j < 3
//     3 np + i           is DEL(l + i),                                      i < np
//     4 np + 4 (i - 1) + b  is INS(l + i, b),                                1 <= i < np, b < 4
// so the numbers ascend as (kind, pos, base) does and end below 8 np - 4 <= 252.  The bases any candidate's windows touch,
// [l - k + 1, f + 2k - 2] clipped to the sequence - at most 94 - are loaded once, a byte or two per lane, and kept as
// three 128-bit planes that every lane holds: the two bits of the code and the not-ACGT mask, bit i = base lo + i.
// The work items (candidate, one of k window starts of the edited sequence) are laid flat over the lanes, 64 a step: a lane
// edits the planes by masks and shifts, cuts its window out of them, interleaves the two code planes into the
// reverse complement's rank and takes the forward rank from that, and searches it (db_search_group at width 1, the loop's
// branch the wave's: one load per step for all 64 lanes, a finished or idle lane reading entry 0).  A left-aligned duplicate, a window past the ends and a
// window that is not clean tally nothing.  The verdicts are gathered per candidate in LDS - support in the low byte, the
// windows below m above it, and the smallest counter - and reduced across the wave; lane 0 stores the record.
__global__ void __launch_bounds__(64)
tbk_repair_kernel(const uint8_t *__restrict__ sep, const uint64_t *__restrict__ offsets, int k, TbkDbView db, uint32_t m, uint32_t min_support,
                  uint64_t *__restrict__ records, uint64_t n_records) {
    __shared__ uint32_t tally[TBK_R_CANDS], depth[TBK_R_CANDS];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t km = k == 32 ? 0xFFFFFFFFu : ((1u << k) - 1u);
    const uint64_t kmask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1ull);
    const uint32_t uk = (uint32_t)k;
    for (uint64_t g = blockIdx.x; g < n_records; g += gridDim.x) {
        const uint64_t read = records[5 * g], f = records[5 * g + 1];
        const uint32_t r = (uint32_t)records[5 * g + 3];
        if (r > uk) {  // LONG (the same in every lane)
            if (lane == 0) records[5 * g + 3] = (uint64_t)r | (4ull << 48);
            continue;
        }
        const uint64_t S = offsets[read] + read, L = offsets[read + 1] - offsets[read];
        const uint64_t l = f + r - 1;
        const uint64_t lo = l >= (uint64_t)(uk - 1) ? l - (uk - 1) : 0;
        const uint64_t hi = std::min<uint64_t>(L - 1, f + 2 * uk - 2);
        const uint32_t n = (uint32_t)(hi - lo + 1);  // <= 3 k - 2
        for (uint32_t i = lane; i < TBK_R_CANDS; i += 64) { tally[i] = 0; depth[i] = 255u; }
        unsigned __int128 p0, p1, bad;
        {
            uint64_t w0[2], w1[2], wb[2];
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                const uint32_t i = 64 * h + lane;
                const uint32_t c = i < n ? sep[S + lo + i] : 0u;
                const uint32_t code = ((c >> 1) ^ (c >> 2)) & 3u;
                const uint32_t expect = 0x41u + 2u * (code & 1u) + 6u * (code >> 1) + 11u * (code & (code >> 1));
                w0[h] = __builtin_amdgcn_ballot_w64(code & 1u);
                w1[h] = __builtin_amdgcn_ballot_w64(code >> 1);
                wb[h] = __builtin_amdgcn_ballot_w64(c != expect);
            }
            p0 = (unsigned __int128)w0[0] | ((unsigned __int128)w0[1] << 64);
            p1 = (unsigned __int128)w1[0] | ((unsigned __int128)w1[1] << 64);
            bad = (unsigned __int128)wb[0] | ((unsigned __int128)wb[1] << 64);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const uint32_t np = uk - r + 1, n_cand = 8 * np - 4, items = n_cand * uk;
        const int64_t sL = (int64_t)L, sk = (int64_t)k;
#pragma unroll 1
        for (uint32_t t0 = 0; t0 < items; t0 += 64) {
            const uint32_t t = t0 + lane;
            const bool active = t < items;
            const uint32_t cand = active ? t / uk : 0, widx = active ? t - cand * uk : 0;
            uint32_t kind, i, b;
            if (cand < 3 * np) { kind = 1; i = cand / 3; b = cand - 3 * i; }
            else if (cand < 4 * np) { kind = 2; i = cand - 3 * np; b = 0; }
            else { kind = 3; i = 1 + ((cand - 4 * np) >> 2); b = (cand - 4 * np) & 3u; }
            const int64_t p = (int64_t)l + (int64_t)i;
            const uint32_t pl = (uint32_t)((uint64_t)p - lo);  // (< 2 k)
            const uint32_t cur = ((uint32_t)(p0 >> pl) & 1u) | (((uint32_t)(p1 >> pl) & 1u) << 1);
            const uint32_t prev = pl ? ((uint32_t)(p0 >> (pl - 1)) & 1u) | (((uint32_t)(p1 >> (pl - 1)) & 1u) << 1) : 0u;
            bool valid = active;
            int64_t upper;
            if (kind == 1) {
                b += b >= cur;
                upper = std::min<int64_t>(p, sL - sk);
            } else if (kind == 2) {
                valid = valid && !(i >= 1 && prev == cur);
                upper = std::min<int64_t>(p - 1, sL - 1 - sk);
            } else {
                valid = valid && !(i >= 2 && prev == b);
                upper = std::min<int64_t>(p, sL + 1 - sk);
            }
            const int64_t start = p - sk + 1 + (int64_t)widx;
            valid = valid && start >= 0 && start <= upper;
            const unsigned __int128 one = 1, at = one << pl, below = at - 1;
            const unsigned __int128 b0 = (unsigned __int128)(b & 1u) << pl, b1 = (unsigned __int128)(b >> 1) << pl;
            unsigned __int128 x0, x1, xb;
            if (kind == 1) {
                x0 = (p0 & ~at) | b0;
                x1 = (p1 & ~at) | b1;
                xb = bad;
            } else if (kind == 2) {
                x0 = (p0 & below) | ((p0 >> 1) & ~below);
                x1 = (p1 & below) | ((p1 >> 1) & ~below);
                xb = (bad & below) | ((bad >> 1) & ~below);
            } else {
                x0 = (p0 & below) | b0 | ((p0 & ~below) << 1);
                x1 = (p1 & below) | b1 | ((p1 & ~below) << 1);
                xb = (bad & below) | ((bad & ~below) << 1);
            }
            const uint32_t j = valid ? (uint32_t)((uint64_t)start - lo) : 0u;  // (start >= lo: the window holds p or p - 1; j + k <= 96)
            const uint32_t a0 = (uint32_t)(x0 >> j) & km, a1 = (uint32_t)(x1 >> j) & km;
            const bool ok = valid && ((uint32_t)(xb >> j) & km) == 0;
            const uint64_t rc = repair_spread(~a0 & km) | (repair_spread(~a1 & km) << 1);  // the reverse complement's rank: 3 - code i at bits 2 i
            const uint64_t fwd = lex_rank(~rc & kmask, k);                                // the window's own: code i at bits 2 (k - 1 - i)
            const uint64_t rank[1] = {fwd < rc ? fwd : rc};
            const bool oks[1] = {ok};
            uint32_t entry[1], cw[1];
            bool hit[1];
            db_search_group<1, true>(db, k, rank, oks, entry, hit, cw);  // (every lane of the wave is here)
            if (ok) {
                atomicAdd(&tally[cand], cw[0] >= m ? 1u : 257u);
                atomicMin(&depth[cand], cw[0]);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        uint32_t accepted = 0, best = TBK_R_CANDS;
        for (uint32_t cand = lane; cand < n_cand; cand += 64) {
            const uint32_t v = tally[cand];
            if ((v >> 8) == 0 && (v & 255u) >= min_support) {
                accepted++;
                best = std::min(best, cand);
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            accepted += __shfl_xor(accepted, d);
            best = std::min(best, (uint32_t)__shfl_xor(best, d));
        }
        if (lane == 0) {
            uint64_t pos = 0, kind = 0, base = 0, support = 0, least = 0;
            if (accepted) {
                uint32_t i, b;
                if (best < 3 * np) {
                    kind = 1; i = best / 3; b = best - 3 * i;
                    const uint32_t pl = (uint32_t)(l + i - lo);
                    b += b >= (((uint32_t)(p0 >> pl) & 1u) | (((uint32_t)(p1 >> pl) & 1u) << 1));
                } else if (best < 4 * np) { kind = 2; i = best - 3 * np; b = 4; }
                else { kind = 3; i = 1 + ((best - 4 * np) >> 2); b = (best - 4 * np) & 3u; }
                pos = l + i;
                base = b == 0 ? 'A' : b == 1 ? 'C' : b == 2 ? 'G' : b == 3 ? 'T' : 0;
                support = tally[best] & 255u;
                least = depth[best];
            }
            records[5 * g + 2] = pos;
            records[5 * g + 3] = (uint64_t)r | ((uint64_t)accepted << 32) | (kind << 48) | (base << 56);
            records[5 * g + 4] = support | (least << 8);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (lane 0's reads of the rows, before the next stretch clears them)
    }
}
static_assert(sizeof(tbk_repair) == 40, "a record is five 64-bit words: read, first, pos, then windows, accepted, kind and base, then support, depth and pad");
static_assert(8 * 32 - 4 <= TBK_R_CANDS, "the candidates of a stretch have a row each");

// =======================================================================================
// launchers (called from tbk_count.cpp; what the arguments hold: tbk_lookup_host.h)
// =======================================================================================
extern "C" hipError_t tbk_launch_repair_lookup(const uint8_t *d_sep, uint64_t total, uint64_t n_passes, int k, TbkDbView db, uint32_t m,
                                               uint32_t *d_clean, uint32_t *d_broken, uint64_t wave_slots, hipStream_t stream) {
    if (!n_passes) return hipSuccess;
    if (!tbk_db_view_ok(db, k) || m < 1 || m > 255) return hipErrorInvalidValue;
    const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_passes, wave_slots))), block(64);
    hipLaunchKernelGGL(tbk_repair_lookup_kernel, grid, block, 0, stream, d_sep, total, n_passes, k, db, m, d_clean, d_broken);
    return hipGetLastError();
}

extern "C" hipError_t tbk_launch_repair_heads(const uint32_t *d_broken, uint64_t n_passes, uint64_t *d_flags, unsigned long long *d_tile_counts,
                                              hipStream_t stream) {
    return compact_launch_tiles(n_passes * TBK_PASS, stream, tbk_repair_heads_kernel, reinterpret_cast<const uint64_t *>(d_broken), n_passes * TBK_PASS,
                                d_flags, d_tile_counts);
}

extern "C" hipError_t tbk_launch_repair_stretches(const uint32_t *d_broken, uint64_t n_passes, const uint64_t *d_offsets, uint64_t n_reads,
                                                  const uint64_t *d_flags, const unsigned long long *d_tile_offsets, tbk_repair *d_records,
                                                  uint64_t n_records, hipStream_t stream) {
    if (!n_records) return hipSuccess;
    if (!n_reads) return hipErrorInvalidValue;
    return compact_launch_tiles(n_passes * TBK_PASS, stream, tbk_repair_stretches_kernel, reinterpret_cast<const uint64_t *>(d_broken),
                                n_passes * TBK_PASS, d_offsets, n_reads, d_flags, d_tile_offsets, reinterpret_cast<uint64_t *>(d_records), n_records);
}

extern "C" hipError_t tbk_launch_repair(const uint8_t *d_sep, const uint64_t *d_offsets, int k, TbkDbView db, uint32_t m, uint32_t min_support,
                                        tbk_repair *d_records, uint64_t n_records, uint64_t wave_slots, hipStream_t stream) {
    if (!n_records) return hipSuccess;
    if (!tbk_db_view_ok(db, k) || m < 1 || m > 255 || min_support < 1 || min_support > 32) return hipErrorInvalidValue;
    const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_records, wave_slots))), block(64);
    hipLaunchKernelGGL(tbk_repair_kernel, grid, block, 0, stream, d_sep, d_offsets, k, db, m, min_support, reinterpret_cast<uint64_t *>(d_records),
                       n_records);
    return hipGetLastError();
}
