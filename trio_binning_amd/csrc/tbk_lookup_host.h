// tbk_lookup_host.h — the window lookup of a query session as the host sees it: what the kernels read of a count database
// (TbkDbView) and the one declaration of every launcher of tbk_query.hip, tbk_depth.hip, tbk_repair.hip, tbk_screen.hip, tbk_read_depth.hip and tbk_pieces.hip;
// included by the .hip files that define the launchers (a signature that drifts is a compile error) and by tbk_count.cpp, which
// calls them.  The kernels' side: tbk_lookup.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tbk.h"

// A sorted count database as a search reads it: its ranks and counters (borrowed) and the directory over the top prefix_bits
// bits of the 2k-bit rank - dir[p] is the first entry whose rank has prefix >= p, dir[2^prefix_bits] = n.  A lane whose search
// is over reads entry 0 again, so keys and counts hold one entry at least: for an empty database the host passes one of padding.
struct TbkDbView {
    const uint64_t *keys;
    const uint8_t *counts;
    const uint32_t *dir;
    uint32_t n;
    int prefix_bits;
};

// what every launcher asks of k and of a view before it launches
inline bool tbk_db_view_ok(const TbkDbView &db, int k) { return k >= 1 && k <= 32 && db.prefix_bits >= 0 && db.prefix_bits <= 2 * k; }

extern "C" {
// ---- tbk_query.hip (tbk_launch_query_directory: tbk_compact_host.h, shared with the het-mer call) ----
// bitmaps: 64 words per pass each; d_bytes (NULL: not asked for): TBK_PASS bytes per pass; d_copies may be NULL
hipError_t tbk_launch_query_lookup(const uint8_t *d_sep, uint64_t total, uint64_t n_passes, int k, TbkDbView db, uint32_t min_count, uint32_t *d_clean,
                                   uint32_t *d_found, uint8_t *d_bytes, unsigned long long *d_hist, uint32_t *d_seen, uint32_t *d_copies,
                                   uint64_t wave_slots, hipStream_t stream);
hipError_t tbk_launch_query_totals(const uint32_t *d_clean, const uint32_t *d_found, const uint64_t *d_offsets, uint64_t n_reads,
                                   unsigned long long *d_totals, uint64_t wave_slots, hipStream_t stream);
hipError_t tbk_launch_query_counts(const uint8_t *d_bytes, const uint64_t *d_offsets, uint64_t n_reads, uint8_t *d_counts, uint64_t wave_slots,
                                   hipStream_t stream);
// d_out: 2 sums, zeroed by the caller (seen and solid, solid)
hipError_t tbk_launch_query_completeness(const uint8_t *d_counts, const uint32_t *d_seen, uint64_t n, uint32_t ci, uint32_t cx,
                                         unsigned long long *d_out, hipStream_t stream);
// d_spec: 6 x 256 sums, zeroed by the caller
hipError_t tbk_launch_query_spectrum(const uint8_t *d_counts, const uint32_t *d_copies, uint64_t n, unsigned long long *d_spec, hipStream_t stream);

// ---- tbk_depth.hip: the copy-number track ----
// bitmaps: 64 words per pass each; d_c and d_a: TBK_PASS bytes per pass each; d_copies: the session's copy counters, beside the
// view's counters; peak: at most 509 (the kernel's comment)
hipError_t tbk_launch_depth_lookup(const uint8_t *d_sep, uint64_t total, uint64_t n_passes, int k, TbkDbView db, const uint32_t *d_copies, uint32_t peak,
                                   uint32_t *d_clean, uint32_t *d_present, uint32_t *d_saturated, uint32_t *d_collapsed, uint32_t *d_expanded,
                                   uint8_t *d_c, uint8_t *d_a, uint64_t wave_slots, hipStream_t stream);
// d_prefix: n_reads + 1 running sums of bins, d_prefix[n_reads] = n_bins; d_bins: n_bins x 24 bytes
hipError_t tbk_launch_depth_bins(uint32_t *d_clean, uint32_t *d_present, uint32_t *d_saturated, uint32_t *d_collapsed, uint32_t *d_expanded, uint8_t *d_c,
                                 uint8_t *d_a, const uint64_t *d_offsets, const uint64_t *d_prefix, uint64_t n_reads, uint64_t n_bins, int k,
                                 uint32_t window, tbk_depth_bin *d_bins, uint64_t wave_slots, hipStream_t stream);

// ---- tbk_repair.hip: the repair candidates ----
// bitmaps: 64 words per pass each; m: the threshold, 1..255
hipError_t tbk_launch_repair_lookup(const uint8_t *d_sep, uint64_t total, uint64_t n_passes, int k, TbkDbView db, uint32_t m, uint32_t *d_clean,
                                    uint32_t *d_broken, uint64_t wave_slots, hipStream_t stream);
// the heads among the n_passes * 2048 stream positions of d_broken: d_flags and d_tile_counts as Compaction holds them for that many
hipError_t tbk_launch_repair_heads(const uint32_t *d_broken, uint64_t n_passes, uint64_t *d_flags, unsigned long long *d_tile_counts, hipStream_t stream);
// d_records: n_records x 40 bytes, read, first and windows of every stretch, in order
hipError_t tbk_launch_repair_stretches(const uint32_t *d_broken, uint64_t n_passes, const uint64_t *d_offsets, uint64_t n_reads, const uint64_t *d_flags,
                                       const unsigned long long *d_tile_offsets, tbk_repair *d_records, uint64_t n_records, hipStream_t stream);
// the records completed in place
hipError_t tbk_launch_repair(const uint8_t *d_sep, const uint64_t *d_offsets, int k, TbkDbView db, uint32_t m, uint32_t min_support,
                             tbk_repair *d_records, uint64_t n_records, uint64_t wave_slots, hipStream_t stream);

// ---- tbk_screen.hip: the read evidence ----
// bitmaps: 64 words per pass each; [c_lo, c_hi]: the counters that hold a window, c_lo >= 1; empty when c_lo > c_hi
hipError_t tbk_launch_screen_lookup(const uint8_t *d_sep, uint64_t total, uint64_t n_passes, int k, TbkDbView db, uint32_t c_lo, uint32_t c_hi,
                                    uint32_t *d_clean, uint32_t *d_held, uint64_t wave_slots, hipStream_t stream);
// d_records: n_reads x 40 bytes.  Four sequences to a block: the grid-stride loop takes a second trip from 4 wave_slots + 1 sequences on.
hipError_t tbk_launch_screen_evidence(const uint32_t *d_clean, const uint32_t *d_held, const uint64_t *d_offsets, uint64_t n_reads, int k,
                                      tbk_read_evidence *d_records, uint64_t wave_slots, hipStream_t stream);

// ---- tbk_read_depth.hip: the read depth ----
// d_clean: 64 words per pass; d_depth: TBK_PASS bytes per pass, every one written; m: the threshold, 1..255
hipError_t tbk_launch_read_depth_lookup(const uint8_t *d_sep, uint64_t total, uint64_t n_passes, int k, TbkDbView db, uint32_t m, uint32_t *d_clean,
                                        uint8_t *d_depth, uint64_t wave_slots, hipStream_t stream);
// d_records: n_reads x 40 bytes; no sequence has 2^32 window starts or more.  Four sequences to a block, as the evidence has them.
hipError_t tbk_launch_read_depth(const uint32_t *d_clean, const uint8_t *d_depth, const uint64_t *d_offsets, uint64_t n_reads, tbk_read_depth *d_records,
                                 uint64_t wave_slots, hipStream_t stream);

// ---- tbk_pieces.hip: the read pieces (the lookup and the evidence are tbk_screen.hip's) ----
// d_side: 64 words per pass, one bit per stream position.  The covered side (uncovered 0) overwrites every word; the uncovered
// side wants the words zeroed by the caller: the separators are scattered into them first and the side replaces them in place.
hipError_t tbk_launch_pieces_side(const uint32_t *d_held, const uint64_t *d_offsets, uint64_t n_reads, uint64_t total, uint64_t n_passes, int k,
                                  int uncovered, uint32_t *d_side, uint64_t wave_slots, hipStream_t stream);
// the starts (end 0) or the last positions (end 1) of the runs among the n_passes * 2048 positions of d_side: d_flags and
// d_tile_counts as Compaction holds them for that many
hipError_t tbk_launch_pieces_flag(const uint32_t *d_side, uint64_t n_passes, int end, uint64_t *d_flags, unsigned long long *d_tile_counts,
                                  hipStream_t stream);
// d_pieces: n_pieces x 24 bytes, in stream order.  The ends first - every record's `end` as a stream position - then the starts,
// which find the record's read, write read and first and bring `end` into the read's coordinates.
hipError_t tbk_launch_pieces_ends(uint64_t n_passes, const uint64_t *d_flags, const unsigned long long *d_tile_offsets, tbk_read_piece *d_pieces,
                                  uint64_t n_pieces, hipStream_t stream);
hipError_t tbk_launch_pieces_starts(uint64_t n_passes, const uint64_t *d_offsets, uint64_t n_reads, const uint64_t *d_flags,
                                    const unsigned long long *d_tile_offsets, tbk_read_piece *d_pieces, uint64_t n_pieces, hipStream_t stream);
// d_keys: n_reads words, zeroed by the caller: per read the largest (length << 32 | ~first) of its pieces of min_length or more
hipError_t tbk_launch_pieces_best(const tbk_read_piece *d_pieces, uint64_t n_pieces, uint64_t min_length, unsigned long long *d_keys,
                                  uint64_t wave_slots, hipStream_t stream);
// the pieces of min_length or more and, with d_keys (NULL: all of them), those that are their read's best: flag, then scatter
hipError_t tbk_launch_pieces_keep_flag(const tbk_read_piece *d_pieces, uint64_t n_pieces, uint64_t min_length, const unsigned long long *d_keys,
                                       uint64_t *d_flags, unsigned long long *d_tile_counts, hipStream_t stream);
hipError_t tbk_launch_pieces_keep(const tbk_read_piece *d_pieces, uint64_t n_pieces, const uint64_t *d_flags, const unsigned long long *d_tile_offsets,
                                  tbk_read_piece *d_out, uint64_t n_out, hipStream_t stream);
}
