"""The later trips of the multi-read kernels' loop over their list of passes (csrc/tbk_kernels.hip: tbk_probe_kernel<.., MULTI = true>
and tbk_probe_entry_kernel<.., MULTI = true>), in every instantiation tbk_launch_probe_range can launch.  Every pass of 2048 window
starts that touches more than one read goes to these kernels, and they walk their list with a fixed grid of min(passes, 16384)
one-wave blocks: from 16 385 multi-read passes on - 33.5 Mbases of short reads - a wave takes a second pass, with LDS tallies that
the pass before it must have cleared, queues and a staged tile that it refills, and - in a sliced batch - foreign passes that it
must skip and go on (a slice's launch has a grid of the slice's passes over the whole batch's list, so a sliced batch loops at any
size: the one way older tests took later trips in the key layouts).  tbk_options.probe_max_blocks caps that grid, so that a batch the oracle can follow takes three and more trips
per wave (ROWS below); two batches of 68 Mbases take them with no cap at all (test_real_size_batch_*).  Counts are compared exactly
with the oracle's (c/kmers.c:245-299)."""
import functools

import numpy as np
import pytest

from test_gpu_full_keys import _assert_counts
from test_gpu_parity import _pack, _rc

pytestmark = pytest.mark.gpu

PASS = 2048       # TBK_PASS: window starts per pass
RCNT = 64         # TBK_RCNT: reads of a pass with tallies in LDS; the hits of later reads go to the global counters one by one
GRID = 16384      # tbk_launch_probe_range: blocks of the multi-read kernels' grid (one wave each)


def _passes(offs):
    """tbk_pass_index_kernel restated: per pass its first read, its last read, whether it is listed (touches more than one read)
    and whether it touches exactly two (the two-read kernel's, where that kernel is built and switched on)."""
    offs = np.asarray(offs).astype(np.int64)
    n, total = offs.size - 1, int(offs[-1])
    p0 = np.arange((total + PASS - 1) // PASS, dtype=np.int64) * PASS
    last = np.minimum(p0 + PASS - 1, total - 1)
    r_first = np.searchsorted(offs, p0, side="right") - 1
    r_last = np.searchsorted(offs, last, side="right") - 1
    r_end = offs[r_first + 1]
    listed = last >= r_end
    two = listed & (r_end > p0) & (offs[np.minimum(r_first + 2, n)] > last)
    return r_first, r_last, listed, two


def _tile(bases, offs, reps):
    offs = np.asarray(offs).astype(np.uint64)
    total = offs[-1]
    tiled = (np.arange(reps, dtype=np.uint64)[:, None] * total + offs[None, :-1]).ravel()
    return np.tile(np.asarray(bases, dtype=np.uint8), reps), np.concatenate([tiled, np.array([total * np.uint64(reps)], dtype=np.uint64)])


@functools.lru_cache(maxsize=None)
def _grid_case(orc, k):
    """One batch per k, built once: lists as in _boundary_case (every other k-mer of a random genome, split between the haplotypes:
    a window across a read boundary would be a hit if a kernel let it through); stretches of the genome cut into consecutive reads
    of 100 to 300 bases (every pass touches 7 to 20 reads), three stretches of tiny reads (list k-mers of both haplotypes on both
    strands as reads of k and k + 1 bases, between empty reads, 1-base reads and reads of k - 1: more than 64 reads a pass), reads
    of 5 to 15 kbases between them (single-read passes, passes that touch exactly two reads, a multi-read list with gaps in its
    pass numbers) and reads with N, lower case and bytes that are no base.  Under 100 kbases."""
    from trio_binning_amd import kmers

    rng = np.random.default_rng(8800 + k)
    genome = "".join("ACGT"[c] for c in rng.integers(0, 4, 60_000))
    starts = rng.permutation(len(genome) - k - 1)[:30_000]
    pos_a, pos_b = starts[:15_000], starts[15_000:]
    canon = lambda x: min(x, _rc(x))
    ka = np.array([kmers.kmer_to_int(canon(genome[p:p + k])) for p in pos_a], dtype=np.uint64)
    kb = np.array([kmers.kmer_to_int(canon(genome[p:p + k])) for p in pos_b], dtype=np.uint64)

    def stretch(at, n):
        out = []
        while n > 0:
            step = min(int(rng.integers(100, 301)), n)
            out.append(genome[at:at + step])
            at, n = at + step, n - step
        return out

    def tiny(n):
        out, used, i = [], 0, 0
        while used < n:
            pa, pb = int(pos_a[int(rng.integers(0, pos_a.size))]), int(pos_b[int(rng.integers(0, pos_b.size))])
            x = int(rng.integers(0, len(genome) - k))
            flip = (lambda s: s) if i % 2 == 0 else _rc
            group = [flip(genome[pa:pa + k]), "", "ACGT"[i % 4], flip(genome[pb:pb + k + 1]), genome[x:x + k - 1],
                     _rc(flip(genome[pb:pb + k])), "", _rc(flip(genome[pa:pa + k + 1])), "N" if i % 5 == 0 else "t"]
            out += group
            used += sum(map(len, group))
            i += 1
        return out

    short_1, short_2, short_3 = stretch(0, 14_500), stretch(41_000, 17_000), stretch(11_000, 16_500)
    tiny_1, tiny_2, tiny_3 = tiny(2_800), tiny(4_500), tiny(2_800)
    for i, (at, what) in enumerate([(20, "N"), (77, "n"), (50, "*"), (99, "R"), (31, "-")]):   # N, a byte that is no base, an IUPAC code
        r = short_2[5 + 9 * i]
        short_2[5 + 9 * i] = r[:at] + what + r[at + 1:]
    short_2[60] = short_2[60][:40] + short_2[60][40:90].lower() + short_2[60][90:]
    short_3[7] = short_3[7].lower()
    reads = (short_1 + [genome[14_500:19_700]] + tiny_1 + [genome[20_000:34_800], genome[35_000:41_100]] + short_2 + tiny_2
             + [genome[1_000:10_300]] + short_3 + tiny_3)
    assert sum(map(len, reads)) <= 100_000
    oa, ob = orc.table_from_keys(ka, k), orc.table_from_keys(kb, k)
    orders = {"forward": reads, "reversed": reads[::-1], "halves_swapped": reads[len(reads) // 2:] + reads[:len(reads) // 2]}
    batches = {}
    for name, order in orders.items():
        bases, offs = _pack(order)
        want = orc.count_batch(bases, offs, oa, ob)
        want.setflags(write=False)
        r_first, r_last, listed, two = _passes(offs)
        n_reads = r_last - r_first + 1
        # on the offsets alone: enough multi-read passes that a grid of three blocks takes them in four trips even where the
        # two-read passes have a kernel of their own, passes of 7 to 20 reads, of exactly two reads, and a list with gaps
        assert (listed & ~two).sum() >= 24 and two.sum() >= 1 and (~listed).sum() >= 8, (k, name)
        assert ((n_reads >= 7) & (n_reads <= 20)).sum() >= 18, (k, name)
        assert (np.diff(np.nonzero(listed)[0]) > 1).sum() >= 3, (k, name)
        assert n_reads.max() > RCNT and (n_reads > RCNT).sum() >= 3, (k, name, n_reads.max())
        # on the oracle's counts alone: reads beyond the 64th of their pass (every window of theirs in that pass) with hits of
        # either haplotype - what count_hits sends to the global counters
        offs_i = np.asarray(offs).astype(np.int64)
        ids = np.nonzero(offs_i[1:] - offs_i[:-1] >= k)[0]
        first_pass, last_pass = offs_i[ids] // PASS, (offs_i[ids + 1] - k) // PASS
        far = ids[(first_pass == last_pass) & (ids - r_first[first_pass] >= RCNT)]
        assert (want[far, 0] > 0).sum() >= 5 and (want[far, 1] > 0).sum() >= 5, (k, name, far.size)
        assert want.sum() > len(bases) // 8
        batches[name] = (bases, offs, want, int(listed.sum()), int(two.sum()), int(listed.size))
    # the short-read part by itself, for the batches of real size: every pass touches several reads
    bases, offs = _pack(short_1 + tiny_1 + short_2)
    want = orc.count_batch(bases, offs, oa, ob)
    assert want.sum() > len(bases) // 8
    return {"ka": ka, "kb": kb, "batches": batches, "short": (bases, offs, want)}


# ---- the variant matrix: one row for every MULTI = true instantiation of tbk_launch_probe_range's switch that kmers.Options reach ----
# The spans.  m <= 16 (32-bit m-mers) with t = m - w from 8 to 16, so that mod-sampling applies: k = 21 has room for w = 2 .. 7,
# w = 8 needs k = 23.  m > 16 (64-bit m-mers): k = 31.
SPAN32 = {2: (21, 16), 3: (21, 15), 4: (21, 16), 5: (21, 15), 6: (21, 16), 7: (21, 15), 8: (23, 16)}
SPAN64 = {2: (31, 18), 3: (31, 19), 4: (31, 18), 5: (31, 17), 6: (31, 18), 7: (31, 17), 8: (31, 18)}

# (layout, k, minimizer_w, minimizer_m, mod_sampling, front, span3)
ROWS = [("keys", 21, 0, 0, 1, 0, -1),       # tbk_probe_kernel<0, false, false, false, true>: plain hashing of the key
        ("keys", 21, 1, 15, 1, 0, -1),      # <1, false, ..>: one m-mer, no sampling rule, no front
        ("keys", 31, 1, 17, 1, 0, -1)]      # <1, true, ..>
# TBK_W(2) .. TBK_W(8): tbk_probe_kernel<W, M64, SAMP, FRONT, true>
ROWS += [("keys", span[w][0], w, span[w][1], samp, front, -1)
         for w in range(2, 9) for span in (SPAN32, SPAN64) for samp in (1, 0) for front in (0, 1)]
# TBK_E(2, 0) .. TBK_E(6, 0): narrow entries, tbk_probe_entry_kernel<W, true, false, 0, LW>, LW = 3 (t = m - 2w) and 2 (t = m - w)
ROWS += [("entries", SPAN32[w][0], w, SPAN32[w][1], 1, 0, span3) for w in range(2, 7) for span3 in (1, 0)]
# TBK_E(2, 2) .. TBK_E(6, 2), TBK_E2(7, 2), TBK_E2(8, 2): short keys, <W, true, false, 2, LW>; w = 7, 8 leave no t = m - 2w >= 4
ROWS += [("short_keys", SPAN32[w][0], w, SPAN32[w][1], 1, 0, span3) for w in range(2, 7) for span3 in (1, 0)]
ROWS += [("short_keys", SPAN32[w][0], w, SPAN32[w][1], 1, 0, -1) for w in (7, 8)]
# TBK_E2(2, 1) .. TBK_E2(8, 1): wide entries, <W, true, false, 1, 2>, and TBK_E2(2, 3) .. TBK_E2(8, 3): full keys, <W, true, false, 3, 2>
ROWS += [(layout, SPAN64[w][0], w, SPAN64[w][1], 1, 0, -1) for layout in ("wide_entries", "full_keys") for w in range(2, 9)]
# Not reached, because no options lead there:
#  - TBK_E2(7, 0), narrow entries at w = 7: tbk_entry_geom wants 4 (o + w - 1) + w <= 30 bits of flanks, and w = 7 needs 31 at o = 0;
#  - the key layouts at w >= 2 with m <= 16 AND m > 16 are both rows above, but front tables at w < 2 do not exist (refused by the
#    launcher), nor does a sampling rule there: W = 0 and W = 1 have the one (two) instantiations listed;
#  - wide entries and full keys with t = m - 2w, short keys and narrow entries at w = 7, 8 with it: the launcher refuses them.
# The same spans with m-mers of 32 bits in wide entries and full keys ((31, 8, 16), (21, 6, 16)) are no instantiations of their own
# (M64 is no template argument of the entry kernels); tests/test_gpu_full_keys.py runs three of them with a capped grid.


def _row_id(row):
    layout, k, w, m, samp, front, span3 = row
    return f"{layout}-k{k}-w{w}-m{m}" + ("" if samp else "-randmin") + ("-front" if front else "") + {1: "-3w", 0: "-2w", -1: ""}[span3]


def _options(row, **fields):
    from trio_binning_amd import kmers

    layout, k, w, m, samp, front, span3 = row
    name = layout if layout != "keys" else "keys" if w < 2 else "keys_front" if front else "keys_whole_lines"
    return kmers.Options.layout(name, minimizer_w=w, minimizer_m=m, mod_sampling=samp, span3=span3, **fields)


def _assert_variant(st, row):
    """the classifier is the instantiation the row names (tbk_mz_params shortens spans quietly, the policy changes layouts quietly)"""
    layout, k, w, m, samp, front, span3 = row
    t = 0 if w < 2 or not samp else m - 2 * w if span3 == 1 else m - w
    assert (st["minimizer_w"], st["minimizer_m"], st["sampling_t"]) == (w, m if w else st["minimizer_m"], t), (row, st)
    flags = (st["entry_layout"], st["wide_entries"], st["short_keys"], st["full_keys"], st["front_layout"])
    want = {"keys": (False, False, False, False, bool(front)), "entries": (True, False, False, False, False),
            "wide_entries": (True, True, False, False, False), "short_keys": (False, False, True, False, False),
            "full_keys": (False, False, False, True, False)}[layout]
    assert flags[:4] == want[:4] and (layout != "keys" or flags[4] == want[4]), (row, st)


def _run(cls, case, row, cap, two):
    """Four batches through one classifier: forwards and reversed in the packed transfer format, then - staged as ASCII - the batch
    with its halves swapped and the first one again.  -> the counts, each the oracle's"""
    st = cls.stats()
    use_two = bool(two) and st["minimizer_w"] >= 2 and st["sampling_t"] > 0   # tbk_probe_has_two_read_kernel
    outs = []
    assert cls.packed_transfer
    for packed, name in ((True, "forward"), (True, "reversed"), (False, "halves_swapped"), (False, "forward")):
        cls.packed_transfer = packed
        bases, offs, want, n_listed, n_two, n_passes = case["batches"][name]
        got = cls.classify_batch(bases, offs)
        assert cls.last_passes() == (n_passes, n_listed), (row, name, cls.last_passes(), n_passes, n_listed)
        # every wave of the capped grid takes three trips of the multi-read kernel's loop, wave 0 a fourth
        assert not cap or n_listed - (n_two if use_two else 0) >= 3 * cap + 1, (row, name, cap, n_listed, n_two)
        _assert_counts(got, want, row, cap, two, name, "packed" if packed else "ascii")
        outs.append(got)
    return outs


# (two_read_kernel, slice_bases): at 0 the passes of two reads join the multi-read list; 2048: an empty ring takes the batch in
# up to eight slices, each a launch of its own over the whole list (the slice filter)
MODES = [(1, 2048), (0, 0), (1, 0), (0, 2048)]


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_later_trips_of_the_multi_read_loop(gpu, orc, row):
    """Every instantiation with no cap and with grids of one, two and three blocks (tbk_options.probe_max_blocks is fixed when a
    classifier is made: each cap is a classifier of its own): a list of 24 and more multi-read passes is then 8 to 24 trips of each
    wave's loop.  Capped counts are the oracle's and, byte for byte, the uncapped classifier's."""
    from trio_binning_amd import kmers

    case = _grid_case(orc, row[1])
    with kmers.HashSet.from_keys(case["ka"], row[1]) as a, kmers.HashSet.from_keys(case["kb"], row[1]) as b:
        for two, slice_bases in MODES:
            plain = None
            for cap in (0, 1, 2, 3):
                with kmers.Classifier(a, b, options=_options(row, two_read_kernel=two, slice_bases=slice_bases, probe_max_blocks=cap)) as cls:
                    _assert_variant(cls.stats(), row)
                    outs = _run(cls, case, row, cap, two)
                if cap == 0:
                    plain = outs
                else:
                    assert all(x.tobytes() == y.tobytes() for x, y in zip(outs, plain)), (row, two, slice_bases, cap)


def test_the_matrix_is_the_launchers_switch():
    """ROWS against the switch it was read from, by count: 3 + 7 x 8 key-layout instantiations, 10 of narrow entries, 12 of short
    keys, 7 of wide entries, 7 of full keys, no row twice."""
    assert len(ROWS) == len(set(ROWS)) == 3 + 56 + 10 + 12 + 7 + 7
    assert {r[2] for r in ROWS if r[0] == "keys"} == set(range(9))
    assert all(m > 16 for _, k, w, m, *_ in ROWS if k == 31) and all(m <= 16 for _, k, w, m, *_ in ROWS if k != 31)


@pytest.mark.parametrize("layout", ["auto", "keys_front"])
def test_real_size_batch_takes_later_trips_with_no_cap(gpu, orc, layout):
    """No hook: the short-read part of the k = 21 batch, tiled until it holds 2 x 16384 + 1 multi-read passes and more (68 Mbases;
    unsliced: the default slice_bases), so that every wave of the real grid takes a second trip and wave 0 a third.  Counts depend
    on the read alone: the expected result is the oracle's counts of the small batch, tiled."""
    from trio_binning_amd import kmers

    case = _grid_case(orc, 21)
    bases, offs, want = case["short"]
    reps = -(-(2 * GRID + 1) * PASS // len(bases)) + 1
    big_bases, big_offs = _tile(bases, offs, reps)
    r_first, r_last, listed, two = _passes(big_offs)
    assert listed.sum() >= 2 * GRID + 1 and listed.all() and not two.any()   # short reads: every pass is the multi-read kernel's
    with kmers.HashSet.from_keys(case["ka"], 21) as a, kmers.HashSet.from_keys(case["kb"], 21) as b, kmers.Classifier(a, b, options=kmers.Options.layout(layout)) as cls:
        st = cls.stats()
        if layout == "keys_front":
            assert st["front_layout"] and not (st["entry_layout"] or st["short_keys"] or st["full_keys"]), st
        got = cls.classify_batch(big_bases, big_offs)
        assert cls.last_passes() == (listed.size, int(listed.sum())), (cls.last_passes(), listed.size, st)
    assert got.shape == (reps * want.shape[0], 2)
    _assert_counts(got, np.tile(want, (reps, 1)), layout, st)
