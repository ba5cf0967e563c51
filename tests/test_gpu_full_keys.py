"""Full keys (csrc/tbk_common.h "full keys"): list k-mers as 64-bit keys in the entry kernels' line, read through
tbk_probe_entry_kernel<W, MULTI, TWO, 3, 2> - and wide entries at m-mers beyond 16 bases, the other half of the 2 x 1e9
31-mer tables.  At the sizes of the other tests the policy picks w = 8 and m = 15 or 16 for full keys, so here the span is
pinned (tbk_options.minimizer_w / minimizer_m) to reach every W from 2 to 8, m-mers of 17 to 24 bases (the 64-bit m-mer
arithmetic) and t = m - w from 8 to 16.  Every case first asserts the layout and span it meant to test - tbk_mz_params
shortens w quietly and the policy falls back to other layouts quietly - then compares the counts with the oracle's
(c/kmers.c:245-299) or with the recorded output of the real reference."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from test_gpu_entry import _case
from test_gpu_parity import _boundary_case, _pack, _rand_reads, _rc, _write

pytestmark = pytest.mark.gpu


def _mz_params(k, w_target, n_keys, m_force):
    """tbk_mz_params (csrc/tbk_common.h) under mod-sampling, restated: (w, m, t)"""
    w_target = min(w_target, 8)
    m_need = 15
    while m_need < 32 and n_keys * w_target > 0.9 * 0.5 * float(1 << (2 * m_need)):
        m_need += 1
    m0 = max(m_need, 16)
    for w in range(w_target, 0, -1):
        for m in ([m_force] if m_force > 0 else [m0, m0 - 1, m0 + 1]):
            if m_force <= 0 and (m < 15 or m < m_need):
                continue
            span = m + w - 1
            if span <= k and (k - span) % 2 == 0:
                return w, m, (m - w if w >= 2 and 8 <= m - w <= 16 else 0)
    return 0, 0, 0


def _full_geom(k, w, m, t):
    """tbk_full_geom (csrc/tbk_common.h) for a span whose t is m - w"""
    return 3 <= k <= 31 and 2 <= w <= 8 and 0 < t <= 16 and 8 <= m <= 24


def _assert_span(st, layout, w, m):
    assert st[layout] and st["minimizer_w"] == w and st["minimizer_m"] == m and st["sampling_t"] == m - w, (layout, w, m, st)


def _assert_counts(got, want, *what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert np.array_equal(got, want), (*what, bad[:10].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


# (k, w, m): every W from 2 to 8, m <= 16 and every m from 17 to 24, t = m - w from 8 ((23, 2, 10), (21, 7, 15)) to 16
# ((31, 8, 24), (31, 2, 18), (31, 3, 19)), k from 17 to 31; (31, 8, 18) is the span of the 2 x 1e9 31-mer table.
# (27, 7, 21) is the one m = 21 case.
FULL = [(31, 8, 18), (31, 8, 24), (31, 2, 18), (31, 3, 19), (31, 4, 18), (31, 5, 17), (31, 6, 20), (29, 7, 17), (29, 8, 22),
        (30, 8, 23), (28, 6, 17), (27, 3, 17), (27, 5, 19), (27, 7, 21), (26, 2, 17), (26, 7, 18), (25, 6, 20), (25, 2, 16),
        (23, 2, 10), (23, 3, 15), (21, 7, 15), (19, 4, 16), (17, 2, 16)]


@pytest.mark.parametrize("k,w,m", FULL)
@pytest.mark.parametrize("load", [0.3, 12.0])
def test_full_keys_counts_equal_the_oracle(gpu, orc, tmp_path, k, w, m, load):
    """The lists and reads of the entry layouts' matrix (tests/test_gpu_entry.py: runs around SNPs, a repeat, low
    complexity, a palindromic stretch, keys shared with hapA, duplicates, stretches whose variants crowd one line) in a
    roomy table and in one whose lines fill (twelve keys asked for per line of fifteen: keys behind the front, keys that
    walk past their line), sliced into passes and in one piece."""
    from trio_binning_amd import kmers

    assert _full_geom(k, *_mz_params(k, w, 1, m)) and _mz_params(k, w, 1, m)[:2] == (w, m)
    rng = np.random.default_rng(50000 + 1000 * k + 10 * m + w + int(load))
    a, b, bases, offs, want, reads = _case(rng, k, tmp_path, orc, crowd_cores=6)
    for slice_bases in (2048, 0):
        with kmers.Classifier(a, b, options=kmers.Options.layout("full_keys", minimizer_w=w, minimizer_m=m, full_load=load, slice_bases=slice_bases)) as cls:
            st = cls.stats()
            _assert_span(st, "full_keys", w, m)
            if load > 1:
                assert st["keys_behind_front"] > 0 and st["keys_past_half"] > 0, st
            got = cls.classify_batch(bases, offs)
        _assert_counts(got, want, k, w, m, load, slice_bases, st)


WIDE_LONG = [(31, 8, 18), (31, 6, 20), (32, 7, 18), (29, 7, 17), (27, 5, 19), (26, 2, 17)]


@pytest.mark.parametrize("k,w,m", WIDE_LONG)
@pytest.mark.parametrize("load", [0.1, 2.8])
def test_wide_entries_at_long_mmers_equal_the_oracle(gpu, orc, tmp_path, k, w, m, load):
    """Wide entries with m-mers of 17 to 20 bases (tbk_wentry_bucket's 64-bit arithmetic: what haplotype-shaped lists of
    2 x 1e9 31-mers get), roomy (0.1 entries per list and line) and crowded (2.8)."""
    from trio_binning_amd import kmers

    rng = np.random.default_rng(60000 + 1000 * k + 10 * m + w + int(load))
    a, b, bases, offs, want, reads = _case(rng, k, tmp_path, orc, crowd_cores=6)
    for slice_bases in (2048, 0):
        with kmers.Classifier(a, b, options=kmers.Options.layout("wide_entries", minimizer_w=w, minimizer_m=m, wentry_load=load, slice_bases=slice_bases)) as cls:
            st = cls.stats()
            _assert_span(st, "wide_entries", w, m)
            assert st["entry_layout"] and st["entries_a"] + st["entries_b"] < st["distinct_a"] + st["distinct_b"], st   # runs merged
            if load > 1:
                assert st["keys_behind_front"] > 0 and st["keys_past_half"] > 0, st
            got = cls.classify_batch(bases, offs)
        _assert_counts(got, want, k, w, m, load, slice_bases, st)


@functools.lru_cache(maxsize=None)
def _boundary(k):
    return _boundary_case(np.random.default_rng(7100 + k), k)


# (layout, k, w, m): every layout of the entry kernels (KIND 0 narrow entries, 1 wide entries, 2 short keys, 3 full keys)
TWO_READ = [("entries", 21, 6, 16), ("short_keys", 21, 6, 16), ("wide_entries", 31, 6, 16), ("wide_entries", 31, 8, 18),
            ("full_keys", 31, 8, 16), ("full_keys", 31, 8, 18), ("full_keys", 25, 6, 18)]


@pytest.mark.parametrize("layout,k,w,m", TWO_READ)
@pytest.mark.parametrize("mode", ["two_read_kernel", "multi_read_kernel", "multi_read_grid_loops"])
def test_entry_kernels_at_every_boundary_offset(gpu, orc, layout, k, w, m, mode):
    """The reads of test_two_read_passes_at_every_boundary_offset (cuts on every offset mod 32, 1 .. k from both ends of a
    pass, dense with list k-mers on both sides and across them) through the entry kernels: passes that touch two reads in
    the two-read kernel (the read boundary folded into the lanes' masks), in the multi-read kernel, and in the multi-read
    kernel with a grid of three blocks that loops over its list."""
    from trio_binning_amd import kmers

    ka, kb, reads = _boundary(k)
    oa, ob = orc.table_from_keys(ka, k), orc.table_from_keys(kb, k)
    a, b = kmers.HashSet.from_keys(ka, k), kmers.HashSet.from_keys(kb, k)
    fields = {"two_read_kernel": {}, "multi_read_kernel": {"two_read_kernel": 0}, "multi_read_grid_loops": {"two_read_kernel": 0, "probe_max_blocks": 3}}[mode]
    flag = {"entries": "entry_layout", "short_keys": "short_keys", "wide_entries": "wide_entries", "full_keys": "full_keys"}[layout]
    orders = [(order, _pack(order)) for order in (reads, reads[::-1])]
    wants = [orc.count_batch(bases, offs, oa, ob) for _, (bases, offs) in orders]
    for slice_bases in (2048, 0):
        with kmers.Classifier(a, b, options=kmers.Options.layout(layout, minimizer_w=w, minimizer_m=m, slice_bases=slice_bases, **fields)) as cls:
            st = cls.stats()
            assert st[flag] and st["minimizer_w"] == w and st["minimizer_m"] == m and st["sampling_t"] > 0, st
            assert st["entry_layout"] == (layout in ("entries", "wide_entries")) and st["wide_entries"] == (layout == "wide_entries"), st
            if layout in ("wide_entries", "full_keys"):
                assert st["sampling_t"] == m - w, st
            for (order, (bases, offs)), want in zip(orders, wants):
                assert want.sum() > len(bases) // 8
                got = cls.classify_batch(bases, offs)
                _assert_counts(got, want, layout, k, mode, slice_bases, order is reads)
                assert cls.last_passes()[1] >= 40   # most cuts leave a pass with two reads


@pytest.mark.parametrize("seed", range(int(os.environ.get("TBK_FUZZ_SEEDS", "24"))))  # more seeds for a soak run
def test_seeded_fuzz_of_full_keys(gpu, orc, tmp_path, seed):
    """Random small full-key configurations: k from 17 to 31, any span, m at the default or pinned from 17 to 24, tables
    from roomy to lines that fill; lists of what makes ranks tie and m-mers palindromic, and the edge keys of the slot
    encoding - A x k (key 0: a stored word of all key bits), T x k (not canonical: dead in the reference), at k = 31
    A x 30 + C (the canonical form of G + T x 30, which is what an invalid window looks up: TBK_FULL_NOKEY) and keys with
    bit 61 set - next to N and across pass boundaries, on both strands."""
    from trio_binning_amd import kmers

    rng = np.random.default_rng(47000 + seed)
    k = 31 if rng.random() < 0.3 else int(rng.integers(17, 31))   # (31 more often than the rest: the slot encoding's edge keys)
    w = int(rng.integers(2, 9))
    pinnable = [x for x in range(17, 25) if _full_geom(k, *_mz_params(k, w, 1, x))]
    m = int(rng.choice(pinnable)) if pinnable and rng.random() < 0.7 else 0
    load = float(rng.choice([0.1, 2.0, 6.0, 12.0]))
    slice_bases = int(rng.choice([2048, 5000, 0]))
    n_a, n_b = int(rng.integers(1, 1500)), int(rng.integers(1, 1500))

    def rand_bases(n):
        return "".join("ACGT"[c] for c in rng.integers(0, 4, n))

    def rand_kmer():
        mode = rng.random()
        if mode < 0.15:   # low complexity: long runs of one base
            return ("ACGT"[int(rng.integers(0, 4))] * k)[: int(rng.integers(0, k + 1))].ljust(k, "ACGT"[int(rng.integers(0, 4))])
        if mode < 0.3:    # short-period repeat
            return (rand_bases(int(rng.integers(1, 5))) * k)[:k]
        if mode < 0.4:    # its own reverse complement in the middle
            half = rand_bases((k + 1) // 2)
            return (half + _rc(half))[:k]
        return rand_bases(k)

    edges = ["A" * k, "T" * k]
    if k == 31:
        edges += ["A" * 30 + "C"]
        edges += ["A" + rand_bases(29) + "G" for _ in range(6)] + ["A" + rand_bases(29) + "T" for _ in range(6)]   # bit 61 set (canonical and not)
    la = [rand_kmer() for _ in range(n_a)]
    lb = [rand_kmer() for _ in range(n_b)]
    run = rand_bases(400)                                                    # runs of overlapping k-mers
    la += [run[i:i + k] for i in range(0, 150)]
    lb += [_rc(run[i:i + k]) for i in range(200, 350)]
    lb += [la[int(i)] for i in rng.integers(0, n_a, min(20, n_a))]          # shared with hapA
    lb += [_rc(la[int(i)]) for i in rng.integers(0, n_a, min(10, n_a))]     # shared, other strand
    la += [la[int(i)] for i in rng.integers(0, n_a, 5)]                     # duplicates
    la += edges[0::2]
    lb += edges[1::2]
    la += [rand_bases(int(rng.integers(1, k))), rand_bases(k + 3)]          # a short and a long line (c/kmers.c:113, 124-146)
    la = [rand_bases(k)] + [la[int(i)] for i in rng.permutation(len(la))]   # (the first line says k)
    fa = _write(tmp_path, "a.txt", "".join(x + "\n" for x in la))
    fb = _write(tmp_path, "b.txt", "\n".join(lb))
    oa, ob = orc.table_from_file(fa), orc.table_from_file(fb)
    a, b = kmers.HashSet.from_file(fa), kmers.HashSet.from_file(fb)
    assert (a.k, b.k, a.num_kmers, b.num_kmers) == (oa.k, ob.k, oa.num_kmers, ob.num_kmers)
    lists = [x for x in la + lb if len(x) == k]
    reads = _rand_reads(rng, int(rng.integers(1, 100)), int(rng.choice([40, 300, 2500, 9000])), lists, k, p_plant=0.9)
    for e in edges:   # the edge keys on both strands, beside an N, and in one read of many
        reads += [e, _rc(e), "N" + e + "N", e + "N" + _rc(e), rand_bases(30) + e + "n" + rand_bases(30)]
    reads.append("".join(x + "N" for x in edges + [_rc(e) for e in edges] + lists[:40]))
    reads += ["", "A" * (k - 1), lists[0], "".join(_rc(x) for x in lb[:40]), run, _rc(run), "A" * 500, "T" * 500, "AT" * 300]
    body = rand_bases(5000)
    for e in edges:   # the edge keys across a pass boundary (2048 window starts per pass)
        reads += [body[: max(0, 2048 - sum(map(len, reads)) % 2048 - k // 2)] + e + _rc(e)]
    reads += [body[: 2048 - sum(map(len, reads)) % 2048], body[:2047], body[:2048 + k - 1], body[:4096]]
    noisy = list(body[:3000])
    for i in rng.integers(0, 3000, 40):
        noisy[int(i)] = "NnacgtR-"[int(rng.integers(0, 8))]
    reads.append("".join(noisy))
    reads = [reads[int(i)] for i in rng.permutation(len(reads))]
    bases, offs = _pack(reads)
    want = orc.count_batch(bases, offs, oa, ob, strict=True)
    zw, zm, zt = _mz_params(k, w, max(len(la), len(lb)), m)
    opts = kmers.Options.layout("full_keys", minimizer_w=w, minimizer_m=m, full_load=load, slice_bases=slice_bases)
    with kmers.Classifier(a, b, options=opts) as cls:
        st = cls.stats()
        if _full_geom(k, zw, zm, zt):
            _assert_span(st, "full_keys", zw, zm)
        else:
            assert not st["full_keys"], (k, w, m, st)   # (a span full keys cannot take: the key layouts)
        got = cls.classify_batch(bases, offs)
        again = cls.classify_batch(bases, offs)
    _assert_counts(got, want, seed, k, w, m, load, slice_bases, st)
    assert np.array_equal(again, want)


@pytest.mark.parametrize("k,w,m", [(27, -1, 0), (27, 8, 18), (27, 6, 20), (31, -1, 0), (31, 8, 18), (31, 6, 20), (32, -1, 0)])
def test_full_keys_on_the_reference_vectors(gpu, tmp_path, k, w, m):
    """The recorded counts of the real reference (tests/golden/diff_vectors.json) through full keys, at the span the policy
    picks and at pinned ones; the per-read entry point (the single-read kernel alone) gives the batch's counts.  k = 32 has
    no full keys (a key and its list bit do not fit 64 bits): asked for, the classifier builds another layout and says so."""
    from trio_binning_amd import kmers

    v = next(x for x in load_golden("diff_vectors.json") if x["k"] == k)
    a = kmers.HashSet.from_file(_write(tmp_path, "a.txt", "".join(x + "\n" for x in v["list_a"])))
    b = kmers.HashSet.from_file(_write(tmp_path, "b.txt", "".join(x + "\n" for x in v["list_b"])))
    assert [a.num_kmers, b.num_kmers] == v["num_kmers"]
    fields = {"minimizer_w": w, "minimizer_m": m} if w > 0 else {}
    with kmers.Classifier(a, b, options=kmers.Options.layout("full_keys", **fields)) as cls:
        st = cls.stats()
        if k == 32:
            assert not st["full_keys"] and not st["entry_layout"] and not st["short_keys"], st
        elif w > 0:
            _assert_span(st, "full_keys", w, m)
        else:
            assert st["full_keys"] and st["sampling_t"] == st["minimizer_m"] - st["minimizer_w"], st
        got = cls.classify_reads(v["reads"])
        assert got.tolist() == v["counts"], st
        if (k, w, m) == (31, 8, 18):
            for i, r in enumerate(v["reads"]):
                assert list(cls.count_read(r)) == v["counts"][i], (i, len(r))


def _host_lists(kind, k, n):
    import ctypes as C

    from test_gpu_sweep import _lists
    from trio_binning_amd._lib import check, lib

    d_a, d_b, n_a, n_b, base = _lists(None, kind, k, n)
    ha, hb = np.empty(n_a, dtype=np.uint64), np.empty(n_b, dtype=np.uint64)
    check(lib.tbk_memcpy_d2h(0, ha.ctypes.data, C.c_void_p(d_a), n_a * 8))
    check(lib.tbk_memcpy_d2h(0, hb.ctypes.data, C.c_void_p(d_b), n_b * 8))
    check(lib.tbk_device_free(0, C.c_void_p(base)))
    return ha, hb


_FULL_BUILD = re.compile(r"^tbk build: full keys(?!,)", re.M)   # a full-key build (kept, thrown away or given up), not the sample


@pytest.mark.parametrize("case", ["uniform_31", "haplotypes_31", "small_haplotypes_31", "uniform_25_m18"])
def test_the_policy_picks_full_keys(gpu, capfd, case):
    """What the lists decide by themselves (tbk_host.cpp classifier_build), told by the build log (build_timing):
    uniform 31-mers get full keys in one build - from 2^22 lines on after a sample by bucket (a sixteenth of the buckets,
    hapA's list alone); haplotype-shaped ones get wide entries - the sample sees them crowd the fronts, and no full-key
    build runs; below 2^22 lines there is no sample: the full-key build is given up after hapA's list, and they still end
    in wide entries; uniform 25-mers whose m-mers are pinned beyond 16 bases (no short keys there) get full keys.  Each
    table is swept key by key (trio_binning_amd/sweep.py), not sampled."""
    from trio_binning_amd import kmers
    from trio_binning_amd.sweep import full_membership_sweep

    kind, k, n, fields = {"uniform_31": ("uniform", 31, 5_000_000, {}), "haplotypes_31": ("haplotypes", 31, 6_000_000, {}),
                          "small_haplotypes_31": ("haplotypes", 31, 300_000, {}), "uniform_25_m18": ("uniform", 25, 1_000_000, {"minimizer_m": 18})}[case]
    ha, hb = _host_lists(kind, k, n)
    capfd.readouterr()
    with kmers.HashSet.from_keys(ha, k) as a, kmers.HashSet.from_keys(hb, k) as b, kmers.Classifier(a, b, options=kmers.Options(build_timing=1, **fields)) as cls:
        st = cls.stats()
        log = capfd.readouterr().err
        sampled = "full keys, a sixteenth of the buckets" in log
        big = ha.size + hb.size >= 2 * (1 << 22)
        assert big == (n > 1_000_000) and sampled == big, (case, ha.size, hb.size, log, st)
        if kind == "uniform":
            assert st["full_keys"] and st["layout_builds"] == 1 and len(_FULL_BUILD.findall(log)) == 1, (case, log, st)
            assert st["n_buckets"] >= (1 << 22) or not big, (case, st)
            if "minimizer_m" in fields:
                _assert_span(st, "full_keys", 6, 18)
        else:
            assert st["wide_entries"] and not st["full_keys"], (case, log, st)
            if big:
                assert not _FULL_BUILD.search(log), (case, log, st)   # the sample alone sent them on
            else:
                assert "tbk build: full keys (given up after hapA's list)" in log, (case, log, st)
        rec = full_membership_sweep(cls, a, b, a.device_keys, b.device_keys, ha.size, hb.size, k, chunk=1 << 20)
        assert rec["ok"], (case, [r for r in rec["legs"] if not r["ok"]])
