"""The hit tracker (kmers.HitTracker: tbk_hit_tracker_marks / _runs) and kmers.phase_blocks against a reference that never
sees the device: marks from numpy, runs and blocks from a Python loop over them (tests/hit_track_ref.py).  Every comparison is
exact.  On every batch the marks are pinned twice more: their per-read sums must be what the CPU oracle counts (strict ACGT),
what Classifier.classify_batch counts on the same lists, and the counts runs() returns beside its runs.

The geometry under test (csrc/tbk_track.hip): the separated stream carries one 'N' behind every read; one wave marks a pass
of 2048 stream positions, lane l its windows 32 l .. 32 l + 31, from chunks of 16 bases; the markers are compacted per pass
and the run heads per tile of 1024 markers."""
import os

import numpy as np
import pytest

import hit_track_ref as ref
import kmerdb_files as kf

pytestmark = pytest.mark.gpu

KS = (5, 16, 21, 31, 32)
PASS = 2048


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _decoys(rng, k, n):
    """keys that are list lines and (for k > 5) almost surely no window's: never 0, never all ones"""
    top = (1 << (2 * k)) - 1 if k < 32 else (1 << 64) - 1
    return np.array([int(x) % (top - 1) + 1 for x in rng.integers(1, 1 << 62, n)], dtype=np.uint64)


def _keys_at(read, k, positions):
    return np.array([ref.canonical(read[p:p + k]) for p in positions], dtype=np.uint64)


class Pair:
    """Two lists on the device and in the oracle, their classifier and their tracker."""

    def __init__(self, orc, keys_a, keys_b, k, sets=None):
        from trio_binning_amd import kmers

        self.k, self.orc = k, orc
        self.keys_a, self.keys_b = np.asarray(keys_a, dtype=np.uint64), np.asarray(keys_b, dtype=np.uint64)
        assert self.keys_a.size >= 3 and self.keys_b.size >= 3  # (the oracle's own table misbehaves below three lines)
        self.sets = sets or (kmers.HashSet.from_keys(self.keys_a, k), kmers.HashSet.from_keys(self.keys_b, k))
        self.oa, self.ob = orc.table_from_keys(self.keys_a, k), orc.table_from_keys(self.keys_b, k)
        self.cls = kmers.Classifier(*self.sets)
        self.tracker = kmers.HitTracker(*self.sets)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.tracker.close()
        self.cls.close()
        for hs in self.sets:
            hs.close()

    def check(self, reads, ignore_case=False, what=""):
        """marks, runs, counts and blocks of one batch against the reference; returns (reference marks, device runs)"""
        from trio_binning_amd import kmers

        bases, offsets = reads if isinstance(reads, tuple) else kmers.pack_reads(reads)
        want = ref.marks(bases, offsets, self.keys_a, self.keys_b, self.k, ignore_case)
        got = self.tracker.marks(bases, offsets, ignore_case)
        assert got.dtype == np.uint8 and got.shape == want.shape, what
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            raise AssertionError(f"{what}: marks differ at batch bytes {bad[:8].tolist()} ({bad.size} in all): {got[bad[:8]].tolist()} for {want[bad[:8]].tolist()}")
        sums = ref.counts_of(want, offsets)
        as_read = ref.upper_acgt(bases) if ignore_case else bases
        assert np.array_equal(sums, self.orc.count_batch(as_read, offsets, self.oa, self.ob, strict=True)), what
        assert np.array_equal(sums, self.cls.classify_batch(as_read, offsets)), what
        runs, counts = self.tracker.runs(bases, offsets, ignore_case)
        assert np.array_equal(counts, sums), what
        want_runs = ref.runs(want, offsets)
        assert runs.dtype == want_runs.dtype
        assert np.array_equal(runs, want_runs), (what, runs[:5], want_runs[:5])
        for min_run in (1, 2, 3):
            assert np.array_equal(kmers.phase_blocks(runs, min_run), ref.blocks(want_runs, min_run)), (what, min_run)
        return want, runs


# ---- read lengths around k and around a pass, alone and behind a first read ------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_read_lengths_alone_and_behind_a_first_read(gpu, orc, k):
    rng = np.random.default_rng(1000 + k)
    lengths = (0, k - 1, k, k + 1, PASS - 1 + k, PASS + k - 1, PASS + k)  # (2047 + k and 2048 + k - 1 are one length: the last window at the pass's end)
    second = {n: _seq(rng, n) for n in lengths}
    # a first read of L bases puts the second read's first window at separated-stream position L + 1
    first = {at: _seq(rng, at - 1) for at in (PASS - 1, PASS, PASS + 1)}
    ka, kb = [], []
    for read in list(second.values()) + list(first.values()):
        if len(read) >= k:
            ends = [0, len(read) - k] + [int(p) for p in rng.integers(0, len(read) - k + 1, 6)]
            ka += _keys_at(read, k, ends[0::2]).tolist()
            kb += _keys_at(read, k, ends[1::2]).tolist()
    with Pair(orc, np.concatenate([np.array(ka, dtype=np.uint64), _decoys(rng, k, 3)]),
              np.concatenate([np.array(kb, dtype=np.uint64), _decoys(rng, k, 3)]), k) as pair:
        hits = 0
        for n, read in second.items():
            want, runs = pair.check([read], what=f"k {k} length {n} alone")
            assert (runs.size > 0) == (n >= k)
            for at, head in first.items():
                want, _ = pair.check([head, read], what=f"k {k} length {n} at stream position {at}")
                hits += int(want[len(head):len(head) + 1].sum() > 0) if n >= k else 0
        assert hits == 3 * sum(n >= k for n in second)  # the second read's first window is a marker wherever it has one


# ---- markers, N and lower-case at pass, lane and chunk edges -----------------------------------------------------------------
PLACES = (15, 16, 31, 32, PASS - 1, PASS)


@pytest.mark.parametrize("ignore_case", [False, True])
@pytest.mark.parametrize("k", KS)
def test_markers_and_bad_bases_at_the_edges(gpu, orc, k, ignore_case):
    rng = np.random.default_rng(2000 + k)
    read = _seq(rng, 2 * PASS + 300)
    keys = _keys_at(read, k, PLACES)
    with Pair(orc, np.concatenate([keys[0::2], _decoys(rng, k, 3)]), np.concatenate([keys[1::2], _decoys(rng, k, 3)]), k) as pair:
        want, _ = pair.check([read], ignore_case, f"k {k} planted")
        assert (want[list(PLACES)] > 0).all()
        for place in PLACES:
            for at in (place, place - (k - 1)):
                if at < 0:
                    continue
                for bad in ("N", read[at].lower()):
                    hurt = read[:at] + bad + read[at + 1:]
                    want, _ = pair.check([hurt], ignore_case, f"k {k} {bad!r} at {at}")
                    # a bad base AT the place spoils its window; k - 1 bases before it, it spoils the k windows up to place - 1 only
                    assert (want[place] > 0) == (at != place or (bad != "N" and ignore_case))


# ---- one long run over three passes; a key both lists hold -------------------------------------------------------------------
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("k", KS)
def test_homopolymer_is_one_run_of_hapA(gpu, orc, k, both):
    rng = np.random.default_rng(3000 + k)
    poly = np.array([0], dtype=np.uint64)  # A x k; its reverse complement T x k packs larger
    keys_b = np.concatenate([poly, _decoys(rng, k, 3)]) if both else _decoys(rng, k, 3)
    with Pair(orc, np.concatenate([_decoys(rng, k, 2), poly]), keys_b, k) as pair:
        _, runs = pair.check(["A" * 5000], what=f"k {k}")
        assert runs.tolist() == [(0, 0, 5000 - k, 5000 - k + 1, 0)]


# ---- more runs of one marker than a tile of the run stage holds ------------------------------------------------------------------
def test_alternating_markers_give_a_run_each(gpu, orc):
    k = 16
    rng = np.random.default_rng(4000)
    read = _seq(rng, 6000)
    keys = _keys_at(read, k, range(len(read) - k + 1))
    assert np.unique(keys).size == keys.size  # the read's canonical 16-mers are distinct: every window is its own key
    with Pair(orc, keys[0::2], keys[1::2], k) as pair:
        _, runs = pair.check([read])
        n = len(read) - k + 1
        assert n > 5 * 1024 and runs.size == n
        assert np.array_equal(runs["first"], np.arange(n)) and np.array_equal(runs["last"], np.arange(n))
        assert (runs["markers"] == 1).all() and np.array_equal(runs["hap"], np.arange(n) % 2)


# ---- a run never crosses a read boundary -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (5, 21, 32))
def test_a_read_boundary_ends_a_run(gpu, orc, k):
    rng = np.random.default_rng(5000 + k)
    one, two = _seq(rng, 300), _seq(rng, 200)
    keys = np.concatenate([_keys_at(one, k, [len(one) - k]), _keys_at(two, k, [0]), _decoys(rng, k, 2)])
    with Pair(orc, keys, _decoys(rng, k, 3), k) as pair:
        _, runs = pair.check([one, two])
        assert runs.size >= 2 and tuple(runs[runs["read"] == 0][-1])[2] == len(one) - k and tuple(runs[runs["read"] == 1][0])[1] == 0
        if k > 5:
            assert runs.tolist() == [(0, len(one) - k, len(one) - k, 1, 0), (1, 0, 0, 1, 0)]


# ---- lists hold their lines verbatim ---------------------------------------------------------------------------------------------------
def test_a_non_canonical_line_never_hits(gpu, orc):
    k = 21
    rng = np.random.default_rng(6000)
    read = _seq(rng, 500)
    kmer = read[100:100 + k]
    other = max(ref.pack(kmer), ref.pack(ref.revcomp(kmer)))
    assert other != ref.canonical(kmer)
    with Pair(orc, np.concatenate([[np.uint64(other)], _decoys(rng, k, 2)]), _decoys(rng, k, 3), k) as pair:
        want, runs = pair.check([read, ref.revcomp(read)])
        assert want.sum() == 0 and runs.size == 0


def test_an_empty_batch_gives_no_run(gpu, orc):
    rng = np.random.default_rng(7000)
    with Pair(orc, _decoys(rng, 21, 3), _decoys(rng, 21, 3), 21) as pair:
        runs, counts = pair.tracker.runs(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
        assert runs.size == 0 and counts.shape == (0, 2)
        assert pair.tracker.marks(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64)).size == 0
        pair.check(["", "", ""], what="empty reads only")


# ---- seeded fuzz ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(int(os.environ.get("TBK_FUZZ_SEEDS", "200"))))  # more seeds for a soak run
def test_fuzz_against_the_reference(gpu, orc, seed):
    rng = np.random.default_rng(8000 + seed)
    k = KS[seed % len(KS)]
    reads = []
    for _ in range(int(rng.integers(1, 41))):
        s = list(_seq(rng, int(rng.integers(0, 5001))))
        for p in rng.integers(0, max(len(s), 1), len(s) // 400):
            s[int(p)] = "N"
        for p in rng.integers(0, max(len(s), 1), len(s) // 300):
            s[int(p)] = s[int(p)].lower()
        reads.append("".join(s))
    # the lists: the reads' own k-mers, singly and in stretches of neighbouring windows (what a variant leaves), plus decoys
    own = [[], []]
    for read in reads:
        clean = read.upper()
        for _ in range(int(rng.integers(0, 6))):
            if len(clean) < k + 40:
                break
            p = int(rng.integers(0, len(clean) - k - 39))
            for w in range(p, p + int(rng.choice([1, 1, 2, 7, 40]))):
                if "N" not in clean[w:w + k]:
                    own[int(rng.integers(0, 2))].append(ref.canonical(clean[w:w + k]))
    keys = [np.concatenate([np.array(o, dtype=np.uint64), _decoys(rng, k, 3)]) for o in own]
    ignore_case = bool(seed & 1)
    with Pair(orc, keys[0], keys[1], k) as pair:
        pair.check(reads, ignore_case, f"seed {seed} k {k} ignore_case {ignore_case}")


# ---- lists that come from two count databases (tbk_table_origin 3) ------------------------------------------------------------------
def _lex_rank(kmer):
    return sum("ACGT".index(c) << (2 * (len(kmer) - 1 - i)) for i, c in enumerate(kmer))


def test_lists_made_from_two_count_databases(gpu, orc, tmp_path):
    from trio_binning_amd import kmers

    k = 21
    rng = np.random.default_rng(9000)
    reads = [_seq(rng, int(n)) for n in (3000, 150, 2500, 21, 4100)]
    ranks = [set(), set()]
    for i, read in enumerate(reads):
        for p in rng.integers(0, len(read) - k + 1, 60):
            kmer = read[int(p):int(p) + k]
            ranks[i % 2].add(min(_lex_rank(kmer), _lex_rank(ref.revcomp(kmer))))  # a database holds the lexicographically smaller strand
    shared = sorted(ranks[0])[:5]
    paths = []
    for hap, mine in enumerate(ranks):
        held = np.array(sorted(mine | (set(shared) if hap else set())), dtype=np.uint64)
        counts = np.full(held.size, 9, dtype=np.uint8)
        hist = np.bincount(counts, minlength=256).astype(np.uint64)
        hist[0] = held.size
        paths.append(str(tmp_path / f"hap{hap}.tbkdb"))
        with open(paths[-1], "wb") as fh:
            fh.write(kf.file_bytes(k, held, counts, hist, reads=1, bases=k))
    with kmers.KmerDatabase.load(paths[0]) as da, kmers.KmerDatabase.load(paths[1]) as db:
        sets = (da.unique_set(db, 2, 255), db.unique_set(da, 2, 255))
    assert sets[0].origin == "databases" and sets[0].num_kmers == len(ranks[0]) - 5
    with Pair(orc, sets[0].keys(), sets[1].keys(), k, sets=sets) as pair:
        want, runs = pair.check(reads)
        assert (want == 1).sum() > 0 and (want == 2).sum() > 0  # (the lines whose smaller strand is also the smaller packed key)
