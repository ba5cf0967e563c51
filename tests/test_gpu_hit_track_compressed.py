"""The hit tracker in homopolymer-compressed space (kmers.HitTracker.runs / .marks with compress=True: tbk_hit_tracker_runs_compressed,
tbk_hit_tracker_marks_compressed) against a reference that never sees the device (tests/hpc_lift_ref.py): the batch compressed
with numpy, marks, runs and blocks of the compressed batch from tests/hit_track_ref.py, their coordinates lifted through the
positions of the keep bits.  Every comparison is exact.  The counts are pinned three more times: to the CPU oracle on the
numpy-compressed batch, to Classifier.classify_batch on the device-compressed batch, and to the sums of the expanded marks.

The geometry under test: compression works in tiles of 4096 input bases and keep words of 64; the tracker's marking in passes of
2048 positions of the separated COMPRESSED stream and its run stage in tiles of 1024 markers; a run's three endpoints are lifted
on the device, the last one possibly the compressed end of its read."""
import os

import numpy as np
import pytest

import hit_track_ref as ref
import hpc_lift_ref as lref
import hpc_ref

pytestmark = pytest.mark.gpu

KS = (5, 21, 32)
PASS = 2048
T = 4096


def _decoys(rng, k, n):
    """keys that are list lines and (for k > 5) almost surely no window's: never 0, never all ones"""
    top = (1 << (2 * k)) - 1 if k < 32 else (1 << 64) - 1
    return np.array([int(x) % (top - 1) + 1 for x in rng.integers(1, 1 << 62, n)], dtype=np.uint64)


def _keys_at(seq, k, positions):
    return np.array([ref.canonical(seq[p:p + k]) for p in positions], dtype=np.uint64)


def _stretched(rng, seq, mean=2.0):
    return lref.stretch(seq, rng.geometric(1.0 / mean, len(seq)))


class Pair:
    """Two lists on the device and in the oracle, their classifier, their tracker and a compression session."""

    def __init__(self, orc, keys_a, keys_b, k):
        from trio_binning_amd import kmers

        self.k, self.orc = k, orc
        self.keys_a, self.keys_b = np.asarray(keys_a, dtype=np.uint64), np.asarray(keys_b, dtype=np.uint64)
        assert self.keys_a.size >= 3 and self.keys_b.size >= 3  # (the oracle's own table misbehaves below three lines)
        self.sets = (kmers.HashSet.from_keys(self.keys_a, k), kmers.HashSet.from_keys(self.keys_b, k))
        self.oa, self.ob = orc.table_from_keys(self.keys_a, k), orc.table_from_keys(self.keys_b, k)
        self.cls = kmers.Classifier(*self.sets)
        self.tracker = kmers.HitTracker(*self.sets)
        self.comp = kmers.HomopolymerCompressor()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.comp.close()
        self.tracker.close()
        self.cls.close()
        for hs in self.sets:
            hs.close()

    def check(self, reads, ignore_case=False, what=""):
        """marks, runs, counts and blocks of one batch in compressed space against the reference; returns (reference, device runs)"""
        from trio_binning_amd import kmers

        bases, offsets = reads if isinstance(reads, tuple) else kmers.pack_reads(reads)
        want = lref.Lifted(bases, offsets, self.keys_a, self.keys_b, self.k, ignore_case)
        got = self.tracker.marks(bases, offsets, ignore_case, compress=True)
        assert got.dtype == np.uint8 and got.shape == want.marks.shape, what
        if not np.array_equal(got, want.marks):
            bad = np.nonzero(got != want.marks)[0]
            raise AssertionError(f"{what}: marks differ at batch bytes {bad[:8].tolist()} ({bad.size} in all): {got[bad[:8]].tolist()} for {want.marks[bad[:8]].tolist()}")
        runs, counts = self.tracker.runs(bases, offsets, ignore_case, compress=True)
        assert runs.dtype == np.dtype(kmers.HIT_RUN_LIFTED_DTYPE) == want.runs.dtype
        assert np.array_equal(runs, want.runs), (what, runs[:5], want.runs[:5])
        # the counts, four ways: the reference's, the oracle's on the numpy-compressed batch, the classifier's on the
        # device-compressed batch, and the sums of the expanded marks
        assert np.array_equal(counts, want.counts), what
        as_read = ref.upper_acgt(want.cb) if ignore_case else want.cb
        assert np.array_equal(counts, self.orc.count_batch(as_read, want.co, self.oa, self.ob, strict=True)), what
        cb, co = self.comp.compress(bases, offsets, fold_case=ignore_case)
        assert np.array_equal(counts, self.cls.classify_batch(ref.upper_acgt(cb) if ignore_case else cb, co)), what
        assert np.array_equal(counts, ref.counts_of(got, offsets)), what
        for min_run in (1, 2, 3):
            assert np.array_equal(kmers.phase_blocks(runs, min_run), lref.blocks(want.runs, min_run)), (what, min_run)
        return want, runs


# ---- the trailing run belongs to the last window; compressed lengths around k -------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_the_last_window_ends_where_the_read_ends(gpu, orc, k):
    rng = np.random.default_rng(100 + k)
    small = lref.compressed_sequence(rng, 300)
    lengths = rng.geometric(0.5, len(small))
    lengths[-1] = 9  # the read ends in a homopolymer of nine
    lengths[0] = 4
    read = lref.stretch(small, lengths)
    keys = _keys_at(small, k, [0, len(small) - k])
    with Pair(orc, np.concatenate([keys, _decoys(rng, k, 2)]), _decoys(rng, k, 3), k) as pair:
        want, runs = pair.check([read], what=f"k {k}")
        first, last = runs[0], runs[-1]
        assert (int(first["read"]), int(first["first"])) == (0, 0) and int(last["end"]) == len(read)
        assert int(last["last"]) == len(read) - int(lengths[-k:].sum())  # the first base of the last window's first run
        if k > 5:
            assert runs.tolist() == [(0, 0, int(last["last"]), len(read), 2, 0)]  # two markers of A, however far apart: one run
        # behind other reads, empty ones among them, and with the same read again
        pair.check(["", read, "", "", read[:-3], read, ""], what=f"k {k} among empty reads")


@pytest.mark.parametrize("k", KS)
def test_compressed_lengths_around_k(gpu, orc, k):
    rng = np.random.default_rng(200 + k)
    small = {n: lref.compressed_sequence(rng, n) for n in (k - 1, k, k + 1)}
    keys = np.concatenate([_keys_at(s, k, range(len(s) - k + 1)) for s in small.values() if len(s) >= k])
    with Pair(orc, np.concatenate([keys, _decoys(rng, k, 2)]), _decoys(rng, k, 3), k) as pair:
        for n, s in small.items():
            for mean in (1.0, 3.0):
                read = _stretched(rng, s, mean)
                want, runs = pair.check([read], what=f"k {k} compressed length {n} alone")
                assert int(want.counts.sum()) == max(n - k + 1, 0) and (runs.size > 0) == (n >= k)
                if n >= k:
                    assert int(runs[0]["first"]) == 0 and int(runs[-1]["end"]) == len(read)
        pair.check([_stretched(rng, s, 2.5) for s in small.values()] * 2, what=f"k {k} together")


# ---- a window that holds a homopolymer longer than a tile -----------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_a_window_over_a_homopolymer_longer_than_a_tile(gpu, orc, k):
    rng = np.random.default_rng(300 + k)
    small = lref.compressed_sequence(rng, 200)
    at = 100  # the window at 100 has the long run as its third letter; the windows around it hold it too
    lengths = rng.geometric(0.5, len(small))
    lengths[at + 2] = T + 500
    read = lref.stretch(small, lengths)
    keys = _keys_at(small, k, [at, 150])
    with Pair(orc, np.concatenate([keys[:1], _decoys(rng, k, 2)]), np.concatenate([keys[1:], _decoys(rng, k, 2)]), k) as pair:
        want, runs = pair.check([read], what=f"k {k}")
        assert want.mk_c[at] == 1 and want.marks[int(lengths[:at].sum())] == 1  # the mark sits on the first base of the window's first run
        if k > 5:  # (5-mers hit elsewhere too, and may join this marker's run)
            assert runs.tolist() == [(0, int(lengths[:at].sum()), int(lengths[:at].sum()), int(lengths[:at + k].sum()), 1, 0),
                                     (0, int(lengths[:150].sum()), int(lengths[:150].sum()), int(lengths[:150 + k].sum()), 1, 1)]
            assert int(runs[0]["end"]) - int(runs[0]["first"]) > T + 500
        pair.check(["ACGT" * 7, read, read[:T + 300]], what=f"k {k} behind another read and cut inside the run")


# ---- markers at the edge of a marking pass of the compressed stream -------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_markers_at_compressed_stream_positions_2047_and_2048(gpu, orc, k):
    rng = np.random.default_rng(400 + k)
    small = lref.compressed_sequence(rng, PASS + 300)
    read = _stretched(rng, small, 1.8)
    keys = _keys_at(small, k, [PASS - 1, PASS, 0, 1])
    with Pair(orc, np.concatenate([keys[0::2], _decoys(rng, k, 2)]), np.concatenate([keys[1::2], _decoys(rng, k, 2)]), k) as pair:
        want, runs = pair.check([read], what=f"k {k}")
        assert want.mk_c[PASS - 1] > 0 and want.mk_c[PASS] > 0 and (k == 5 or (want.mk_c[PASS - 1] == 1 and want.mk_c[PASS] == 2))
        # a first read of compressed length L puts the second read's windows 0 and 1 at separated stream positions L + 1 and L + 2
        for head in (PASS - 2, PASS - 1, PASS):
            first = _stretched(rng, lref.compressed_sequence(rng, head), 1.5)
            want, runs = pair.check([first, read], what=f"k {k} head {head}")
            assert int(want.co[1]) == head and want.mk_c[head] > 0 and want.mk_c[head + 1] > 0
            assert k == 5 or (want.mk_c[head] == 1 and want.mk_c[head + 1] == 2)  # (a 5-mer of list B may be in list A too, by chance)


# ---- hapA is asked first --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_a_key_in_both_lists_marks_a(gpu, orc, k):
    rng = np.random.default_rng(500 + k)
    small = lref.compressed_sequence(rng, 400)
    read = _stretched(rng, small)
    both, only_b = _keys_at(small, k, [50, 51, 52]), _keys_at(small, k, [200])
    with Pair(orc, np.concatenate([both, _decoys(rng, k, 2)]), np.concatenate([both, only_b, _decoys(rng, k, 2)]), k) as pair:
        want, runs = pair.check([read], what=f"k {k}")
        assert (want.mk_c[50:53] == 1).all() and want.mk_c[200] == 2


# ---- more one-marker runs in one read than a tile of the run stage holds ------------------------------------------------------------------------
def test_alternating_markers_give_a_lifted_run_each(gpu, orc):
    k = 21
    rng = np.random.default_rng(600)
    small = lref.compressed_sequence(rng, 1400)
    keys = _keys_at(small, k, range(len(small) - k + 1))
    assert np.unique(keys).size == keys.size  # every window is its own key
    lengths = rng.geometric(0.5, len(small))
    read = lref.stretch(small, lengths)
    with Pair(orc, keys[0::2], keys[1::2], k) as pair:
        _, runs = pair.check([read])
        n = len(small) - k + 1
        assert n > 1024 and runs.size == n and (runs["markers"] == 1).all() and np.array_equal(runs["hap"], np.arange(n) % 2)
        starts = np.concatenate([[0], np.cumsum(lengths)])
        assert np.array_equal(runs["first"], starts[:n]) and np.array_equal(runs["last"], starts[:n]) and np.array_equal(runs["end"], starts[k:k + n])


# ---- soft-masked bytes: fold_case follows ignore_case ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_ignore_case_folds_the_compression_too(gpu, orc, k):
    rng = np.random.default_rng(700 + k)
    small = lref.compressed_sequence(rng, 3 * k)
    # every letter written twice, lower case then upper: one kept byte folded ("aA" -> "a"), two unfolded ("a", "A")
    read = "".join(c.lower() + c for c in small)
    keys = _keys_at(small, k, range(len(small) - k + 1))
    with Pair(orc, np.concatenate([keys[0::2], _decoys(rng, k, 2)]), np.concatenate([keys[1::2], _decoys(rng, k, 2)]), k) as pair:
        want, runs = pair.check([read], ignore_case=True, what=f"k {k} folded")
        assert want.cb.size == len(small) and int(want.counts.sum()) == len(small) - k + 1 and int(runs[-1]["end"]) == len(read)
        want, runs = pair.check([read], ignore_case=False, what=f"k {k} unfolded")
        assert want.cb.size == 2 * len(small) and int(want.counts.sum()) == 0 and runs.size == 0
        # soft-masked stretches in a stretched read, an N, and a case change inside a run
        masked = list(_stretched(rng, small, 2.5))
        for i in range(len(masked)):
            if (i // 7) % 3 == 0:
                masked[i] = masked[i].lower()
        masked = "".join(masked)
        for ignore_case in (True, False):
            pair.check([masked, masked[:40] + "N" + masked[41:], "aA" * 5, ""], ignore_case=ignore_case, what=f"k {k} masked, ignore_case {ignore_case}")


# ---- seeded fuzz; the plain calls of the same tracker afterwards -------------------------------------------------------------------------------------
def _fuzz_batch(rng, k, ignore_case):
    reads = []
    for _ in range(int(rng.integers(1, 13))):
        n = int(rng.integers(0, 5001))
        letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n + 1)]
        s = list(bytes(np.repeat(letters, rng.geometric(0.55, letters.size))[:n]).decode())
        for p in rng.integers(0, max(len(s), 1), len(s) // 400):
            s[int(p)] = "N"
        for p in rng.integers(0, max(len(s), 1), len(s) // 300):
            s[int(p)] = s[int(p)].lower()
        reads.append("".join(s))
    # the lists: k-mers of the compressed reads, singly and in stretches of neighbouring windows, plus decoys
    from trio_binning_amd import kmers

    bases, offsets = kmers.pack_reads(reads)
    cb, co = hpc_ref.compress_np(bases, offsets, ignore_case)
    text = bytes(cb).decode().upper()
    own = [[], []]
    for r in range(len(reads)):
        clean = text[int(co[r]):int(co[r + 1])]
        for _ in range(int(rng.integers(0, 6))):
            if len(clean) < k + 40:
                break
            p = int(rng.integers(0, len(clean) - k - 39))
            for w in range(p, p + int(rng.choice([1, 1, 2, 7, 40]))):
                if "N" not in clean[w:w + k]:
                    own[int(rng.integers(0, 2))].append(ref.canonical(clean[w:w + k]))
    return reads, [np.concatenate([np.array(o, dtype=np.uint64), _decoys(rng, k, 3)]) for o in own]


@pytest.mark.parametrize("seed", range(int(os.environ.get("TBK_FUZZ_SEEDS", "100"))))  # more seeds for a soak run
def test_fuzz_against_the_reference(gpu, orc, seed):
    rng = np.random.default_rng(9000 + seed)
    k = KS[seed % len(KS)]
    ignore_case = bool((seed // len(KS)) & 1)
    reads, keys = _fuzz_batch(rng, k, ignore_case)
    with Pair(orc, keys[0], keys[1], k) as pair:
        pair.check(reads, ignore_case, f"seed {seed} k {k} ignore_case {ignore_case}")


def test_the_plain_calls_of_the_same_tracker_are_unchanged_afterwards(gpu, orc):
    from trio_binning_amd import kmers

    k = 21
    rng = np.random.default_rng(800)
    reads, keys = _fuzz_batch(rng, k, False)
    plain_keys = [np.concatenate([ks, _keys_at(reads[0].upper().replace("N", "A"), k, range(0, max(len(reads[0]) - k, 0), 97))]) for ks in keys]
    with Pair(orc, plain_keys[0], plain_keys[1], k) as pair:
        bases, offsets = kmers.pack_reads(reads)
        for _ in range(2):
            pair.check(reads, False, "compressed")
            mk = ref.marks(bases, offsets, pair.keys_a, pair.keys_b, k, False)
            assert np.array_equal(pair.tracker.marks(bases, offsets), mk)
            runs, counts = pair.tracker.runs(bases, offsets)
            assert runs.dtype == np.dtype(kmers.HIT_RUN_DTYPE) and np.array_equal(runs, ref.runs(mk, offsets))
            assert np.array_equal(counts, ref.counts_of(mk, offsets))
