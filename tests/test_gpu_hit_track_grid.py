"""The second trip of the hit tracker's strided loops (csrc/tbk_track.hip): tbk_track_separate_kernel and tbk_track_marks_kernel
stride over the reads, tbk_track_mark_kernel over the passes, all by the session's wave_slots - compute units x 32, thousands on
a real device, so no batch a Python reference can follow ever wraps them.  tbk_hit_tracker_set_wave_slots_ (a test hook) makes
the grid 1, 2, 3 or 5 waves, and one batch of 23 reads over 8 passes then takes up to eight trips: the LDS stage is refilled, the
pass counts - the tile counts of the marker compaction - are written on a later trip, and the bitmaps of a pass come from a wave
that has marked another pass before.

Everything is held to the references of tests/test_gpu_hit_track.py and tests/test_gpu_hit_track_compressed.py (their Pair.check,
unchanged: marks, runs, counts and phase blocks, plain and with compress=True), and byte for byte to what a session with the
device's own grid returns.  Every comparison is exact."""
import numpy as np
import pytest

import hit_track_ref as ref
import hpc_ref
from test_gpu_hit_track import Pair as PlainPair
from test_gpu_hit_track_compressed import Pair as CompressedPair

pytestmark = pytest.mark.gpu

KS = (5, 21, 32)
PASS = 2048
PASSES = 8
SLOTS = (1, 2, 3, 5)
STREAM = (PASSES - 1) * PASS + 1000  # the separated stream of the batch: seven full passes and a partial one
BAD_EDGE = 3 * PASS                  # the pass edge with an N and a lower-case base on each side
RUN_EDGE = 5 * PASS                  # the pass edge that a run of list A crosses


def _decoys(rng, k, n):
    """keys that are list lines and (for k > 5) almost surely no window's: never 0, never all ones"""
    top = (1 << (2 * k)) - 1 if k < 32 else (1 << 64) - 1
    return np.array([int(x) % (top - 1) + 1 for x in rng.integers(1, 1 << 62, n)], dtype=np.uint64)


def _seq(rng, n):
    """n bases with a homopolymer here and there: compression takes about a tenth away"""
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[(np.cumsum(rng.integers(1, 4, n + 1)) + rng.integers(0, 4)) % 4]
    return bytes(np.repeat(letters, rng.geometric(0.9, letters.size))[:n]).decode()


def _layout(k):
    """The lengths of the 23 reads.  A number is a length as it stands; ("edge", p) is a read that ends 250 + 10 p positions
    behind stream position 2048 p, whatever came before it; "rest" fills the stream up to STREAM."""
    plan = [1500, 0, k - 1, ("edge", 1), k, 0, 1200, ("edge", 2), 2, 900, ("edge", 3), 0, 1, 1300, ("edge", 4), k + 1, 700, ("edge", 5),
            1000, ("edge", 6), 31, ("edge", 7), "rest"]
    lengths, at = [], 0  # at: the stream position of the next read's first base
    for item in plan:
        if item == "rest":
            n = STREAM - 1 - at
        elif isinstance(item, tuple):
            n = item[1] * PASS + 250 + 10 * item[1] - at
            assert at <= item[1] * PASS - 200  # the read holds the 200 positions on either side of the edge
        else:
            n = item
        assert n >= 0
        lengths.append(n)
        at += n + 1
    assert at == STREAM and len(lengths) == 23
    return lengths


class Batch:
    """The 23 reads and the two lists for one k and one ignore_case."""

    def __init__(self, k, ignore_case, seed):
        rng = np.random.default_rng(seed)
        self.k, self.ignore_case = k, ignore_case
        lengths = _layout(k)
        starts = np.concatenate([[0], np.cumsum(np.array(lengths) + 1)])[:-1]  # stream position of every read's first base
        reads = [list(_seq(rng, n)) for n in lengths]

        def place(p):
            """(read, position in it) of stream position p"""
            r = int(np.searchsorted(starts, p, side="right")) - 1
            assert 0 <= p - starts[r] < lengths[r], p
            return r, int(p - starts[r])

        # one N and one lower-case base on each side of BAD_EDGE, as close as the windows at its two sides allow: the window at
        # BAD_EDGE - 1 begins behind the two on the left, the window at BAD_EDGE ends before the two on the right
        for p, bad in ((BAD_EDGE - 3, "N"), (BAD_EDGE - 2, None), (BAD_EDGE + k, "N"), (BAD_EDGE + k + 1, None)):
            r, i = place(p)
            reads[r][i] = bad or reads[r][i].lower()
        self.reads = ["".join(s) for s in reads]
        assert sum(len(s) == 0 for s in self.reads) >= 3 and sum(0 < len(s) < k for s in self.reads) >= 3

        # the planted markers: the first and the last window of every pass, the lists alternating from pass to pass, so the
        # two sides of an edge are in different lists - but for RUN_EDGE, where seven windows in a row are list A's
        own = [[], []]
        self.planted = []  # (stream position, list)
        for p in range(PASSES):
            self.planted.append((p * PASS, p % 2))
            self.planted.append(((p + 1) * PASS - 1 if p < PASSES - 1 else STREAM - 1 - k, p % 2))
        self.planted = [(p, 0 if p in (RUN_EDGE - 1, RUN_EDGE) else hap) for p, hap in self.planted]
        self.planted += [(RUN_EDGE + d, 0) for d in (-4, -3, -2, 1, 2)]
        for p, hap in self.planted:
            r, i = place(p)
            window = self.reads[r][i:i + k]
            assert len(window) == k and set(window) <= set("ACGT"), (p, window)
            own[hap].append(ref.canonical(window))
        fixed = set(own[0]) | set(own[1])  # (no other key may move a planted window to the other list)
        # and what a variant leaves: stretches of neighbouring windows, of the reads as given and of the compressed reads
        from trio_binning_amd import kmers

        self.bases, self.offsets = kmers.pack_reads(self.reads)
        cb, co = hpc_ref.compress_np(self.bases, self.offsets, ignore_case)
        self.passes_c = (int(co[-1]) + len(self.reads) + PASS - 1) // PASS
        texts = (self.reads, [bytes(cb[int(co[r]):int(co[r + 1])]).decode() for r in range(len(self.reads))])
        for text in texts:
            for s in text:
                clean = s.upper()
                for _ in range(4):
                    if len(clean) < k + 40:
                        break
                    p = int(rng.integers(0, len(clean) - k - 39))
                    hap = int(rng.integers(0, 2))
                    for w in range(p, p + int(rng.choice([1, 2, 7, 40]))):
                        if "N" not in clean[w:w + k] and ref.canonical(clean[w:w + k]) not in fixed:
                            own[hap].append(ref.canonical(clean[w:w + k]))
        # the compressed stream's own pass edges: the windows on their two sides, where a read holds both
        cstarts = co[:-1].astype(np.int64) + np.arange(len(self.reads))
        for e in range(PASS, self.passes_c * PASS, PASS):
            r = int(np.searchsorted(cstarts, e - 1, side="right")) - 1
            i = e - 1 - int(cstarts[r])
            s = texts[1][r].upper()
            for j, hap in ((i, (e // PASS) % 2), (i + 1, (e // PASS) % 2)):
                if 0 <= j and j + k <= len(s) and "N" not in s[j:j + k] and ref.canonical(s[j:j + k]) not in fixed:
                    own[hap].append(ref.canonical(s[j:j + k]))
        self.keys = [np.concatenate([np.array(o, dtype=np.uint64), _decoys(rng, k, 3)]) for o in own]

        # a second, different batch: fewer reads in another order, other pass edges, no empty read at the same place
        self.second = [self.reads[r] for r in (20, 7, 1, 16, 3, 2, 22, 0, 10, 11, 14, 19, 4)]


class GridPair(PlainPair):
    """tests/test_gpu_hit_track.py's Pair with the compressed check of tests/test_gpu_hit_track_compressed.py beside its own:
    both go through self.tracker, which the test swaps between a session with the device's grid and a hooked one."""

    check_compressed = CompressedPair.check

    def __init__(self, orc, keys_a, keys_b, k):
        from trio_binning_amd import kmers

        super().__init__(orc, keys_a, keys_b, k)
        self.comp = kmers.HomopolymerCompressor()
        self.hooked = kmers.HitTracker(*self.sets)
        self.own = self.tracker

    def __exit__(self, *exc):
        self.tracker = self.own
        self.hooked.close()
        self.comp.close()
        super().__exit__(*exc)

    def everything(self, reads, ignore_case):
        """every answer of self.tracker to one batch, as bytes"""
        from trio_binning_amd import kmers

        bases, offsets = kmers.pack_reads(reads)
        out = []
        for compress in (False, True):
            runs, counts = self.tracker.runs(bases, offsets, ignore_case, compress=compress)
            out += [self.tracker.marks(bases, offsets, ignore_case, compress=compress).tobytes(), runs.tobytes(), counts.tobytes()]
            out += [kmers.phase_blocks(runs, min_run).tobytes() for min_run in (1, 2, 3)]
        return out


def _stream_of(runs, offsets, field):
    return offsets[runs["read"].astype(np.int64)].astype(np.int64) + runs["read"].astype(np.int64) + runs[field].astype(np.int64)


@pytest.mark.parametrize("ignore_case", [False, True])
@pytest.mark.parametrize("k", KS)
def test_every_grid_gives_what_the_devices_own_grid_gives(gpu, orc, k, ignore_case):
    batch = Batch(k, ignore_case, 100 * k + int(ignore_case))
    n_reads = len(batch.reads)
    # not vacuous: with every hooked grid the pass loop and the read loops (four waves to a block) take a second trip, in
    # compressed space too; one wave takes all eight passes and four waves take 23 reads in six trips
    assert n_reads == 23 and int(batch.offsets[-1]) + n_reads == STREAM and (STREAM + PASS - 1) // PASS == PASSES and STREAM % PASS
    assert all(PASSES > s and batch.passes_c > s and n_reads > 4 * s for s in SLOTS)
    assert (n_reads + 3) // 4 == 6 and [len(range(b, PASSES, 3)) for b in range(3)] == [3, 3, 2] and n_reads - 4 * 5 == 3
    with GridPair(orc, batch.keys[0], batch.keys[1], k) as pair:
        want, runs = pair.check((batch.bases, batch.offsets), ignore_case, f"k {k}, the device's own grid")
        pair.check_compressed((batch.bases, batch.offsets), ignore_case, f"k {k}, the device's own grid, compressed")
        # the batch is what it is meant to be: a marker in the first and in the last window of every pass, of the planted
        # list where k-mers do not collide; a run across RUN_EDGE; the bad bases at BAD_EDGE cost the windows they should
        stream = np.zeros(STREAM, dtype=np.uint8)  # the marks by stream position
        for r in range(n_reads):
            lo, hi = int(batch.offsets[r]), int(batch.offsets[r + 1])
            stream[lo + r:hi + r] = want[lo:hi]
        for p, hap in batch.planted:
            assert stream[p] > 0 and (k == 5 or stream[p] == hap + 1), (p, hap)
        assert stream[BAD_EDGE - 3 - (k - 1):BAD_EDGE - 2].sum() == 0 and stream[BAD_EDGE + 1:BAD_EDGE + k + 1].sum() == 0
        if not ignore_case:
            assert stream[BAD_EDGE - 2] == 0 and stream[BAD_EDGE + k + 1] == 0
        first, last = _stream_of(runs, batch.offsets, "first"), _stream_of(runs, batch.offsets, "last")
        assert ((first < RUN_EDGE) & (last >= RUN_EDGE) & (runs["hap"] == 0)).any()
        assert ((first < PASS) & (last >= PASS)).sum() == 0 or k == 5  # (and no run across an edge whose sides are in two lists)
        base_first = pair.everything(batch.reads, ignore_case)
        base_second = pair.everything(batch.second, ignore_case)

        pair.tracker = pair.hooked
        for slots in SLOTS:
            assert gpu.lib.tbk_hit_tracker_set_wave_slots_(pair.hooked._h, slots) == 0
            what = f"k {k}, ignore_case {ignore_case}, wave_slots {slots}"
            pair.check((batch.bases, batch.offsets), ignore_case, what)
            pair.check_compressed((batch.bases, batch.offsets), ignore_case, what + ", compressed")
            assert pair.everything(batch.reads, ignore_case) == base_first, what
            # the same hooked session, another batch: nothing of the first is left in the bitmaps or the pass counts
            pair.check(batch.second, ignore_case, what + ", second batch")
            pair.check_compressed(batch.second, ignore_case, what + ", second batch, compressed")
            assert pair.everything(batch.second, ignore_case) == base_second, what


def test_the_hook_refuses_zero_and_null(gpu, orc):
    from trio_binning_amd import _lib

    k = 21
    batch = Batch(k, False, 7)
    with GridPair(orc, batch.keys[0], batch.keys[1], k) as pair:
        pair.tracker = pair.hooked
        assert gpu.lib.tbk_hit_tracker_set_wave_slots_(pair.hooked._h, 2) == 0
        before = pair.everything(batch.reads, False)
        assert gpu.lib.tbk_hit_tracker_set_wave_slots_(pair.hooked._h, 0) == _lib.TBK_ERR_INVALID
        assert gpu.lib.tbk_hit_tracker_set_wave_slots_(None, 3) == _lib.TBK_ERR_INVALID
        pair.check((batch.bases, batch.offsets), False, "after a refused 0")  # the session is as it was: it still runs
        assert pair.everything(batch.reads, False) == before
