"""kmers.DatabaseQuery.track (tbk_kmerdb_query_track; kernels: csrc/tbk_depth.hip) against tests/copy_track_ref.py, bin for bin
and field for field, at the smallest shapes where the two kernels can go wrong: a sequence whose windows cross two pass edges
(a pass is 2048 stream positions), bins that straddle them, sequences shorter than k between longer ones, a sequence of exactly k
bases, N and lower case on the edges, every window size at which the bin pass takes another path, copy counters of 0 and above
255, the capped counter, the medians' edge cases, an empty database and the strided loops' later trips.  The batch of a case is
judged by the numpy reference (the loop reference joins it once per k); tests/test_host_copy_track.py holds the two to each
other.  Everything is integers: every comparison is exact."""
import numpy as np
import pytest

import copy_track_ref as ctr
import db_query_ref as ref

pytestmark = pytest.mark.gpu

PASS = 2048
KS = (1, 2, 4, 21, 31, 32)  # the smallest odd and even k of a database; 2, 4 and 32 with k-mers that are their own reverse complement
COUNTERS = (2, 5, 10, 15, 20, 30, 127, 254, 255)
LONG = 4500  # the first sequence: its windows cross the pass edges at 2048 and 4096


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _own_reverse_complement(k):
    half = "ACGGTCAATCGATTGC"[:k // 2]
    return half + ref.revcomp(half)


class Case:
    """One database and two batches for one k, with everything the references need."""

    def __init__(self, k):
        from trio_binning_amd import kmers

        rng = np.random.default_rng(900 + k)
        self.k = k
        genome = list(_seq(rng, 9000))
        if k == 32:  # (at k = 2 and 4 a random sequence holds them by itself)
            for at in (700, 2040, 4090):
                genome[at:at + k] = _own_reverse_complement(k)
        genome = "".join(genome)
        windows = ref.window_kmers(genome, k)
        held = sorted({km for i, km in enumerate(windows) if not 6000 <= i < 6300})
        if k <= 4:  # nearly every small k-mer occurs somewhere: drop some for absent windows
            held = [km for i, km in enumerate(held) if i % 3 != 1]
        self.db = {km: COUNTERS[(ref.lex_rank(km) * 7 + len(km)) % len(COUNTERS)] for km in held}
        first = list(genome[:LONG])
        first[2047] = "N"
        first[4090:4110] = [c.lower() for c in first[4090:4110]]
        first[LONG - 1] = first[LONG - 1].lower()
        short = [genome[i:i + max(k - 1, 0)] for i in (10, 20, 30)] + ["", genome[40:40 + k // 2], ""]
        self.first = ["".join(first)] + short + [genome[5000:5000 + k]] + short[::-1] + [genome[4400:6700]] + short + \
            [ref.revcomp(genome[100:1700]), _seq(rng, 700), "n" + genome[6701:9000].lower(), genome[2000:5000]]
        self.second = [genome[:1500], genome[:1500], ref.revcomp(genome[300:900]), genome[5990:6310]]
        self.nw = LONG - k + 1
        stream = sum(len(s) + 1 for s in self.first)
        assert stream > 7 * PASS  # a grid of three waves takes a third trip over the passes
        assert sum(len(s) < k for s in self.first) >= (9 if k > 1 else 4)
        if k in (2, 4, 32):
            assert any(km == ref.revcomp(km) for km in self.db)
        ranks = np.array(sorted(ref.lex_rank(km) for km in self.db), dtype=np.uint64)
        by_rank = {ref.lex_rank(km): c for km, c in self.db.items()}
        self.ranks, self.counters = ranks, np.array([by_rank[int(r)] for r in ranks], dtype=np.uint8)
        self.file = ref.database_bytes(self.db, k)
        self.packed = {id(b): kmers.pack_reads(b) for b in (self.first, self.second)}
        self.wanted = {}

    def tally(self):
        return ref.TallyNp(self.ranks, self.counters)

    def want(self, tally, state, batch, window, peak):
        """the reference's answer, computed once per (state of the session, batch, window, peak)"""
        key = (state, id(batch), window, peak)
        if key not in self.wanted:
            self.wanted[key] = ctr.track_np(tally, *self.packed[id(batch)], self.k, window, peak)
        return self.wanted[key]


_CASES = {}


@pytest.fixture(scope="module")
def case(gpu):
    def get(k):
        if k not in _CASES:
            _CASES[k] = Case(k)
        return _CASES[k]

    yield get
    _CASES.clear()


@pytest.fixture()
def load(gpu, tmp_path):
    """load(file bytes) -> KmerDatabase; closed at the end of the test"""
    from trio_binning_amd import kmers

    opened = []

    def _load(data):
        path = tmp_path / "db{}.tbkdb".format(len(opened))
        path.write_bytes(data)
        opened.append(kmers.KmerDatabase.load(str(path)))
        return opened[-1]

    yield _load
    for d in opened:
        d.close()


def _state(query):
    return query.histogram(), query.completeness(), query.completeness(10, 200), query.copy_spectrum()


def _same_state(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3])


def _check(query, c, tally, state, batch, window, peak):
    want, want_prefix = c.want(tally, state, batch, window, peak)
    before = _state(query)
    bins, prefix = query.track(*c.packed[id(batch)], window, peak)
    what = "k {}, state {}, window {}, peak {}".format(c.k, state, window, peak)
    assert bins.dtype == ctr.BIN and prefix.dtype == np.uint64 and np.array_equal(prefix, want_prefix), what
    assert ctr.equal(bins, want), (what, ctr.first_difference(bins, want))
    assert _same_state(_state(query), before), what  # the call only reads the session
    return bins


# ---- 1. every k, every window size, every peak -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_every_window_size_against_the_reference(case, load, k):
    c = case(k)
    with load(c.file).query(copies=True) as query:
        tally = c.tally()
        # a == 0: nothing was added yet - present windows, no expansion, copies 0
        bins = _check(query, c, tally, 0, c.first, 64, 10)
        assert int(bins["clean"].sum()) > int(bins["absent"].sum()) > 0 and int(bins["expanded"].sum()) == 0 and int(bins["copies"].max()) == 0
        assert k < 21 or int(bins["collapsed"].sum()) > 0
        query.add(*c.packed[id(c.first)])
        tally.add(*c.packed[id(c.first)], k)
        for window in (1, 2, 63, 64, 65, c.nw - 1, c.nw, c.nw + 1, 1 << 31):
            bins = _check(query, c, tally, 1, c.first, window, 10)
            if window == 64:  # not vacuous: every field is at work, and bins of both parities of present windows
                for f in ctr.FIELDS if k >= 21 else ("clean", "absent", "depth", "copies"):  # (a database of a few small k-mers has few counters)
                    assert int(bins[f].max()) > 0, f
                present = (bins["clean"] - bins["absent"]).astype(np.int64)
                assert (present % 2 == 0).any() and (present % 2 == 1).any() and (k < 21 or (present == 0).any())
            if window == c.nw - 1:  # the first sequence's last bin holds one window
                assert int(bins[1]["clean"]) <= 1 and len(bins) == 2 + sum(len(s) >= k for s in c.first[1:])
        for peak in (1, 254):
            _check(query, c, tally, 1, c.first, 65, peak)
        # the loop reference, once: the whole batch at one window size
        loop = ref.Tally(c.db)
        loop.add(c.first, k)
        want = ctr.as_array(ctr.track(loop, c.first, k, 65, 10))[0]
        assert ctr.equal(c.want(tally, 1, c.first, 65, 10)[0], want)
        # more copies, and a batch that was not the one added
        query.add(*c.packed[id(c.second)])
        tally.add(*c.packed[id(c.second)], k)
        bins = _check(query, c, tally, 2, c.first, 63, 10)
        assert int(bins["copies"].max()) >= 3
        _check(query, c, tally, 2, c.second, 64, 10)
        query.reset()
        _check(query, c, c.tally(), 0, c.first, 64, 10)  # after a reset the copies are 0 again


# ---- 2. the later trips of both strided loops ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (4, 21))
def test_small_grids_take_later_trips(gpu, case, load, k):
    c = case(k)
    with load(c.file).query(copies=True) as query:
        tally = c.tally()
        query.add(*c.packed[id(c.first)])
        tally.add(*c.packed[id(c.first)], k)
        n_bins = c.want(tally, 1, c.first, 64, 10)[0].size
        assert n_bins > 3 * 3 and sum(len(s) + 1 for s in c.first) > 7 * PASS  # a third trip over the bins and over the passes
        for slots in (1, 2, 3):
            assert gpu.lib.tbk_kmerdb_query_set_wave_slots_(query._h, slots) == 0
            _check(query, c, tally, 1, c.first, 64, 10)
            _check(query, c, tally, 1, c.first, 1 << 31, 10)
            _check(query, c, tally, 1, c.first, c.nw - 1, 254)


# ---- 3. small batches at the edges ----------------------------------------------------------------------------------------------------
def _small(load, db, k, added, tracked, window, peak, times=1):
    """add `added` `times` times, track `tracked`: (bins, prefix), held to both references"""
    from trio_binning_amd import kmers

    with load(ref.database_bytes(db, k)).query(copies=True) as query:
        loop = ref.Tally(db)
        for _ in range(times):
            if added:
                query.add(*kmers.pack_reads(added))
                loop.add(added, k)
        before = _state(query)
        bins, prefix = query.track(*kmers.pack_reads(tracked), window, peak)
        assert _same_state(_state(query), before)
        want, want_prefix = ctr.as_array(ctr.track(loop, tracked, k, window, peak))
        assert np.array_equal(prefix, want_prefix) and ctr.equal(bins, want), ctr.first_difference(bins, want)
        return bins, prefix


def _tuples(bins):
    return [tuple(int(b[f]) for f in ctr.FIELDS) for b in bins]


@pytest.mark.parametrize("k", KS)
def test_one_sequence_of_exactly_k_bases(load, k):
    rng = np.random.default_rng(30 + k)
    s = _seq(rng, k)
    db = {ref.canonical(s): 20, ("C" if ref.canonical(s) == "A" * k else "A") * k: 7}
    bins, prefix = _small(load, db, k, [s], [s], 10000, 10)
    assert prefix.tolist() == [0, 1] and _tuples(bins) == [(1, 0, 0, 1, 0, 20, 1)]
    bins, prefix = _small(load, db, k, [s], [s.lower(), s[:k - 1], "N" * k], 1, 10)
    assert prefix.tolist() == [0, 1, 1, 2] and _tuples(bins) == [(1, 0, 0, 1, 0, 20, 1), (0, 0, 0, 0, 0, 0, 0)]


def test_the_medians_edge_cases(load):
    """k = 5; u, v, w, x are 5-mers with counters 10, 30, 31 and none.  Spelled by window: an N between any two of them."""
    k = 5
    u, v, w, x = "ACCGA", "CATTG", "GGATC", "TTTTT"
    db = {ref.canonical(u): 10, ref.canonical(v): 30, ref.canonical(w): 31}
    row = lambda *kmers_: "N".join(kmers_)  # noqa: E731  (each k-mer is one clean window; the five behind it hold the N)
    # even: two present windows 10, 30 -> the lower one; odd: 10, 30, 31 -> 30; all absent; all equal (a = 4: 60 < 7 x 10, expanded)
    for sequence, want in ((row(u, v), (2, 0, 0, 1, 0, 10, 1)), (row(v, u, w), (3, 0, 0, 2, 0, 30, 1)), (row(x, x, x), (3, 3, 0, 0, 0, 0, 0)),
                           (row(v, v, v, v), (4, 0, 0, 0, 4, 30, 4))):
        bins, _ = _small(load, db, k, [sequence], [sequence], 1000, 10)
        assert _tuples(bins) == [want], sequence
    # the copies' median on its own: u once and v three times in the assembly -> sorted a = 1, 3, 3, 3
    bins, _ = _small(load, db, k, [row(u, v, v, v)], [row(u, v, v, v)], 1000, 10)
    assert _tuples(bins) == [(4, 0, 0, 0, 0, 30, 3)]  # (v: 60 > 70 is false and 60 < 50 is false)


@pytest.mark.parametrize("k", (2, 21, 32))
def test_more_than_255_copies_and_the_capped_counter(load, k):
    """A run of 300 + k - 1 A: 300 windows of one k-mer, so a = 300 where the byte the bin pass sees says 255."""
    rng = np.random.default_rng(70 + k)
    other = _seq(rng, 40 + k)
    db = {km: 10 for km in ref.window_kmers(other, k)}
    db["A" * k] = 10
    capped = next(km for km in ref.window_kmers(other, k)[5:] if km != "A" * k)
    db[capped] = 255
    run = "A" * (300 + k - 1)
    bins, prefix = _small(load, db, k, [run, other], [run, other], 128, 10)
    assert prefix.tolist()[:2] == [0, 3] and [int(b["copies"]) for b in bins[:3]] == [255, 255, 255]
    assert [int(b["expanded"]) for b in bins[:3]] == [128, 128, 44] and int(bins["saturated"].sum()) >= 1
    # twice: a = 600 and 2; a track of the run alone before anything was added: a = 0
    bins, _ = _small(load, db, k, [run, other], [other, run], 300, 1, times=2)
    assert k < 21 or int(bins[0]["copies"]) == 2  # (a random 2-mer occurs more often than that)
    bins, _ = _small(load, db, k, [], [run], 300, 10)
    assert _tuples(bins) == [(300, 0, 0, 300, 0, 10, 0)]  # (held by the reads, by the assembly never: 20 > 1 x 10)


@pytest.mark.parametrize("k", (1, 21))
def test_an_empty_database(load, k):
    rng = np.random.default_rng(80 + k)
    sequences = [_seq(rng, 2100), "", _seq(rng, 90) + "N" + _seq(rng, 50)]
    bins, prefix = _small(load, {}, k, sequences, sequences, 64, 10)
    assert int(bins["clean"].sum()) == int(bins["absent"].sum()) > 2000 and not bins["depth"].any() and not bins["copies"].any()
    assert bins.size == int(prefix[-1]) == -(-(2100 - k + 1) // 64) + -(-(141 - k + 1) // 64)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_session_usable(gpu, case, load):
    from trio_binning_amd import _lib, kmers

    c = case(21)
    bases, offsets = c.packed[id(c.second)]
    n = offsets.size - 1
    database = load(c.file)
    with database.query() as plain:
        out = np.zeros(4, dtype=ctr.BIN)
        assert gpu.lib.tbk_kmerdb_query_track(plain._h, bases.ctypes.data, offsets.ctypes.data, n, 64, 10, out.ctypes.data, 4) == _lib.TBK_ERR_INVALID
        assert "without copies" in _lib.last_error()
        with pytest.raises(ValueError, match="without copies"):
            plain.track(bases, offsets, 64, 10)
        assert int(plain.add(bases, offsets)[:, 0].sum()) > 0
    with database.query(copies=True) as query:
        tally = c.tally()
        query.add(bases, offsets)
        tally.add(bases, offsets, 21)
        want, prefix = c.want(tally, "refusals", c.second, 64, 10)
        before = _state(query)
        out = np.full(want.size + 1, 0xEE, dtype=np.uint8).repeat(24).view(ctr.BIN)
        untouched = out.tobytes()

        def call(window, peak, n_bins):
            return gpu.lib.tbk_kmerdb_query_track(query._h, bases.ctypes.data, offsets.ctypes.data, n, window, peak, out.ctypes.data, n_bins)

        for window, peak, n_bins, word in ((0, 10, want.size, "window"), (64, 0, want.size, "peak"), (64, 10, want.size + 1, "bins"),
                                           (64, 10, want.size - 1, "bins"), (64, 10, 0, "bins"), (65, 10, want.size, "bins")):
            assert call(window, peak, n_bins) == _lib.TBK_ERR_INVALID, (window, peak, n_bins)
            assert word in _lib.last_error() and out.tobytes() == untouched
        for window, peak in ((0, 10), (64, 0), (-1, 10), (64, -5), (1 << 32, 10), (64, 1 << 32)):
            with pytest.raises(ValueError):
                query.track(bases, offsets, window, peak)
        assert _same_state(_state(query), before)
        assert call(64, 10, want.size) == 0 and ctr.equal(out[:want.size], want) and out[want.size:].tobytes() == untouched[-24:]
        # nothing to do is no refusal
        empty = np.zeros(1, dtype=np.uint64)
        assert gpu.lib.tbk_kmerdb_query_track(query._h, None, empty.ctypes.data, 0, 64, 10, None, 0) == 0
        short = kmers.pack_reads(["ACGT", "", "A" * 20])
        bins, short_prefix = query.track(*short, 64, 10)
        assert bins.size == 0 and short_prefix.tolist() == [0, 0, 0, 0]
        bins, empty_prefix = query.track(np.zeros(0, dtype=np.uint8), empty, 64, 10)
        assert bins.size == 0 and empty_prefix.tolist() == [0]
        _check(query, c, tally, "refusals", c.second, 64, 10)
