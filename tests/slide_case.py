"""A batch whose sequences slide through every offset of the separated stream: the helper of tests/test_gpu_query_slide.py,
tests/test_gpu_hit_track_slide.py and tests/test_host_slide_case.py.  pytest does not collect it.

The count-database query kernels and the hit tracker read a batch as one stream, every sequence followed by one 'N', in passes
of 2048 window starts, 32 windows to a lane, 16 bases to a staged chunk, 32 positions to a bitmap word, 4 counter bytes to a
word and 1024 positions to a compaction tile.  What a sequence must answer does not depend on where it lies in that stream;
what the kernels do with it does.  SlideCase(k) holds a fixed CARGO of sequences behind a LEAD, L[:s], that is sequence 0 of the
batch: shift s moves every boundary of the cargo by s stream positions (s = 0: an empty first sequence), and the cargo's
records are the same at every shift, with `read` moved by one.  The references (db_query_ref, screen_ref, read_depth_ref,
repair_ref, copy_track_ref, hit_track_ref) are asked once per k for the cargo alone and for L; the lead's record at shift s
comes from the first s - k + 1 window counters of L.  tests/test_host_slide_case.py holds what is assembled here to the
references run on whole shifted batches, and the shift set to what it claims to reach.  Nothing here touches a device.

The cargo, in this order (NAMES): sequences of 0, 1, k - 1, k and k + 1 bases; of 31, 32 and 33 windows; 160 bases with an N and
a lower-case stretch; about 400 bases (397) cut from the genome with planted edits - two substitutions at its first two bases (a stretch of
2 broken windows that no one edit mends: NONE), a substitution (k windows, SUB), a deletion (k - 1 windows, INS mends it), an
insertion (k windows, DEL), two substitutions side by side (k + 1 windows: LONG), a k-mer whose counter is 2 (broken from
min_count 3 on) and a substitution at its last base (1 window); and one sequence of 2100 + k bases, longer than a pass, all of
whose windows the database holds with a counter that changes from window to window.  First and last windows are mixed: a
sequence that ends in held windows is followed by one that begins with held windows, one that ends in absent windows by one that
begins with absent ones, so a bit or byte that bleeds in from a neighbour changes an answer.

The database holds every k-mer of L, with counters from 3, 5, 20, 254 and 255 - no 2, so that the lead has no broken window at
min_count 2 or 3 and yields no repair record - and chosen windows of the cargo with counters from 2, 3, 5, 20, 254 and 255.
Below k = 8 a random L would hold nearly every k-mer there is and leave the cargo no absent window: there L, the long sequence
and the source of the 400 bases are drawn from A, C and G alone, which keeps the database to under half of the k-mers, and
the reference alone says what the planted shapes come to."""
import numpy as np

import copy_track_ref as ctr
import db_query_ref as ref
import hit_track_ref as htr
import read_depth_ref as rd
import repair_ref as rr
import screen_ref as sr

PASS = 2048
TILE = 1024
LEAD = 2050  # two more than a pass: the first cargo boundary is stream position s + 1, and it too has to reach E + 2 of the pass edge 2048
KS = (5, 21, 32)
SMALL = tuple(range(36))
COUNTERS = (2, 3, 5, 20, 254, 255)
NAMES = ("empty", "one", "k-1", "k", "k+1", "w31", "w32", "w33", "n160", "edited400", "long")
TRACK_WINDOWS = (64, 100)
PEAK = 8  # a = 1: c = 2, 3 expanded (2c < 8), c = 5 neither, c = 20, 254 collapsed (2c > 24), c = 255 saturated
REPAIR_PARAMS = ((2, 1), (3, 2))      # (min_count, min_support)
EVIDENCE_PARAMS = ((1, 255), (10, 20))  # (min_count, max_count)
DEPTH_PARAMS = (1, 20)                 # min_count
COMPLETENESS = ((2, 255), (5, 254))


def _seq(rng, n, letters="ACGT"):
    return "".join(letters[c] for c in rng.integers(0, len(letters), n))


def _other(base, step=1):
    return "ACGT"[("ACGT".index(base) + step) % 4]


def _mix(x):
    """a fixed scramble of a k-mer's rank: which counter it gets and which list holds it do not follow its text"""
    x = (x * 0x9E3779B97F4A7C15 + 0x7F4A7C15) & ((1 << 64) - 1)
    return (x ^ (x >> 29)) % 1000003


def pack(sequences):
    """(bases uint8, offsets uint64) of a batch, as kmers.pack_reads gives them"""
    offsets = np.zeros(len(sequences) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in sequences], out=offsets[1:])
    return np.frombuffer("".join(sequences).encode(), dtype=np.uint8), offsets


class SlideCase:
    def __init__(self, k, empty=False):
        """empty: the same lead, cargo and lists against a database without an entry"""
        assert 2 <= k <= 32
        self.k, self.empty = k, empty
        rng = np.random.default_rng(6100 + k)
        narrow = "ACG" if k < 8 else "ACGT"
        self.L = _seq(rng, LEAD, narrow)
        planted = {}  # canonical k-mer -> counter

        def plant(source, windows, counters=COUNTERS):
            for w in windows:
                km = ref.canonical(source[w:w + k].upper())
                planted.setdefault(km, counters[_mix(ref.lex_rank(km)) % len(counters)])

        plant(self.L, range(LEAD - k + 1), COUNTERS[1:])
        long = _seq(rng, 2100 + k, narrow)
        plant(long, range(2101), COUNTERS[1:])
        # the short ones: (held windows, counters) - ends mixed, see the module's text
        k1, w31, w32, w33 = _seq(rng, k + 1), _seq(rng, k + 30), _seq(rng, k + 31), _seq(rng, k + 32)
        exactly_k = _seq(rng, k)
        plant(exactly_k, (0,), (255,))
        plant(k1, (1,), (5,))
        plant(w31, [0, 1] + [w for w in range(2, 29) if w * 7 % 5 < 2])           # begins held, ends absent
        plant(w32, [w for w in range(3, 30) if w * 3 % 7 < 3] + [30, 31])         # begins absent, ends held
        plant(w33, [0, 1, 2] + [w for w in range(3, 30) if w % 4 == 1] + [31, 32], COUNTERS[1:])  # held at both ends
        # 160 bases: held but for windows 20..24 and its last three; an N at 60, lower case over 100..129
        n160 = _seq(rng, 160)
        plant(n160, [w for w in range(160 - k + 1 - 3) if not 20 <= w < 25])
        n160 = n160[:60] + "N" + n160[61:100] + n160[100:130].lower() + n160[130:]
        # 400 bases with planted edits, far enough apart that their stretches do not meet
        source = list(_seq(rng, 397, narrow))
        if k < 8:  # every window over the two bases that become T holds an A as well: no k-mer of A, C and G, nor the mirror of one
            source[276:280] = source[282:286] = "AAAA"
        source = "".join(source)
        plant(source, range(397 - k + 1), COUNTERS[1:])
        low = ref.canonical(source[325:325 + k])
        if low not in ref.window_kmers(self.L, k) and low not in ref.window_kmers(long, k):
            planted[low] = 2  # held at min_count 2, broken at 3
        e = list(source)
        for p, step in ((0, 1), (1, 2), (70, 1), (280, 1), (281, 3), (396, 2)):
            e[p] = "T" if k < 8 else _other(e[p], step)
        # a deleted base that differs from both neighbours costs all k - 1 windows over the joint; an inserted one, all k over it
        gone = next(p for p in range(140, 160) if e[p - 1] != e[p] != e[p + 1])
        inserted = next(b for b in "TGCA" if b not in (e[209], e[210]))
        edited = "".join(e[:gone] + e[gone + 1:210] + [inserted] + e[210:])
        assert len(edited) == 397
        if k < 8:  # (a short random sequence above may have planted one of those windows by chance)
            for w in range(276, 282):
                planted.pop(ref.canonical(edited[w:w + k]), None)
        self.cargo = ["", "G", _seq(rng, k - 1), exactly_k, k1, w31, w32, w33, n160, edited, long]
        assert len(self.cargo) == len(NAMES)
        self.index = {name: i for i, name in enumerate(NAMES)}
        lead_kmers = set(ref.window_kmers(self.L, k))
        assert all(planted[km] >= 3 for km in lead_kmers)  # (L was planted first, without a 2)
        self.full_db = planted
        self.db = {} if empty else self.full_db
        self.file = ref.database_bytes(self.db, k)
        self.ranks = np.array(sorted(ref.lex_rank(km) for km in self.db), dtype=np.uint64)
        by_rank = {ref.lex_rank(km): c for km, c in self.db.items()}
        self.counters = np.array([by_rank[int(r)] for r in self.ranks], dtype=np.uint8)
        # the tracker's lists: of the full database's k-mers 3 in 8 to hapA alone, 3 in 8 to hapB alone, 1 in 8 to both (hapA wins)
        lots = {km: _mix(ref.lex_rank(km) + 17) % 8 for km in self.full_db}
        self.keys_a = np.array(sorted(htr.canonical(km) for km, lot in lots.items() if lot in (0, 1, 2, 6)), dtype=np.uint64)
        self.keys_b = np.array(sorted(htr.canonical(km) for km, lot in lots.items() if lot in (3, 4, 5, 6)), dtype=np.uint64)
        self.in_both = sum(lot == 6 for lot in lots.values())

        # ---- geometry: the cargo's boundaries in the stream at shift 0 (the lead's separator is position s) ----
        self.lengths = [len(s) for s in self.cargo]
        self.starts0 = [1 + sum(n + 1 for n in self.lengths[:i]) for i in range(len(self.cargo))]
        self.ends0 = [a + n for a, n in zip(self.starts0, self.lengths)]  # the separator behind each
        self.cargo_stream = sum(n + 1 for n in self.lengths)
        self.cargo_bytes = np.frombuffer("".join(self.cargo).encode(), dtype=np.uint8)
        self.lead_bytes = np.frombuffer(self.L.encode(), dtype=np.uint8)
        self.cargo_offsets = np.zeros(len(self.cargo) + 1, dtype=np.uint64)
        np.cumsum(self.lengths, out=self.cargo_offsets[1:])

        # ---- the references, once: the cargo alone, and L ----
        self.cargo_counters = sr.window_counters(self.db, self.cargo, k)
        self.lead_counters = sr.window_counters(self.db, [self.L], k)[0]
        assert None not in self.lead_counters
        if not empty:
            assert min(self.lead_counters) >= 3 and not rr.stretches(self.db, self.L, k, 3)  # no prefix of L has a broken window
        self.broken400 = rr.stretches(self.full_db, self.cargo[self.index["edited400"]].upper(), k, 2)
        self._cache = {}

    # ---- batches -------------------------------------------------------------------------------------------------------------
    def lead(self, s):
        return self.L[:s]

    def batch(self, s):
        return [self.lead(s)] + self.cargo

    def packed(self, s):
        """(bases, offsets) of the batch at shift s, without a string being built"""
        offsets = np.concatenate([[0], self.cargo_offsets + np.uint64(s)]).astype(np.uint64)
        return np.concatenate([self.lead_bytes[:s], self.cargo_bytes]), offsets

    def total(self, s):
        """the length of the separated stream: bytes at or past it are refused"""
        return s + 1 + self.cargo_stream

    def boundaries(self):
        """[(name, 'start' or 'end', stream position at shift 0)]: a start is a sequence's first base, an end its separator"""
        out = []
        for name, a, b in zip(NAMES, self.starts0, self.ends0):
            out += [(name, "start", a), (name, "end", b)]
        return out

    def stretch_edges(self):
        """stream positions at shift 0 of the first window of each broken stretch of the 400 bases, and of the window behind its last"""
        a = self.starts0[self.index["edited400"]]
        return sorted({a + f for f, _ in self.broken400} | {a + l + 1 for _, l in self.broken400})

    def shifts(self, thin=False):
        """every s in 0..129; every s in 0..LEAD that puts a cargo boundary at E - (k + 2) .. E + 2 of a pass edge E, or at
        -2 .. +2 of a tile edge; the same -2 .. +2 of a tile edge for the edges of the 400 bases' broken stretches.
        thin: the pass edges in full for the k-base, the 33-window and the long sequence only, -2 .. +2 for the others."""
        out = set(range(130))
        full = ("k", "w33", "long")
        for name, _, at in self.boundaries():
            for edge in (PASS, 2 * PASS):
                lo = -(self.k + 2) if not thin or name in full else -2
                out.update(edge + d - at for d in range(lo, 3))
            for edge in range(TILE, self.total(LEAD) + TILE, TILE):
                out.update(edge + d - at for d in range(-2, 3))
        for at in self.stretch_edges():
            for edge in range(TILE, self.total(LEAD) + TILE, TILE):
                out.update(edge + d - at for d in range(-2, 3))
        return sorted(s for s in out if 0 <= s <= LEAD)

    def place(self, s, i):
        """for a failure's message: where cargo sequence i lies at shift s"""
        a, b = s + self.starts0[i], s + self.ends0[i]
        return "shift {}, sequence {} ({}, read {}): start {} (mod 4: {}, mod 32: {}, mod 2048: {}), end {} (mod 4: {}, mod 32: {}, mod 2048: {}), total {}".format(
            s, i, NAMES[i], i + 1, a, a % 4, a % 32, a % PASS, b, b % 4, b % 32, b % PASS, self.total(s))

    def _once(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def _lead_windows(self, s):
        return max(s - self.k + 1, 0)

    # ---- add: per_read and the count bytes -----------------------------------------------------------------------------------
    def want_add(self, s, min_count=2):
        def cargo():
            per_read, counts = ref.Tally(self.db).add(self.cargo, self.k, min_count)
            lead = np.array(self.lead_counters, dtype=np.uint8)
            found = np.concatenate([[0], np.cumsum(lead >= max(2, min_count))])
            return per_read, counts, lead, found

        per_read, counts, lead, found = self._once(("add", min_count), cargo)
        n = self._lead_windows(s)
        first = np.array([[n, found[n]]], dtype=np.uint64)
        return np.concatenate([first, per_read]), np.concatenate([lead[:n], np.zeros(s - n, dtype=np.uint8), counts])

    def tally(self):
        return ref.TallyNp(self.ranks, self.counters)

    # ---- track ---------------------------------------------------------------------------------------------------------------
    def want_track(self, s, tally, window, peak=PEAK):
        """(bins, prefix) at shift s against a tally that was given the unshifted cargo once (`cargo_tally`)"""
        bins, prefix = self._once(("track", window, peak), lambda: ctr.track_np(tally, self.cargo_bytes, self.cargo_offsets, self.k, window, peak))
        lead_bins, lead_prefix = ctr.track_np(tally, self.lead_bytes[:s], np.array([0, s], dtype=np.uint64), self.k, window, peak)
        return np.concatenate([lead_bins, bins]), np.concatenate([lead_prefix[:1], prefix + lead_prefix[1]])

    def cargo_tally(self):
        tally = self.tally()
        tally.add(self.cargo_bytes, self.cargo_offsets, self.k)
        return tally

    # ---- repairs -------------------------------------------------------------------------------------------------------------
    def want_repairs(self, s, min_count, min_support):
        def cargo():
            evaluated = self._once(("evaluated", min_count), lambda: rr.evaluate(self.db, self.cargo, self.k, min_count))
            arr = rr.as_array(rr.records(evaluated, self.k, min_support))
            arr["read"] += 1
            return arr

        arr = self._once(("repairs", min_count, min_support), cargo)
        if not self.empty or s < self.k:
            return arr  # the lead has no broken window
        return np.concatenate([rr.as_array(rr.repairs(self.db, [self.lead(s)], self.k, min_count, min_support)), arr])

    # ---- evidence ------------------------------------------------------------------------------------------------------------
    def _lead_evidence(self, min_count, max_count):
        """the records of L[:s] for every s in 0..LEAD in one walk: window s - k joins at step s, and the bases it covers are
        new from the end of the covered run before it on.  tests/test_host_slide_case.py holds it to screen_ref.record."""
        k, m = self.k, sr.threshold(min_count)
        out = np.zeros(LEAD + 1, dtype=sr.READ_EVIDENCE)
        clean = held = covered = longest = stretches = 0
        run_start = run_end = -1  # the last covered run is [run_start, run_end)
        for s in range(1, LEAD + 1):
            w = s - k
            if w >= 0:
                c = self.lead_counters[w]
                clean += 1
                if m <= c <= max_count:
                    held += 1
                    if run_end >= w and run_start >= 0:  # it touches or overlaps the last run
                        covered += w + k - run_end
                    else:
                        covered += k
                        stretches += 1
                        run_start = w
                    run_end = w + k
                    longest = max(longest, run_end - run_start)
            out[s] = (clean, held, covered, longest, stretches)
        return out

    def want_evidence(self, s, min_count, max_count):
        cargo = self._once(("evidence", min_count, max_count),
                           lambda: sr.as_array(sr.records(self.cargo_counters, self.lengths, self.k, min_count, max_count)))
        lead = self._once(("lead evidence", min_count, max_count), lambda: self._lead_evidence(min_count, max_count))
        return np.concatenate([lead[s:s + 1], cargo])

    # ---- read depth ----------------------------------------------------------------------------------------------------------
    def want_read_depth(self, s, min_count):
        cargo = self._once(("depth", min_count), lambda: rd.as_array(rd.records(self.cargo_counters, min_count)))
        lead = rd.as_array([rd.record(self.lead_counters[:self._lead_windows(s)], rd.threshold(min_count))])
        return np.concatenate([lead, cargo])

    # ---- the hit tracker -----------------------------------------------------------------------------------------------------
    def want_track_marks(self, s, ignore_case=False):
        """(marks, runs, counts) of the batch at shift s"""
        def once():
            marks = htr.marks(self.cargo_bytes, self.cargo_offsets, self.keys_a, self.keys_b, self.k, ignore_case)
            runs = htr.runs(marks, self.cargo_offsets)
            runs["read"] += 1
            lead = htr.marks(self.lead_bytes, np.array([0, LEAD], dtype=np.uint64), self.keys_a, self.keys_b, self.k, ignore_case)
            return marks, runs, htr.counts_of(marks, self.cargo_offsets), lead

        marks, runs, counts, lead = self._once(("marks", ignore_case), once)
        n = self._lead_windows(s)
        mine = np.concatenate([lead[:n], np.zeros(s - n, dtype=np.uint8)])
        offsets = np.array([0, s], dtype=np.uint64)
        lead_runs = htr.runs(mine, offsets)
        if not lead_runs.size:
            lead_runs = np.zeros(0, dtype=htr.RUN_DTYPE)
        return np.concatenate([mine, marks]), np.concatenate([lead_runs, runs]), np.concatenate([htr.counts_of(mine, offsets), counts])


_CASES = {}


def case(k, empty=False):
    """one SlideCase per (k, empty) and process: the references are asked once"""
    if (k, empty) not in _CASES:
        _CASES[k, empty] = SlideCase(k, empty)
    return _CASES[k, empty]
