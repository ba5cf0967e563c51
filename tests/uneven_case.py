"""One crafted k = 21 count database whose directory is uneven, and one batch that walks through it: what
tests/test_host_query_uneven.py asserts from numpy alone and tests/test_gpu_query_uneven.py gives to a query session.

The database holds between 2^18 and 2^19 entries, so a session's directory has 17 prefix bits - the first eight bases and one
bit of the ninth - and a mean bucket of two to three entries.  Into that it plants one DEEP bucket, the one of the prefix
CCCCCCCC[AC]: windows 0 .. 3 of 2000 sequences `C * 12 + 30 random bases`, more than 4096 entries, a bisection of 13 steps.
The buckets directly before and behind it are kept empty, rank 0 (A * 21) is the first entry, and the counters are 1 (in the
full twin alone), 2, 5, 10, 20, 127 and 255.  The batch is small enough for the Python-loop references (repair_ref,
screen_ref) over tests/rank_db.py.  `claims` asserts, on the inputs and on the references' answers, everything the batch was
built for, and returns the numbers.  Nothing here touches a device."""
import time

import numpy as np

import copy_track_ref as ctr
import db_query_ref as ref
import kmerdb_files as kf
import rank_db
import repair_ref as rr
import screen_ref as sr

K = 21
PASS = 2048
PREFIX_BITS = 17
SHIFT = 2 * K - PREFIX_BITS
GENOME = 300_000
DEEP_SEQUENCES = 2000
RUN = "C" * 12
FULL = b"TBKKMFB1"
LOW, HIGH = (1, 2, 5), (10, 20, 127, 255)
REPAIR_PARAMETERS = {False: ((2, 1), (10, 11)), True: ((2, 1), (10, 11), (1, 1))}
RANGES = ((1, 255), (10, 20), (255, 255), (1, 1))
WINDOWS = (1, 64, 1 << 31)
PEAK = 10
_LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def _text(codes):
    return _LETTERS[codes].tobytes().decode()


def _ranks_of(sequences):
    """(rank, clean) per base of the sequences, back to back, and their offsets"""
    bases = np.frombuffer("".join(sequences).encode(), dtype=np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in sequences])]).astype(np.uint64)
    return ref.window_ranks(bases, offsets, K) + (offsets,)


def _forward(kmer):
    """the k-mer is canonical as it stands"""
    return ref.canonical(kmer) == kmer


class Case:
    def __init__(self):
        rng = np.random.default_rng(1700)
        genome = _text(rng.integers(0, 4, GENOME))
        self.genome = genome
        deep = [RUN + _text(rng.integers(0, 4, 30)) for _ in range(DEEP_SEQUENCES)]
        self.prefix = ref.lex_rank("C" * 9 + "A" * 12) >> SHIFT  # the deep bucket: CCCCCCCC and a ninth base of A or C

        # ---- the sequences whose every window the database holds: a flank, a deep sequence, a flank ----------------------------
        # (behind the run they go on with A and then A or C: the window behind the four deep ones falls into the deep bucket too, and
        # the one behind that two buckets below it - neither into a neighbour, which stay empty; no two equal bases where the errors go)
        whole = [d for d in deep if all(_forward(d[w:w + K]) for w in range(4))]  # all four windows are canonical as they stand: in the deep bucket
        apt = [d for d in whole if d[12] == "A" and d[13] in "AC" and all(d[i] != d[i + 1] for i in range(14, 22))]
        assert len(apt) >= 7
        flank = lambda i, n: genome[1000 + 700 * i:1000 + 700 * i + n]  # noqa: E731
        carriers = {name: flank(2 * i, 40) + apt[i] + flank(2 * i + 1, 40) for i, name in enumerate(("clean", "sub", "sub_lower", "missing", "extra", "mirrored"))}
        walks = [flank(20 + 2 * i, 40 + i) + [d for d in whole if d not in apt][i] + flank(21 + 2 * i, 40) for i in range(8)]  # eight alignments of the deep run; only its four windows are held
        # the sequences in front of the one that crosses the pass edge, by length: 16 of k bases, the walks, three carriers
        before_edge = 16 * (K + 1) + sum(len(w) + 1 for w in walks) + (122 + 1) + 122 + 1 + (121 + 1)
        self.edge_flank = PASS - 2 - before_edge  # its deep windows are the stream positions 2046 .. 2049
        assert 30 <= self.edge_flank <= 600, self.edge_flank
        carriers["edge"] = genome[200_000:200_000 + self.edge_flank] + apt[6] + flank(40, 40)
        self.carriers = carriers

        # ---- the database ---------------------------------------------------------------------------------------------------------
        rank, clean, _ = _ranks_of([genome])
        from_genome = np.unique(rank[clean])
        from_genome = from_genome[np.abs((from_genome >> np.uint64(SHIFT)).astype(np.int64) - self.prefix) > 1]  # the deep bucket's neighbours stay empty
        rank, clean, offsets = _ranks_of(deep)
        from_deep = np.concatenate([rank[int(o):int(o) + 4] for o in offsets[:-1]])
        rank, clean, _ = _ranks_of(list(carriers.values()))
        from_carriers = np.unique(rank[clean])
        ranks = np.unique(np.concatenate([from_genome, from_deep, from_carriers, np.zeros(1, dtype=np.uint64)]))
        h = (ranks * np.uint64(7) + np.uint64(K)) % np.uint64(907)
        counters = np.where(h < 3, np.array(LOW, dtype=np.uint8)[np.minimum(h, 2).astype(np.int64)], np.array(HIGH, dtype=np.uint8)[(h % np.uint64(4)).astype(np.int64)])
        carried = np.isin(ranks, from_carriers)
        counters[carried] = np.array(HIGH, dtype=np.uint8)[(h[carried] % np.uint64(4)).astype(np.int64)]  # a carrier is held at every threshold up to 10
        in_deep = np.flatnonzero((ranks >> np.uint64(SHIFT)).astype(np.int64) == self.prefix)
        self.deep_first, self.deep_last, self.deep_middle = int(in_deep[0]), int(in_deep[-1]), int(in_deep[in_deep.size // 2])
        self.chosen = {"rank 0": (0, 255), "last": (ranks.size - 1, 127), "deep first": (self.deep_first, 2), "deep last": (self.deep_last, 5),
                       "deep middle": (self.deep_middle, 20)}
        for at, c in self.chosen.values():
            counters[at] = c
        solid = counters >= 2
        self.ranks = {True: ranks, False: ranks[solid]}
        self.counters = {True: counters.astype(np.uint8), False: counters[solid].astype(np.uint8)}
        self.db = {full: rank_db.RankDb(self.ranks[full], self.counters[full], K) for full in (False, True)}
        hist = np.bincount(counters, minlength=256).astype(np.uint64)
        hist[0] = ranks.size
        self.files = {True: kf.file_bytes(K, ranks, counters, hist, reads=1, bases=GENOME, magic=FULL),
                      False: kf.file_bytes(K, self.ranks[False], self.counters[False], hist, reads=1, bases=GENOME)}

        # ---- the batch ------------------------------------------------------------------------------------------------------------
        name = lambda at: rank_db.kmer_string(ranks[at], K)  # noqa: E731
        first, last, middle, top = name(self.deep_first), name(self.deep_last), name(self.deep_middle), name(ranks.size - 1)
        between_at = next(j for j in range(self.deep_middle + 1, self.deep_last) if ranks[j] + np.uint64(1) < ranks[j + 1] and _forward(rank_db.kmer_string(int(ranks[j]) + 1, K)))
        self.misses = {"below": "C" * 8 + "A" + "ACGTACGTACGA", "above": "C" * 9 + "T" * 10 + "GA",
                       "between": rank_db.kmer_string(int(ranks[between_at]) + 1, K),
                       "empty before": "C" * 7 + "A" + "T" + "ACGTACGTACGA", "empty behind": "C" * 8 + "G" + "ACGTACGTACGA"}
        singles = [first, last, middle] + list(self.misses.values()) + ["A" * K, "T" * K, "a" * K, "t" * K, top, ref.revcomp(top), top.lower(), ref.revcomp(top).lower()]
        self.single_names = ["deep first", "deep last", "deep middle"] + list(self.misses) + ["rank 0"] * 4 + ["last"] * 4
        # the errors, in the random tail of a carrier's deep sequence: bases 57 .. 59 of the carrier, five to seven behind the run
        truth = carriers
        other = lambda c, *avoid: next(b for b in "ACGT" if b != c and b not in avoid)  # noqa: E731
        sub = truth["sub"][:57] + other(truth["sub"][57]) + truth["sub"][58:]
        sub_lower = (truth["sub_lower"][:58] + other(truth["sub_lower"][58]) + truth["sub_lower"][59:]).lower()
        missing = truth["missing"][:59] + truth["missing"][60:]
        extra = truth["extra"][:58] + other(truth["extra"][57], truth["extra"][58]) + truth["extra"][58:]
        assert len(singles) == 16 and all(_forward(m) for m in self.misses.values()) and [len(s) for s in (sub, missing)] == [122, 121]
        long_read = list(genome[50_000:53_200])
        long_read[700] = "N"
        long_read[900:960] = [c.lower() for c in long_read[900:960]]
        # (the long read fills the second pass: what follows it lies in the third and fourth)
        named = [("clean", truth["clean"]), ("sub", sub), ("missing", missing), ("edge", truth["edge"]), ("long", "".join(long_read)), ("extra", extra),
                 ("sub_lower", sub_lower), ("mirrored", ref.revcomp(truth["mirrored"])), ("late", truth["clean"])]
        self.batch = singles + walks + [s for _, s in named] + ["", truth["clean"][:K - 1], genome[1000:1040] + RUN + "ACGTTGCA", ref.revcomp(genome[60_000:60_400]).lower()]
        self.reads = dict({"walks": range(16, 24)}, **{name: 24 + i for i, (name, _) in enumerate(named)})
        self.bases = np.frombuffer("".join(self.batch).encode(), dtype=np.uint8)
        self.offsets = np.concatenate([[0], np.cumsum([len(s) for s in self.batch])]).astype(np.uint64)
        self.packed = (self.bases, self.offsets)
        self.lengths = [len(s) for s in self.batch]
        self.stream = np.arange(self.bases.size) + np.repeat(np.arange(len(self.batch)), self.lengths)  # a separator behind every sequence
        self._repairs, self._counters, self._tracks = {}, {}, {}
        self.seconds = {}

    # ---- the references' answers, each computed once -----------------------------------------------------------------------------
    def tally(self, full):
        return ref.TallyNp(self.ranks[full], self.counters[full])

    def want_repairs(self, min_count, min_support, full):
        key = (min_count, full)
        if key not in self._repairs:
            t0 = time.perf_counter()
            self._repairs[key] = rr.evaluate(self.db[full], self.batch, K, min_count, floor=1 if full else 2)
            self.seconds["repairs", min_count, full] = time.perf_counter() - t0
        return rr.as_array(rr.records(self._repairs[key], K, min_support))

    def want_evidence(self, min_count, max_count, full):
        if full not in self._counters:
            t0 = time.perf_counter()
            self._counters[full] = sr.window_counters(self.db[full], self.batch, K)
            self.seconds["evidence", full] = time.perf_counter() - t0
        return sr.as_array(sr.records(self._counters[full], self.lengths, K, min_count, max_count, floor=1 if full else 2))

    def want_track(self, tally, state, full, window):
        """`state` names what was added to `tally` so far"""
        key = (state, full, window)
        if key not in self._tracks:
            self._tracks[key] = ctr.track_np(tally, self.bases, self.offsets, K, window, PEAK)
        return self._tracks[key]


_CASE = []


def case():
    if not _CASE:
        _CASE.append(Case())
    return _CASE[0]


def claims(c):
    """Every claim of the module's docstring, asserted from numpy on the inputs and on the references' answers.  Returns the
    numbers that make the tests on this case non-vacuous."""
    out = {}
    rank, clean = ref.window_ranks(c.bases, c.offsets, K)
    assert c.bases.size <= 12_000 and int(c.offsets[-1]) == c.bases.size
    out["bases"], out["stream positions"] = int(c.bases.size), int(c.stream[-1]) + 2
    where = lambda read, w=0: int(c.offsets[read]) + w  # noqa: E731
    for full in (False, True):
        ranks, counters = c.ranks[full], c.counters[full]
        n = int(ranks.size)
        # the directory, as tbk_count.cpp chooses it: floor(log2 n) - 1 bits, and the buckets' sizes
        assert 1 << 18 < n < 1 << 19 and n.bit_length() - 2 == PREFIX_BITS
        sizes = np.bincount((ranks >> np.uint64(SHIFT)).astype(np.int64), minlength=1 << PREFIX_BITS)
        assert sizes.size == 1 << PREFIX_BITS and int(sizes.sum()) == n
        deep_size = int(sizes[c.prefix])
        assert 4096 <= deep_size < 8192 and deep_size.bit_length() == 13  # a bisection of 13 steps
        assert int(sizes[c.prefix - 1]) == 0 and int(sizes[c.prefix + 1]) == 0
        rest = np.delete(sizes, c.prefix)
        assert int(rest.max()) <= 24 and 2 <= n / sizes.size < 4
        assert int(ranks[0]) == 0 and int(counters[0]) == 255 and int(counters[-1]) == 127
        assert set(np.unique(counters).tolist()) == set((LOW if full else LOW[1:]) + HIGH)
        in_deep = np.flatnonzero((ranks >> np.uint64(SHIFT)).astype(np.int64) == c.prefix)
        first, last = int(in_deep[0]), int(in_deep[-1])
        assert in_deep.size == deep_size and last - first + 1 == deep_size
        assert ranks[first] == c.ranks[True][c.deep_first] and ranks[last] == c.ranks[True][c.deep_last]  # the same in both databases
        # what the numpy reference finds, window by window
        tally = c.tally(full)
        _, counts = tally.add(c.bases, c.offsets, K)
        size_of = np.where(clean, sizes[(rank >> np.uint64(SHIFT)).astype(np.int64)], -1)
        in_bucket = clean & ((rank >> np.uint64(SHIFT)).astype(np.int64) == c.prefix)
        # ---- the singles: hits at the deep bucket's edges and middle, the misses' three kinds, an empty bucket, the extremes ----
        for read, name in enumerate(c.single_names):
            w = where(read)
            assert c.lengths[read] == K and clean[w], name
            if name in c.chosen:
                entry, counter = c.chosen[name]
                assert rank[w] == c.ranks[True][entry] and int(counts[w]) == counter, name
                assert name[:4] != "deep" or in_bucket[w]
            else:
                assert int(counts[w]) == 0, name
                if name == "below":
                    assert in_bucket[w] and rank[w] < ranks[first]
                elif name == "above":
                    assert in_bucket[w] and rank[w] > ranks[last]
                elif name == "between":
                    below = int(np.searchsorted(ranks, rank[w])) - 1
                    assert in_bucket[w] and first <= below < last and ranks[below] < rank[w] < ranks[below + 1]
                else:
                    assert int(size_of[w]) == 0 and abs(int(rank[w] >> np.uint64(SHIFT)) - c.prefix) == 1, name
        assert c.batch[8:12] == ["A" * K, "T" * K, "a" * K, "t" * K] and c.batch[13] == ref.revcomp(c.batch[12]) and c.batch[14] == c.batch[12].lower() != c.batch[12]
        assert int(tally.copies[0]) == 4 and int(tally.copies[-1]) == 4 and int(tally.copies[first]) >= 1 and int(tally.copies[last]) >= 1
        # ---- the groups of four: stream positions 4g .. 4g + 3 are one lane's searches in flight together ----------------------
        deep = size_of >= 4096
        shallow = clean & (size_of <= 4)
        group = c.stream // 4
        n_groups = int(group[-1]) + 1
        with_shallow = np.bincount(group[shallow], minlength=n_groups) > 0
        deep_first = np.zeros(n_groups, dtype=bool)
        deep_last = np.zeros(n_groups, dtype=bool)
        deep_first[group[deep & (c.stream % 4 == 0)]] = True
        deep_last[group[deep & (c.stream % 4 == 3)]] = True
        mixes = (int((deep_first & with_shallow).sum()), int((deep_last & with_shallow).sum()))
        assert mixes[0] >= 4 and mixes[1] >= 4, mixes
        # a deep search that hits beside a shallow one that hits, in one group
        hit = clean & (counts > 0)
        both = (np.bincount(group[deep & hit], minlength=n_groups) > 0) & (np.bincount(group[shallow & hit], minlength=n_groups) > 0)
        assert int(both.sum()) >= 1, int(both.sum())
        # every walk and carrier enters the deep bucket from a flank and leaves it again: four searches in a row there, at every
        # alignment - hits, but in the sequences with an error, whose deep windows hold the error and miss
        alignments = set()
        for read in list(c.reads["walks"]) + [c.reads[name] for name in ("clean", "sub", "missing", "edge", "extra", "sub_lower")]:
            lo, hi = int(c.offsets[read]), int(c.offsets[read + 1])
            run = lo + (40 + read - c.reads["walks"][0] if read in c.reads["walks"] else c.edge_flank if read == c.reads["edge"] else 40)  # behind the flank
            erroneous = read in [c.reads[name] for name in ("sub", "missing", "extra", "sub_lower")]
            assert c.batch[read][run - lo:run - lo + 12].upper() == RUN and deep[run:run + 4].any() and not deep[run - 8:run - 1].any(), read
            assert not hit[run:run + 4].any() if erroneous else (hit[run:run + 4].all() and deep[run:run + 4].all()), read
            for outside in (slice(lo, lo + 10), slice(hi - K - 9, hi - K + 1)):  # ten windows of a flank at either end
                assert clean[outside].all() and not deep[outside].any() and shallow[outside].any(), read
            alignments.add(int(c.stream[run]) % 4)
        assert alignments == {0, 1, 2, 3}
        lo = int(c.offsets[c.reads["mirrored"]])
        assert (deep[lo:lo + 122] & hit[lo:lo + 122]).sum() >= 4  # and as a reverse complement
        # ---- the pass edge at stream position 2048 lies inside a run of deep hits ------------------------------------------------
        edge = where(c.reads["edge"], c.edge_flank)
        assert c.stream[edge:edge + 4].tolist() == [PASS - 2, PASS - 1, PASS, PASS + 1] and (deep[edge:edge + 4] & hit[edge:edge + 4]).all()
        # and deep hits and stretches lie in the third pass or behind it: a later trip for a grid of one or two waves
        assert out["stream positions"] > 3 * PASS and (deep & hit & (c.stream >= 2 * PASS)).sum() >= 8
        assert all(c.stream[where(c.reads[name])] >= 2 * PASS for name in ("extra", "sub_lower", "mirrored", "late"))
        # ---- every feature of a track speaks ------------------------------------------------------------------------------------
        bins = c.want_track(tally, 1, full, 64)[0]
        assert all(int(bins[f].max()) > 0 for f in ctr.FIELDS), [int(bins[f].max()) for f in ctr.FIELDS]
        # ---- the repairs ----------------------------------------------------------------------------------------------------------
        plain = c.want_repairs(2, 1, full)
        kinds = np.bincount(plain["kind"], minlength=5)
        for name, kind in (("sub", rr.SUB), ("sub_lower", rr.SUB), ("missing", rr.INS), ("extra", rr.DEL)):
            mine = plain[plain["read"] == c.reads[name]]
            assert mine.size == 1 and int(mine["kind"][0]) == kind and int(mine["accepted"][0]) >= 1, (name, mine)
            # the candidates' windows: some in the deep bucket, some elsewhere
            f, windows = int(mine["first"][0]), int(mine["windows"][0])
            lo = where(c.reads[name])
            truth = ref.window_ranks(np.frombuffer(c.carriers[name].encode(), dtype=np.uint8), [0, len(c.carriers[name])], K)[0][f:f + windows]
            inside = (truth >> np.uint64(SHIFT)).astype(np.int64) == c.prefix
            assert 4 <= int(inside.sum()) < windows and windows <= K, name
            assert int(mine["base"][0]) == (0 if kind == rr.DEL else ord(c.carriers[name][int(mine["pos"][0])])), name  # the edit restores the carrier
        assert all(kinds[kind] >= 1 for kind in (rr.NONE, rr.SUB, rr.DEL, rr.INS, rr.LONG)), kinds
        assert not (plain["read"] == c.reads["clean"]).any() and not (plain["read"] == c.reads["edge"]).any()
        for min_count, min_support in REPAIR_PARAMETERS[full][1:]:
            assert c.want_repairs(min_count, min_support, full).tobytes() != plain.tobytes(), (min_count, min_support)
        # ---- the evidence ---------------------------------------------------------------------------------------------------------
        whole = c.want_evidence(1, 255, full)
        assert tuple(int(v) for v in whole[c.reads["clean"]]) == (102, 102, 122, 122, 1)
        answers = [c.want_evidence(lo, hi, full).tobytes() for lo, hi in RANGES]
        assert len(set(answers)) == 4 and (full or not c.want_evidence(1, 1, False)["held"].any())
        assert c.want_evidence(255, 255, full)["held"].any() and (not full or c.want_evidence(1, 1, True)["held"].any())
        out[full] = {"entries": n, "directory bits": n.bit_length() - 2, "deep bucket": deep_size, "largest other bucket": int(rest.max()),
                     "groups with the deep search first": mixes[0], "groups with the deep search last": mixes[1],
                     "groups with a deep and a shallow hit": int(both.sum()),
                     "repair records by kind (none, sub, del, ins, long)": kinds.tolist()}
    out["seconds"] = {" ".join(str(x) for x in key): round(v, 2) for key, v in c.seconds.items()}
    assert all(v < 30 for v in c.seconds.values()), c.seconds
    return out
