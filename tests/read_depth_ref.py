"""The reference of the read depth's tests (include/tbk.h, "read depth") and of read_depth's rule, in plain Python on top of
db_query_ref's canonical k-mers and screen_ref.window_counters: per sequence the list of the depths of its clean windows, sorted()
and indexed as the header says.  No histogram and no bit tricks.  The rule is written in Python integers, splitmix64 in
arbitrary-precision ints masked to 64 bits.  tests/test_host_read_depth_ref.py holds all of it to a second formulation and to
hand-worked records.  Nothing here touches a device."""
import numpy as np

import screen_ref as sr

# tbk_read_depth (40 bytes)
READ_DEPTH = np.dtype([("clean", "<u8"), ("present", "<u8"), ("saturated", "<u8"), ("sum", "<u8"), ("lowest", "u1"), ("q1", "u1"), ("median", "u1"),
                       ("q3", "u1"), ("highest", "u1"), ("present_median", "u1"), ("pad", "u1", (2,))])
assert READ_DEPTH.itemsize == 40
FIELDS = ("clean", "present", "saturated", "sum", "lowest", "q1", "median", "q3", "highest", "present_median")
BINS = {"A": "kept", "B": "dropped", "U": "unjudged"}
STATISTICS = {"median": 6, "present-median": 9, "q1": 5, "q3": 7, "lowest": 4, "highest": 8}  # --by: the place in FIELDS
MASK = (1 << 64) - 1

threshold = sr.threshold
window_counters = sr.window_counters


def depths(counters, m):
    """the depths of a sequence's clean windows, in window order: the counter when it is m or more, else 0"""
    return [c if c >= m else 0 for c in counters if c is not None]


def record(counters, m):
    """the tuple of FIELDS of one sequence from its windows' counters"""
    d = depths(counters, m)
    clean = len(d)
    if not clean:
        return (0,) * 10
    v = sorted(d)
    there = [x for x in v if x >= 1]
    five = [v[j * (clean - 1) // 4] for j in range(5)]
    return (clean, len(there), sum(1 for x in d if x == 255), sum(d), *five, there[2 * (len(there) - 1) // 4] if there else 0)


def records(counters, min_count=1, floor=2):
    """one tuple of FIELDS per sequence, from `window_counters`' answer"""
    m = threshold(min_count, floor)
    return [record(c, m) for c in counters]


def read_depth(db, sequences, k, min_count=1, floor=2):
    """one tuple of FIELDS per sequence of the batch: the rule as the header has it"""
    return records(window_counters(db, sequences, k), min_count, floor)


def as_array(recs):
    out = np.zeros(len(recs), dtype=READ_DEPTH)
    for i, rec in enumerate(recs):
        for name, value in zip(FIELDS, rec):
            out[i][name] = value
    return out


first_difference = sr.first_difference


# ---- read_depth's rule and its tables -------------------------------------------------------------------------------------------------
def splitmix64(seed, n):
    """the n-th output (n >= 1) of splitmix64 from state `seed`"""
    x = (seed + n * 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def draw(seed, i):
    """u(seed, i): the upper 32 bits of the (i + 1)-th output"""
    return splitmix64(seed, i + 1) >> 32


def bin_of(rec, ordinal, by="median", min_depth=0, max_depth=255, target=None, seed=0):
    """'U', 'A' (kept) or 'B' (dropped) for one record (a tuple of FIELDS) of the read at 0-based place `ordinal` of the input"""
    if rec[0] == 0:
        return "U"
    s = rec[STATISTICS[by]]
    if s < min_depth or s > max_depth:
        return "B"
    if target is not None and s > target and draw(seed, ordinal) * s >= target * (1 << 32):
        return "B"
    return "A"


def bins_of(recs, **rule):
    return "".join(bin_of(rec, i, **rule) for i, rec in enumerate(recs))


def table(names, sequences, recs, bins):
    """the --table file: name length, the ten FIELDS, bin"""
    return "".join("\t".join([name, str(len(s))] + [str(v) for v in rec] + [BINS[b]]) + "\n" for name, s, rec, b in zip(names, sequences, recs, bins))


def spectrum(sequences, recs, bins, by="median"):
    """the --spectrum file: 256 lines depth reads bases kept_reads kept_bases, over the judged reads by their statistic"""
    lines = []
    for depth in range(256):
        judged = [len(s) for s, rec, b in zip(sequences, recs, bins) if b != "U" and rec[STATISTICS[by]] == depth]
        kept = [len(s) for s, rec, b in zip(sequences, recs, bins) if b == "A" and rec[STATISTICS[by]] == depth]
        lines.append("{}\t{}\t{}\t{}\t{}\n".format(depth, len(judged), sum(judged), len(kept), sum(kept)))
    return "".join(lines)


def summary(sequences, bins, m, by="median", min_depth=0, max_depth=255, target=None, seed=0):
    """stdout: reads and bases per bin, then the rule with the lower bound in force"""
    lines = []
    for code in "ABU":
        mine = [s for s, b in zip(sequences, bins) if b == code]
        lines.append("#{}\t{}\t{}".format(BINS[code], len(mine), sum(len(s) for s in mine)))
    lines.append("\t".join(["#rule", str(m), by, str(min_depth), str(max_depth), "-" if target is None else str(target), str(seed)]))
    return "".join(line + "\n" for line in lines)
