"""The reference of the read evidence's tests (include/tbk.h, "read evidence") and of screen_reads' rule, in plain Python on top
of db_query_ref's canonical k-mers: a loop over the windows of each sequence that marks the k bases of every held window in a
list of booleans, and a loop over the bases that counts the runs.  No bit tricks.  The rule is written with fractions.Fraction.
tests/test_host_screen_ref.py holds the loops to a second formulation and to hand-worked records.  Nothing here touches a device."""
from fractions import Fraction

import numpy as np

import db_query_ref as ref

# tbk_read_evidence (40 bytes)
READ_EVIDENCE = np.dtype([("clean", "<u8"), ("held", "<u8"), ("covered", "<u8"), ("longest", "<u8"), ("stretches", "<u8")])
assert READ_EVIDENCE.itemsize == 40
FIELDS = ("clean", "held", "covered", "longest", "stretches")
BINS = {"A": "matched", "B": "unmatched", "U": "unjudged"}


def threshold(min_count, floor=2):
    return max(floor, min_count)


def window_counters(db, sequences, k):
    """per sequence, per window start: the database's counter of the window's canonical k-mer (0: absent), None for a window that
    is not clean.  What does not depend on the counter range, computed once."""
    return [[None if km is None else db.get(km, 0) for km in ref.window_kmers(s, k)] for s in sequences]


def record(counters, length, k, m, max_count):
    """(clean, held, covered, longest, stretches) of one sequence of `length` bases from its windows' counters"""
    clean = held = 0
    covered = [False] * length
    for w, c in enumerate(counters):
        if c is None:
            continue
        clean += 1
        if m <= c <= max_count:
            held += 1
            for p in range(w, w + k):
                covered[p] = True
    longest = stretches = run = 0
    for p in range(length):
        if covered[p]:
            run += 1
            if run == 1:
                stretches += 1
            if run > longest:
                longest = run
        else:
            run = 0
    return clean, held, sum(covered), longest, stretches


def records(counters, lengths, k, min_count=1, max_count=255, floor=2):
    """one tuple of FIELDS per sequence, from `window_counters`' answer"""
    m = threshold(min_count, floor)
    return [record(c, n, k, m, max_count) for c, n in zip(counters, lengths)]


def evidence(db, sequences, k, min_count=1, max_count=255, floor=2):
    """one tuple of FIELDS per sequence of the batch: the rule as the header has it"""
    return records(window_counters(db, sequences, k), [len(s) for s in sequences], k, min_count, max_count, floor)


def as_array(recs):
    out = np.zeros(len(recs), dtype=READ_EVIDENCE)
    for i, rec in enumerate(recs):
        for name, value in zip(FIELDS, rec):
            out[i][name] = value
    return out


def first_difference(got, want):
    if got.size != want.size:
        return "{} records, not {}".format(got.size, want.size)
    for i in range(got.size):
        if got[i].tobytes() != want[i].tobytes():
            return "record {}: {} != {}".format(i, got[i], want[i])
    return None


# ---- screen_reads' rule and its two tables ----------------------------------------------------------------------------------------
def bin_of(rec, length, min_hits=1, min_share="0", min_covered="0", min_stretch=0):
    """'U', 'A' or 'B' for one record (a tuple of FIELDS) of a read of `length` bases; the shares are decimal strings, compared as
    exact rationals"""
    clean, held, covered, longest, _ = rec
    if clean == 0:
        return "U"
    matched = (held >= min_hits and Fraction(held, clean) >= Fraction(min_share) and Fraction(covered, length) >= Fraction(min_covered)
               and longest >= min_stretch)
    return "A" if matched else "B"


def table(names, sequences, recs, bins):
    """the --table file: name length clean held covered longest stretches bin"""
    return "".join("\t".join([name, str(len(s))] + [str(v) for v in rec] + [BINS[b]]) + "\n" for name, s, rec, b in zip(names, sequences, recs, bins))


def summary(sequences, bins, m, max_count, min_hits=1, min_share="0", min_covered="0", min_stretch=0):
    """stdout: reads and bases per bin, then the rule with the lower bound in force and the shares as given"""
    lines = []
    for code in "ABU":
        mine = [s for s, b in zip(sequences, bins) if b == code]
        lines.append("#{}\t{}\t{}".format(BINS[code], len(mine), sum(len(s) for s in mine)))
    lines.append("\t".join(["#rule", str(m), str(max_count), str(min_hits), min_share, min_covered, str(min_stretch)]))
    return "".join(line + "\n" for line in lines)
