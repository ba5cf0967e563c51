"""The reference of the repair candidates' tests (include/tbk.h, "repair candidates"), written twice in plain Python on top of
db_query_ref.  `repairs` is the rule as the header states it: a loop over stretches and candidates, left-aligned, with the
windows of the edited sequence from the min/max formulas.  `repairs_brute` is independent of both: it tries every one-base edit
at the positions of P and the gaps of Q, decides which edits are the same by comparing the edited strings, keeps the smallest
position of each group and finds the windows to verify by asking each window of the edited string whether it holds the edited
index.  tests/test_host_repair_ref.py holds the two to each other.  Nothing here touches a device."""
import numpy as np

import db_query_ref as ref

NONE, SUB, DEL, INS, LONG = 0, 1, 2, 3, 4

# tbk_repair (40 bytes)
REPAIR = np.dtype([("read", "<u8"), ("first", "<u8"), ("pos", "<u8"), ("windows", "<u4"), ("accepted", "<u2"), ("kind", "u1"), ("base", "u1"),
                   ("support", "u1"), ("depth", "u1"), ("pad", "u1", (6,))])
assert REPAIR.itemsize == 40
FIELDS = ("read", "first", "pos", "windows", "accepted", "kind", "base", "support", "depth")


def threshold(min_count, floor=2):
    return max(floor, min_count)


def stretches(db, sequence, k, m):
    """[(f, l)] of the maximal runs of broken window starts - clean, counter below m - of one sequence"""
    out, start = [], None
    windows = ref.window_kmers(sequence, k)
    for w, km in enumerate(windows):
        if km is not None and db.get(km, 0) < m:
            if start is None:
                start = w
        elif start is not None:
            out.append((start, w - 1))
            start = None
    if start is not None:
        out.append((start, len(windows) - 1))
    return out


_RC = str.maketrans("ACGT", "TGCA")
_ACGT = frozenset("ACGT")


def _verdict(db, edited, starts, k, m):
    """(support, depth, every clean window has c >= m) of the windows of `edited` that start at `starts`"""
    support, depth, rejected = 0, 255, False
    for j in starts:
        window = edited[j:j + k]
        assert len(window) == k
        if not _ACGT.issuperset(window):
            continue
        c = db.get(min(window, window.translate(_RC)[::-1]), 0)  # (ref.canonical, without its loop)
        support += 1
        depth = min(depth, c)
        rejected = rejected or c < m
    return support, depth, not rejected


def candidates(s, f, l, k):
    """the candidates of stretch [f, l] of the upper-case sequence s in the order of (kind, pos, base): (kind, pos, base, edited
    sequence, window starts that count)"""
    L, lo, hi = len(s), l, f + k - 1
    for p in range(lo, hi + 1):
        for b in "ACGT":
            if b != s[p]:
                yield SUB, p, b, s[:p] + b + s[p + 1:], range(max(0, p - k + 1), min(p, L - k) + 1)
    for p in range(lo, hi + 1):
        if p - 1 >= lo and s[p - 1] == s[p]:
            continue
        yield DEL, p, "", s[:p] + s[p + 1:], range(max(0, p - k + 1), min(p - 1, L - 1 - k) + 1)
    for q in range(lo + 1, hi + 1):
        for b in "ACGT":
            if q - 1 >= lo + 1 and s[q - 1] == b:
                continue
            yield INS, q, b, s[:q] + b + s[q:], range(max(0, q - k + 1), min(q, L + 1 - k) + 1)


def _record(read, f, l, k, accepted):
    """accepted: [(kind, pos, base, support, depth)]"""
    r = l - f + 1
    if r > k:
        return (read, f, 0, r, 0, LONG, 0, 0, 0)
    if not accepted:
        return (read, f, 0, r, 0, NONE, 0, 0, 0)
    kind, pos, base, support, depth = min(accepted)
    return (read, f, pos, r, len(accepted), kind, ord(base) if base else 0, support, depth)


def evaluate(db, sequences, k, min_count=2, floor=2):
    """what does not depend on min_support, computed once: [(read, f, l, [(kind, pos, base, support, depth, whole)])] per stretch,
    `whole` when every clean window of the candidate has c >= m; no candidates for a long stretch"""
    m, out = threshold(min_count, floor), []
    for read, sequence in enumerate(sequences):
        s = sequence.upper()
        for f, l in stretches(db, s, k, m):
            tried = []
            if l - f + 1 <= k:
                tried = [(kind, pos, base) + _verdict(db, edited, starts, k, m) for kind, pos, base, edited, starts in candidates(s, f, l, k)]
            out.append((read, f, l, tried))
    return out


def records(evaluated, k, min_support=1):
    """one tuple of FIELDS per stretch of `evaluate`'s answer"""
    return [_record(read, f, l, k, [c[:5] for c in tried if c[5] and c[3] >= min_support]) for read, f, l, tried in evaluated]


def repairs(db, sequences, k, min_count=2, min_support=1, floor=2):
    """(A) one tuple of FIELDS per stretch of the batch, ordered by (read, first): the rule as the header has it"""
    return records(evaluate(db, sequences, k, min_count, floor), k, min_support)


def repairs_brute(db, sequences, k, min_count=2, min_support=1, floor=2):
    """(B) the same answer by brute force: every edit, grouped by the edited string, windows by a membership test"""
    m, out = threshold(min_count, floor), []
    for read, sequence in enumerate(sequences):
        s = sequence.upper()
        for f, l in stretches(db, s, k, m):
            accepted = []
            if l - f + 1 <= k:
                groups = {}  # (kind, edited string) -> (smallest pos, base)
                shared = [p for p in range(len(s)) if all(w <= p < w + k for w in range(f, l + 1))]          # P
                gaps = [q for q in range(1, len(s) + 1) if all(w < q < w + k for w in range(f, l + 1))]      # Q: gap q in front of base q
                assert shared == list(range(l, f + k)) and gaps == list(range(l + 1, f + k))
                for p in shared:
                    for b in "ACGT":
                        if b != s[p]:
                            groups.setdefault((SUB, s[:p] + b + s[p + 1:]), (p, b))
                    groups.setdefault((DEL, s[:p] + s[p + 1:]), (p, ""))
                for q in gaps:
                    for b in "ACGT":
                        groups.setdefault((INS, s[:q] + b + s[q:]), (q, b))
                for (kind, edited), (pos, base) in groups.items():
                    need = (pos - 1, pos) if kind == DEL else (pos,)
                    starts = [j for j in range(len(edited) - k + 1) if all(j <= i < j + k for i in need)]
                    support, depth, whole = _verdict(db, edited, starts, k, m)
                    if whole and support >= min_support:
                        accepted.append((kind, pos, base, support, depth))
            out.append(_record(read, f, l, k, accepted))
    return out


def as_array(records):
    out = np.zeros(len(records), dtype=REPAIR)
    for i, rec in enumerate(records):
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


def apply_edits(sequence, edits):
    """the sequence (a str) with (kind, pos, base) edits applied, none of them overlapping: a plain loop from the right"""
    s = sequence
    for kind, pos, base in sorted(edits, key=lambda e: e[1], reverse=True):
        if kind == SUB:
            s = s[:pos] + base + s[pos + 1:]
        elif kind == DEL:
            s = s[:pos] + s[pos + 1:]
        else:
            s = s[:pos] + base + s[pos:]
    return s
