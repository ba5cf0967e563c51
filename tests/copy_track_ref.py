"""The reference of the copy-number track's tests (tbk_kmerdb_query_track, include/tbk.h "copy-number track"), written
twice: a plain Python loop over windows and bins on top of db_query_ref.Tally, and the same with numpy on top of
db_query_ref.TallyNp for batches the loop cannot follow.  tests/test_host_copy_track.py holds the two to each other and to a
hand-worked case.  Nothing here touches a device, and neither function changes the tally it reads."""
import numpy as np

import db_query_ref as ref

FIELDS = ("clean", "absent", "saturated", "collapsed", "expanded", "depth", "copies")
BIN = np.dtype([("clean", "<u4"), ("absent", "<u4"), ("saturated", "<u4"), ("collapsed", "<u4"), ("expanded", "<u4"),
                ("depth", "u1"), ("copies", "u1"), ("pad", "u1", (2,))])


def lower_median(values):
    """v[(m - 1) / 2] of the m sorted values; 0 of none"""
    v = sorted(values)
    return v[(len(v) - 1) // 2] if v else 0


def verdicts(c, a, peak):
    """(collapsed, expanded) of one present window: Python's integers cannot wrap"""
    if c == 255:
        return False, False
    return 2 * c > (2 * a + 1) * peak, a >= 1 and 2 * c < (2 * a - 1) * peak


def track(tally, sequences, k, window, peak):
    """[one list of bins per sequence], a bin a dict of FIELDS: the loop.  tally: a db_query_ref.Tally, whose copies are read as they are."""
    assert window >= 1 and peak >= 1
    out = []
    for s in sequences:
        windows = ref.window_kmers(s, k)  # (empty for a sequence shorter than k)
        bins = []
        for start in range(0, len(windows), window):
            clean = absent = saturated = collapsed = expanded = 0
            cs, copies = [], []
            for km in windows[start:start + window]:
                if km is None:
                    continue
                clean += 1
                c = tally.db.get(km, 0)
                if c == 0:
                    absent += 1
                    continue
                a = tally.copies.get(km, 0)
                cs.append(c)
                copies.append(min(a, 255))
                saturated += c == 255
                col, exp = verdicts(c, a, peak)
                collapsed += col
                expanded += exp
            bins.append({"clean": clean, "absent": absent, "saturated": saturated, "collapsed": collapsed, "expanded": expanded,
                         "depth": lower_median(cs), "copies": lower_median(copies)})
        out.append(bins)
    return out


def as_array(per_sequence):
    """(BIN array, uint64 prefix) of track()'s lists: what DatabaseQuery.track returns"""
    flat = [b for bins in per_sequence for b in bins]
    arr = np.zeros(len(flat), dtype=BIN)
    for f in FIELDS:
        arr[f] = [b[f] for b in flat]
    prefix = np.zeros(len(per_sequence) + 1, dtype=np.uint64)
    np.cumsum([len(bins) for bins in per_sequence], out=prefix[1:])
    return arr, prefix


def track_np(tally, bases, offsets, k, window, peak):
    """(BIN array, uint64 prefix) with numpy.  tally: a db_query_ref.TallyNp, whose copies are read as they are."""
    assert window >= 1 and peak >= 1
    off = np.asarray(offsets).astype(np.int64)
    n = off.size - 1
    rank, clean = ref.window_ranks(bases, offsets, k)
    c = np.zeros(rank.size, dtype=np.int64)
    a = np.zeros(rank.size, dtype=np.int64)
    if tally.ranks.size:
        at = np.minimum(np.searchsorted(tally.ranks, rank), tally.ranks.size - 1)
        hit = clean & (tally.ranks[at] == rank)
        c[hit] = tally.counters[at[hit]]
        a[hit] = tally.copies[at[hit]].astype(np.int64)  # (a < 2^32: the products below stay far inside int64 for peak < 2^29)
    assert peak < 1 << 29
    present = c > 0
    judged = present & (c < 255)
    collapsed = judged & (2 * c > (2 * a + 1) * peak)
    expanded = judged & (a >= 1) & (2 * c < (2 * a - 1) * peak)
    starts = np.maximum(np.diff(off) - k + 1, 0)
    prefix = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum((starts + window - 1) // window, out=prefix[1:])
    bins = np.zeros(int(prefix[-1]), dtype=BIN)
    # [lo, hi) of every bin in the batch's own coordinates: window w of sequence r is base off[r] + w
    lo = np.concatenate([np.arange(off[r], off[r] + starts[r], window) for r in range(n)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    end = np.repeat(off[:-1] + starts, np.diff(prefix.astype(np.int64)))
    hi = np.minimum(lo + window, end)
    assert lo.size == bins.size and (hi > lo).all()

    def per_bin(flags):
        before = np.concatenate([[0], np.cumsum(flags)])
        return before[hi] - before[lo]

    bins["clean"] = per_bin(clean)
    bins["absent"] = per_bin(clean & ~present)
    bins["saturated"] = per_bin(c == 255)
    bins["collapsed"] = per_bin(collapsed)
    bins["expanded"] = per_bin(expanded)
    capped = np.minimum(a, 255)
    for g in np.flatnonzero(per_bin(present)):
        here = present[lo[g]:hi[g]]
        m = int(here.sum())
        bins[g]["depth"] = np.sort(c[lo[g]:hi[g]][here])[(m - 1) // 2]
        bins[g]["copies"] = np.sort(capped[lo[g]:hi[g]][here])[(m - 1) // 2]
    return bins, prefix


def equal(got, want):
    """every field of every bin, pad included"""
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def first_difference(got, want):
    """for an assertion's message"""
    if got.shape != want.shape:
        return "shapes {} and {}".format(got.shape, want.shape)
    for i in range(got.size):
        if got[i].tobytes() != want[i].tobytes():
            return "bin {}: got {}, want {}".format(i, got[i], want[i])
    return None


# ---- what the command writes, formatted from bins ------------------------------------------------------------------------------
def command_tables(names, lengths, per_sequence, window, peak):
    """(stdout, --track file) of copy_track for sequences whose bins track() gave"""
    summed = ("clean", "absent", "saturated", "collapsed", "expanded")
    out, lines, total = [], [], [0] * 6
    for name, length, bins in zip(names, lengths, per_sequence):
        sums = [sum(b[f] for b in bins) for f in summed]
        out.append("\t".join([name, str(length)] + [str(x) for x in sums]) + "\n")
        total = [total[0] + length] + [t + x for t, x in zip(total[1:], sums)]
        for i, b in enumerate(bins):
            end = length if i == len(bins) - 1 else (i + 1) * window
            lines.append("\t".join(str(x) for x in (name, i * window, end, b["clean"], b["absent"], b["saturated"], b["depth"], b["copies"],
                                                     b["collapsed"], b["expanded"])) + "\n")
    out.append("\t".join(["#total"] + [str(x) for x in total] + [str(peak), str(window)]) + "\n")
    return "".join(out), "".join(lines)
