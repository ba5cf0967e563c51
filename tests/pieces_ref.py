"""The reference of the read pieces' tests (include/tbk.h, "read pieces"), of the writer's text of a piece and of trim_reads'
tables, in plain Python on top of screen_ref.window_counters: a loop over the windows of a sequence that marks the k bases of
every held window in a list of booleans, and a walk along the list for the runs that are - or are not - marked.  No bit tricks.
tests/test_host_pieces_ref.py holds it to hand-worked cases and to screen_ref.record.  Nothing here touches a device."""
import numpy as np

import screen_ref as sr

# tbk_read_piece (24 bytes)
READ_PIECE = np.dtype([("read", "<u8"), ("first", "<u8"), ("end", "<u8")])
assert READ_PIECE.itemsize == 24
BINS = {"A": "kept", "B": "dropped", "U": "unjudged"}


def covered_mask(counters, length, k, m, max_count):
    """one boolean per base: does a held window - clean, with m <= c <= max_count - hold it?"""
    covered = [False] * length
    for w, c in enumerate(counters):
        if c is not None and m <= c <= max_count:
            for p in range(w, w + k):
                covered[p] = True
    return covered


def runs(mask, on):
    """the maximal runs [first, end) of positions p with mask[p] == on, in order"""
    out, first = [], None
    for p, value in enumerate(mask):
        if value == on:
            if first is None:
                first = p
        elif first is not None:
            out.append((first, p))
            first = None
    if first is not None:
        out.append((first, len(mask)))
    return out


def select(found, which="all", min_length=1):
    """`found` without the runs shorter than min_length; with which == "longest" only the longest of the rest, the first among equals"""
    found = [(f, e) for f, e in found if e - f >= min_length]
    if which == "longest" and found:
        best = found[0]
        for f, e in found[1:]:
            if e - f > best[1] - best[0]:
                best = (f, e)
        found = [best]
    return found


def sequence_pieces(counters, length, k, m, max_count, side="covered", which="all", min_length=1):
    """the pieces [first, end) of one sequence of `length` bases from its windows' counters"""
    return select(runs(covered_mask(counters, length, k, m, max_count), side == "covered"), which, min_length)


def pieces_from(counters, lengths, k, min_count=1, max_count=255, side="covered", which="all", min_length=1, floor=2):
    """(read, first, end) of every piece of the batch, ordered by (read, first), from `screen_ref.window_counters`' answer"""
    m = sr.threshold(min_count, floor)
    return [(r, f, e) for r, (c, n) in enumerate(zip(counters, lengths)) for f, e in sequence_pieces(c, n, k, m, max_count, side, which, min_length)]


def pieces(db, sequences, k, min_count=1, max_count=255, side="covered", which="all", min_length=1, floor=2):
    """the rule as the header has it"""
    return pieces_from(sr.window_counters(db, sequences, k), [len(s) for s in sequences], k, min_count, max_count, side, which, min_length, floor)


def as_array(recs):
    out = np.zeros(len(recs), dtype=READ_PIECE)
    for i, (read, first, end) in enumerate(recs):
        out[i] = (read, first, end)
    return out


def first_difference(got, want):
    if got.size != want.size:
        return "{} pieces, not {}".format(got.size, want.size)
    for i in range(got.size):
        if got[i].tobytes() != want[i].tobytes():
            return "piece {}: {} != {}".format(i, got[i], want[i])
    return None


# ---- the text of a record and of a piece ------------------------------------------------------------------------------------------
def record_text(header, sequence, quality):
    """what the bin writer writes for a whole record: FASTQ when it has a non-empty quality string, else FASTA; the name is the
    header up to the first space"""
    name = header.split(" ")[0]
    if quality:
        return "@{}\n{}\n+\n{}\n".format(name, sequence, quality)
    return ">{}\n{}\n".format(name, sequence)


def piece_name(header, length, first, end, suffix):
    name = header.split(" ")[0]
    if suffix and (first, end) != (0, length):
        name += ":{}-{}".format(first + 1, end)  # 1-based and closed
    return name


def piece_text(header, sequence, quality, first, end, suffix):
    """the record cut to [first, end): sequence and quality both, renamed name:F-E when `suffix` and the piece is not the whole record"""
    return record_text(piece_name(header, len(sequence), first, end, suffix), sequence[first:end], quality[first:end] if quality else quality)


def bins_text(records, found, bins, suffix):
    """the text of the three bins for `records` - (header, sequence, quality) - their pieces (read, first, end) and one letter per
    record: an 'A' record's pieces to the first, a 'B' record whole to the second, any other whole to the third"""
    out = {"A": [], "B": [], "U": []}
    for i, ((header, sequence, quality), code) in enumerate(zip(records, bins)):
        if code == "A":
            out["A"] += [piece_text(header, sequence, quality, f, e, suffix) for r, f, e in found if r == i]
        else:
            out["B" if code == "B" else "U"].append(record_text(header, sequence, quality))
    return tuple("".join(out[code]) for code in "ABU")


# ---- trim_reads: bins, tables, summary --------------------------------------------------------------------------------------------
def trim(db, records, k, min_count=1, max_count=255, keep="covered", which="longest", min_length=1, floor=2):
    """trim_reads in one function: (pieces, evidence records, one bin letter per read).  A read without a clean window is 'U' on
    either side, a read with a clean window and a piece is 'A', the rest is 'B'."""
    sequences = [s for _, s, _ in records]
    evidence = sr.evidence(db, sequences, k, min_count, max_count, floor)
    found = pieces(db, sequences, k, min_count, max_count, keep, which, min_length, floor)
    has = {r for r, _, _ in found}
    bins = "".join("U" if rec[0] == 0 else "A" if i in has else "B" for i, rec in enumerate(evidence))
    found = [(r, f, e) for r, f, e in found if bins[r] == "A"]
    return found, evidence, bins


def table(records, found, evidence, bins):
    """the --table file: name length clean held covered pieces kept_bases bin"""
    lines = []
    for i, ((header, sequence, _), rec, code) in enumerate(zip(records, evidence, bins)):
        mine = [(f, e) for r, f, e in found if r == i and code == "A"]
        lines.append("\t".join([header.split(" ")[0], str(len(sequence)), str(rec[0]), str(rec[1]), str(rec[2]), str(len(mine)),
                                str(sum(e - f for f, e in mine)), BINS[code]]) + "\n")
    return "".join(lines)


def bed(records, found):
    """the --bed file: name first end of every kept piece"""
    return "".join("{}\t{}\t{}\n".format(records[r][0].split(" ")[0], f, e) for r, f, e in found)


def summary(records, found, bins, m, max_count, keep, which, min_length):
    """stdout: reads, pieces and bases kept; reads and bases dropped and unjudged; the bases cut off kept reads; the rule"""
    lengths = [len(s) for _, s, _ in records]
    kept_bases = sum(e - f for _, f, e in found)
    lines = ["#kept\t{}\t{}\t{}".format(bins.count("A"), len(found), kept_bases)]
    for code in "BU":
        lines.append("#{}\t{}\t{}".format(BINS[code], bins.count(code), sum(n for n, b in zip(lengths, bins) if b == code)))
    lines.append("#cut\t{}".format(sum(n for n, b in zip(lengths, bins) if b == "A") - kept_bases))
    lines.append("\t".join(["#rule", str(m), str(max_count), keep, which, str(min_length)]))
    return "".join(line + "\n" for line in lines)
