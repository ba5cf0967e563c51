"""K-mer multiplicity against GC content of one k-mer count database.

    python -m trio_binning_amd.gc_spectrum lib.tbkdb [--min-count N --max-count N] [--matrix gc.tsv]

How many distinct k-mers of lib.tbkdb have g G-or-C bases and counter c (``tbk_kmerdb_gc_spectrum``): the matrix ``kat gcp``
plots.  A contaminant - bacterial, organellar - is a second cloud at another GC and another depth; a library that under-covers
AT-rich or GC-rich sequence shows in the rows of those GC values, whose mode and mean fall below the others'.  A cloud that
is seen can be carved out as a database with ``select_database --min-gc N --max-gc N --min-count N --max-count N``.

stdout is a TSV: a header line, then one line per GC value 0..k with the columns

    gc  kmers  share  occurrences  mode  mean

over the counters --min-count..--max-count (default: the file's floor..255, so a file kept without its once-seen k-mers starts
at 2).  kmers: the distinct k-mers of that GC with a counter in the range; share: that row's part of all k-mers in the range;
occurrences: the sum of counter x k-mers - a LOWER BOUND, since a counter saturates at 255; mode: the counter most k-mers of
the row have, the lowest on a tie; mean: occurrences / kmers.  An empty row has ``-`` for mode and mean.  A last line
``#total`` has the same columns over all rows.  GC is counted in bases, not per cent; in a homopolymer-compressed database it
is the GC of the compressed k-mers.  --matrix writes the whole matrix, whatever the range: ``#`` lines that name the file, k,
floor and space, then row g as 256 tab-separated columns.  stderr says what the file is.  No verdict is computed: no threshold
has been measured on a real library.  The header is checked before a device is touched.
"""
import argparse
import os
import sys
from os.path import isfile

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

import numpy as np  # noqa: E402

from . import find_unique_kmers as fu  # noqa: E402
from . import kmers  # noqa: E402

PROG = "gc_spectrum"
COLUMNS = ("gc", "kmers", "share", "occurrences", "mode", "mean")
SPACES = {False: "plain", True: "homopolymer-compressed"}


# ---- from the matrix to the report's lines: a pure function ------------------------------------------------------------------------
def _row(name, cells, lo: int, total: int) -> str:
    """``cells``: the k-mers by counter lo, lo + 1, ... of one row (or of all rows together)"""
    n = int(cells.sum())
    occurrences = sum(int(v) * (lo + j) for j, v in enumerate(cells))  # (Python integers: nothing wraps)
    share = "{:.6f}".format(n / total) if total else "nan"
    if not n:
        return "{}\t0\t{}\t0\t-\t-".format(name, share)
    return "{}\t{}\t{}\t{}\t{}\t{:.6f}".format(name, n, share, occurrences, lo + int(np.argmax(cells)), occurrences / n)


def summary(spec, count_range) -> list:
    """The TSV lines of a (k + 1) x 256 matrix over the counters ``count_range`` (inclusive): the header, a line per row, ``#total``."""
    spec = np.asarray(spec, dtype=np.uint64)
    lo, hi = count_range
    part = spec[:, lo:hi + 1]
    total = int(part.sum())
    lines = ["\t".join(COLUMNS)]
    lines += [_row(g, part[g], lo, total) for g in range(spec.shape[0])]
    lines.append(_row("#total", part.sum(axis=0), lo, total))
    return lines


# ---- the matrix as a file ---------------------------------------------------------------------------------------------------------
def _replace(path: str, write) -> None:
    """``write(fh)`` into path + ".tmp", renamed over path once it is whole."""
    tmp = path + ".tmp"
    try:
        with open(tmp, "w") as fh:
            write(fh)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


def write_matrix(path: str, spec, name: str, k: int, floor: int, compressed: bool) -> None:
    """``#`` lines that name the file, k, floor and space, then row g of the matrix (g G-or-C bases): 256 tab-separated columns,
    column c the k-mers with counter c."""
    spec = np.asarray(spec, dtype=np.uint64).reshape(k + 1, 256)

    def write(fh):
        fh.write("# GC x count matrix: line 1 + g below these comments is row g (G-or-C bases of the k-mer, 0..{}), its 256 columns "
                 "are the counter; column 0 is 0\n".format(k))
        fh.write("# file = {}\n".format(name))
        fh.write("# k = {}; floor = {}; space = {}\n".format(k, floor, SPACES[bool(compressed)]))
        for row in spec:
            fh.write("\t".join(str(int(v)) for v in row) + "\n")
    _replace(path, write)


def read_matrix(path: str) -> np.ndarray:
    """The (k + 1) x 256 matrix ``write_matrix`` wrote."""
    rows = [line.rstrip("\n").split("\t") for line in open(path) if not line.startswith("#")]
    if not 2 <= len(rows) <= 33 or any(len(row) != 256 or not all(f.isdigit() for f in row) for row in rows):
        raise ValueError("{}: {} rows, not 2 to 33 rows (k + 1) of 256 counts".format(path, len(rows)))
    return np.array(rows, dtype=np.uint64)


# ---- the command ------------------------------------------------------------------------------------------------------------------
def _parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog=PROG, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("database", metavar="lib.tbkdb", help="the count database to look into")
    parser.add_argument("--min-count", type=int, default=None, metavar="N", help="lowest counter the summary lines cover (default: the file's floor)")
    parser.add_argument("--max-count", type=int, default=None, metavar="N", help="highest counter the summary lines cover (default 255)")
    parser.add_argument("--matrix", default=None, metavar="gc.tsv", help="write the whole (k + 1) x 256 matrix here")
    return parser


def parse_args(argv=None):
    """The arguments, with every refusal the command line and the file's header decide; no device is touched.  ``args.info`` is
    the header, ``args.range`` the settled counter range."""
    parser = _parser()
    args = parser.parse_args(argv)
    if not fu.is_database_path(args.database):
        parser.error("{} is not a count database (*{})".format(args.database, fu.DATABASE_SUFFIX))
    for name, value in (("--min-count", args.min_count), ("--max-count", args.max_count)):
        if value is not None and not 1 <= value <= 255:
            parser.error("{} {}: a counter is 1..255".format(name, value))
    if args.matrix is not None and os.path.abspath(args.matrix) == os.path.abspath(args.database):
        parser.error("--matrix {} names the input: the matrix goes to a file of its own".format(args.matrix))
    if not isfile(args.database):
        sys.exit("{}: {} does not exist or is not a file".format(PROG, args.database))
    try:
        args.info = kmers.database_file_info(args.database)
    except (IOError, ValueError) as exc:
        sys.exit("{}: {}: {}".format(PROG, args.database, exc))
    lo = args.info["floor"] if args.min_count is None else args.min_count
    hi = 255 if args.max_count is None else args.max_count
    if lo > hi:
        parser.error("--min-count {} --max-count {}: need 1 <= min <= max <= 255".format(lo, hi))
    args.range = (lo, hi)
    return args


def main(argv=None):
    args = parse_args(argv)
    info = args.info
    with kmers.KmerDatabase.load(args.database) as db:
        spec = db.gc_spectrum()
    print("\n".join(summary(spec, args.range)))
    if args.matrix is not None:
        write_matrix(args.matrix, spec, args.database, info["k"], info["floor"], info["compressed"])
    print("{}: {}: {} {} {}-mers, floor {}; counters {}..{}. No verdict is computed".format(
        PROG, args.database, info["n"], SPACES[bool(info["compressed"])], info["k"], info["floor"], args.range[0], args.range[1]), file=sys.stderr)


if __name__ == "__main__":
    main()
