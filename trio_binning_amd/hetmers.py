"""Het-mer pairs of a k-mer count database: the k-mers that differ from exactly one other in their middle base alone.

    python -m trio_binning_amd.hetmers child.tbkdb [--min-count N --max-count N] [--matrix het.tsv] [--pairs pairs.tsv] \\
        [--parent-a A.tbkdb --parent-b B.tbkdb [--min-count-a N --max-count-a N --min-count-b N --max-count-b N]]

A heterozygous SNP leaves, among the windows over it, one with the SNP in the middle: two k-mers that differ in their middle
base only, whose two counters are the coverage of the two alleles.  This command finds those pairs inside one database
(``tbk_kmerdb_hetmers``; include/tbk.h has the exact definitions): among the k-mers with a counter in
[--min-count, --max-count] - left out, the two cut-offs find-unique-kmers would choose from the file's histogram - those with
exactly one middle partner in that range.  It is the k-mer-pair look of Smudgeplot / PloidyPlot at a library before any
assembly: how heterozygous is it, and does it look diploid (k-mers with two or three partners are what a polyploid or a
repeat-rich library adds).  k must be odd.  The file is loaded as it is, a full one (--keep-singletons) included.

With both parents' databases every pair is also split by who holds its members, each parent asked at the cut-offs
classify-by-kmers would use for it (or --min-count-a ... --max-count-b), full files in their solid form: a pair with one member
only parent A holds and the other only parent B holds is a heterozygous site the hap-mers will phase.

--matrix writes ``minor<TAB>major<TAB>pairs`` for every non-empty cell of the pair spectrum, --pairs one line per pair,
``KMER<TAB>COUNT<TAB>KMER<TAB>COUNT``, minor first (lower counter; on a tie the lower k-mer), with the two members' classes
(neither, a_only, b_only, both) behind them when the parents are given.  stdout is ``name<TAB>value`` lines (INTEGRATION.md
lists them).  No verdict and no ploidy is computed: no threshold has been measured on a real library.  Headers are checked
before a device is touched.
"""
import argparse
import os
import sys
from types import SimpleNamespace

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

import numpy as np  # noqa: E402

from . import classify_by_kmers as cbk  # noqa: E402
from . import find_unique_kmers as fu  # noqa: E402
from . import kmers  # noqa: E402

PROG = "hetmers"
CLASSES = ("neither", "a_only", "b_only", "both")  # an origin class 0..3: bit 0 parent A holds the k-mer, bit 1 parent B does
_PARENT_CUTOFFS = ("min_count_a", "max_count_a", "min_count_b", "max_count_b")


# ---- from the tallies to the report's lines: pure functions ---------------------------------------------------------------------
def _ratio(num: int, den: int) -> str:
    return "{:.6f}".format(num / den) if den else "nan"


def report(result: dict, k: int, compressed: bool, count_range, parent_ranges=None) -> list:
    """The ``name<TAB>value`` lines of a result of ``KmerDatabase.hetmers``; ``parent_ranges``: (range of A, range of B) when the
    parents were asked, which adds the origin table and its three shares."""
    partners = [int(v) for v in result["partners"]]
    pairs, candidates = int(result["pairs"]), int(result["candidates"])
    lines = [("k", k), ("space", "compressed" if compressed else "plain"), ("range", "{},{}".format(*count_range)), ("candidates", candidates)]
    lines += [("candidates_with_{}_partners".format(j), partners[j]) for j in range(4)]
    lines += [("pairs", pairs), ("candidates_in_pairs_share", _ratio(2 * pairs, candidates))]
    if parent_ranges is not None:
        origin = np.asarray(result["origin"], dtype=np.uint64).reshape(4, 4)
        lines += [("range_a", "{},{}".format(*parent_ranges[0])), ("range_b", "{},{}".format(*parent_ranges[1]))]
        lines += [("pairs_minor_{}_major_{}".format(CLASSES[i], CLASSES[j]), int(origin[i, j])) for i in range(4) for j in range(4)]
        split = int(origin[1, 2]) + int(origin[2, 1])
        inside = int(origin[1, 1]) + int(origin[2, 2])
        orphan = int(origin[0, :].sum()) + int(origin[:, 0].sum()) - int(origin[0, 0])
        lines += [("pairs_split_between_parents", split), ("pairs_split_between_parents_share", _ratio(split, pairs)),
                  ("pairs_inside_one_parent", inside), ("pairs_inside_one_parent_share", _ratio(inside, pairs)),
                  ("pairs_with_a_member_in_neither", orphan), ("pairs_with_a_member_in_neither_share", _ratio(orphan, pairs))]
    return ["{}\t{}".format(name, value) for name, value in lines]


# ---- the tables as files ----------------------------------------------------------------------------------------------------------
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


def write_matrix(path: str, spec, k: int, count_range, name: str) -> None:
    """One ``#`` line with k, the range and the file, then ``minor<TAB>major<TAB>pairs`` for every non-empty cell, by row."""
    spec = np.asarray(spec, dtype=np.uint64).reshape(256, 256)

    def write(fh):
        fh.write("# het-mer pair spectrum: k = {}; range = {},{}; file = {}; columns: minor counter, major counter, pairs\n".format(
            k, count_range[0], count_range[1], name))
        for i, j in zip(*np.nonzero(spec)):
            fh.write("{}\t{}\t{}\n".format(int(i), int(j), int(spec[i, j])))
    _replace(path, write)


def read_matrix(path: str) -> np.ndarray:
    """The 256 x 256 matrix ``write_matrix`` wrote."""
    spec = np.zeros((256, 256), dtype=np.uint64)
    for number, line in enumerate(open(path), 1):
        if line.startswith("#"):
            continue
        fields = line.rstrip("\n").split("\t")
        if len(fields) != 3 or not all(f.isdigit() for f in fields) or int(fields[0]) > 255 or int(fields[1]) > 255:
            raise ValueError("{}: line {} is not minor<TAB>major<TAB>pairs with counters up to 255".format(path, number))
        spec[int(fields[0]), int(fields[1])] += np.uint64(int(fields[2]))
    return spec


def kmers_of_ranks(ranks, k: int) -> list:
    """The k-mers of lexicographic ranks (base 0 in the top bits), as strings."""
    ranks = np.asarray(ranks, dtype=np.uint64)
    shifts = np.arange(2 * (k - 1), -2, -2, dtype=np.uint64)
    codes = ((ranks[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    return [row.tobytes().decode("ascii") for row in letters]


def write_pairs(path: str, records, k: int, with_classes: bool) -> None:
    """``KMER<TAB>COUNT<TAB>KMER<TAB>COUNT`` per record of ``KmerDatabase.hetmers(pairs=True)``, minor first, in the records'
    order; ``with_classes``: the minor's and the major's class behind them, in words."""
    minor, major = kmers_of_ranks(records["minor"], k), kmers_of_ranks(records["major"], k)

    def write(fh):
        for i in range(len(minor)):
            fields = [minor[i], str(int(records["c_minor"][i])), major[i], str(int(records["c_major"][i]))]
            if with_classes:
                fields += [CLASSES[int(records["cls_minor"][i])], CLASSES[int(records["cls_major"][i])]]
            fh.write("\t".join(fields) + "\n")
    _replace(path, write)


def read_pairs(path: str) -> list:
    """[(minor k-mer, its counter, major k-mer, its counter)] of the file ``write_pairs`` wrote, with the two class words
    behind them where the file has them."""
    out = []
    for number, line in enumerate(open(path), 1):
        fields = line.rstrip("\n").split("\t")
        if len(fields) not in (4, 6) or not fields[1].isdigit() or not fields[3].isdigit() or (len(fields) == 6 and not set(fields[4:]) <= set(CLASSES)):
            raise ValueError("{}: line {} is not KMER<TAB>COUNT<TAB>KMER<TAB>COUNT[<TAB>class<TAB>class]".format(path, number))
        out.append((fields[0], int(fields[1]), fields[2], int(fields[3])) + tuple(fields[4:]))
    return out


# ---- the command ------------------------------------------------------------------------------------------------------------------
def _parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog=PROG, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("database", metavar="child.tbkdb", help="the count database to look inside (odd k)")
    parser.add_argument("--min-count", type=int, default=None, metavar="N",
                        help="lowest counter of a candidate (give both, or neither: then the cut-offs find-unique-kmers would choose)")
    parser.add_argument("--max-count", type=int, default=None, metavar="N", help="highest counter of a candidate")
    parser.add_argument("--matrix", default=None, metavar="het.tsv", help="write the pair spectrum here: minor, major, pairs per non-empty cell")
    parser.add_argument("--pairs", default=None, metavar="pairs.tsv", help="write the pairs here: KMER, COUNT, KMER, COUNT, minor first")
    parser.add_argument("--parent-a", default=None, metavar="A.tbkdb", help="parent A's count database (give both parents or neither)")
    parser.add_argument("--parent-b", default=None, metavar="B.tbkdb", help="parent B's count database")
    for hap in "ab":
        for bound in ("min", "max"):
            parser.add_argument("--{}-count-{}".format(bound, hap), type=int, default=None, metavar="N",
                                help="count cut-offs of parent {} chosen by hand (give both) instead of the ones find-unique-kmers "
                                     "would choose from its histogram".format(hap.upper()))
    return parser


def _info(path: str) -> dict:
    if not os.path.isfile(path):
        sys.exit("{}: {} does not exist or is not a file".format(PROG, path))
    try:
        return kmers.database_file_info(path)
    except (IOError, ValueError) as exc:
        sys.exit("{}: {}: {}".format(PROG, path, exc))


def default_range(info: dict, path: str):
    """The two cut-offs ``find_unique_kmers.analyze_histogram`` chooses from a header's histogram (the rows write_histogram
    would write of it); a histogram it refuses ends the run with the advice to give them by hand."""
    rows = [(c, 0 if c == 1 else int(info["histogram"][c])) for c in range(1, 256)]
    try:
        lo, hi = fu.analyze_histogram(rows, path)
    except fu.HistogramError:
        sys.exit("{}: could not find min and max counts in the histogram of {}. Choose the cut-offs by hand and give them with "
                 "--min-count and --max-count.".format(PROG, path))
    return int(lo), min(255, int(hi))


def parse_args(argv=None):
    """The arguments, with every refusal the command line and the files' headers decide; no device is touched.  ``args.range``
    is the candidates' range, ``args.info`` the database's header, ``args.parents`` None or the settled
    ``classify_by_kmers.DatabasePair`` of the two parents."""
    parser = _parser()
    args = parser.parse_args(argv)
    given = [args.database] + [p for p in (args.parent_a, args.parent_b) if p is not None]
    for path in given:
        if not fu.is_database_path(path):
            parser.error("{} is not a count database (*{})".format(path, fu.DATABASE_SUFFIX))
    if (args.parent_a is None) != (args.parent_b is None):
        parser.error("--parent-a and --parent-b go together: a pair is split between two parents")
    trio = args.parent_a is not None
    if (args.min_count is None) != (args.max_count is None):
        parser.error("--min-count and --max-count go together")
    if args.min_count is not None and not 1 <= args.min_count <= args.max_count <= 255:
        parser.error("--min-count {} --max-count {}: need 1 <= min <= max <= 255".format(args.min_count, args.max_count))
    for name in _PARENT_CUTOFFS:
        if getattr(args, name) is not None and not trio:
            parser.error("--{} chooses among a parent's k-mers: give --parent-a and --parent-b too".format(name.replace("_", "-")))
    for hap in "ab":
        lo, hi = getattr(args, "min_count_" + hap), getattr(args, "max_count_" + hap)
        if (lo is None) != (hi is None):
            parser.error("--min-count-{0} and --max-count-{0} go together".format(hap))
        if lo is not None and not 1 <= lo <= hi:  # (classify-by-kmers' rule: a maximum above 255 means 255)
            parser.error("--min-count-{0} {1} --max-count-{0} {2}: need 1 <= min <= max".format(hap, lo, hi))
        if lo is not None and lo > 255:
            parser.error("--min-count-{} {}: a counter is at most 255".format(hap, lo))
    for out in (args.matrix, args.pairs):
        if out is not None and any(os.path.abspath(out) == os.path.abspath(path) for path in given):
            parser.error("{} names an input: the tables go to files of their own".format(out))
    if args.matrix is not None and args.pairs is not None and os.path.abspath(args.matrix) == os.path.abspath(args.pairs):
        parser.error("--matrix and --pairs name one file")
    infos = [_info(path) for path in given]
    args.info = infos[0]
    if args.info["k"] % 2 == 0:
        sys.exit("{}: {} holds {}-mers: het-mer pairs differ in the middle base, which must be its own mirror under reverse "
                 "complement, and only an odd k has such a position".format(PROG, args.database, args.info["k"]))
    spaces = {False: "plain (uncompressed)", True: "homopolymer-compressed"}
    for path, info in zip(given[1:], infos[1:]):
        if info["k"] != args.info["k"]:
            sys.exit("{}: {} holds {}-mers, but {} holds {}-mers".format(PROG, args.database, args.info["k"], path, info["k"]))
        if info["compressed"] != args.info["compressed"]:
            sys.exit("{}: {} holds {} k-mers, but {} holds {} ones: count all three the same way".format(
                PROG, args.database, spaces[args.info["compressed"]], path, spaces[info["compressed"]]))
    args.range = (args.min_count, args.max_count) if args.min_count is not None else default_range(args.info, args.database)
    args.parents = None
    if trio:  # classify-by-kmers' own settling of two parents, under this command's name
        asked = SimpleNamespace(haplotype_a_kmers=args.parent_a, haplotype_b_kmers=args.parent_b, child_database=None, min_count_child=None,
                                **{name: getattr(args, name) for name in _PARENT_CUTOFFS})
        args.parents = cbk._settle_databases(asked, prog=PROG)
        for hap in "AB":
            lo, hi = args.parents.ranges[hap]
            args.parents.ranges[hap] = (max(1, lo), min(255, hi))
    return args


def find_hetmers(args) -> dict:
    """The result of ``KmerDatabase.hetmers`` for the settled arguments; every database is closed before this returns."""
    want = args.pairs is not None
    with kmers.KmerDatabase.load(args.database) as db:
        if args.parents is None:
            return db.hetmers(args.range[0], args.range[1], pairs=want)
        pair = args.parents
        with kmers.load_solid_database(pair.paths["A"]) as a, kmers.load_solid_database(pair.paths["B"]) as b:
            return db.hetmers(args.range[0], args.range[1], y=a, z=b, y_range=pair.ranges["A"], z_range=pair.ranges["B"], pairs=want)


def main(argv=None):
    args = parse_args(argv)
    result = find_hetmers(args)
    k = args.info["k"]
    parent_ranges = None if args.parents is None else (args.parents.ranges["A"], args.parents.ranges["B"])
    print("\n".join(report(result, k, args.info["compressed"], args.range, parent_ranges)))
    if args.matrix is not None:
        write_matrix(args.matrix, result["spec"], k, args.range, args.database)
    if args.pairs is not None:
        write_pairs(args.pairs, result["records"], k, args.parents is not None)


if __name__ == "__main__":
    main()
