"""Hold k-mer count databases against each other.

    python -m trio_binning_amd.compare_databases x.tbkdb y.tbkdb [--matrix joint.tsv]
    python -m trio_binning_amd.compare_databases A.tbkdb B.tbkdb --child-database child.tbkdb [--spectra trio.tsv]

Two databases: how many distinct k-mers each holds, how many both hold, Jaccard index and containment, and with --matrix the
joint k-mer spectrum - how many k-mers have counter cx in the first database and cy in the second (``tbk_kmerdb_joint_spectrum``).
The files are loaded as they are, full ones (kept with --keep-singletons) included.

A trio (--child-database): what share of the child's solid k-mers neither parent holds, and what share of each parent's own
k-mers the child inherited, at the cut-offs classify-by-kmers would use (--min-count-a ... --min-count-child, or the ones
chosen from each histogram).  In a true trio the first share is near 0 and both inherited shares are near 1/2; no verdict is
computed, because no threshold has been measured on real data.  --spectra writes the three tables the figures are sums of
(``tbk_kmerdb_origin_spectrum``), counter by counter: error k-mers inherit at about 0 and true heterozygous ones at about
1/2, which is the evidence to choose cut-offs by.  Full files are used in their solid form.

stdout is ``name<TAB>value`` lines (INTEGRATION.md lists them).  Headers are checked before a device is touched.
"""
import argparse
import sys

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

import numpy as np  # noqa: E402

from . import classify_by_kmers as cbk  # noqa: E402
from . import find_unique_kmers as fu  # noqa: E402
from . import kmers  # noqa: E402

PROG = "compare-databases"
CLASSES = ("neither", "first_only", "second_only", "both")  # the four rows of an origin spectrum, by class 0..3
_CUTOFFS = ("min_count_a", "max_count_a", "min_count_b", "max_count_b", "min_count_child")


# ---- from spectra to the report's lines: pure functions ------------------------------------------------------------------------
def _ratio(num: int, den: int) -> str:
    return "{:.6f}".format(num / den) if den else "nan"


def _lines(pairs) -> list:
    return ["{}\t{}".format(name, value) for name, value in pairs]


def report_two(spec, k: int, compressed: bool, floor_x: int, floor_y: int) -> list:
    """The lines of the two-database report from a joint spectrum (256 x 256; row: counter in x, column: counter in y)."""
    spec = np.asarray(spec, dtype=np.uint64).reshape(256, 256)
    kmers_x, kmers_y = int(spec[1:, :].sum()), int(spec[:, 1:].sum())
    shared, only_x, only_y, union = int(spec[1:, 1:].sum()), int(spec[1:, 0].sum()), int(spec[0, 1:].sum()), int(spec.sum())
    return _lines([
        ("k", k), ("space", "compressed" if compressed else "plain"), ("floor_x", floor_x), ("floor_y", floor_y),
        ("kmers_x", kmers_x), ("kmers_y", kmers_y), ("shared", shared), ("only_x", only_x), ("only_y", only_y), ("union", union),
        ("jaccard", _ratio(shared, union)), ("containment_x_in_y", _ratio(shared, kmers_x)), ("containment_y_in_x", _ratio(shared, kmers_y)),
    ])


def report_trio(child, a, b, k: int, compressed: bool, range_a, range_b, min_count_child: int) -> list:
    """The lines of the trio report from three origin spectra (4 x 256 each): ``child`` is the child against A (bit 0) and B
    (bit 1); ``a`` is A against B (bit 0) and the child (bit 1); ``b`` is B against A (bit 0) and the child (bit 1)."""
    child, a, b = (np.asarray(t, dtype=np.uint64).reshape(4, 256) for t in (child, a, b))
    solid = child[:, max(0, min_count_child):]
    neither, only_a, only_b, both = (int(solid[cls].sum()) for cls in range(4))
    child_solid = neither + only_a + only_b + both
    pairs = [
        ("k", k), ("space", "compressed" if compressed else "plain"),
        ("range_a", "{},{}".format(*range_a)), ("range_b", "{},{}".format(*range_b)), ("min_count_child", min_count_child),
        ("child_solid", child_solid), ("child_in_both", both), ("child_only_a", only_a), ("child_only_b", only_b),
        ("child_in_neither", neither), ("child_in_neither_share", _ratio(neither, child_solid)),
    ]
    for hap, table, (lo, hi) in (("a", a, range_a), ("b", b, range_b)):
        own = table[:, max(0, lo):max(0, min(hi, 255) + 1)]
        inherited = int(own[2].sum())          # the other parent lacks it, the child holds it
        unique = int(own[0].sum()) + inherited  # the other parent lacks it
        pairs += [("unique_" + hap, unique), ("inherited_" + hap, inherited), ("inherited_{}_share".format(hap), _ratio(inherited, unique))]
    return _lines(pairs)


# ---- the tables as files ----------------------------------------------------------------------------------------------------------
def write_matrix(path: str, spec, name_x: str, name_y: str, floor_x: int, floor_y: int) -> None:
    """``#`` lines that name the files, their floors and the meaning of row and column 0, then row cx of the joint spectrum:
    256 tab-separated columns."""
    spec = np.asarray(spec, dtype=np.uint64).reshape(256, 256)
    with open(path, "w") as fh:
        fh.write("# joint k-mer spectrum: line 1 + cx below these comments is row cx (counter in x), its 256 columns are cy (counter in y)\n")
        fh.write("# x = {} (floor {})\n".format(name_x, floor_x))
        fh.write("# y = {} (floor {})\n".format(name_y, floor_y))
        fh.write("# row 0: k-mers x holds no entry for; column 0: k-mers y holds no entry for. A database of floor 2 holds no entry "
                 "for a k-mer seen once, one of floor 1 does (counter 1); the cell (0,0) is 0\n")
        for row in spec:
            fh.write("\t".join(str(int(v)) for v in row) + "\n")


def read_matrix(path: str) -> np.ndarray:
    """The matrix ``write_matrix`` wrote."""
    rows = [line.split("\t") for line in open(path) if not line.startswith("#")]
    spec = np.array(rows, dtype=np.uint64)
    if spec.shape != (256, 256):
        raise ValueError("{}: {} rows of {} columns, not 256 x 256".format(path, len(rows), spec.shape[1:] or "no"))
    return spec


def write_spectra(path: str, tables) -> None:
    """``tables``: (title, 4 x 256 origin spectrum) in order.  Each goes under a ``#`` line with its title and one naming the
    columns: the counter, then its entries in the four classes."""
    with open(path, "w") as fh:
        for title, table in tables:
            table = np.asarray(table, dtype=np.uint64).reshape(4, 256)
            fh.write("# {}\n".format(title))
            fh.write("# counter\t" + "\t".join(CLASSES) + "\n")
            for c in range(256):
                fh.write("{}\t{}\n".format(c, "\t".join(str(int(table[cls, c])) for cls in range(4))))


def read_spectra(path: str) -> list:
    """[(title, 4 x 256 array)] of the file ``write_spectra`` wrote."""
    out, title, rows = [], None, []
    for line in open(path):
        if line.startswith("# counter\t"):
            continue
        if line.startswith("#"):
            if title is not None:
                out.append((title, rows))
            title, rows = line[2:].rstrip("\n"), []
            continue
        rows.append(line.split("\t"))
    if title is not None:
        out.append((title, rows))
    tables = []
    for title, rows in out:
        table = np.array(rows, dtype=np.uint64)
        if table.shape != (256, 5) or not np.array_equal(table[:, 0], np.arange(256, dtype=np.uint64)):
            raise ValueError("{}: the table under '{}' is not 256 counters by four classes".format(path, title))
        tables.append((title, table[:, 1:].T.copy()))
    return tables


def trio_titles(pair) -> list:
    """The ``#`` titles of the three tables of --spectra, in their order: the child, A, B."""
    a, b, child, cmin = pair.paths["A"], pair.paths["B"], pair.child_path, pair.child_min
    return [
        "base = child {}; first = A {} [2,255]; second = B {} [2,255]".format(child, a, b),
        "base = A {}; first = B {} [2,255]; second = child {} [{},255]".format(a, b, child, cmin),
        "base = B {}; first = A {} [2,255]; second = child {} [{},255]".format(b, a, child, cmin),
    ]


# ---- the command ------------------------------------------------------------------------------------------------------------------
def _parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog=PROG, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("haplotype_a_kmers", metavar="x.tbkdb", help="the first count database (with --child-database: parent A's)")
    parser.add_argument("haplotype_b_kmers", metavar="y.tbkdb", help="the second count database (with --child-database: parent B's)")
    parser.add_argument("--matrix", default=None, metavar="joint.tsv", help="two databases: write the 256 x 256 joint spectrum here")
    parser.add_argument("--spectra", default=None, metavar="trio.tsv",
                        help="with --child-database: write the three origin spectra (child, A, B) here, counter by counter")
    cbk._add_database_options(parser)
    return parser


def _info(path: str) -> dict:
    try:
        return kmers.database_file_info(path)
    except (IOError, ValueError) as exc:
        sys.exit("{}: {}: {}".format(PROG, path, exc))


def parse_args(argv=None):
    """The arguments, with every refusal the command line and the files' headers decide; no device is touched.  Two databases:
    ``args.infos`` holds both headers.  A trio: ``args.databases`` is the settled ``classify_by_kmers.DatabasePair``."""
    parser = _parser()
    args = parser.parse_args(argv)
    given = [args.haplotype_a_kmers, args.haplotype_b_kmers] + ([args.child_database] if args.child_database is not None else [])
    for path in given:
        if not fu.is_database_path(path):
            parser.error("{} is not a count database (*{})".format(path, fu.DATABASE_SUFFIX))
    trio = args.child_database is not None
    if trio and args.matrix is not None:
        parser.error("--matrix is the joint spectrum of two databases; with --child-database ask for --spectra")
    if not trio and args.spectra is not None:
        parser.error("--spectra holds a trio's three tables: give --child-database too (two databases have a --matrix)")
    if not trio:
        for name in _CUTOFFS:
            if getattr(args, name) is not None:
                parser.error("--{} chooses among a trio's k-mers: give --child-database too".format(name.replace("_", "-")))
        paths = given
        args.infos = [_info(path) for path in paths]
        if args.infos[0]["k"] != args.infos[1]["k"]:
            sys.exit("{}: {} holds {}-mers, but {} holds {}-mers".format(PROG, paths[0], args.infos[0]["k"], paths[1], args.infos[1]["k"]))
        if args.infos[0]["compressed"] != args.infos[1]["compressed"]:
            spaces = {False: "plain (uncompressed)", True: "homopolymer-compressed"}
            sys.exit("{}: {} holds {} k-mers, but {} holds {} ones: they share no k-mer worth comparing".format(
                PROG, paths[0], spaces[args.infos[0]["compressed"]], paths[1], spaces[args.infos[1]["compressed"]]))
        args.databases = None
        return args
    cbk._check_kmer_arguments(parser, args, prog=PROG)
    if args.min_count_child is not None and args.min_count_child > 255:
        parser.error("--min-count-child {}: a counter is at most 255".format(args.min_count_child))
    for path in given:
        _info(path)  # (a file that cannot be read or is no database: this command's words, before the shared code opens it)
    args.databases = cbk._settle_databases(args, prog=PROG)
    args.k = kmers.database_file_info(args.haplotype_a_kmers)["k"]
    return args


def compare_two(path_x: str, path_y: str) -> np.ndarray:
    with kmers.KmerDatabase.load(path_x) as x, kmers.KmerDatabase.load(path_y) as y:
        return x.joint_spectrum(y)


def compare_trio(pair) -> tuple:
    """(child, a, b): the three origin spectra ``report_trio`` takes, of the solid forms of the three files."""
    with kmers.load_solid_database(pair.paths["A"]) as a, kmers.load_solid_database(pair.paths["B"]) as b, \
            kmers.load_solid_database(pair.child_path) as child:
        held = (max(1, min(255, pair.child_min)), 255)
        return (child.origin_spectrum(a, b, (2, 255), (2, 255)), a.origin_spectrum(b, child, (2, 255), held),
                b.origin_spectrum(a, child, (2, 255), held))


def main(argv=None):
    args = parse_args(argv)
    if args.databases is None:
        x, y = args.infos
        spec = compare_two(args.haplotype_a_kmers, args.haplotype_b_kmers)
        print("\n".join(report_two(spec, x["k"], x["compressed"], x["floor"], y["floor"])))
        if args.matrix is not None:
            write_matrix(args.matrix, spec, args.haplotype_a_kmers, args.haplotype_b_kmers, x["floor"], y["floor"])
        return
    pair = args.databases
    tables = compare_trio(pair)
    print("\n".join(report_trio(*tables, args.k, pair.compressed, pair.ranges["A"], pair.ranges["B"], pair.child_min)))
    if args.spectra is not None:
        write_spectra(args.spectra, zip(trio_titles(pair), tables))


if __name__ == "__main__":
    main()
