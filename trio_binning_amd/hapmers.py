"""Hap-mer databases of a trio: the parental k-mers the child inherited, with the child's counters.

    python -m trio_binning_amd.hapmers -o DIR A.tbkdb B.tbkdb --child-database child.tbkdb \\
        [--min-count-a N --max-count-a N --min-count-b N --max-count-b N --min-count-child N]

Writes DIR/haplotypeA.hapmers.tbkdb and DIR/haplotypeB.hapmers.tbkdb from the three count databases find-unique-kmers
--keep-databases left.  Haplotype A's file holds the child's k-mers with a counter of at least the child's cut-off that parent
A holds with a counter within A's cut-offs and parent B does not hold at all - exactly the k-mers
``classify-by-kmers --child-database`` finds for haplotype A, chosen by the same cut-off rule with the same refusals, and now
kept with the child's counters (``tbk_kmerdb_select``); B's file likewise.  These are the databases Merqury's hapmers.sh makes,
and what they are for is scoring a haplotype assembly:

    python -m trio_binning_amd.assembly_qv hapA_asm.fa DIR/haplotypeA.hapmers.tbkdb --min-count 1

whose ``#total`` completeness is then the hap-mer completeness of that assembly; the same line with haplotypeB.hapmers.tbkdb is
the share of the wrong parent's hap-mers it holds.

stderr has one line per haplotype: the number of hap-mers, the share they are of that parent's own k-mers within its cut-offs
(those the other parent lacks; near 1/2 in a true trio), and the child's cut-off.  No verdict is computed, as compare-databases
computes none.  Full files are used in their solid form; homopolymer-compressed databases are accepted when all three are, and
the result says so.  Headers are checked before a device is touched.
"""
import argparse
import os
import sys

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

from . import classify_by_kmers as cbk  # noqa: E402
from . import find_unique_kmers as fu  # noqa: E402
from . import kmers  # noqa: E402

PROG = "hapmers"
OUT_NAME = "haplotype{}.hapmers" + fu.DATABASE_SUFFIX


def _parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog=PROG, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-o", "--outpath", required=True, metavar="DIR", help="the directory the two hap-mer databases go to (made if missing)")
    parser.add_argument("haplotype_a_kmers", metavar="A.tbkdb", help="parent A's count database")
    parser.add_argument("haplotype_b_kmers", metavar="B.tbkdb", help="parent B's count database")
    cbk._add_database_options(parser)
    return parser


def parse_args(argv=None):
    """The arguments, with every refusal the command line and the files' headers decide; no device is touched.
    ``args.databases`` is the settled ``classify_by_kmers.DatabasePair``."""
    parser = _parser()
    args = parser.parse_args(argv)
    if args.child_database is None:
        parser.error("--child-database is required: hap-mers are the parental k-mers the child inherited")
    given = [args.haplotype_a_kmers, args.haplotype_b_kmers, args.child_database]
    for path in given:
        if not fu.is_database_path(path):
            parser.error("{} is not a count database (*{})".format(path, fu.DATABASE_SUFFIX))
    cbk._check_kmer_arguments(parser, args, prog=PROG)
    for hap in "ab":
        lo = getattr(args, "min_count_" + hap)
        if lo is not None and lo > 255:
            parser.error("--min-count-{} {}: a counter is at most 255".format(hap, lo))
    if args.min_count_child is not None and args.min_count_child > 255:
        parser.error("--min-count-child {}: a counter is at most 255".format(args.min_count_child))
    if os.path.exists(args.outpath) and not os.path.isdir(args.outpath):
        parser.error("-o {} exists and is not a directory".format(args.outpath))
    for path in given:
        try:
            kmers.database_file_info(path)  # (a file that cannot be read or is no database: this command's words)
        except (IOError, ValueError) as exc:
            sys.exit("{}: {}: {}".format(PROG, path, exc))
    args.databases = cbk._settle_databases(args, prog=PROG)
    return args


def select_hapmers(pair) -> dict:
    """{"A": (database, own), "B": ...}: each haplotype's hap-mer database, open, and the number of that parent's own k-mers
    within its cut-offs.  The three inputs are loaded in their solid form and closed before this returns."""
    out = {}
    held = (max(1, min(255, pair.child_min)), 255)
    with kmers.load_solid_database(pair.paths["A"]) as a, kmers.load_solid_database(pair.paths["B"]) as b, \
            kmers.load_solid_database(pair.child_path) as child:
        try:
            for hap, own, other in (("A", a, b), ("B", b, a)):
                lo, hi = max(1, pair.ranges[hap][0]), min(255, pair.ranges[hap][1])
                # the share's denominator is no count of the child's selection: the parent's own k-mers, selected and dropped
                with own.select(lo, hi, exclude=[other]) as parents_own:
                    n_own = len(parents_own)
                out[hap] = (child.select(held[0], held[1], require=[(own, lo, hi)], exclude=[other]), n_own)
        except BaseException:
            for db, _ in out.values():
                db.close()
            raise
    return out


def main(argv=None):
    args = parse_args(argv)
    pair = args.databases
    os.makedirs(args.outpath, exist_ok=True)
    picked = select_hapmers(pair)
    try:
        for hap in "AB":
            db, n_own = picked[hap]
            path = os.path.join(args.outpath, OUT_NAME.format(hap))
            db.save(path)
            share = "{:.6f}".format(len(db) / n_own) if n_own else "nan"
            print("{}: haplotype {}: {} hap-mers ({}-mers) written to {}: {} of the {} k-mers of {} with a count in [{},{}] that the other "
                  "parent lacks; child's counts from {} on".format(PROG, hap, len(db), db.k, path, share, n_own, pair.paths[hap],
                                                                    pair.ranges[hap][0], pair.ranges[hap][1], pair.child_min), file=sys.stderr)
            if not len(db):
                print("{}: haplotype {}: no hap-mer at these cut-offs: {} is an empty database".format(PROG, hap, path), file=sys.stderr)
    finally:
        for db, _ in picked.values():
            db.close()


if __name__ == "__main__":
    main()
