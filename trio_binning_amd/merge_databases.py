"""Unite k-mer count databases: ``python -m trio_binning_amd.merge_databases -o out.tbkdb [--solid] a.tbkdb [b.tbkdb ...]``.

Every input must be a FULL database - one that holds the k-mers seen once too, kept by find-unique-kmers --keep-databases
--keep-singletons - of one k and one space (plain or homopolymer-compressed).  The result is the database one count of all
the inputs' reads would have left, byte for byte (``tbk_kmerdb_union``: a merge of the ascending key arrays with saturating
counter addition, on the device).  ``--solid`` writes the form without the once-seen k-mers, the file the same count without
--keep-singletons would have left; with one input that is a plain conversion.  Headers are checked before a device is touched.
"""
import argparse
import sys
from os.path import isfile

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

from . import find_unique_kmers as fu  # noqa: E402
from . import kmers  # noqa: E402

PROG = "merge_databases"


def parse_args(argv=None):
    """The arguments, refused where they can be from the command line and the inputs' headers alone (``args.infos``, one
    ``kmers.database_file_info`` per input).  No device is touched."""
    parser = argparse.ArgumentParser(prog=PROG, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-o", "--output", required=True, metavar="out.tbkdb", help="the database to write")
    parser.add_argument("--solid", action="store_true",
                        help="write the form without the k-mers seen once: what a count without --keep-singletons leaves")
    parser.add_argument("databases", nargs="+", metavar="db.tbkdb", help="full count databases (find-unique-kmers --keep-singletons)")
    args = parser.parse_args(argv)
    if not args.output.endswith(fu.DATABASE_SUFFIX):
        parser.error("-o {}: a count database's name ends in {}".format(args.output, fu.DATABASE_SUFFIX))
    if len(args.databases) == 1 and not args.solid:
        parser.error("one database and no --solid: nothing to unite and nothing to convert")
    args.infos = []
    for path in args.databases:
        if not isfile(path):
            sys.exit("{}: {} does not exist or is not a file".format(PROG, path))
        try:
            info = kmers.database_file_info(path)
        except (IOError, ValueError) as exc:
            sys.exit("{}: {}: {}".format(PROG, path, exc))
        if info["floor"] != 1:
            sys.exit("{}: {} was kept without the k-mers seen once and cannot be united exactly (a k-mer seen once in each of two "
                     "databases is in neither): count it again with find-unique-kmers --keep-databases --keep-singletons".format(PROG, path))
        first = args.infos[0] if args.infos else info
        if info["k"] != first["k"]:
            sys.exit("{}: {} holds {}-mers, {} {}-mers".format(PROG, path, info["k"], args.databases[0], first["k"]))
        if info["compressed"] != first["compressed"]:
            sys.exit("{}: {} holds {} k-mers, {} {} ones: they cannot be united".format(
                PROG, path, "homopolymer-compressed" if info["compressed"] else "plain", args.databases[0],
                "homopolymer-compressed" if first["compressed"] else "plain"))
        args.infos.append(info)
    return args


def main(argv=None):
    args = parse_args(argv)
    db = kmers.KmerDatabase.load(args.databases[0])
    try:
        for path in args.databases[1:]:
            more = kmers.KmerDatabase.load(path)
            try:
                united = db.union(more)
            finally:
                more.close()
            db.close()
            db = united
        if args.solid:
            solid = db.solid()
            db.close()
            db = solid
        db.save(args.output)
        n, stats = len(db), db.stats()
    finally:
        db.close()
    print("{}: {} k-mers of {} reads written to {}".format(PROG, n, stats["reads_added"], args.output), file=sys.stderr)


if __name__ == "__main__":
    main()
