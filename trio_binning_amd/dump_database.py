"""Write a k-mer count database as a counted dump: ``python -m trio_binning_amd.dump_database in.tbkdb -o out.txt
[--min-count N] [--max-count N]``.

The file is what ``kmc_dump -ciMIN -cxMAX`` writes: one line per k-mer whose counter lies in [MIN, MAX], the k-mer, a tab, its
counter, in lexicographic order (``tbk_kmerdb_dump_text``).  Any database is taken - solid or full, plain or
homopolymer-compressed; a solid one holds no counter below 2.  import-database reads the file back into the same database.
"""
import argparse
import sys
from os.path import isfile

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

from . import kmers  # noqa: E402

PROG = "dump_database"


def parse_args(argv=None):
    """The arguments, refused where they can be from the command line and the database's header (``args.info``) alone."""
    parser = argparse.ArgumentParser(prog=PROG, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("database", metavar="in.tbkdb", help="a count database")
    parser.add_argument("-o", "--output", required=True, metavar="out.txt", help="the dump to write")
    parser.add_argument("--min-count", type=int, default=1, help="lowest counter to write (default 1)")
    parser.add_argument("--max-count", type=int, default=255, help="highest counter to write (default 255)")
    args = parser.parse_args(argv)
    if args.min_count < 0 or args.max_count < 0:
        parser.error("--min-count and --max-count are not negative")
    if not isfile(args.database):
        sys.exit("{}: {} does not exist or is not a file".format(PROG, args.database))
    try:
        args.info = kmers.database_file_info(args.database)
    except (IOError, ValueError) as exc:
        sys.exit("{}: {}: {}".format(PROG, args.database, exc))
    return args


def main(argv=None):
    args = parse_args(argv)
    print("\033[92mLoading the k-mer database...\033[0m", file=sys.stderr)
    db = kmers.KmerDatabase.load(args.database)
    try:
        print("\033[92mDumping k-mers with counts in range [{},{}]...\033[0m".format(max(db.floor, args.min_count), min(255, args.max_count)),
              file=sys.stderr)
        n = db.dump(args.output, args.min_count, args.max_count)
    finally:
        db.close()
    print("{}: {} {}-mers written to {}".format(PROG, n, args.info["k"], args.output), file=sys.stderr)


if __name__ == "__main__":
    main()
