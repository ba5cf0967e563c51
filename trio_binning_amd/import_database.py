"""Make a k-mer count database of counted dumps: ``python -m trio_binning_amd.import_database -o out.tbkdb [-k K]
[--floor auto|1|2] [--compress] [--reads N --bases N] dump.txt[,dump2.txt ...]``.

A counted dump is what ``kmc_dump``, ``meryl print`` and ``jellyfish dump -c`` print: one line per k-mer, the k-mer, one tab
or space, its count.  The k-mers are made canonical, counts above 255 saturate, a k-mer listed more than once (both strands,
several lanes' dumps) gets the saturating sum of its counts (``tbk_kmerdb_import_text``, on the device).  ``--floor 2`` leaves
the k-mers counted once out of the entries, as ``kmc`` with its default -ci2 does; ``--floor 1`` keeps them (a full database,
which merge_databases can unite); ``auto`` keeps them when the dump holds any.  ``--compress`` states that the k-mers were
counted in homopolymer-compressed space, and every line is held to it.  The result is what find-unique-kmers
--keep-databases leaves: classify-by-kmers, assembly-qv, phase-blocks and merge-databases take it as it is.
"""
import argparse
import sys
from os.path import isfile

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

from . import find_unique_kmers as fu  # noqa: E402
from . import kmers  # noqa: E402

PROG = "import_database"


def parse_args(argv=None):
    """The arguments, refused where they can be without a device: ``args.dumps`` the files, ``args.k`` the k-mer size (taken
    from the first dump's first line when -k is not given)."""
    parser = argparse.ArgumentParser(prog=PROG, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-o", "--output", required=True, metavar="out.tbkdb", help="the database to write")
    parser.add_argument("-k", "--kmer-size", type=int, default=None, help="default: the length of the first line's k-mer")
    parser.add_argument("--floor", default="auto", help="auto, 1 (keep the k-mers counted once) or 2 (leave them out)")
    parser.add_argument("--compress", action="store_true", help="the dump holds homopolymer-compressed k-mers")
    parser.add_argument("--reads", type=int, default=None, help="reads that were counted, for the header (a dump does not say)")
    parser.add_argument("--bases", type=int, default=None, help="bases that were counted, for the header")
    parser.add_argument("dumps", metavar="dump.txt[,dump2.txt ...]", help="counted dumps, comma-separated")
    args = parser.parse_args(argv)
    if not args.output.endswith(fu.DATABASE_SUFFIX):
        parser.error("-o {}: a count database's name ends in {}".format(args.output, fu.DATABASE_SUFFIX))
    if args.floor not in ("auto", "1", "2"):
        parser.error("--floor {}: one of auto, 1, 2".format(args.floor))
    args.floor = args.floor if args.floor == "auto" else int(args.floor)
    if args.kmer_size is not None and not 1 <= args.kmer_size <= 32:
        parser.error("-k {}: a database holds k-mers of 1 to 32 bases".format(args.kmer_size))
    if (args.reads is None) != (args.bases is None):
        parser.error("--reads and --bases are given together")
    if args.reads is not None and (args.reads < 0 or args.bases < 0):
        parser.error("--reads and --bases are not negative")
    args.dumps = [p for p in args.dumps.split(",") if p]
    if not args.dumps:
        parser.error("no dump given")
    for path in args.dumps:
        if not isfile(path):
            sys.exit("{}: {} does not exist or is not a file".format(PROG, path))
    args.k = args.kmer_size
    return args


def main(argv=None):
    args = parse_args(argv)
    print("\033[92mImporting {} counted dump{}...\033[0m".format(len(args.dumps), "" if len(args.dumps) == 1 else "s"), file=sys.stderr)
    db = kmers.KmerDatabase.from_dump(args.dumps, k=args.k, floor=args.floor, compressed=args.compress, reads=args.reads or 0,
                                      bases=args.bases or 0)
    try:
        print("\033[92mWriting the k-mer database...\033[0m", file=sys.stderr)
        db.save(args.output)
        n, k, floor, distinct = len(db), db.k, db.floor, int(db.histogram()[0])
    finally:
        db.close()
    print("{}: {} {}-mers ({} distinct in the dump{}) written to {}".format(
        PROG, n, k, distinct, "; the ones counted once are left out" if floor == 2 else "", args.output), file=sys.stderr)


if __name__ == "__main__":
    main()
