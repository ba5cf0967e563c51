"""Select from k-mer count databases into a database.

    python -m trio_binning_amd.select_database -o out.tbkdb [--min-count N] [--max-count N] [--min-gc N] [--max-gc N] \\
        [--require DB[:MIN[:MAX]]]... [--exclude DB[:MIN[:MAX]]]... [--counter base|min|sum] base.tbkdb

The k-mers of base.tbkdb with a counter in [--min-count, --max-count] (default 1..255) that every --require database holds with
a counter in its MIN..MAX (default 1..255) and no --exclude database does, written as a database again (``tbk_kmerdb_select``):
the k-mers two lanes share (--require), a library minus a contaminant or organelle database (--exclude), and with both a
hap-mer database (the ``hapmers`` command does that for a trio).  All ranges are taken literally, 1 <= MIN <= MAX <= 255: ask a
full database (kept with --keep-singletons) with MIN 2 to ignore its k-mers seen once.  At most two partners in all; chain runs
for more.  --counter: the counters written are base's ("base", the default), the minimum of base's and the --require
databases' ("min"), or their sum capped at 255 ("sum").  The files are loaded as they are, full ones included, and may be of
either space as long as all are of one.  --min-gc and --max-gc keep only the k-mers with that many G-or-C bases (integers in
0..k, counted in bases, not per cent; either may be given alone): a cloud of the ``gc_spectrum`` matrix carved out as a database.

The result is a FULL database (its header states exactly the k-mers and counters it holds; reads and bases are 0): it merges
exactly with merge_databases, dumps with dump_database and scores with assembly_qv.  An empty selection is written too.
Headers are checked before a device is touched.
"""
import argparse
import os
import sys
from os.path import isfile

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

from . import find_unique_kmers as fu  # noqa: E402
from . import kmers  # noqa: E402

PROG = "select_database"
SPACES = {False: "plain", True: "homopolymer-compressed"}


def partner_spec(text: str):
    """``DB[:MIN[:MAX]]`` -> (path, min, max).  Up to two trailing all-digit fields are the range; what stands before them is the
    path, colons included.  MAX alone cannot be given; a missing MIN is 1, a missing MAX 255."""
    fields = text.split(":")
    numbers = []
    while len(fields) > 1 and len(numbers) < 2 and fields[-1].isdigit():
        numbers.insert(0, int(fields.pop()))
    return (":".join(fields), numbers[0] if numbers else 1, numbers[1] if len(numbers) > 1 else 255)


def _same_file(a: str, b: str) -> bool:
    try:
        return os.path.samefile(a, b)
    except OSError:
        return os.path.abspath(a) == os.path.abspath(b)


def parse_args(argv=None):
    """The arguments, refused where they can be from the command line and the inputs' headers alone; no device is touched.
    ``args.partners``: (path, min, max, "require" | "exclude") in the order given, --require first; ``args.info`` the base's
    header."""
    parser = argparse.ArgumentParser(prog=PROG, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-o", "--output", required=True, metavar="out.tbkdb", help="the database to write")
    parser.add_argument("--min-count", type=int, default=1, metavar="N", help="lowest counter of base.tbkdb that is kept (default 1)")
    parser.add_argument("--max-count", type=int, default=255, metavar="N", help="highest counter of base.tbkdb that is kept (default 255)")
    parser.add_argument("--min-gc", type=int, default=None, metavar="N", help="fewest G-or-C bases of a k-mer that is kept (0..k; default: no bound)")
    parser.add_argument("--max-gc", type=int, default=None, metavar="N", help="most G-or-C bases of a k-mer that is kept (0..k; default: no bound)")
    parser.add_argument("--require", action="append", default=[], type=partner_spec, metavar="DB[:MIN[:MAX]]",
                        help="keep only k-mers this database holds with a counter in MIN..MAX (default 1..255)")
    parser.add_argument("--exclude", action="append", default=[], type=partner_spec, metavar="DB[:MIN[:MAX]]",
                        help="drop the k-mers this database holds with a counter in MIN..MAX (default 1..255)")
    parser.add_argument("--counter", choices=sorted(_lib.SELECT_COUNTERS), default="base",
                        help="the counters written: base's, the minimum with the --require databases', or the sum capped at 255")
    parser.add_argument("base", metavar="base.tbkdb", help="the count database to select from")
    args = parser.parse_args(argv)
    if not args.output.endswith(fu.DATABASE_SUFFIX):
        parser.error("-o {}: a count database's name ends in {}".format(args.output, fu.DATABASE_SUFFIX))
    args.partners = [p + ("require",) for p in args.require] + [p + ("exclude",) for p in args.exclude]
    if len(args.partners) > 2:
        parser.error("{} --require and --exclude databases: a selection takes at most two; run it again on its result for more".format(len(args.partners)))
    if not 1 <= args.min_count <= args.max_count <= 255:
        parser.error("--min-count {} --max-count {}: need 1 <= min <= max <= 255".format(args.min_count, args.max_count))
    for path, lo, hi, mode in args.partners:
        if not 1 <= lo <= hi <= 255:
            parser.error("--{} {}: counter range {}..{}: need 1 <= MIN <= MAX <= 255".format(mode, path, lo, hi))
    for name, value in (("--min-gc", args.min_gc), ("--max-gc", args.max_gc)):
        if value is not None and not 0 <= value <= 32:
            parser.error("{} {}: a number of G-or-C bases, 0..k".format(name, value))
    if args.min_gc is not None and args.max_gc is not None and args.min_gc > args.max_gc:
        parser.error("--min-gc {} --max-gc {}: need min <= max".format(args.min_gc, args.max_gc))
    inputs = [args.base] + [p[0] for p in args.partners]
    for path in inputs:
        if _same_file(args.output, path):
            parser.error("-o {} names an input: the result goes to a file of its own".format(args.output))
    infos = []
    for path in inputs:
        if not isfile(path):
            sys.exit("{}: {} does not exist or is not a file".format(PROG, path))
        try:
            info = kmers.database_file_info(path)
        except (IOError, ValueError) as exc:
            sys.exit("{}: {}: {}".format(PROG, path, exc))
        first = infos[0] if infos else info
        if info["k"] != first["k"]:
            sys.exit("{}: {} holds {}-mers, {} {}-mers".format(PROG, path, info["k"], args.base, first["k"]))
        if info["compressed"] != first["compressed"]:
            sys.exit("{}: {} holds {} k-mers, {} {} ones: they share no k-mer to select by".format(
                PROG, path, SPACES[info["compressed"]], args.base, SPACES[first["compressed"]]))
        infos.append(info)
    args.info = infos[0]
    for name, value in (("--min-gc", args.min_gc), ("--max-gc", args.max_gc)):
        if value is not None and value > args.info["k"]:
            parser.error("{} {}: {} holds {}-mers: a number of G-or-C bases, 0..{}".format(name, value, args.base, args.info["k"], args.info["k"]))
    args.gc = None if args.min_gc is None and args.max_gc is None else (args.min_gc, args.max_gc)
    return args


def gc_words(gc, k: int) -> str:
    """what the stderr line says of a GC range: nothing when none was given"""
    if gc is None:
        return ""
    return " with {}..{} G-or-C bases".format(0 if gc[0] is None else gc[0], k if gc[1] is None else gc[1])


def main(argv=None):
    args = parse_args(argv)
    loaded = {}  # by real path: a database named twice - base as its own partner, say - is loaded once
    try:
        def database(path):
            key = os.path.realpath(path)
            if key not in loaded:
                loaded[key] = kmers.KmerDatabase.load(path)
            return loaded[key]

        base = database(args.base)
        groups = {"require": [], "exclude": []}
        for path, lo, hi, mode in args.partners:
            groups[mode].append((database(path), lo, hi))
        with base.select(args.min_count, args.max_count, require=groups["require"], exclude=groups["exclude"], counter=args.counter,
                         gc=args.gc) as picked:
            picked.save(args.output)
            kept, of = len(picked), len(base)
    finally:
        for db in loaded.values():
            db.close()
    gc = gc_words(args.gc, args.info["k"])
    if kept:
        print("{}: {} of the {} k-mers of {} kept{} and written to {}".format(PROG, kept, of, args.base, gc, args.output), file=sys.stderr)
    else:
        print("{}: none of the {} k-mers of {} kept{}: {} is an empty database".format(PROG, of, args.base, gc, args.output), file=sys.stderr)


if __name__ == "__main__":
    main()
