"""Copy-number track of an assembly against a k-mer count database of the reads: where is it collapsed or duplicated?

Every window of every sequence of a FASTA/FASTQ file is looked up in one count database (``*.tbkdb``, as kept by
find-unique-kmers --keep-databases) twice.  The first pass counts how often the assembly holds each of the database's
k-mers (its copies, ``a``); the second reads the reads' counter ``c`` and ``a`` back along the sequences and compares them
at ``--peak``, the read depth of a k-mer the assembly should hold once.  A clean window (ACGT only, either case) whose
k-mer the database holds is *collapsed* when ``2c > (2a + 1) peak`` - the reads hold it more often than the assembly
does: a collapsed repeat or haplotype - and *expanded* when ``2c < (2a - 1) peak`` - the assembly holds it more often than
the reads do: a false duplication.  Windows with ``c == 255`` are *saturated*: the counter is capped there, and no verdict
is drawn.  Ties are consistent.

stdout gets one TSV line per sequence - ``name length clean absent saturated collapsed expanded`` - and a last line
``#total length clean absent saturated collapsed expanded peak window``.  ``--track`` writes one line per bin of
``--window`` window starts: ``name start end clean absent saturated depth copies collapsed expanded``, where ``depth`` and
``copies`` are the lower medians of ``c`` and of ``min(a, 255)`` over the bin's present windows (0 when there are none),
``start = b W`` and ``end = (b + 1) W``, but the sequence's length for its last bin.

No verdict on the assembly is computed: the counts say where to look.  For a trio-binned pair, score the two haplotype
assemblies concatenated against the child's database with ``--peak`` at the heterozygous (one-copy) peak: homozygous
k-mers then have ``a = 2`` at twice that depth, and both kinds of sequence read as consistent.

Without ``--peak`` the depth is chosen from the database header's histogram: the cut-offs ``[lo, hi]`` that
find-unique-kmers would choose, and in them the counter (254 at most) with the most k-mers, the lowest on a tie.
"""
# Run as ``python -m trio_binning_amd.copy_track``.  Both passes are on the device (kmers.DatabaseQuery.add and .track);
# the host sums a sequence's bins and formats the tables.

import argparse
import os
import sys
from os.path import isfile

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

from . import find_unique_kmers as fu, kmers, seq  # noqa: E402

PROG = "copy_track"

# Whole records, as for assembly_qv: a record longer than the limit arrives alone in a batch of its own length.
_BATCH_BASES = int(os.environ.get("TBK_BATCH_BASES", str(64 << 20)))
_BATCH_READS = int(os.environ.get("TBK_BATCH_READS", str(1 << 20)))

TSV_COLUMNS = ("name", "length", "clean", "absent", "saturated", "collapsed", "expanded")
TOTAL_COLUMNS = ("#total", "length", "clean", "absent", "saturated", "collapsed", "expanded", "peak", "window")
TRACK_COLUMNS = ("name", "start", "end", "clean", "absent", "saturated", "depth", "copies", "collapsed", "expanded")
SUMMED = ("clean", "absent", "saturated", "collapsed", "expanded")


def _parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog=PROG, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("assembly", help="contigs to score, FASTA/FASTQ(.gz) or BAM.")
    parser.add_argument("database", help="the count database of the reads (*.tbkdb, kept by find-unique-kmers --keep-databases)")
    parser.add_argument("--window", type=int, default=10000, metavar="W", help="window starts per bin of the track (1 or more; default 10000)")
    parser.add_argument("--peak", type=int, default=None, metavar="N",
                        help="the read depth of a k-mer the assembly should hold once (1..254; default: chosen from the database's histogram)")
    parser.add_argument("--track", default=None, metavar="PATH", help="write the track: one line per bin of every sequence")
    return parser


def default_peak(info: dict, path: str) -> int:
    """The counter with the most k-mers among the cut-offs ``find_unique_kmers.analyze_histogram`` chooses from a header's
    histogram (the rows write_histogram would write of it: row 1 as 0, whichever floor the database has), the lowest on a tie
    and 254 at most; a histogram it refuses ends the run with the advice to give --peak."""
    rows = [(c, 0 if c == 1 else int(info["histogram"][c])) for c in range(1, 256)]
    try:
        lo, hi = fu.analyze_histogram(rows, path)
    except fu.HistogramError:
        sys.exit("{}: could not find min and max counts in the histogram of {}. Choose the one-copy read depth by hand and give it "
                 "with --peak.".format(PROG, path))
    lo, hi = max(int(lo), 1), min(int(hi), 254)
    return max(range(lo, hi + 1), key=lambda c: (rows[c - 1][1], -c))


def parse_args(argv=None):
    """The arguments, refused where they can be from the command line and the database's header alone; ``args.info`` is
    that header (``kmers.database_file_info``) and ``args.peak`` is settled.  No device is touched."""
    parser = _parser()
    args = parser.parse_args(argv)
    if args.window < 1:
        parser.error("--window {}: need 1 <= W".format(args.window))
    if args.window >= 1 << 32:
        parser.error("--window {}: need W < 2^32".format(args.window))
    if args.peak is not None and not 1 <= args.peak <= 254:
        parser.error("--peak {}: need 1 <= N <= 254".format(args.peak))
    for what in (args.assembly, args.database):
        if not isfile(what):
            sys.exit("{}: {} does not exist or is not a file".format(PROG, what))
    if not fu.is_database_path(args.database):
        sys.exit("{}: {} is not a count database (*{}): a k-mer list holds no counts to score against - keep the reads' database with "
                 "find-unique-kmers --keep-databases".format(PROG, args.database, fu.DATABASE_SUFFIX))
    try:
        args.info = kmers.database_file_info(args.database)
    except (IOError, ValueError) as exc:
        sys.exit("{}: {}: {}".format(PROG, args.database, exc))
    if args.info["compressed"]:
        sys.exit("{}: {} holds homopolymer-compressed k-mers (find-unique-kmers --compress): positions along a sequence are not "
                 "defined in compressed space. Give a plain database.".format(PROG, args.database))
    if args.peak is None:
        args.peak = default_peak(args.info, args.database)
        print("\033[92mUsing {} as the one-copy read depth.\033[0m".format(args.peak), file=sys.stderr)
    return args


def sequence_line(name: str, length: int, bins) -> str:
    """The stdout line of one sequence from its bins (a ``kmers.DEPTH_BIN`` array, maybe empty)."""
    return "\t".join([name, str(length)] + [str(int(bins[f].sum(dtype="uint64"))) for f in SUMMED]) + "\n"


def track_lines(name: str, length: int, bins, window: int) -> str:
    """The --track lines of one sequence."""
    last = len(bins) - 1
    return "".join("{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\n".format(
        name, b * window, length if b == last else (b + 1) * window, int(x["clean"]), int(x["absent"]), int(x["saturated"]), int(x["depth"]),
        int(x["copies"]), int(x["collapsed"]), int(x["expanded"])) for b, x in enumerate(bins))


def _batches(path):
    """(bases, base offsets, names) of every batch of whole records of a file"""
    with seq.BatchReader(path) as reader:
        batch = seq.Batch()
        try:
            while reader.next_batch(batch, _BATCH_BASES, _BATCH_READS):
                bases, base_off, names, name_off = batch.arrays()[:4]
                text = bytes(names)
                yield bases, base_off, [text[int(name_off[i]):int(name_off[i + 1])].decode() for i in range(batch.n_reads)]
        finally:
            batch.close()


def main(argv=None):
    """Main method of program"""
    args = parse_args(argv)
    import numpy as np

    track_tmp = args.track + ".tmp" if args.track else None  # written beside its place and renamed: a run that fails leaves no half a file
    out = sys.stdout
    total = np.zeros(1 + len(SUMMED), dtype=np.uint64)  # length, then the summed columns
    try:
        with kmers.KmerDatabase.load(args.database) as database, database.query(copies=True) as query, open(track_tmp or os.devnull, "w") as track:
            for bases, base_off, _ in _batches(args.assembly):  # pass 1: the assembly's copies of every k-mer
                query.add(bases, base_off)
            for bases, base_off, label in _batches(args.assembly):  # pass 2: read them back along the sequences
                bins, prefix = query.track(bases, base_off, args.window, args.peak)
                off = base_off.astype(np.int64)
                lines = []
                for i, name in enumerate(label):
                    length, mine = int(off[i + 1] - off[i]), bins[int(prefix[i]):int(prefix[i + 1])]
                    lines.append(sequence_line(name, length, mine))
                    total[0] += np.uint64(length)
                    for j, f in enumerate(SUMMED):
                        total[1 + j] += mine[f].sum(dtype=np.uint64)
                    if track_tmp:
                        track.write(track_lines(name, length, mine, args.window))
                out.write("".join(lines))
        out.write("\t".join(["#total"] + [str(int(x)) for x in total] + [str(args.peak), str(args.window)]) + "\n")
        out.flush()
        if track_tmp:
            os.replace(track_tmp, args.track)
    except BaseException:
        if track_tmp and os.path.exists(track_tmp):
            os.remove(track_tmp)
        raise


if __name__ == "__main__":
    main()
