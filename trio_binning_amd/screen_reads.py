"""Screen reads against a k-mer count database: which reads carry its k-mers, and the library with and without them.

Every window of every read of a FASTA/FASTQ(.gz) or BAM file is looked up in one count database (``*.tbkdb``: a library's own,
kept by find-unique-kmers --keep-databases, or a part of one carved out by select_database - a contaminant cloud, an organelle,
PhiX, a region's k-mers).  A clean window (ACGT only, either case) is *held* when the database holds its k-mer with a counter in
``[--min-count, --max-count]``; a base is *covered* when it lies in a held window.  Per read that gives ``clean`` and ``held``
windows, ``covered`` bases, the number of ``stretches`` of consecutive covered bases and the ``longest`` of them.

A read without a clean window - shorter than k, or an N in every window - is *unjudged*.  Any other read is *matched* when all
of these hold, and *unmatched* if not:

    held >= --min-hits                 (default 1)
    held / clean >= --min-share        (default 0)
    covered / length >= --min-covered  (default 0)
    longest >= --min-stretch           (default 0)

The shares are decimal numbers in [0, 1] with at most 9 decimals and are compared exactly, in integers.

The reads go to three bins, ``matched``, ``unmatched`` and ``unjudged`` + the reads' extension, gzip'ed unless
--no-gzip-output says otherwise; with BAM input, ``--bam-output`` writes them as BAM files that hold every record whole.
stdout gets four lines: ``#matched reads bases``, ``#unmatched reads bases``, ``#unjudged reads bases`` and
``#rule min_count max_count min_hits min_share min_covered min_stretch``, where min_count is the bound in force (2 at
least for a database kept without the k-mers seen once).  ``--table`` writes one line per read:
``name length clean held covered longest stretches bin``.

No verdict about the library is computed, and no threshold beyond --min-hits 1 is chosen for you.
"""
# Run as ``python -m trio_binning_amd.screen_reads``.  The lookup and the per-read reduction are on the device
# (kmers.DatabaseQuery.evidence); the host applies the rule to five numbers per read and hands the bins to seq.BinWriter.

import argparse
import os
import re
import sys
from fractions import Fraction
from os.path import isfile

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

from . import find_unique_kmers as fu, kmers, seq  # noqa: E402
from .classify_by_kmers import output_extension  # noqa: E402

PROG = "screen_reads"

_BATCH_BASES = int(os.environ.get("TBK_BATCH_BASES", str(64 << 20)))
_BATCH_READS = int(os.environ.get("TBK_BATCH_READS", str(1 << 20)))

BINS = ("matched", "unmatched", "unjudged")
BIN_BYTES = b"ABU"  # what seq.BinWriter.write takes per read: its first, second and third file
TABLE_COLUMNS = ("name", "length", "clean", "held", "covered", "longest", "stretches", "bin")
RULE_COLUMNS = ("#rule", "min_count", "max_count", "min_hits", "min_share", "min_covered", "min_stretch")

_SHARE = re.compile(r"(\d+(\.\d{1,9})?|\.\d{1,9})\Z")


def parse_share(text: str) -> Fraction:
    """A share as the command line gives it: a decimal number in [0, 1] with at most 9 decimals, kept exact.  ``ValueError``
    for anything else - an exponent, a sign, a tenth decimal, a value above 1."""
    if not _SHARE.match(text):
        raise ValueError("{!r} is not a decimal number with at most 9 decimals".format(text))
    share = Fraction(text)
    if not 0 <= share <= 1:
        raise ValueError("{} does not lie in [0, 1]".format(text))
    return share


def _parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog=PROG, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("reads", help="reads to screen, FASTA/FASTQ(.gz) or BAM (unaligned, such as reads.hifi_reads.bam).")
    parser.add_argument("database", help="the count database whose k-mers are looked for (*.tbkdb)")
    parser.add_argument("--min-count", type=int, default=1, metavar="N", help="a window is held from this counter on (1..255; default 1)")
    parser.add_argument("--max-count", type=int, default=255, metavar="N", help="a window is held up to this counter (min-count..255; default 255)")
    parser.add_argument("--min-hits", type=int, default=1, metavar="N", help="matched: at least this many held windows (default 1)")
    parser.add_argument("--min-share", default="0", metavar="F", help="matched: held / clean windows at least this (0..1, at most 9 decimals; default 0)")
    parser.add_argument("--min-covered", default="0", metavar="F", help="matched: covered bases / length at least this (0..1, at most 9 decimals; default 0)")
    parser.add_argument("--min-stretch", type=int, default=0, metavar="N", help="matched: a stretch of at least this many covered bases (default 0)")
    parser.add_argument("--matched-out-prefix", default="matched", help="prefix for the file of matched reads")
    parser.add_argument("--unmatched-out-prefix", default="unmatched", help="prefix for the file of unmatched reads")
    parser.add_argument("--unjudged-out-prefix", default="unjudged", help="prefix for the file of reads without a clean window")
    parser.add_argument("--no-gzip-output", action="store_true", default=False, help="don't gzip the output")
    parser.add_argument("--bam-output", action="store_true", default=False,
                        help="BAM input only: write the bins as BAM files (<prefix>.bam) that hold every read's input record whole")
    parser.add_argument("--table", default=None, metavar="PATH", help="write the evidence: one line per read")
    return parser


def parse_args(argv=None):
    """The arguments, refused where they can be from the command line and the database's header alone; ``args.info`` is that
    header (``kmers.database_file_info``), ``args.share`` and ``args.covered`` are the two shares as ``Fraction`` and
    ``args.threshold`` is the lower counter bound in force.  No device is touched."""
    parser = _parser()
    args = parser.parse_args(argv)
    if not 1 <= args.min_count <= 255:
        parser.error("--min-count {}: need 1 <= N <= 255".format(args.min_count))
    if not args.min_count <= args.max_count <= 255:
        parser.error("--max-count {}: need min-count ({}) <= N <= 255".format(args.max_count, args.min_count))
    for option, value in (("--min-hits", args.min_hits), ("--min-stretch", args.min_stretch)):
        if not 0 <= value < 1 << 63:
            parser.error("{} {}: need 0 <= N < 2^63".format(option, value))
    try:
        args.share = parse_share(args.min_share)
    except ValueError as exc:
        parser.error("--min-share: {}".format(exc))
    try:
        args.covered = parse_share(args.min_covered)
    except ValueError as exc:
        parser.error("--min-covered: {}".format(exc))
    if args.bam_output:
        if not args.reads.endswith(".bam"):
            parser.error("--bam-output keeps BAM records whole: the reads must be a .bam file, not {}".format(args.reads))
        if args.no_gzip_output:
            parser.error("--bam-output and --no-gzip-output exclude each other: BAM bins are bgzf-compressed")
    for what in (args.reads, args.database):
        if not isfile(what):
            sys.exit("{}: {} does not exist or is not a file".format(PROG, what))
    if not fu.is_database_path(args.database):
        sys.exit("{}: {} is not a count database (*{}): a k-mer list holds no counts to screen by - keep a library's database with "
                 "find-unique-kmers --keep-databases, or carve one out with select_database".format(PROG, args.database, fu.DATABASE_SUFFIX))
    try:
        args.info = kmers.database_file_info(args.database)
    except (IOError, ValueError) as exc:
        sys.exit("{}: {}: {}".format(PROG, args.database, exc))
    if args.info["compressed"]:
        sys.exit("{}: {} holds homopolymer-compressed k-mers (find-unique-kmers --compress): coverage along a read is not defined in "
                 "compressed space. Give a plain database.".format(PROG, args.database))
    args.threshold = max(int(args.info["floor"]), args.min_count)
    return args


def decide(records, lengths, min_hits: int = 1, min_share: Fraction = Fraction(0), min_covered: Fraction = Fraction(0), min_stretch: int = 0) -> bytes:
    """The rule: one byte per read for ``seq.BinWriter.write`` - ``U`` (unjudged) for a read without a clean window, else
    ``A`` (matched) when ``held >= min_hits``, ``held / clean >= min_share``, ``covered / length >= min_covered`` and
    ``longest >= min_stretch`` all hold, else ``B`` (unmatched).  ``records`` is a ``kmers.READ_EVIDENCE`` array and ``lengths``
    the reads' lengths; the shares are ``Fraction`` and every comparison is one of integers, cross-multiplied."""
    import numpy as np

    lengths = np.asarray(lengths)
    if lengths.size != records.size:
        raise ValueError("decide: {} records, {} lengths".format(records.size, lengths.size))
    # Python integers where a product might not fit 63 bits (a denominator is 10^9 at most: sequences of 2^33 windows or more)
    limit = (1 << 63) // max(min_share.denominator, min_covered.denominator, min_share.numerator, min_covered.numerator, 1)
    largest = max(int(lengths.max()), int(records["clean"].max())) if records.size else 0
    kind = np.int64 if largest < limit and max(min_hits, min_stretch) < 1 << 63 else object
    clean, held, covered, longest = (records[f].astype(kind) for f in ("clean", "held", "covered", "longest"))
    length = lengths.astype(kind)
    matched = ((held >= min_hits) & (held * min_share.denominator >= min_share.numerator * clean) &
               (covered * min_covered.denominator >= min_covered.numerator * length) & (longest >= min_stretch)).astype(bool)
    bins = np.where(records["clean"] == 0, BIN_BYTES[2], np.where(matched, BIN_BYTES[0], BIN_BYTES[1])).astype(np.uint8)
    return bins.tobytes()


def table_lines(names, lengths, records, bins: bytes) -> str:
    """The --table lines of a batch."""
    word = {code: name for code, name in zip(BIN_BYTES, BINS)}
    return "".join("{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\n".format(
        name, int(length), int(x["clean"]), int(x["held"]), int(x["covered"]), int(x["longest"]), int(x["stretches"]), word[code])
        for name, length, x, code in zip(names, lengths, records, bins))


def summary_lines(tally, args) -> str:
    """stdout: the reads and bases of each bin (``tally``: {bin byte: [reads, bases]}) and the rule that made them."""
    lines = ["#{}\t{}\t{}".format(name, *tally[code]) for code, name in zip(BIN_BYTES, BINS)]
    lines.append("\t".join(["#rule", str(args.threshold), str(args.max_count), str(args.min_hits), args.min_share, args.min_covered,
                            str(args.min_stretch)]))
    return "".join(line + "\n" for line in lines)


def main(argv=None):
    """Main method of program"""
    args = parse_args(argv)
    import numpy as np

    table_tmp = args.table + ".tmp" if args.table else None  # written beside its place and renamed: a run that fails leaves no half a file
    tally = {code: [0, 0] for code in BIN_BYTES}
    gzip_output = not args.no_gzip_output
    level = int(os.environ.get("TBK_GZIP_LEVEL", "-1"))
    prefixes = (args.matched_out_prefix, args.unmatched_out_prefix, args.unjudged_out_prefix)
    try:
        with kmers.KmerDatabase.load(args.database) as database, database.query() as query, open(table_tmp or os.devnull, "w") as table, \
                seq.BatchReader(args.reads, keep_records=args.bam_output) as reader:
            if args.bam_output:  # (BAM output begins with the input's header)
                writer = seq.BinWriter(*prefixes, ".bam", True, level, device=database.device, bam_header=reader.bam_header())
            else:
                writer = seq.BinWriter(*prefixes, output_extension(args.reads), gzip_output, level, device=database.device if gzip_output else None)
            batch = seq.Batch()
            try:
                while reader.next_batch(batch, _BATCH_BASES, _BATCH_READS):
                    bases, base_off, names, name_off = batch.arrays()[:4]
                    records = query.evidence(bases, base_off, args.min_count, args.max_count)
                    lengths = np.diff(base_off.astype(np.int64))
                    bins = decide(records, lengths, args.min_hits, args.share, args.covered, args.min_stretch)
                    writer.write(batch, bins)
                    codes = np.frombuffer(bins, dtype=np.uint8)
                    for code in BIN_BYTES:
                        mine = codes == code
                        tally[code][0] += int(mine.sum())
                        tally[code][1] += int(lengths[mine].sum())
                    if table_tmp:
                        text = bytes(names)
                        table.write(table_lines([text[int(name_off[i]):int(name_off[i + 1])].decode() for i in range(batch.n_reads)],
                                                lengths, records, bins))
                writer.close()
            finally:
                batch.close()
        sys.stdout.write(summary_lines(tally, args))
        sys.stdout.flush()
        if table_tmp:
            os.replace(table_tmp, args.table)
    except BaseException:
        if table_tmp and os.path.exists(table_tmp):
            os.remove(table_tmp)
        raise


if __name__ == "__main__":
    main()
