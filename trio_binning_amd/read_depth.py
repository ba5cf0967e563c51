"""Per-read k-mer depth from a count database: how often the library saw each read's k-mers, and the reads kept, dropped or thinned by it.

Every window of every read of a FASTA/FASTQ(.gz) or BAM file is looked up in one count database (``*.tbkdb``, kept by
find-unique-kmers --keep-databases).  The *depth* of a clean window (ACGT only, either case) is its k-mer's counter when that is
``--min-count`` or more (and 2 or more for a database kept without the k-mers seen once), else 0.  Per read that gives the
``clean`` windows, the ``present`` (depth >= 1) and ``saturated`` (depth 255) ones, the ``sum`` of the depths, and the sorted
depths at the ranks ``j * (clean - 1) // 4``: ``lowest``, ``q1``, ``median`` (the lower one), ``q3`` and ``highest``;
``present_median`` is the lower median over the present windows alone, 0 when there are none - the copy depth of a read most
of whose k-mers carry a sequencing error.  What ``kat sect`` reports, and what BBNorm and khmer's ``normalize-by-median`` and
``filter-abund`` decide by.

A read without a clean window - shorter than k, or an N in every window - is *unjudged*.  For any other read let ``s`` be its
``--by`` statistic (default ``median``).  It is *dropped* when ``s < --min-depth`` or ``s > --max-depth``.  With ``--target T``
a library is thinned evenly to depth T (digital normalisation): a read with ``s > T`` is dropped when ``u * s >= T * 2^32``,
where ``u`` is the upper 32 bits of the ``(i + 1)``-th splitmix64 output from state ``--seed`` and ``i`` the read's 0-based place
in the input file - it is kept with probability T / s, the same reads in every run and for every batch size.  Every other read
is *kept*.  Integers only.

The reads go to three bins, ``kept``, ``dropped`` and ``unjudged`` + the reads' extension, gzip'ed unless --no-gzip-output
says otherwise; with BAM input, ``--bam-output`` writes them as BAM files that hold every record whole.  stdout gets four
lines: ``#kept reads bases``, ``#dropped reads bases``, ``#unjudged reads bases`` and
``#rule min_count by min_depth max_depth target seed``, where min_count is the bound in force and target is ``-`` when none
is given.  ``--table`` writes one line per read:
``name length clean present saturated sum lowest q1 median q3 highest present_median bin``.  ``--spectrum`` writes 256 lines
``depth reads bases kept_reads kept_bases`` over the judged reads by their ``--by`` statistic: the file to choose --min-depth,
--max-depth and --target from, and what a --target run did to the depth distribution.

No verdict about the library is computed, and no threshold is chosen for you.
"""
# Run as ``python -m trio_binning_amd.read_depth``.  The lookup and the per-read reduction are on the device
# (kmers.DatabaseQuery.read_depth); the host applies the rule to one number per read and hands the bins to seq.BinWriter.

import argparse
import os
import sys
from os.path import isfile

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

from . import find_unique_kmers as fu, kmers, seq  # noqa: E402
from .classify_by_kmers import output_extension  # noqa: E402

PROG = "read_depth"

_BATCH_BASES = int(os.environ.get("TBK_BATCH_BASES", str(64 << 20)))
_BATCH_READS = int(os.environ.get("TBK_BATCH_READS", str(1 << 20)))

BINS = ("kept", "dropped", "unjudged")
BIN_BYTES = b"ABU"  # what seq.BinWriter.write takes per read: its first, second and third file
STATISTICS = {"median": "median", "present-median": "present_median", "q1": "q1", "q3": "q3", "lowest": "lowest", "highest": "highest"}
RECORD_COLUMNS = ("clean", "present", "saturated", "sum", "lowest", "q1", "median", "q3", "highest", "present_median")
TABLE_COLUMNS = ("name", "length") + RECORD_COLUMNS + ("bin",)
SPECTRUM_COLUMNS = ("depth", "reads", "bases", "kept_reads", "kept_bases")
RULE_COLUMNS = ("#rule", "min_count", "by", "min_depth", "max_depth", "target", "seed")

_MASK = (1 << 64) - 1


def _parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog=PROG, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("reads", help="reads to measure, FASTA/FASTQ(.gz) or BAM (unaligned, such as reads.hifi_reads.bam).")
    parser.add_argument("database", help="the count database of the library the depths are read from (*.tbkdb)")
    parser.add_argument("--min-count", type=int, default=1, metavar="N", help="a counter below this reads as depth 0 (1..255; default 1)")
    parser.add_argument("--by", choices=sorted(STATISTICS), default="median", help="the statistic the rule looks at (default median)")
    parser.add_argument("--min-depth", type=int, default=0, metavar="N", help="dropped: statistic below this (0..255; default 0)")
    parser.add_argument("--max-depth", type=int, default=255, metavar="N", help="dropped: statistic above this (min-depth..255; default 255)")
    parser.add_argument("--target", type=int, default=None, metavar="N", help="thin the reads above this depth to it (1..255; default: no thinning)")
    parser.add_argument("--seed", type=int, default=None, metavar="N", help="with --target: the state the thinning's numbers start from (0..2^64 - 1; default 0)")
    parser.add_argument("--kept-out-prefix", default="kept", help="prefix for the file of kept reads")
    parser.add_argument("--dropped-out-prefix", default="dropped", help="prefix for the file of dropped reads")
    parser.add_argument("--unjudged-out-prefix", default="unjudged", help="prefix for the file of reads without a clean window")
    parser.add_argument("--no-gzip-output", action="store_true", default=False, help="don't gzip the output")
    parser.add_argument("--bam-output", action="store_true", default=False,
                        help="BAM input only: write the bins as BAM files (<prefix>.bam) that hold every read's input record whole")
    parser.add_argument("--table", default=None, metavar="PATH", help="write the depths: one line per read")
    parser.add_argument("--spectrum", default=None, metavar="PATH", help="write the reads and bases, all and kept, per value of the statistic: 256 lines")
    return parser


def parse_args(argv=None):
    """The arguments, refused where they can be from the command line and the database's header alone; ``args.info`` is that
    header (``kmers.database_file_info``), ``args.threshold`` the lower counter bound in force and ``args.seed`` 0 when none was
    given.  No device is touched."""
    parser = _parser()
    args = parser.parse_args(argv)
    if not 1 <= args.min_count <= 255:
        parser.error("--min-count {}: need 1 <= N <= 255".format(args.min_count))
    if not 0 <= args.min_depth <= 255:
        parser.error("--min-depth {}: need 0 <= N <= 255".format(args.min_depth))
    if not 0 <= args.max_depth <= 255:
        parser.error("--max-depth {}: need 0 <= N <= 255".format(args.max_depth))
    if args.min_depth > args.max_depth:
        parser.error("--min-depth {} is above --max-depth {}: every read would be dropped".format(args.min_depth, args.max_depth))
    if args.target is not None and not 1 <= args.target <= 255:
        parser.error("--target {}: need 1 <= N <= 255".format(args.target))
    if args.seed is not None:
        if args.target is None:
            parser.error("--seed without --target: nothing is thinned, so nothing is drawn")
        if not 0 <= args.seed <= _MASK:
            parser.error("--seed {}: need 0 <= N < 2^64".format(args.seed))
    else:
        args.seed = 0
    if args.bam_output:
        if not args.reads.endswith(".bam"):
            parser.error("--bam-output keeps BAM records whole: the reads must be a .bam file, not {}".format(args.reads))
        if args.no_gzip_output:
            parser.error("--bam-output and --no-gzip-output exclude each other: BAM bins are bgzf-compressed")
    for what in (args.reads, args.database):
        if not isfile(what):
            sys.exit("{}: {} does not exist or is not a file".format(PROG, what))
    if not fu.is_database_path(args.database):
        sys.exit("{}: {} is not a count database (*{}): a k-mer list holds no counts to read a depth from - keep a library's database with "
                 "find-unique-kmers --keep-databases".format(PROG, args.database, fu.DATABASE_SUFFIX))
    try:
        args.info = kmers.database_file_info(args.database)
    except (IOError, ValueError) as exc:
        sys.exit("{}: {}: {}".format(PROG, args.database, exc))
    if args.info["compressed"]:
        sys.exit("{}: {} holds homopolymer-compressed k-mers (find-unique-kmers --compress): the depth of a read in compressed space is out "
                 "of scope here. Give a plain database.".format(PROG, args.database))
    args.threshold = max(int(args.info["floor"]), args.min_count)
    return args


def draws(seed: int, ordinals):
    """``u(seed, i)`` for every ``i`` of ``ordinals``: the upper 32 bits of the ``(i + 1)``-th splitmix64 output from state ``seed``,
    as a uint64 array.  numpy's uint64 arithmetic is arithmetic mod 2^64."""
    import numpy as np

    i = np.asarray(ordinals, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = np.uint64(seed & _MASK) + (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x >> np.uint64(32)


def decide(records, ordinals, by: str = "median", min_depth: int = 0, max_depth: int = 255, target=None, seed: int = 0) -> bytes:
    """The rule: one byte per read for ``seq.BinWriter.write`` - ``U`` (unjudged) for a read without a clean window; else, with
    ``s`` the read's ``by`` statistic (a key of ``STATISTICS``), ``B`` (dropped) when ``s < min_depth`` or ``s > max_depth`` or,
    with a ``target`` T, when ``s > T`` and ``u * s >= T * 2^32``, ``u = draws(seed, ordinal)``; else ``A`` (kept).  ``records``
    is a ``kmers.READ_DEPTH`` array and ``ordinals`` the reads' 0-based places in the input file, so the answer does not depend
    on how the file is cut into batches.  Every comparison is one of integers: ``u * s < 2^40``.
    A read with ``s = 255`` is thinned as if its depth were 255: the counter stops there, so that is a lower bound on the
    thinning the read deserves."""
    import numpy as np

    ordinals = np.asarray(ordinals, dtype=np.uint64)
    if ordinals.size != records.size:
        raise ValueError("decide: {} records, {} ordinals".format(records.size, ordinals.size))
    s = records[STATISTICS[by]].astype(np.uint64)
    dropped = (s < np.uint64(min_depth)) | (s > np.uint64(max_depth))
    if target is not None:
        dropped |= (s > np.uint64(target)) & (draws(seed, ordinals) * s >= np.uint64(int(target) << 32))
    bins = np.where(records["clean"] == 0, BIN_BYTES[2], np.where(dropped, BIN_BYTES[1], BIN_BYTES[0])).astype(np.uint8)
    return bins.tobytes()


def table_lines(names, lengths, records, bins: bytes) -> str:
    """The --table lines of a batch."""
    word = {code: name for code, name in zip(BIN_BYTES, BINS)}
    return "".join("\t".join([name, str(int(length))] + [str(int(x[f])) for f in RECORD_COLUMNS] + [word[code]]) + "\n"
                   for name, length, x, code in zip(names, lengths, records, bins))


def spectrum_rows(records, lengths, bins: bytes, by: str = "median"):
    """(256, 4) int64 of a batch: per value of the ``by`` statistic the judged reads and their bases, and the kept ones of them.
    The batches' rows add up."""
    import numpy as np

    codes = np.frombuffer(bins, dtype=np.uint8)
    s = records[STATISTICS[by]].astype(np.int64)
    lengths = np.asarray(lengths).astype(np.int64)
    rows = np.zeros((256, 4), dtype=np.int64)
    for column, mine in ((0, codes != BIN_BYTES[2]), (2, codes == BIN_BYTES[0])):
        np.add.at(rows[:, column], s[mine], 1)
        np.add.at(rows[:, column + 1], s[mine], lengths[mine])  # (integers: bincount's weights would be floats)
    return rows


def spectrum_lines(rows) -> str:
    """The --spectrum file from the summed ``spectrum_rows``: 256 lines ``depth reads bases kept_reads kept_bases``."""
    return "".join("{}\t{}\t{}\t{}\t{}\n".format(d, *(int(v) for v in rows[d])) for d in range(256))


def summary_lines(tally, args) -> str:
    """stdout: the reads and bases of each bin (``tally``: {bin byte: [reads, bases]}) and the rule that made them."""
    lines = ["#{}\t{}\t{}".format(name, *tally[code]) for code, name in zip(BIN_BYTES, BINS)]
    lines.append("\t".join(["#rule", str(args.threshold), args.by, str(args.min_depth), str(args.max_depth),
                            "-" if args.target is None else str(args.target), str(args.seed)]))
    return "".join(line + "\n" for line in lines)


def main(argv=None):
    """Main method of program"""
    args = parse_args(argv)
    import numpy as np

    # the side files are written beside their places and renamed: a run that fails leaves no half a file
    table_tmp = args.table + ".tmp" if args.table else None
    spectrum_tmp = args.spectrum + ".tmp" if args.spectrum else None
    tally = {code: [0, 0] for code in BIN_BYTES}
    spectrum = np.zeros((256, 4), dtype=np.int64)
    seen = 0  # reads before this batch: a read's ordinal in the input file
    gzip_output = not args.no_gzip_output
    level = int(os.environ.get("TBK_GZIP_LEVEL", "-1"))
    prefixes = (args.kept_out_prefix, args.dropped_out_prefix, args.unjudged_out_prefix)
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
                    records = query.read_depth(bases, base_off, args.min_count)
                    lengths = np.diff(base_off.astype(np.int64))
                    ordinals = np.arange(seen, seen + batch.n_reads, dtype=np.uint64)
                    seen += batch.n_reads
                    bins = decide(records, ordinals, args.by, args.min_depth, args.max_depth, args.target, args.seed)
                    writer.write(batch, bins)
                    codes = np.frombuffer(bins, dtype=np.uint8)
                    for code in BIN_BYTES:
                        mine = codes == code
                        tally[code][0] += int(mine.sum())
                        tally[code][1] += int(lengths[mine].sum())
                    spectrum += spectrum_rows(records, lengths, bins, args.by)
                    if table_tmp:
                        text = bytes(names)
                        table.write(table_lines([text[int(name_off[i]):int(name_off[i + 1])].decode() for i in range(batch.n_reads)],
                                                lengths, records, bins))
                writer.close()
            finally:
                batch.close()
        if spectrum_tmp:
            with open(spectrum_tmp, "w") as out:
                out.write(spectrum_lines(spectrum))
        sys.stdout.write(summary_lines(tally, args))
        sys.stdout.flush()
        if table_tmp:
            os.replace(table_tmp, args.table)
        if spectrum_tmp:
            os.replace(spectrum_tmp, args.spectrum)
    except BaseException:
        for tmp in (table_tmp, spectrum_tmp):
            if tmp and os.path.exists(tmp):
                os.remove(tmp)
        raise


if __name__ == "__main__":
    main()
