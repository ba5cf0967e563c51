"""Trim reads by a k-mer count database: keep the stretches its k-mers vouch for, or cut out the stretches it holds.

Every window of every read of a FASTA/FASTQ(.gz) or BAM file is looked up in one count database (``*.tbkdb``: a library's own,
kept by find-unique-kmers --keep-databases, or a part of one carved out by select_database or import_database - adapters, PhiX, an
organelle, a contaminant).  A clean window (ACGT only, either case) is *held* when the database holds its k-mer with a counter in
``[--min-count, --max-count]``; a base is *covered* when it lies in a held window.  A *piece* is a maximal run of consecutive
bases of one read that are covered (``--keep covered``, the default: error-trimming by a library's solid k-mers, as khmer's
trim-low-abund and BBDuk's ktrim do) or that are not (``--keep uncovered``: what is left of a read around an adapter or a foreign
stretch, as BBDuk's kmask and a split do).  Pieces shorter than ``--min-length`` are left out, and with ``--pieces longest``, the
default, only a read's longest piece stays - the first among equals; ``--pieces all`` keeps every one, which is how a chimeric
read is split at a foreign stretch.

A read without a clean window - shorter than k, or an N in every window - is *unjudged* and goes whole to ``unjudged``, on either
side.  A read with a clean window and at least one piece goes to ``kept`` as its pieces, in order; every other read goes whole to
``dropped``, so nothing vanishes.  The three files are the prefixes + the reads' extension, gzip'ed unless --no-gzip-output says
otherwise; BAM records come out as FASTQ text.  A piece is its record cut to ``[first, end)``, sequence and quality both.  With
``--pieces all`` a piece that is not its whole record is named ``name:F-E``, 1-based and closed as samtools faidx names a region;
with ``--pieces longest`` names stay as they came.

stdout gets five lines: ``#kept reads pieces bases``, ``#dropped reads bases``, ``#unjudged reads bases``, ``#cut bases`` - the
bases of kept reads that lie in no written piece - and ``#rule min_count max_count keep pieces min_length``, where min_count is
the bound in force (2 at least for a database kept without the k-mers seen once).  ``--table`` writes one line per read:
``name length clean held covered pieces kept_bases bin``; ``--bed`` one line per kept piece: ``name first end``, 0-based and
half-open.

No verdict about the library is computed.
"""
# Run as ``python -m trio_binning_amd.trim_reads``.  The lookup, the per-read evidence and the list of pieces are made on the
# device (kmers.DatabaseQuery.pieces); the host chooses a bin per read and seq.BinWriter.write_pieces cuts the records.

import argparse
import os
import sys
from os.path import isfile

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

from . import find_unique_kmers as fu, kmers, seq  # noqa: E402
from .classify_by_kmers import output_extension  # noqa: E402

PROG = "trim_reads"

_BATCH_BASES = int(os.environ.get("TBK_BATCH_BASES", str(64 << 20)))
_BATCH_READS = int(os.environ.get("TBK_BATCH_READS", str(1 << 20)))

BINS = ("kept", "dropped", "unjudged")
BIN_BYTES = b"ABU"  # what seq.BinWriter.write_pieces takes per read: its first, second and third file
TABLE_COLUMNS = ("name", "length", "clean", "held", "covered", "pieces", "kept_bases", "bin")
RULE_COLUMNS = ("#rule", "min_count", "max_count", "keep", "pieces", "min_length")


def _parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog=PROG, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("reads", help="reads to trim, FASTA/FASTQ(.gz) or BAM (unaligned, such as reads.hifi_reads.bam).")
    parser.add_argument("database", help="the count database whose k-mers are looked for (*.tbkdb)")
    parser.add_argument("--min-count", type=int, default=1, metavar="N", help="a window is held from this counter on (1..255; default 1)")
    parser.add_argument("--max-count", type=int, default=255, metavar="N", help="a window is held up to this counter (min-count..255; default 255)")
    parser.add_argument("--keep", choices=sorted(kmers.PIECES_SIDES), default="covered", help="the side of a read that is kept (default covered)")
    parser.add_argument("--pieces", choices=sorted(kmers.PIECES_WHICH), default="longest", help="a read's longest piece, or all of them (default longest)")
    parser.add_argument("--min-length", type=int, default=1, metavar="N", help="leave out pieces of fewer bases (default 1)")
    parser.add_argument("--kept-out-prefix", default="kept", help="prefix for the file of pieces")
    parser.add_argument("--dropped-out-prefix", default="dropped", help="prefix for the file of reads without a piece")
    parser.add_argument("--unjudged-out-prefix", default="unjudged", help="prefix for the file of reads without a clean window")
    parser.add_argument("--no-gzip-output", action="store_true", default=False, help="don't gzip the output")
    parser.add_argument("--table", default=None, metavar="PATH", help="write one line per read")
    parser.add_argument("--bed", default=None, metavar="PATH", help="write one line per kept piece: name first end")
    return parser


def parse_args(argv=None):
    """The arguments, refused where they can be from the command line and the database's header alone; ``args.info`` is that
    header (``kmers.database_file_info``) and ``args.threshold`` the lower counter bound in force.  No device is touched."""
    parser = _parser()
    args = parser.parse_args(argv)
    if not 1 <= args.min_count <= 255:
        parser.error("--min-count {}: need 1 <= N <= 255".format(args.min_count))
    if not args.min_count <= args.max_count <= 255:
        parser.error("--max-count {}: need min-count ({}) <= N <= 255".format(args.max_count, args.min_count))
    if not 1 <= args.min_length < 1 << 63:
        parser.error("--min-length {}: need 1 <= N < 2^63".format(args.min_length))
    for what in (args.reads, args.database):
        if not isfile(what):
            sys.exit("{}: {} does not exist or is not a file".format(PROG, what))
    if not fu.is_database_path(args.database):
        sys.exit("{}: {} is not a count database (*{}): a k-mer list holds no counts to trim by - keep a library's database with "
                 "find-unique-kmers --keep-databases, or carve one out with select_database".format(PROG, args.database, fu.DATABASE_SUFFIX))
    try:
        args.info = kmers.database_file_info(args.database)
    except (IOError, ValueError) as exc:
        sys.exit("{}: {}: {}".format(PROG, args.database, exc))
    if args.info["compressed"]:
        sys.exit("{}: {} holds homopolymer-compressed k-mers (find-unique-kmers --compress): the coordinates of a piece are not defined in "
                 "compressed space. Give a plain database.".format(PROG, args.database))
    args.threshold = max(int(args.info["floor"]), args.min_count)
    return args


def decide(evidence, pieces):
    """(bins, kept): one byte per read for ``seq.BinWriter.write_pieces`` - ``U`` (unjudged) for a read without a clean window,
    else ``A`` (kept) for a read with a piece and ``B`` (dropped) for one without - and the pieces of the ``A`` reads.
    ``evidence`` is a ``kmers.READ_EVIDENCE`` array, ``pieces`` a ``kmers.READ_PIECE`` array ordered by (read, first)."""
    import numpy as np

    has = np.zeros(evidence.size, dtype=bool)
    has[pieces["read"].astype(np.int64)] = True
    bins = np.where(evidence["clean"] == 0, BIN_BYTES[2], np.where(has, BIN_BYTES[0], BIN_BYTES[1])).astype(np.uint8)
    kept = pieces[bins[pieces["read"].astype(np.int64)] == BIN_BYTES[0]]
    return bins.tobytes(), kept


def per_read(kept, n_reads):
    """(pieces, kept bases) per read of the batch, two int64 arrays, from the kept pieces"""
    import numpy as np

    reads = kept["read"].astype(np.int64)
    count = np.bincount(reads, minlength=n_reads).astype(np.int64)
    total = np.zeros(n_reads, dtype=np.int64)
    np.add.at(total, reads, (kept["end"] - kept["first"]).astype(np.int64))
    return count, total


def table_lines(names, lengths, evidence, count, total, bins: bytes) -> str:
    """The --table lines of a batch."""
    word = {code: name for code, name in zip(BIN_BYTES, BINS)}
    return "".join("{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\n".format(
        name, int(length), int(x["clean"]), int(x["held"]), int(x["covered"]), int(c), int(t), word[code])
        for name, length, x, c, t, code in zip(names, lengths, evidence, count, total, bins))


def bed_lines(names, kept) -> str:
    """The --bed lines of a batch."""
    return "".join("{}\t{}\t{}\n".format(names[int(p["read"])], int(p["first"]), int(p["end"])) for p in kept)


def summary_lines(tally, pieces: int, kept_bases: int, args) -> str:
    """stdout: the reads and bases of each bin (``tally``: {bin byte: [reads, bases]}), the pieces and the bases kept, the bases
    cut off kept reads, and the rule that made them."""
    kept, dropped, unjudged = (tally[code] for code in BIN_BYTES)
    lines = ["#kept\t{}\t{}\t{}".format(kept[0], pieces, kept_bases), "#dropped\t{}\t{}".format(*dropped), "#unjudged\t{}\t{}".format(*unjudged),
             "#cut\t{}".format(kept[1] - kept_bases),
             "\t".join(["#rule", str(args.threshold), str(args.max_count), args.keep, args.pieces, str(args.min_length)])]
    return "".join(line + "\n" for line in lines)


def main(argv=None):
    """Main method of program"""
    args = parse_args(argv)
    import numpy as np

    # written beside their places and renamed: a run that fails leaves no half a file
    table_tmp = args.table + ".tmp" if args.table else None
    bed_tmp = args.bed + ".tmp" if args.bed else None
    tally = {code: [0, 0] for code in BIN_BYTES}
    n_pieces = kept_bases = 0
    gzip_output = not args.no_gzip_output
    level = int(os.environ.get("TBK_GZIP_LEVEL", "-1"))
    prefixes = (args.kept_out_prefix, args.dropped_out_prefix, args.unjudged_out_prefix)
    suffix = args.pieces == "all"
    try:
        with kmers.KmerDatabase.load(args.database) as database, database.query() as query, open(table_tmp or os.devnull, "w") as table, \
                open(bed_tmp or os.devnull, "w") as bed, seq.BatchReader(args.reads) as reader:
            writer = seq.BinWriter(*prefixes, output_extension(args.reads), gzip_output, level, device=database.device if gzip_output else None)
            batch = seq.Batch()
            try:
                while reader.next_batch(batch, _BATCH_BASES, _BATCH_READS):
                    bases, base_off, names, name_off = batch.arrays()[:4]
                    pieces, evidence = query.pieces(bases, base_off, args.min_count, args.max_count, args.keep, args.pieces, args.min_length, evidence=True)
                    lengths = np.diff(base_off.astype(np.int64))
                    bins, kept = decide(evidence, pieces)
                    writer.write_pieces(batch, kept, bins, suffix)
                    count, total = per_read(kept, batch.n_reads)
                    codes = np.frombuffer(bins, dtype=np.uint8)
                    for code in BIN_BYTES:
                        mine = codes == code
                        tally[code][0] += int(mine.sum())
                        tally[code][1] += int(lengths[mine].sum())
                    n_pieces += int(kept.size)
                    kept_bases += int(total.sum())
                    if table_tmp or bed_tmp:
                        text = bytes(names)
                        read_names = [text[int(name_off[i]):int(name_off[i + 1])].decode() for i in range(batch.n_reads)]
                        if table_tmp:
                            table.write(table_lines(read_names, lengths, evidence, count, total, bins))
                        if bed_tmp:
                            bed.write(bed_lines(read_names, kept))
                writer.close()
            finally:
                batch.close()
        sys.stdout.write(summary_lines(tally, n_pieces, kept_bases, args))
        sys.stdout.flush()
        for tmp, path in ((table_tmp, args.table), (bed_tmp, args.bed)):
            if tmp:
                os.replace(tmp, path)
    except BaseException:
        for tmp in (table_tmp, bed_tmp):
            if tmp and os.path.exists(tmp):
                os.remove(tmp)
        raise


if __name__ == "__main__":
    main()
