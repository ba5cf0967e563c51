"""Score an assembly against a k-mer count database of the reads: consensus quality (QV), k-mer completeness, spectrum.

Every window of every sequence of a FASTA/FASTQ file is looked up in one count database (``*.tbkdb``, as kept by
find-unique-kmers --keep-databases).  stdout gets one TSV line per sequence - ``name length clean found qv`` - and a last
line ``#total length clean found qv seen solid completeness error_rate``: ``clean`` windows hold ACGT only (either
case), ``found`` ones are k-mers the reads hold at least --min-count times, ``qv = -10 log10(1 - (found / clean) ** (1 / k))``,
``error_rate = 1 - (found / clean) ** (1 / k)``, ``solid`` is the number of the database's k-mers with a counter in
[--min-count, --max-count], ``seen`` those of them the assembly holds, ``completeness = seen / solid``.

Floats have a fixed format: ``qv`` four decimals (``inf`` when every clean window is found, ``nan`` without a clean
window), ``completeness`` six decimals (``nan`` when nothing is solid), ``error_rate`` six significant digits as
``d.ddddde-xx`` (``nan`` without a clean window).

Merqury counts presence: a k-mer the reads hold once is found.  A database kept with find-unique-kmers --keep-singletons (a
full one) holds those k-mers, and ``--min-count 1`` then is Merqury's definition.  A database kept without the flag holds only
k-mers the reads hold at least twice (kmc's -ci2): there a k-mer seen once counts as absent, --min-count starts at 2 and the
QV is a lower bound of Merqury's at the same k.
"""
# Run as ``python -m trio_binning_amd.assembly_qv``.  The lookup is on the device (kmers.DatabaseQuery: a directory over the
# database's ranks, one wave per 2048 window starts); the QV arithmetic, the absent stretches and the tables run on the host.
# A session takes at most 2^32 - 1 window starts: a larger assembly ends with the library's message.

import argparse
import os
import sys
from os.path import isfile

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

from . import find_unique_kmers as fu, kmers, seq  # noqa: E402

PROG = "assembly_qv"

# Whole records, as for phase_blocks: a record longer than the limit arrives alone in a batch of its own length.
_BATCH_BASES = int(os.environ.get("TBK_BATCH_BASES", str(64 << 20)))
_BATCH_READS = int(os.environ.get("TBK_BATCH_READS", str(1 << 20)))

TSV_COLUMNS = ("name", "length", "clean", "found", "qv")
TOTAL_COLUMNS = ("#total", "length", "clean", "found", "qv", "seen", "solid", "completeness", "error_rate")
COPY_LABELS = ("0", "1", "2", "3", "4", ">4")


def _parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog=PROG, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("assembly", help="contigs (or reads) to score, FASTA/FASTQ(.gz) or BAM.")
    parser.add_argument("database", help="the count database of the reads (*.tbkdb, kept by find-unique-kmers --keep-databases)")
    parser.add_argument("--min-count", type=int, default=2, metavar="N",
                        help="the counter a k-mer needs to count as found, and as solid for completeness (2..255; default 2). "
                             "1 - presence, Merqury's definition - needs a full database, kept with find-unique-kmers --keep-singletons")
    parser.add_argument("--max-count", type=int, default=255, metavar="N", help="completeness only: the largest counter of a solid k-mer (2..255; default 255)")
    parser.add_argument("--spectrum", default=None, metavar="PATH",
                        help="write the copy spectrum: one line 'counter copies kmers' per non-empty cell, copies 0..4 and >4 "
                             "(takes 4 bytes more per k-mer of the database on the device)")
    parser.add_argument("--absent-bed", default=None, metavar="PATH",
                        help="write one BED line per maximal stretch of consecutive clean windows that were not found - name, start, "
                             "end + k, windows - the loci of likely consensus errors")
    return parser


def parse_args(argv=None):
    """The arguments, refused where they can be from the command line and the database's header alone; ``args.info`` is
    that header (``kmers.database_file_info``).  No device is touched."""
    parser = _parser()
    args = parser.parse_args(argv)
    presence = args.min_count == 1  # k-mers seen once count as found: only a full database holds them (checked below, by its header)
    for name in ("min_count", "max_count"):
        if not 2 <= getattr(args, name) <= 255 and not (name == "min_count" and presence):
            parser.error("--{} {}: need 2 <= N <= 255".format(name.replace("_", "-"), getattr(args, name)))
    if args.min_count > args.max_count:
        parser.error("--min-count {} is larger than --max-count {}".format(args.min_count, args.max_count))
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
        sys.exit("{}: {} holds homopolymer-compressed k-mers (find-unique-kmers --compress): a QV is not defined in compressed "
                 "space. Give a plain database.".format(PROG, args.database))
    if presence and args.info["floor"] != 1:
        parser.error("--min-count 1: need 2 <= N <= 255 with this database, which was kept without the k-mers seen once; keep it "
                     "with find-unique-kmers --keep-databases --keep-singletons to count presence")
    return args


def format_qv(found: int, clean: int, k: int) -> str:
    return "{:.4f}".format(kmers.qv(found, clean, k))


def format_error_rate(found: int, clean: int, k: int) -> str:
    if clean == 0:
        return "nan"
    return "{:.5e}".format(1.0 - (found / clean) ** (1.0 / k) if found < clean else 0.0)


def format_completeness(seen: int, solid: int) -> str:
    return "{:.6f}".format(seen / solid) if solid else "nan"


def clean_windows(bases, k: int):
    """bool per window start 0 .. len - k of one sequence's bytes: the k bases are all ACGT, either case."""
    import numpy as np

    bases = np.asarray(bases, dtype=np.uint8)
    n = bases.size - k + 1
    if n <= 0:
        return np.zeros(0, dtype=bool)
    bad = np.zeros(bases.size + 1, dtype=np.int64)
    np.cumsum(~np.isin(bases, np.frombuffer(b"ACGTacgt", dtype=np.uint8)), out=bad[1:])
    return bad[k:k + n] == bad[:n]


def absent_stretches(counts, clean):
    """(first, last) window starts of every maximal stretch of consecutive clean windows whose counter is 0, as two int64
    arrays.  ``counts``: ``DatabaseQuery.counts`` of one sequence, at least as long as ``clean``."""
    import numpy as np

    clean = np.asarray(clean, dtype=bool)
    absent = clean & (np.asarray(counts)[:clean.size] == 0)
    edge = np.diff(np.concatenate(([0], absent.astype(np.int8), [0])))
    return np.flatnonzero(edge == 1).astype(np.int64), np.flatnonzero(edge == -1).astype(np.int64) - 1


def spectrum_lines(spec) -> str:
    """The --spectrum table of ``DatabaseQuery.copy_spectrum``: 'counter copies kmers' per non-empty cell, by counter, then copies."""
    return "".join("{}\t{}\t{}\n".format(c, COPY_LABELS[m], int(spec[m][c])) for c in range(256) for m in range(6) if int(spec[m][c]))


def main(argv=None):
    """Main method of program"""
    args = parse_args(argv)
    import numpy as np

    k = args.info["k"]
    bed_tmp = args.absent_bed + ".tmp" if args.absent_bed else None  # written beside their places and renamed: a run that fails leaves no half a file
    spectrum_tmp = args.spectrum + ".tmp" if args.spectrum else None
    out = sys.stdout
    total = [0, 0, 0]  # length, clean, found
    try:
        with kmers.KmerDatabase.load(args.database) as database, database.query(copies=args.spectrum is not None) as query, \
                seq.BatchReader(args.assembly) as reader, open(bed_tmp or os.devnull, "w") as bed:
            batch = seq.Batch()
            try:
                while reader.next_batch(batch, _BATCH_BASES, _BATCH_READS):
                    bases, base_off, names, name_off = batch.arrays()[:4]
                    n = batch.n_reads
                    if bed_tmp:
                        per_read, counts = query.add(bases, base_off, args.min_count, return_counts=True)
                    else:
                        per_read = query.add(bases, base_off, args.min_count)
                    text = bytes(names)
                    label = [text[int(name_off[i]):int(name_off[i + 1])].decode() for i in range(n)]
                    off = base_off.astype(np.int64)
                    lines = []
                    for i in range(n):
                        length, clean, found = int(off[i + 1] - off[i]), int(per_read[i, 0]), int(per_read[i, 1])
                        lines.append("{}\t{}\t{}\t{}\t{}\n".format(label[i], length, clean, found, format_qv(found, clean, k)))
                        total[0] += length; total[1] += clean; total[2] += found
                        if bed_tmp and clean:
                            part = slice(int(off[i]), int(off[i + 1]))
                            first, last = absent_stretches(counts[part], clean_windows(np.asarray(bases)[part], k))
                            bed.write("".join("{}\t{}\t{}\t{}\n".format(label[i], int(a), int(b) + k, int(b - a + 1)) for a, b in zip(first, last)))
                    out.write("".join(lines))
            finally:
                batch.close()
            seen, solid = query.completeness(args.min_count, args.max_count)
            if spectrum_tmp:
                with open(spectrum_tmp, "w") as fh:
                    fh.write(spectrum_lines(query.copy_spectrum()))
        out.write("\t".join(["#total", str(total[0]), str(total[1]), str(total[2]), format_qv(total[2], total[1], k), str(seen), str(solid),
                             format_completeness(seen, solid), format_error_rate(total[2], total[1], k)]) + "\n")
        out.flush()
        if bed_tmp:
            os.replace(bed_tmp, args.absent_bed)
        if spectrum_tmp:
            os.replace(spectrum_tmp, args.spectrum)
    except BaseException:
        for tmp in (bed_tmp, spectrum_tmp):
            if tmp and os.path.exists(tmp):
                os.remove(tmp)
        raise


if __name__ == "__main__":
    main()
