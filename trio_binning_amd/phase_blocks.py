"""Locate haplotype k-mer hits along sequences and report phase blocks.

For every sequence of a FASTA/FASTQ file (contigs or reads) this prints where the k-mers unique to
haplotype A and to haplotype B lie: one TSV line per sequence on stdout and one BED line per phase
block in a file.  A block is a stretch of the sequence whose markers are all of one haplotype.
"""
# Run as ``python -m trio_binning_amd.phase_blocks``.  The two k-mer arguments are what classify-by-kmers takes - two
# text lists or two count databases, settled by its own code and refused in its own words - and a sequence's marker
# columns are the counts classify-by-kmers scores it by.  The positions come from the hit tracker (kmers.HitTracker:
# marking and run extraction on the device); the block rule (kmers.phase_blocks) and the tables run on the host.
# With --compress the markers are looked for in homopolymer-compressed space (lists or databases made with
# find-unique-kmers --compress) and every coordinate is lifted back on the device: the outputs speak the coordinates of
# the sequence as given, and a block covers [first, end) - its last window's end, which takes the trailing run with it.

import argparse
import os
import sys
from os.path import isfile

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

from . import classify_by_kmers as cbk, kmers, seq  # noqa: E402

PROG = "phase_blocks"

# Sequences come in whole records: the reader closes a batch behind the record that reaches a limit, so a record
# longer than _BATCH_BASES arrives whole, alone in a batch of its own length (tbk_fastx_next never splits or truncates
# one); the device buffers then grow to it, and a sequence they cannot hold ends the run with the library's message.
_BATCH_BASES = int(os.environ.get("TBK_BATCH_BASES", str(64 << 20)))
_BATCH_READS = int(os.environ.get("TBK_BATCH_READS", str(1 << 20)))

TSV_COLUMNS = ("name", "length", "markers_a", "markers_b", "blocks", "switches", "bases_in_a_blocks", "bases_in_b_blocks", "longest_block")


def _parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog=PROG, description=__doc__, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("sequences", help="contigs or reads to locate the k-mers in, FASTA/FASTQ(.gz) or BAM.")
    parser.add_argument(
        "haplotype_a_kmers", metavar="hapA",
        help="a list of k-mers unique to haplotype A, one per line; or the count database of that parent kept by "
             "find-unique-kmers --keep-databases (*.tbkdb; then both parents must be databases)",
    )
    parser.add_argument("haplotype_b_kmers", metavar="hapB", help="a list of k-mers unique to haplotype B, one per line; or that parent's count database (*.tbkdb)")
    parser.add_argument("--bed", default="phase_blocks.bed", metavar="PATH", help="file for the blocks, one BED line each: name, start, end, A|B, markers")
    parser.add_argument(
        "--min-run", type=int, default=1, metavar="N",
        help="drop every raw run (consecutive markers of one haplotype) of fewer than N markers, once, then merge the neighbours "
             "that are left and agree. An error k-mer hits as one isolated window, a real variant as up to k neighbouring ones. "
             "This is this project's rule, not Merqury's short-range-switch rule",
    )
    parser.add_argument("--ignore-case", action="store_true", default=False,
                        help="read lower-case acgt (soft-masked sequence) as upper-case; by default they are not ACGT, as for classify-by-kmers")
    parser.add_argument(
        "--compress", action="store_true", default=False,
        help="k-mer lists or count databases made by find-unique-kmers --compress: markers are looked for in the sequence with every "
             "run of equal bases written once, and reported at the coordinates of the sequence as given. A block then runs from the "
             "first base of its first marker's window to the end of its last marker's window, homopolymer runs included; the marker "
             "columns are what classify-by-kmers counts in compressed mode",
    )
    cbk._add_database_options(parser)
    return parser


def parse_args(argv=None):
    """The arguments, refused where they can be from the command line and the files' headers alone; ``args.databases`` is the
    settled pair of count databases, or None when two text lists were given."""
    parser = _parser()
    args = parser.parse_args(argv)
    if args.min_run < 1:
        parser.error("--min-run {}: need 1 <= N".format(args.min_run))
    is_db = cbk._check_kmer_arguments(parser, args, PROG)
    for what in (args.sequences, args.haplotype_a_kmers, args.haplotype_b_kmers, args.child_database):
        if what is not None and not isfile(what):
            sys.exit("{}: {} does not exist or is not a file".format(PROG, what))
    args.databases = cbk._settle_databases(args, PROG) if is_db else None
    if args.databases is None:
        if args.compress:
            for list_path in (args.haplotype_a_kmers, args.haplotype_b_kmers):
                cbk.check_compressed_list(list_path, PROG)
    elif args.databases.compressed and not args.compress:
        # (the outputs change meaning with compression, so the switch is explicit here and does not follow the headers)
        sys.exit(PROG + ": {} and {} hold homopolymer-compressed k-mers (find-unique-kmers --compress): their markers lie in compressed "
                 "space. Give --compress to look for them there and report the positions along the sequence as given, or give plain "
                 "databases.".format(args.haplotype_a_kmers, args.haplotype_b_kmers))
    elif args.compress and not args.databases.compressed:
        sys.exit(PROG + ": --compress was given, but {} and {} hold plain (uncompressed) k-mers: count the parents with "
                 "find-unique-kmers --compress".format(args.haplotype_a_kmers, args.haplotype_b_kmers))
    return args


def block_ends(blocks, k: int):
    """One past the last base of every block: last + k, or - of lifted blocks (--compress) - the end of the last window."""
    import numpy as np

    return blocks["end"] if "end" in blocks.dtype.names else blocks["last"] + np.uint64(k)


def sequence_rows(n_reads: int, lengths, counts, blocks, k: int):
    """The TSV columns behind the name for every sequence of a batch, as integer arrays: length, markers_a, markers_b,
    blocks, switches, bases_in_a_blocks, bases_in_b_blocks, longest_block.  A block's extent in bases is last + k - first;
    a lifted block's (--compress) is end - first."""
    import numpy as np

    read = blocks["read"].astype(np.int64)
    extent = (block_ends(blocks, k) - blocks["first"]).astype(np.int64)
    n_blocks = np.bincount(read, minlength=n_reads).astype(np.int64)
    in_hap = np.zeros((2, n_reads), dtype=np.int64)
    np.add.at(in_hap, (blocks["hap"].astype(np.int64), read), extent)
    longest = np.zeros(n_reads, dtype=np.int64)
    np.maximum.at(longest, read, extent)
    return (np.asarray(lengths, dtype=np.int64), counts[:, 0].astype(np.int64), counts[:, 1].astype(np.int64), n_blocks,
            np.maximum(n_blocks - 1, 0), in_hap[0], in_hap[1], longest)


def main(argv=None):
    """Main method of program"""
    args = parse_args(argv)
    if args.databases is not None:
        hap_a, hap_b = args.databases.load()
    else:
        hap_a, hap_b = kmers.create_kmer_hash_set(args.haplotype_a_kmers), kmers.create_kmer_hash_set(args.haplotype_b_kmers)
    import numpy as np

    bed_tmp = args.bed + ".tmp"  # written beside its place and renamed, like the databases: a run that fails leaves no half a file
    out = sys.stdout
    try:
        with kmers.HitTracker(hap_a, hap_b) as tracker, seq.BatchReader(args.sequences) as reader, open(bed_tmp, "w") as bed:
            k = tracker.k
            batch = seq.Batch()
            try:
                while reader.next_batch(batch, _BATCH_BASES, _BATCH_READS):
                    bases, base_off, names, name_off = batch.arrays()[:4]
                    n = batch.n_reads
                    runs, counts = tracker.runs(bases, base_off, args.ignore_case, compress=args.compress)
                    blocks = kmers.phase_blocks(runs, args.min_run)
                    text = bytes(names)
                    label = [text[int(name_off[i]):int(name_off[i + 1])].decode() for i in range(n)]
                    columns = sequence_rows(n, np.diff(base_off.astype(np.int64)), counts, blocks, k)
                    out.write("".join("\t".join([label[i]] + [str(int(c[i])) for c in columns]) + "\n" for i in range(n)))
                    bed.write("".join("{}\t{}\t{}\t{}\t{}\n".format(label[int(b["read"])], int(b["first"]), int(end), "AB"[int(b["hap"])],
                                                                    int(b["markers"])) for b, end in zip(blocks, block_ends(blocks, k))))
            finally:
                batch.close()
        out.flush()
        os.replace(bed_tmp, args.bed)
    except BaseException:
        if os.path.exists(bed_tmp):
            os.remove(bed_tmp)
        raise
    finally:
        hap_a.close()
        hap_b.close()


if __name__ == "__main__":
    main()
