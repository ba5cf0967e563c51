"""Classify reads into bins based on kmers.

This is a script for classifying sequence reads into parental bins
based on the presence of k-mers.
"""
# The module docstring above is the CLI description the reference prints for --help
# (classify_by_kmers.py:1-5,17; asserted by its tests/test_classify_by_kmers.py:16) and is
# kept word for word because it is user-visible output.
#
# Host driver of the MI355X path.  Same command line, defaults, stdout TSV and bin files
# as the reference driver (src/trio_binning/classify_by_kmers.py:14-117); what changes is
# the loop: instead of one ctypes call per read (:99-102) the native reader fills batches
# (pinned memory, C-ABI layout), they stream through the HIP classifier with the next batch's
# copy overlapping the current batch's kernel, and each batch is scored, binned and written by
# the native writer in input order.

import argparse
import os
import sys
from os import path
from typing import Optional, Tuple

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

from . import find_unique_kmers as fu, kmers, seq  # noqa: E402

# bases per batch handed to the GPU; 3 batches may be in flight
_BATCH_BASES = int(os.environ.get("TBK_BATCH_BASES", str(64 << 20)))  # small enough that pinning the batch buffers is not what a short run waits for
_BATCH_READS = int(os.environ.get("TBK_BATCH_READS", str(1 << 20)))


class DatabasePair:
    """Both parents given as count databases (``find-unique-kmers --keep-databases``): the paths and each parent's
    cut-offs, settled from the files' headers alone.  ``load`` makes the two lists where the databases lie.  With the child's
    database (``child_path``, its counts from ``child_min`` on) the lists hold only what the child inherited."""

    def __init__(self, path_a: str, path_b: str, range_a: Tuple[int, int], range_b: Tuple[int, int],
                 child_path: Optional[str] = None, child_min: int = 2, prog: str = "classify-by-kmers", compressed: bool = False):
        self.prog = prog  # the command its refusals speak for
        self.compressed = compressed  # what the headers say, all alike: the databases hold homopolymer-compressed k-mers
        self.paths = {"A": path_a, "B": path_b}
        self.ranges = {"A": range_a, "B": range_b}
        self.child_path, self.child_min = child_path, child_min

    def load(self) -> Tuple[kmers.HashSet, kmers.HashSet]:
        """Each parent's k-mers with a counter in its range that the other parent does not hold, as the lists
        find-unique-kmers would dump and ``create_kmer_hash_set`` read back - without the text; with a child, those of them
        that the child holds too.  All databases are closed before this returns: 9 bytes per kept k-mer must not stand beside
        the paired table."""
        dbs, sets = {}, {}
        try:
            for hap in "AB":
                print(f"Loading the k-mer database of haplotype {hap} from {self.paths[hap]}...", file=sys.stderr)
                dbs[hap] = kmers.load_solid_database(self.paths[hap])  # (a full file: its solid form)
            third = {}
            if self.child_path is not None:
                print(f"Loading the k-mer database of the child from {self.child_path}...", file=sys.stderr)
                dbs["child"] = kmers.load_solid_database(self.child_path)
                third = {"child": dbs["child"], "child_min": self.child_min, "child_max": 255}
            for hap, other in ("AB", "BA"):
                lo, hi = self.ranges[hap]
                try:
                    sets[hap] = dbs[hap].unique_set(dbs[other], lo, hi, **third)
                except ValueError as exc:
                    if "empty k-mer list" not in str(exc):
                        raise
                    if third:
                        sys.exit(f"{self.prog}: haplotype {hap} has no k-mer with a count in [{lo},{hi}] that haplotype {other} lacks "
                                 f"and the child holds with a count in [{self.child_min},255] ({self.paths[hap]} minus {self.paths[other]}, "
                                 f"within {self.child_path}): nothing to classify by. Choose other cut-offs with --min-count-{hap.lower()}, "
                                 f"--max-count-{hap.lower()} and --min-count-child.")
                    sys.exit(f"{self.prog}: haplotype {hap} has no k-mer with a count in [{lo},{hi}] that haplotype {other} lacks "
                             f"({self.paths[hap]} minus {self.paths[other]}): nothing to classify by. Choose other cut-offs with "
                             f"--min-count-{hap.lower()} and --max-count-{hap.lower()}.")
                found = "unique to haplotype {} and inherited by the child".format(hap) if third else "unique to haplotype {}".format(hap)
                print(f"Found {sets[hap].num_kmers} {sets[hap].k}-mers {found} (in HBM on device {sets[hap].device}).", file=sys.stderr)
        except BaseException:
            for hs in sets.values():
                hs.close()
            raise
        finally:
            for db in dbs.values():
                db.close()
        return sets["A"], sets["B"]


def _parser(kmer_list_type) -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(
        description=__doc__, formatter_class=argparse.ArgumentDefaultsHelpFormatter
    )
    parser.add_argument(
        "reads",
        help="reads to classify into bins, in fasta/q format: FASTA/FASTQ(.gz) or BAM (unaligned, such as reads.hifi_reads.bam).",
    )
    parser.add_argument(
        "haplotype_a_kmers",
        type=kmer_list_type,
        help="a list of k-mers unique to haplotype A, one per line; or the count database of that parent kept by "
             "find-unique-kmers --keep-databases (*.tbkdb; then both parents must be databases)",
    )
    parser.add_argument(
        "haplotype_b_kmers",
        type=kmer_list_type,
        help="a list of k-mers unique to haplotype B, one per line; or that parent's count database (*.tbkdb)",
    )
    parser.add_argument("--haplotype-a-out-prefix", default="hapA", help="prefix for haplotype A output file")
    parser.add_argument("--haplotype-b-out-prefix", default="hapB", help="prefix for haplotype B output file")
    parser.add_argument("--unclassified-out-prefix", default="unclassified", help="prefix for unclassified output file")
    parser.add_argument("--no-gzip-output", action="store_true", default=False, help="don't gzip the output")
    parser.add_argument(
        "--bam-output", action="store_true", default=False,
        help="BAM input only: write the bins as BAM files (<prefix>.bam) that hold every read's input record whole - tags, flags "
             "and the header as they came - instead of FASTQ text",
    )
    parser.add_argument(
        "--haplotag-output", default=None, metavar="PATH",
        help="BAM input only: instead of the three bins write ONE BAM file, PATH, in input order, in which every read carries its bin "
             "as the tag HP (1: haplotype A, 2: haplotype B, none: unclassified) and its two k-mer counts as the tags ka and kb; the "
             "records are otherwise as they came",
    )
    parser.add_argument(
        "--compress", action="store_true", default=False,
        help="k-mer lists made by find-unique-kmers --compress: every run of equal bases of a read is written once before it is "
             "probed (the bins still hold the reads as they came). Count databases say by themselves which space they are in",
    )
    _add_database_options(parser)
    return parser


def _add_database_options(parser) -> None:
    """The options that choose from count databases (shared with phase_blocks)."""
    for hap in "ab":
        for bound in ("min", "max"):
            parser.add_argument(
                "--{}-count-{}".format(bound, hap), type=int, default=None, metavar="N",
                help="count databases only: count cut-offs of haplotype {} chosen by hand (give both) instead of the ones "
                     "find-unique-kmers would choose from its histogram".format(hap.upper()),
            )
    parser.add_argument(
        "--child-database", default=None, metavar="child.tbkdb",
        help="count databases only: the child's count database (find-unique-kmers --child ... --keep-databases). The reads are "
             "then classified by the parental k-mers the child inherited alone: those this database holds too",
    )
    parser.add_argument(
        "--min-count-child", type=int, default=None, metavar="N",
        help="with --child-database: the child's lower count cut-off chosen by hand instead of the one find-unique-kmers would "
             "choose from its histogram (the upper one is 255)",
    )


def _settle_databases(args, prog: str = "classify-by-kmers") -> DatabasePair:
    """Everything about a pair of databases, and the child's beside them, that their headers decide - the same k, each
    library's cut-offs - before any device is touched; every refusal is a message."""
    paths = {"A": args.haplotype_a_kmers, "B": args.haplotype_b_kmers}
    infos = {hap: kmers.database_file_info(paths[hap]) for hap in "AB"}
    if infos["A"]["k"] != infos["B"]["k"]:
        sys.exit(prog + ": {} holds {}-mers, but {} holds {}-mers".format(paths["A"], infos["A"]["k"], paths["B"], infos["B"]["k"]))
    spaces = {False: "plain (uncompressed)", True: "homopolymer-compressed"}
    compressed = infos["A"]["compressed"]
    if infos["B"]["compressed"] != compressed:
        sys.exit(prog + ": {} holds {} k-mers, but {} holds {} ones: count both parents the same way".format(
            paths["A"], spaces[compressed], paths["B"], spaces[not compressed]))
    child_info = None
    if args.child_database is not None:
        child_info = kmers.database_file_info(args.child_database)
        if child_info["compressed"] != compressed:
            sys.exit(prog + ": {} holds {} k-mers, but the child's {} holds {} ones: count all three the same way".format(
                paths["A"], spaces[compressed], args.child_database, spaces[not compressed]))
        if child_info["k"] != infos["A"]["k"]:
            sys.exit(prog + ": {} holds {}-mers, but {} holds {}-mers".format(
                paths["A"], infos["A"]["k"], args.child_database, child_info["k"]))
    ranges = {}
    for hap in "AB":
        given = getattr(args, "min_count_" + hap.lower()), getattr(args, "max_count_" + hap.lower())
        if given[0] is None:
            # the rows find_unique_kmers.write_histogram would write of this database's histogram; no file is written
            rows = [(c, 0 if c == 1 else int(infos[hap]["histogram"][c])) for c in range(1, 256)]
            try:
                given = fu.analyze_histogram(rows, paths[hap])
            except fu.HistogramError:
                sys.exit(prog + ": could not find min and max counts in the histogram of {} (haplotype {}). Choose cut-offs by "
                         "hand and give them with --min-count-a, --max-count-a, --min-count-b and --max-count-b.".format(paths[hap], hap))
        print("\033[92mUsing counts in range [{},{}].\033[0m".format(*given), file=sys.stderr)
        ranges[hap] = (int(given[0]), int(given[1]))
    child_min = args.min_count_child
    if child_info is not None and child_min is None:
        rows = [(c, 0 if c == 1 else int(child_info["histogram"][c])) for c in range(1, 256)]
        try:
            child_min = fu.analyze_histogram(rows, args.child_database)[0]  # (its maximum is not used)
        except fu.HistogramError:
            sys.exit(prog + ": could not find the minimum count in the histogram of {} (the child). Choose it by hand and "
                     "give it with --min-count-child.".format(args.child_database))
    if child_info is not None:
        print("\033[92mUsing counts in range [{},255] for the child.\033[0m".format(child_min), file=sys.stderr)
        return DatabasePair(paths["A"], paths["B"], ranges["A"], ranges["B"], args.child_database, int(child_min), prog=prog, compressed=compressed)
    return DatabasePair(paths["A"], paths["B"], ranges["A"], ranges["B"], prog=prog, compressed=compressed)


def refuse_compressed(databases: Optional[DatabasePair], prog: str) -> None:
    """For the commands that report coordinates or a QV: neither is defined in homopolymer-compressed space."""
    if databases is not None and databases.compressed:
        sys.exit(prog + ": {} and {} hold homopolymer-compressed k-mers (find-unique-kmers --compress): positions along a "
                 "sequence are not defined in compressed space. Give plain databases.".format(databases.paths["A"], databases.paths["B"]))


_LIST_LINES_CHECKED = 1000


def check_compressed_list(list_path: str, prog: str = "classify-by-kmers") -> None:
    """A k-mer with two equal adjacent bases cannot occur in a compressed read: a list that has one among its first
    lines was made without --compress, and every read would score (0, 0) against it."""
    try:
        fh = open(list_path, "r", errors="replace")
    except OSError:
        return  # (the table's own constructor reports a file that cannot be read, in the usual words)
    with fh:
        for number, line in enumerate(fh, 1):
            if number > _LIST_LINES_CHECKED:
                break
            kmer = line.strip().upper()
            if any(x == y for x, y in zip(kmer, kmer[1:])):
                sys.exit(prog + ": --compress: line {} of {} ({}) has two equal adjacent bases: this list was not made with --compress".format(
                    number, list_path, kmer))


def parse_args():
    """Parse arguments (same positionals, options, defaults and help as the reference,
    classify_by_kmers.py:14-54; the k-mer tables of text lists are built by the ``type=`` callbacks).

    The command line is read twice.  The first reading takes the two k-mer arguments as the strings they are and decides
    what they name: two text lists - then the second reading is the reference's, whose ``type=`` callbacks build the
    tables - or two count databases, which are settled from their headers (``args.databases``) and loaded by ``main``."""
    parser = _parser(str)
    args = parser.parse_args()
    if _check_kmer_arguments(parser, args):
        args.databases = _settle_databases(args)
        if args.compress and not args.databases.compressed:
            sys.exit("classify-by-kmers: --compress was given, but {} and {} hold plain (uncompressed) k-mers: count the parents "
                     "with find-unique-kmers --compress".format(args.haplotype_a_kmers, args.haplotype_b_kmers))
        args.compress = args.databases.compressed  # the mode follows the headers
        return args
    if args.compress:
        for list_path in (args.haplotype_a_kmers, args.haplotype_b_kmers):
            check_compressed_list(list_path)
    args = _parser(kmers.create_kmer_hash_set).parse_args()
    args.databases = None
    return args


def _check_kmer_arguments(parser, args, prog: str = "classify-by-kmers") -> bool:
    """What the two k-mer arguments name - True: two count databases, False: two text lists - and every refusal of the
    options beside them that needs no file opened (shared with phase_blocks)."""
    if getattr(args, "bam_output", False):
        if not args.reads.endswith(".bam"):
            parser.error("--bam-output keeps BAM records whole: the reads must be a .bam file, not {}".format(args.reads))
        if args.no_gzip_output:
            parser.error("--bam-output and --no-gzip-output exclude each other: BAM bins are bgzf-compressed")
    if getattr(args, "haplotag_output", None) is not None:
        if not args.reads.endswith(".bam"):
            parser.error("--haplotag-output tags BAM records: the reads must be a .bam file, not {}".format(args.reads))
        if args.bam_output:
            parser.error("--haplotag-output and --bam-output exclude each other: one tagged BAM file, or three BAM bins")
        if args.no_gzip_output:
            parser.error("--haplotag-output and --no-gzip-output exclude each other: a BAM file is bgzf-compressed")
    is_db = [fu.is_database_path(args.haplotype_a_kmers), fu.is_database_path(args.haplotype_b_kmers)]
    if is_db[0] != is_db[1]:
        sys.exit(prog + ": {} is a {} and {} is a {}: give two k-mer lists or two count databases (*{})".format(
            args.haplotype_a_kmers, "count database" if is_db[0] else "k-mer list", args.haplotype_b_kmers,
            "count database" if is_db[1] else "k-mer list", fu.DATABASE_SUFFIX))
    for hap in "ab":
        lo, hi = getattr(args, "min_count_" + hap), getattr(args, "max_count_" + hap)
        if (lo is None) != (hi is None):
            parser.error("--min-count-{0} and --max-count-{0} go together".format(hap))
        if lo is not None and not 1 <= lo <= hi:
            parser.error("--min-count-{0} {1} --max-count-{0} {2}: need 1 <= min <= max".format(hap, lo, hi))
        if lo is not None and not is_db[0]:
            parser.error("--min-count-{0} and --max-count-{0} choose from a count database (*{1}); a k-mer list was given".format(hap, fu.DATABASE_SUFFIX))
    if args.child_database is not None and not is_db[0]:
        parser.error("--child-database selects from two count databases (*{}); k-mer lists were given".format(fu.DATABASE_SUFFIX))
    if args.child_database is not None and not fu.is_database_path(args.child_database):
        parser.error("--child-database {} is not a count database (*{})".format(args.child_database, fu.DATABASE_SUFFIX))
    if args.min_count_child is not None and args.child_database is None:
        parser.error("--min-count-child chooses from the child's counts: give --child-database too")
    if args.min_count_child is not None and args.min_count_child < 1:
        parser.error("--min-count-child {}: need 1 <= min".format(args.min_count_child))
    return is_db[0]


def calculate_scaling_factors(haplotype_a_kmers: kmers.HashSet, haplotype_b_kmers: kmers.HashSet) -> Tuple[float, float]:
    """Scaling factors for the k-mer scores (reference classify_by_kmers.py:57-77):
    each count is multiplied by max(nA, nB) / n of its own list, in float64."""
    num_kmers_a = kmers.get_number_kmers_in_set(haplotype_a_kmers)
    num_kmers_b = kmers.get_number_kmers_in_set(haplotype_b_kmers)
    max_num_kmers = max(num_kmers_a, num_kmers_b)
    return 1.0 * max_num_kmers / num_kmers_a, 1.0 * max_num_kmers / num_kmers_b


def output_extension(reads_path: str) -> str:
    """Extension of the bin files.  The reference computes
    ``splitext(reads.rstrip(".gz"))[1]`` (classify_by_kmers.py:90): ``rstrip`` strips the
    character set {'.', 'g', 'z'}, not the suffix, and that quirk decides file names."""
    if reads_path.endswith(".bam"):  # BAM input: the bins hold the reads' FASTQ text (include/tbk.h "BAM input")
        return ".fastq"
    return path.splitext(reads_path.rstrip(".gz"))[1]


def make_classifier(haplotype_a_kmers, haplotype_b_kmers):
    """The classify pipeline of this run: one feeder thread and stream ring per device of TBK_DEVICES
    (default: every visible device; a device may repeat), tables replicated, batches dealt to them and
    taken back in input order - the library's ``tbk_pipeline``, also when that is a single device."""
    # (how the table is built is an argument of the library - kmers.Options; the command line has no flags for it, as the
    # reference has none, so the TBK_* variables of the environment are its fallback: Options.from_env)
    # A table built by inserts that merge keys (entries, wide entries) is asked for every line of both lists before the library
    # hands it out, on every device (tbk_options.verify_build; c/kmers.c:112-122 stores every line): a wrong table fails here.
    # TBK_VERIFY_BUILD=1 extends that to every layout, =0 switches it off.
    options = kmers.Options.from_env() if _lib.HAS_OPTIONS else None
    classifier = kmers.MultiClassifier(haplotype_a_kmers, haplotype_b_kmers, kmers.visible_devices(), options=options)
    if os.environ.get("TBK_VERIFY_BUILD", "") not in ("", "0") or os.environ.get("TBK_STATS", "") not in ("", "0"):
        print("tbk-verify " + str([classifier._part(i).verified() for i in range(len(classifier.devices))]), file=sys.stderr)
    return classifier


def classify_compressed(args, num_a: int, num_b: int) -> dict:
    """The loop in homopolymer-compressed space, in Python over native pieces as phase_blocks runs its own: the reader
    fills a batch, a compressor session writes every run of equal bases once on the device (case as it came: lower case
    stays not-ACGT for the probe), the classifier probes the compressed batch where it lies, and the ORIGINAL batch is
    scored, binned, printed and written.  Two batches and two sessions take turns, so batch i + 1 is read and compressed
    while batch i is probed.  One device: the first of TBK_DEVICES."""
    import time

    import numpy as np

    devices = kmers.visible_devices()
    if len(devices) > 1:
        print("classify-by-kmers: compressed mode runs on one device; using device {} of {}.".format(devices[0], devices), file=sys.stderr)
    options = kmers.Options.from_env() if _lib.HAS_OPTIONS else None
    spent = {"read_s": 0.0, "compress_s": 0.0, "probe_wait_s": 0.0, "write_s": 0.0, "bases": 0, "compressed_bases": 0, "reads": 0}
    t_start = time.perf_counter()
    classifier = kmers.Classifier(args.haplotype_a_kmers, args.haplotype_b_kmers, options=options)
    spent["table_build_s"] = time.perf_counter() - t_start
    device = classifier.device
    print("Classifying in homopolymer-compressed space: the reads are compressed on device {} before they are probed.".format(device), file=sys.stderr)
    gzip_output = not args.no_gzip_output
    reader = None
    if args.bam_output or args.haplotag_output is not None:  # (BAM output begins with the input's header: the reader comes first)
        reader = seq.BatchReader(args.reads, keep_records=True)
        try:
            writer = seq.BinWriter(args.haplotype_a_out_prefix, args.haplotype_b_out_prefix, args.unclassified_out_prefix, ".bam", True,
                                   int(os.environ.get("TBK_GZIP_LEVEL", "-1")), device=device, bam_header=reader.bam_header(),
                                   haplotag_path=args.haplotag_output)
        except BaseException:
            reader.close()
            classifier.close()
            raise
    else:
        writer = seq.BinWriter(args.haplotype_a_out_prefix, args.haplotype_b_out_prefix, args.unclassified_out_prefix, output_extension(args.reads),
                               gzip_output, int(os.environ.get("TBK_GZIP_LEVEL", "-1")), device=device if gzip_output else None)
    batches = [seq.Batch(), seq.Batch()]
    sessions = [kmers.HomopolymerCompressor(device), kmers.HomopolymerCompressor(device)]
    out = sys.stdout

    def finish(ticket, batch):
        t0 = time.perf_counter()
        counts = classifier.wait(ticket)
        t1 = time.perf_counter()
        score_a, score_b, bins = kmers.score_and_bin(counts, num_a, num_b)
        out.write(seq.format_tsv(batch, bins, score_a, score_b))
        if args.haplotag_output is not None:
            writer.write_counts(batch, bins, counts)  # (the counts of compressed space, as the TSV's scores are)
        else:
            writer.write(batch, bins)
        spent["probe_wait_s"] += t1 - t0
        spent["write_s"] += time.perf_counter() - t1

    try:
        with (reader if reader is not None else seq.BatchReader(args.reads)) as reader:
            pending, turn = None, 0
            while True:
                batch, session = batches[turn], sessions[turn]
                t0 = time.perf_counter()
                n = reader.next_batch(batch, _BATCH_BASES, _BATCH_READS)
                t1 = time.perf_counter()
                spent["read_s"] += t1 - t0
                if not n:
                    break
                d_bases, d_offsets, total = session.compress_batch(batch, False)
                spent["compress_s"] += time.perf_counter() - t1
                spent["reads"] += n
                spent["bases"] += int(batch.arrays()[1][-1])
                spent["compressed_bases"] += total
                ticket = classifier.submit_device(d_bases, d_offsets, n, total, np.zeros((n, 2), dtype=np.int32))
                if pending is not None:
                    finish(*pending)
                pending, turn = (ticket, batch), 1 - turn
            if pending is not None:
                finish(*pending)
        out.flush()
        t0 = time.perf_counter()
        writer.close()
        spent["write_s"] += time.perf_counter() - t0
    finally:
        for session in sessions:
            session.close()
        for batch in batches:
            batch.close()
        classifier.close()
    spent["total_s"] = time.perf_counter() - t_start
    spent["devices"] = [device]
    return spent


def main():
    """Main method of program"""
    args = parse_args()
    if args.databases is not None:
        args.haplotype_a_kmers, args.haplotype_b_kmers = args.databases.load()

    num_a = kmers.get_number_kmers_in_set(args.haplotype_a_kmers)
    num_b = kmers.get_number_kmers_in_set(args.haplotype_b_kmers)
    if args.compress:
        stats = classify_compressed(args, num_a, num_b)
        if os.environ.get("TBK_STATS"):
            import json

            stats["gbases_per_s"] = stats["bases"] / stats["total_s"] / 1e9 if stats["total_s"] > 0 else 0.0
            print("tbk-stats " + json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in stats.items()}), file=sys.stderr)
        return
    import time

    t_start = time.perf_counter()
    classifier = make_classifier(args.haplotype_a_kmers, args.haplotype_b_kmers)
    t_built = time.perf_counter()

    # The loop of the reference (classify_by_kmers.py:99-117: count, score, bin, print one read at a time)
    # runs inside the library on native threads - a reader filling batches in pinned memory (their bases
    # packed for the link on the way), this thread feeding the device(s) and taking the batches back in
    # input order, a writer scoring, binning, writing the three bins and the TSV.  Python only names the
    # files; the TSV goes to the process's stdout descriptor.
    mode = 2 if args.bam_output else not args.no_gzip_output
    if args.haplotag_output is not None:
        names, mode = (args.haplotag_output, "", ""), 3  # one tagged BAM file; the three bins are not written
    elif args.bam_output:
        names = seq.output_names(args.haplotype_a_out_prefix, args.haplotype_b_out_prefix, args.unclassified_out_prefix, ".bam", False)
    else:
        names = seq.output_names(args.haplotype_a_out_prefix, args.haplotype_b_out_prefix, args.unclassified_out_prefix,
                                 output_extension(args.reads), not args.no_gzip_output)
    # zlib level of the gzip members when zlib is asked for (TBK_GZIP_ENCODER): default 6; the reference's
    # gzip.open uses 9, which only changes the container bytes, never the decompressed bins
    level = int(os.environ.get("TBK_GZIP_LEVEL", "-1"))
    sys.stdout.flush()
    spool = None
    try:
        tsv_fd = sys.stdout.fileno()
    except (AttributeError, OSError, ValueError):  # stdout is not a file (a test harness's capture): spool, then hand over
        import tempfile

        spool = tempfile.TemporaryFile()
        tsv_fd = spool.fileno()
    try:
        stats = classifier.classify_file(args.reads, num_a, num_b, names, mode, level, tsv_fd, _BATCH_BASES, _BATCH_READS)
    finally:
        if spool is not None:
            spool.seek(0)
            sys.stdout.write(spool.read().decode())
            spool.close()
    devices = list(getattr(classifier, "devices", [classifier.device]))
    classifier.close()
    if os.environ.get("TBK_STATS"):
        # stderr is free-form in the reference too (progress chatter); stdout stays pure TSV
        import json

        stats["loop_s"] = stats["total_s"]  # the native read / classify / write loop alone
        stats["table_build_s"] = t_built - t_start
        stats["devices"] = devices
        stats["numpy_loaded"] = "numpy" in sys.modules  # (the command line's path needs none of it: kmers imports it at first use)
        stats["total_s"] = time.perf_counter() - t_start
        stats["gbases_per_s"] = stats["bases"] / stats["total_s"] / 1e9 if stats["total_s"] > 0 else 0.0
        print("tbk-stats " + json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in stats.items()}), file=sys.stderr)


if __name__ == "__main__":
    main()
