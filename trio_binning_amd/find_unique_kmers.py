"""find-unique-kmers -- given two short-read libraries, find k-mers that are unique to each.

Host driver of the MI355X path for the reference's find_unique_kmers.py: same command line, same
output files (`hapA_only_kmers.txt`, `hapB_only_kmers.txt` under --outpath), same choice of count
cut-offs; the KMC subprocesses (`kmc`, `kmc_tools transform ... histogram`, `kmc_tools simple ...
kmers_subtract`, `kmc_dump`; find_unique_kmers.py:62-233) are replaced by a counting table in HBM
behind the C-ABI (`tbk_counter_*`).  What KMC does at those call sites is restated from its
documentation (canonical counting, -ci2, -cs255, lexicographic dump); KMC is not part of the
reference checkout, so equality with its output is not pinned by any fixture.  Whoever has KMC can check it now (nobody
has yet): `kmc -k<k> -ci1 -cs255 @files db tmp` and `kmc_dump db db.txt`, then `python -m trio_binning_amd.import_database
-o kmc.tbkdb --floor 2 --reads N --bases N db.txt`, and compare kmc.tbkdb byte for byte with the haplotypeA.tbkdb that this
command leaves with --keep-databases on the same files.
"""
import argparse
import os
import sys
from typing import List, Sequence, Tuple

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

from . import kmers, seq  # noqa: E402

_BATCH_BASES = int(os.environ.get("TBK_BATCH_BASES", str(256 << 20)))
_BATCH_READS = int(os.environ.get("TBK_BATCH_READS", str(4 << 20)))


class HistogramError(Exception):
    """Same message as the reference's (find_unique_kmers.py:15-22), minus the command to re-run."""

    def __init__(self, histogram_path: str):
        self.message = (
            "Could not find min and max counts in histogram. "
            + "Take a look at the histogram in {} and choose cutoffs manually.".format(histogram_path)
        )
        super().__init__(self.message)


def parse_args(argv=None):
    """Same options as the reference (find_unique_kmers.py:25-59); --path-to-kmc and --threads are
    accepted and ignored (there is no kmc to find or to give threads to)."""
    parser = argparse.ArgumentParser(
        description="Given multiple short-read libraries, find k-mers that are unique to each library."
    )
    parser.add_argument("-k", "--kmer-size", type=int, required=True)
    parser.add_argument("--path-to-kmc", default="kmc", help="ignored: k-mers are counted on the GPU")
    parser.add_argument("-p", "--threads", type=int, default=1, help="ignored: k-mers are counted on the GPU")
    parser.add_argument("-o", "--outpath", default=".", help="Prefix to write output haplotypes to")
    parser.add_argument("-s", "--scratch-dir", default=".", help="Directory for the count histograms")
    parser.add_argument(
        "--capacity", type=int, default=0,
        help="distinct k-mers each counting table must hold (sequencing errors included); default: an estimate "
             "from the input sizes, within the free HBM",
    )
    parser.add_argument(
        "--passes", type=int, default=0,
        help="count each library in this many passes over its reads, which are kept on the GPU in packed form: a "
             "table then holds 1/N of the distinct k-mers at a time (for libraries whose k-mers, sequencing errors "
             "included, outgrow the HBM); 1: one pass, nothing kept; default 0: the fewest passes that fit (choose_passes)",
    )
    parser.add_argument(
        "--keep-databases", action="store_true",
        help="leave each parent's count database as <outpath>/haplotypeA.tbkdb and haplotypeB.tbkdb (where kmc leaves "
             "haplotypeA.* in the reference) and go on from them: a later run takes such a file in place of a parent's "
             "reads and dumps again, at other cut-offs, without counting",
    )
    for hap in "ab":
        for bound in ("min", "max"):
            parser.add_argument(
                "--{}-count-{}".format(bound, hap), type=int, default=None, metavar="N",
                help="count cut-offs of haplotype {} chosen by hand (give both): its histogram is written but not "
                     "analyzed".format(hap.upper()),
            )
    parser.add_argument(
        "--child", default=None, metavar="FILES",
        help="one comma-separated list of the child's short-read files, or its count database (one path ending in .tbkdb): "
             "the output then holds only the parental k-mers the child inherited, those its library holds too (seen at least "
             "twice, with a count from its own lower cut-off on). The child is counted third, through count databases; with "
             "--keep-databases its database is left as <outpath>/child.tbkdb",
    )
    parser.add_argument(
        "--min-count-child", type=int, default=None, metavar="N",
        help="lower count cut-off of the child chosen by hand (the upper one is 255): its histogram is written but not analyzed",
    )
    parser.add_argument(
        "--compress", action="store_true",
        help="count in homopolymer-compressed space: every run of equal bases of a read is written once before k-mers are cut "
             "(for parents that will bin ONT or HiFi reads, whose dominant error is the length of such runs). Both parents and "
             "the child are counted that way, --keep-databases leaves compressed databases, and the lists hold compressed "
             "k-mers: give them to classify-by-kmers --compress. A database given in place of reads must agree with the run",
    )
    parser.add_argument(
        "--keep-singletons", action="store_true",
        help="the databases this run keeps are FULL ones: they hold the k-mers seen once too, so a later run can unite them "
             "exactly with more reads of the same library (mother.tbkdb,new_lane.fq.gz) or with another database "
             "(python -m trio_binning_amd.merge_databases). Needs a run that goes through databases (--keep-databases, "
             "--child, or a database among the arguments); the run itself works on their solid form, so lists and "
             "histograms are those of a run without the flag. A full database takes 9 bytes for every distinct k-mer",
    )
    parser.add_argument(
        "read_files", nargs=2,
        help="one comma-separated list of file paths for both libraries being compared. Files can "
             "be FASTA/FASTQ(.gz) or BAM (unaligned). A single path ending in .tbkdb is a count "
             "database kept by --keep-databases: it is loaded instead of counted. A list may also mix full databases "
             "(kept with --keep-singletons) and read files: the reads are counted and united with the databases.",
    )
    args = parser.parse_args(argv)
    for hap in "ab":
        lo, hi = getattr(args, "min_count_" + hap), getattr(args, "max_count_" + hap)
        if (lo is None) != (hi is None):
            parser.error("--min-count-{0} and --max-count-{0} go together".format(hap))
        if lo is not None and not 1 <= lo <= hi:
            parser.error("--min-count-{0} {1} --max-count-{0} {2}: need 1 <= min <= max".format(hap, lo, hi))
    if args.min_count_child is not None and args.child is None:
        parser.error("--min-count-child chooses from the child's counts: give --child too")
    if args.min_count_child is not None and args.min_count_child < 1:
        parser.error("--min-count-child {}: need 1 <= min".format(args.min_count_child))
    arguments = list(args.read_files) + ([args.child] if args.child is not None else [])
    if args.keep_singletons and not (args.keep_databases or args.child is not None
                                     or any(is_database_path(s) or is_mixed_argument(s) for s in arguments)):
        parser.error("--keep-singletons keeps full databases: give --keep-databases (or --child, or a database among the arguments)")
    for files_string in arguments:
        if not is_mixed_argument(files_string):
            continue
        # every database of a mixed list is united with freshly counted reads: its header must allow that, before anything is counted
        for path in split_mixed_argument(files_string)[0]:
            try:
                info = kmers.database_file_info(path)
            except (IOError, ValueError) as exc:
                parser.error("{}: {}".format(path, exc))
            if info["floor"] != 1:
                parser.error("{} was kept without the k-mers seen once and cannot be united exactly with more reads or another "
                             "database: count that library again with --keep-databases --keep-singletons".format(path))
            if info["k"] != args.kmer_size:
                parser.error("{} holds {}-mers, but -k {} was given".format(path, info["k"], args.kmer_size))
            if info["compressed"] != args.compress:
                parser.error("{} holds {} k-mers, but this run {}".format(
                    path, "homopolymer-compressed" if info["compressed"] else "plain (uncompressed)",
                    "was not given --compress" if info["compressed"] else "was given --compress"))
    return args


def is_database_path(files_string: str) -> bool:
    """A parent argument that names one count database (*.tbkdb) and no read files."""
    return "," not in files_string and files_string.endswith(DATABASE_SUFFIX)


def split_mixed_argument(files_string: str) -> Tuple[List[str], List[str]]:
    """(databases, read files) of a comma-separated library argument, each in the order given."""
    parts = [p for p in files_string.split(",") if p]
    return [p for p in parts if p.endswith(DATABASE_SUFFIX)], [p for p in parts if not p.endswith(DATABASE_SUFFIX)]


def is_mixed_argument(files_string: str) -> bool:
    """A library argument that names at least one count database among several comma-separated entries, read files or
    further databases (mother.tbkdb,new_lane.fq.gz): the reads are counted and everything is united.  One database alone is
    `is_database_path`'s case, read files alone are neither."""
    return "," in files_string and bool(split_mixed_argument(files_string)[0])


def analyze_histogram(rows: Sequence[Tuple[int, int]], histogram_path: str = "") -> Tuple[int, int]:
    """Choose the minimum and maximum k-mer count from histogram rows (count, number of k-mers), as
    the reference does (find_unique_kmers.py:132-168): the minimum is the row before the counts first
    rise again (the row of count 2 is only remembered), the maximum the first later row that drops
    below the count at the minimum.  Raises HistogramError when either is not found (0 counts as not
    found, as in the reference); warns on stderr when they are less than 5 apart."""
    low = high = 0        # 0 doubles as "not found yet", which is how the reference treats a cut-off of 0
    floor = None          # number of k-mers in the row of the minimum
    previous = -1         # number of k-mers in the row before this one
    for count, n_kmers in rows:
        if count == 2:    # the row of count 2 is only remembered
            previous = n_kmers
            continue
        if not low:
            if n_kmers > previous:       # the histogram starts rising: the row before is the minimum
                low, floor = count - 1, previous
        elif n_kmers < floor:            # first row after the peak that falls below the minimum's row
            high = count
            break
        previous = n_kmers
    if not low or not high:
        raise HistogramError(histogram_path)
    min_coverage, max_coverage = low, high
    if max_coverage - min_coverage < 5:
        print(
            "WARNING: min and max coverage not very far apart. This may be a result of coverage being too low. "
            'Try taking a look at the histogram in "{}" yourself.'.format(histogram_path),
            file=sys.stderr,
        )
    return min_coverage, max_coverage


def count_library(paths: List[str], k: int, capacity: int, passes: int = 1, compress: bool = False,
                  keep_singletons: bool = False) -> "kmers.KmerCounter":
    """Count the canonical k-mers of all files of one library (what `kmc -k<k> @files` does).
    The files are read side by side, one reader thread each (a gzip stream inflates on one core, but
    a library usually comes as many files); this thread feeds their batches to the GPU."""
    import queue
    import threading

    counter = kmers.KmerCounter(k, capacity, passes=passes, compress=compress, keep_singletons=keep_singletons)
    n_readers = max(1, min(len(paths), kmers.host_threads()))
    todo: "queue.Queue" = queue.Queue()
    for p in paths:
        todo.put(p)
    filled: "queue.Queue" = queue.Queue(maxsize=2 * n_readers)
    failure: List[BaseException] = []
    batches: List[seq.Batch] = []  # every batch made; closed by this thread at the end

    def read_files() -> None:
        free: "queue.Queue" = queue.Queue()
        for _ in range(2):
            b = seq.Batch()
            batches.append(b)
            free.put(b)
        try:
            while not failure:
                try:
                    path = todo.get_nowait()
                except queue.Empty:
                    break
                reader = seq.BatchReader(path)
                try:
                    while not failure:
                        batch = free.get()
                        if not reader.next_batch(batch, _BATCH_BASES, _BATCH_READS):
                            free.put(batch)
                            break
                        filled.put((batch, free))
                finally:
                    reader.close()
        except BaseException as exc:  # handed to the counting thread
            failure.append(exc)
        finally:
            filled.put(None)

    threads = [threading.Thread(target=read_files, name="tbk-reader-%d" % i, daemon=True) for i in range(n_readers)]
    for t in threads:
        t.start()
    live = n_readers
    try:
        while live:
            item = filled.get()
            if item is None:
                live -= 1
                continue
            batch, free = item
            if not failure:
                try:
                    counter.add_batch(batch)
                except BaseException as exc:
                    failure.append(exc)
            free.put(batch)
    finally:
        for t in threads:
            t.join(timeout=5)
        for b in batches:
            b.close()
    if failure:
        counter.close()
        raise failure[0]
    return counter


def estimate_bases(paths: List[str]) -> int:
    """Bases of a library from its file sizes: uncompressed FASTQ spends two bytes per base, gzip
    compresses it about fourfold; a BAM file (bgzf) is counted as a gzip file."""
    bases = 0
    for p in paths:
        size = os.path.getsize(p)
        bases += size * 2 if p.endswith((".gz", ".bam")) else size // 2 + 1
    return bases


DATABASE_SUFFIX = ".tbkdb"
MAX_PASSES = 1024          # TBK_COUNTER_MAX_PASSES
PLAN_FRACTION = (4, 5)     # choose_passes plans with 4/5 of the free HBM
TABLE_BYTES = (80, 3)      # per distinct k-mer of a table: 16 bytes per slot at load 0.6
STORE_BYTES = (1, 2)       # per base kept: one 64-bit word per 16 bases
DATABASE_SHARE = 8         # 1 / this of a parent's distinct k-mers is planned to be seen twice or more ...
DATABASE_BYTES = 9         # ... and costs a key and a one-byte counter


def choose_passes(capacity: int, bases_estimate: int, free_bytes: int, databases: int = 2, database_share: int = DATABASE_SHARE) -> int:
    """The fewest passes in which one parent of `capacity` distinct k-mers and `bases_estimate` bases can be
    counted within `free_bytes` of HBM.  A pure function of its arguments; all arithmetic in integers.

    The budget is 4/5 of the free bytes (the rest is left to the batch staging, the sort of the dump and
    the allocator).  With table(P) = ceil(capacity / P) * 80 // 3 bytes (16 bytes per slot at load 0.6):

    * P = 1 (one pass, nothing kept: both parents' tables stay resident until the dumps are written, and a
      table that doubles is held beside its twice as large successor) fits if 4 * table(1) <= budget;
    * P > 1 fits if  store + 3 * table(P) + databases <= budget, where store = ceil(bases_estimate / 2) (the
      reads of the parent being counted, 0.5 bytes per base), 3 * table(P) is one class's table beside its
      doubling twin, and databases = `databases` * 9 * (capacity // 8) is what the libraries leave behind (two
      parents; three with a child): a ninth byte on every key seen at least twice, planned as an eighth of the
      distinct k-mers (the others are the k-mers seen once that -ci2 drops).  `database_share` is that 8; a run that keeps
      the once-seen k-mers (--keep-singletons) passes 1: every distinct k-mer is kept.

    Returns the smallest such P; ValueError when the store and the databases alone pass the budget, or when
    more than 1024 passes would be needed."""
    if capacity < 1 or bases_estimate < 0 or free_bytes < 0 or databases < 0 or database_share < 1:
        raise ValueError("choose_passes: capacity and database_share must be positive, bases, free bytes and databases not negative")
    budget = free_bytes * PLAN_FRACTION[0] // PLAN_FRACTION[1]

    def table(p: int) -> int:
        return -(-capacity // p) * TABLE_BYTES[0] // TABLE_BYTES[1]

    if 4 * table(1) <= budget:
        return 1
    store = -(-bases_estimate * STORE_BYTES[0] // STORE_BYTES[1])
    fixed = store + databases * DATABASE_BYTES * (capacity // database_share)
    if store > budget:
        raise ValueError(
            "the reads alone ({} bases, {} bytes packed) do not fit the {} bytes planned of {} free on the GPU: "
            "keeping reads on the host is not supported".format(bases_estimate, store, budget, free_bytes))
    for p in range(2, MAX_PASSES + 1):
        if fixed + 3 * table(p) <= budget:
            return p
    raise ValueError(
        "{} distinct k-mers of {} bases cannot be counted in up to {} passes within the {} bytes planned of {} free "
        "on the GPU (packed reads and databases: {} bytes); give --capacity (the distinct k-mers expected) or --passes".format(
            capacity, bases_estimate, MAX_PASSES, budget, free_bytes, fixed))


def estimate_capacity(paths: List[str]) -> int:
    """Distinct k-mers cannot outnumber the bases (estimate_bases).  Bounded by what two tables
    (16 bytes per slot at load 0.6) may take of the free HBM."""
    bases = estimate_bases(paths)
    free, _total = kmers.device_mem_info()
    fit = int(0.35 * free / 16 * 0.6)
    return max(1 << 16, min(bases, fit))


def write_histogram(path: str, hist: Sequence[int]) -> List[Tuple[int, int]]:
    """The rows `kmc_tools transform <db> histogram` writes: count <tab> number of k-mers; the
    database holds no k-mer seen once (kmc's default -ci2)."""
    rows = [(c, 0 if c == 1 else int(hist[c])) for c in range(1, 256)]
    with open(path, "w") as fh:
        for c, n in rows:
            fh.write("{}\t{}\n".format(c, n))
    return rows


def main(argv=None):
    args = parse_args(argv)
    k = args.kmer_size
    libraries = []  # (counter or database, min_count, max_count)
    if args.passes < 0 or args.passes > MAX_PASSES:
        raise ValueError("--passes must be between 0 and {}".format(MAX_PASSES))
    hap_ids = ["A", "B"]
    from_file = [is_database_path(s) for s in args.read_files]
    mixed = [is_mixed_argument(s) for s in args.read_files]
    # with none of the database options both counters stay live until the dumps are written, as ever; a child is a third
    # library, and three are only ever held as databases
    by_database = args.keep_databases or any(from_file) or any(mixed) or args.child is not None
    given = {"A": (args.min_count_a, args.max_count_a), "B": (args.min_count_b, args.max_count_b)}
    counted = list(zip(args.read_files, from_file))  # every library: (its argument, whether that is a database)
    if args.child is not None:
        counted.append((args.child, is_database_path(args.child)))
    for path, is_db in counted:
        if is_db:  # its header says what it holds: checked before anything is counted
            info = kmers.database_file_info(path)
            if info["k"] != k:
                sys.exit("find-unique-kmers: {} holds {}-mers, but -k {} was given".format(path, info["k"], k))
            if info["compressed"] != args.compress:
                sys.exit("find-unique-kmers: {} holds {} k-mers, but this run {}".format(
                    path, "homopolymer-compressed" if info["compressed"] else "plain (uncompressed)",
                    "was not given --compress" if info["compressed"] else "was given --compress"))
    passes = args.passes
    if not passes:
        # both parents are counted in the same number of passes (their classes must match): the larger need decides
        passes, free = 1, kmers.device_mem_info()[0] if not all(is_db for _, is_db in counted) else 0
        for files_string, is_db in counted:
            if is_db:
                continue
            paths = [p for p in split_mixed_argument(files_string)[1] if os.path.isfile(p)]  # (a missing file is reported below, in its turn)
            bases = estimate_bases(paths)
            share = 1 if args.keep_singletons or is_mixed_argument(files_string) else DATABASE_SHARE  # (full databases keep every distinct k-mer)
            passes = max(passes, choose_passes(args.capacity or max(1 << 16, bases), bases, free, databases=len(counted), database_share=share))
    kept = {}      # haplotype (or "child") -> the database file it can be dumped from again
    held = None    # the first HistogramError of a --keep-databases run: raised once every database is on disk
    child = [None, args.min_count_child]  # the child's database and its lower cut-off
    try:
        for hap_id, files_string, is_db in zip(hap_ids, args.read_files, from_file):
            if is_db:
                print("\033[92mLoading the k-mer database of haplotype {}...\033[0m".format(hap_id), file=sys.stderr)
                libraries.append([kmers.load_solid_database(files_string), None, None])
                kept[hap_id] = files_string
            elif by_database:
                keep_as = os.path.join(args.outpath, "haplotype{}{}".format(hap_id, DATABASE_SUFFIX)) if args.keep_databases else None
                libraries.append([library_database(files_string, "haplotype " + hap_id, args, passes, keep_as), None, None])
                if keep_as:
                    kept[hap_id] = keep_as
            else:
                print("\033[92mCounting k-mers in haplotype {}...\033[0m".format(hap_id), file=sys.stderr)
                paths = files_string.split(",")
                for p in paths:
                    if not os.path.isfile(p):
                        raise IOError("no such file: {}".format(p))
                # (in passes the table holds one class and is not bound by what two resident tables may take)
                capacity = args.capacity or (estimate_capacity(paths) if passes == 1 else max(1 << 16, estimate_bases(paths)))
                libraries.append([count_library(paths, k, capacity, passes, args.compress), None, None])
            print("\033[92mComputing and analyzing histogram...\033[0m", file=sys.stderr)
            histogram_path = os.path.join(args.scratch_dir, "haplotype{}.histogram".format(hap_id))
            rows = write_histogram(histogram_path, libraries[-1][0].histogram())
            if given[hap_id][0] is not None:
                min_count, max_count = given[hap_id]
            else:
                try:
                    min_count, max_count = analyze_histogram(rows, histogram_path)
                except HistogramError as exc:
                    if not args.keep_databases:
                        raise
                    held = held or exc
                    continue
            print("\033[92mUsing counts in range [{},{}].\033[0m".format(min_count, max_count), file=sys.stderr)
            libraries[-1][1:] = [min_count, max_count]
        if args.child is not None:
            # third, when each parent's counter has become its database and is closed
            if counted[2][1]:
                print("\033[92mLoading the k-mer database of the child...\033[0m", file=sys.stderr)
                child[0] = kmers.load_solid_database(args.child)
                kept["child"] = args.child
            else:
                keep_as = os.path.join(args.outpath, "child" + DATABASE_SUFFIX) if args.keep_databases else None
                child[0] = library_database(args.child, "the child", args, passes, keep_as)
                if keep_as:
                    kept["child"] = keep_as
            print("\033[92mComputing and analyzing histogram...\033[0m", file=sys.stderr)
            histogram_path = os.path.join(args.scratch_dir, "child.histogram")
            rows = write_histogram(histogram_path, child[0].histogram())
            if child[1] is None:
                try:
                    child[1] = analyze_histogram(rows, histogram_path)[0]  # (its maximum is not used: the child's range ends at 255)
                except HistogramError as exc:
                    if not args.keep_databases:
                        raise
                    held = held or exc
            if child[1] is not None:
                print("\033[92mUsing counts in range [{},255] for the child.\033[0m".format(child[1]), file=sys.stderr)
        if held is not None:
            print(redump_advice(args, kept, libraries, child[1]), file=sys.stderr)
            raise held
        (counter_a, min_a, max_a), (counter_b, min_b, max_b) = libraries
        # (with a child all three are databases: only KmerDatabase.unique takes one)
        third = {} if child[0] is None else {"child": child[0], "child_min": child[1], "child_max": 255}
        print("\033[92mFinding and dumping k-mers unique to haplotype A...\033[0m", file=sys.stderr)
        n_a = counter_a.unique(counter_b, min_a, max_a, os.path.join(args.outpath, "hapA_only_kmers.txt"), **third)
        print("\033[92mFinding and dumping k-mers unique to haplotype B...\033[0m", file=sys.stderr)
        n_b = counter_b.unique(counter_a, min_b, max_b, os.path.join(args.outpath, "hapB_only_kmers.txt"), **third)
    finally:
        for lib in libraries:
            lib[0].close()
        if child[0] is not None:
            child[0].close()
    what = "unique k-mers" if args.child is None else "unique k-mers the child inherited"
    print("\n\n\033[94m# of {} in haplotype A: {}\033[0m".format(what, n_a), file=sys.stderr)
    print("\033[94m# of {} in haplotype B: {}\033[0m".format(what, n_b), file=sys.stderr)


def library_database(files_string: str, whose: str, args, passes: int, keep_as=None) -> "kmers.KmerDatabase":
    """The database a run works on, for a library given as read files or as a mix of full databases and read files
    (`is_mixed_argument`; parse_args has checked the databases' headers).  The reads are counted - keeping the once-seen
    k-mers when the result is to be united or kept full - and exported, the counter's table leaves the HBM, and the loaded
    databases are united with the result one after the other, each input freed as the fold goes.  `keep_as` saves what was
    made: the united database, full with --keep-singletons or a mixed list.  What comes back is its solid form."""
    databases, paths = split_mixed_argument(files_string)
    full = bool(databases) or args.keep_singletons
    for p in paths:
        if not os.path.isfile(p):
            raise IOError("no such file: {}".format(p))
    db = None
    try:
        if paths:
            print("\033[92mCounting k-mers in {}...\033[0m".format(whose), file=sys.stderr)
            # (in passes the table holds one class and is not bound by what two resident tables may take)
            capacity = args.capacity or (estimate_capacity(paths) if passes == 1 else max(1 << 16, estimate_bases(paths)))
            counter = count_library(paths, args.kmer_size, capacity, passes, args.compress, keep_singletons=full)
            try:
                db = counter.database()  # the database takes the counter's place
            finally:
                counter.close()
        for path in databases:
            print("\033[92mUniting {} with the k-mer database {}...\033[0m".format(whose, path), file=sys.stderr)
            more = kmers.KmerDatabase.load(path)
            if db is None:
                db = more
                continue
            try:
                united = db.union(more)
            finally:
                more.close()
            db.close()
            db = united
        if keep_as:
            db.save(keep_as)
        if db.floor >= 2:
            return db
        solid = db.solid()
    except BaseException:
        if db is not None:
            db.close()
        raise
    db.close()
    return solid


def redump_advice(args, kept, libraries, child_min=None) -> str:
    """What to run once cut-offs have been chosen by hand: the databases are on disk, nothing is counted again."""
    words = ["find-unique-kmers", "-k", str(args.kmer_size), "-o", args.outpath, "-s", args.scratch_dir]
    for hap_id, (_, lo, hi) in zip("AB", libraries):
        words += ["--min-count-" + hap_id.lower(), str(lo) if lo else "MIN", "--max-count-" + hap_id.lower(), str(hi) if hi else "MAX"]
    where = "{} and {}".format(kept["A"], kept["B"])
    if "child" in kept:
        words += ["--child", kept["child"], "--min-count-child", str(child_min) if child_min else "MIN"]
        where = "{}, {} and {}".format(kept["A"], kept["B"], kept["child"])
    words += [kept["A"], kept["B"]]
    return ("The k-mer databases are kept in {}. Choose the cut-offs marked MIN and MAX from the histograms and dump "
            "again, without counting:\n  {}".format(where, " ".join(words)))


if __name__ == "__main__":
    main()
