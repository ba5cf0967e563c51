"""Say what is wrong where an assembly disagrees with the reads: the one-base edit that mends each absent stretch.

Every window of every sequence of a FASTA/FASTQ file is looked up in one count database of the reads (``*.tbkdb``, as kept by
find-unique-kmers --keep-databases).  A maximal stretch of clean windows whose k-mers the reads hold fewer than --min-count times
- one line of ``assembly_qv --absent-bed`` - is what an isolated one-base error leaves behind: all its windows share the edited
position.  For every stretch of at most k windows, each substitution, deleted base and inserted base at the positions its windows
share is tried, and accepted when every window over the edit becomes a k-mer the reads hold, with at least --min-support clean
windows to say so (default (k + 1) // 2: an edit verified by one window beside an N or a contig end is weak evidence).

stdout gets one TSV line per sequence - ``name length stretches mended ambiguous unmended long`` - and a last line ``#total
length stretches mended ambiguous unmended long min_count min_support`` (with --apply also ``applied conflicting``).  A stretch
is ``mended`` when exactly one edit was accepted, ``ambiguous`` when several were, ``unmended`` when none was and ``long`` when
it has more than k windows - more than one error, or something larger - and was not attempted.

--edits writes one line per stretch: ``name first windows verdict kind pos ref alt accepted support depth``; ``kind`` is sub,
del, ins or ``.``; ``pos`` is the edited base, or the base an insertion goes in front of; ``ref`` is the sequence's base there
in upper case (``.`` for ins), ``alt`` the new base (``.`` for del); for an ambiguous stretch they describe the first accepted
edit by (kind, pos, base).  --apply writes every sequence as FASTA, one line each, with its mended edits applied: new bases in upper
case, every other base as given.  A mended edit fewer than k positions from another mended edit of the same sequence is not
applied - each was verified with the other's base still in place - and counts as ``conflicting``; ambiguous edits are never
applied.  No verdict on the assembly is computed.
"""
# Run as ``python -m trio_binning_amd.repair_candidates``.  Lookup, stretches and candidates are on the device
# (kmers.DatabaseQuery.repairs); the tables and the application of the edits run on the host.

import argparse
import os
import sys
from os.path import isfile

from . import _lib

_lib.warm_up()  # the HIP runtime starts beside the imports and the argument parsing below

from . import find_unique_kmers as fu, kmers, seq  # noqa: E402

PROG = "repair_candidates"

# Whole records, as for assembly_qv: a record longer than the limit arrives alone in a batch of its own length.
_BATCH_BASES = int(os.environ.get("TBK_BATCH_BASES", str(64 << 20)))
_BATCH_READS = int(os.environ.get("TBK_BATCH_READS", str(1 << 20)))

TSV_COLUMNS = ("name", "length", "stretches", "mended", "ambiguous", "unmended", "long")
EDIT_COLUMNS = ("name", "first", "windows", "verdict", "kind", "pos", "ref", "alt", "accepted", "support", "depth")
KIND_NAMES = (".", "sub", "del", "ins", ".")


def _parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog=PROG, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("assembly", help="contigs to look at, FASTA/FASTQ(.gz) or BAM.")
    parser.add_argument("database", help="the count database of the reads (*.tbkdb, kept by find-unique-kmers --keep-databases)")
    parser.add_argument("--min-count", type=int, default=2, metavar="N",
                        help="the counter a k-mer needs to count as held by the reads (2..255; default 2). 1 - presence - needs a full "
                             "database, kept with find-unique-kmers --keep-singletons")
    parser.add_argument("--min-support", type=int, default=None, metavar="N",
                        help="the clean windows over an edit that must vouch for it (1..32; default (k + 1) // 2)")
    parser.add_argument("--edits", default=None, metavar="PATH", help="write one TSV line per stretch with its verdict and first accepted edit")
    parser.add_argument("--apply", default=None, metavar="PATH", help="write the sequences as FASTA with the mended edits applied")
    return parser


def parse_args(argv=None):
    """The arguments, refused where they can be from the command line and the database's header alone; ``args.info`` is
    that header (``kmers.database_file_info``).  No device is touched."""
    parser = _parser()
    args = parser.parse_args(argv)
    presence = args.min_count == 1  # only a full database holds the k-mers seen once (checked below, by its header)
    if not 2 <= args.min_count <= 255 and not presence:
        parser.error("--min-count {}: need 2 <= N <= 255".format(args.min_count))
    if args.min_support is not None and not 1 <= args.min_support <= 32:
        parser.error("--min-support {}: need 1 <= N <= 32".format(args.min_support))
    for what in (args.assembly, args.database):
        if not isfile(what):
            sys.exit("{}: {} does not exist or is not a file".format(PROG, what))
    if not fu.is_database_path(args.database):
        sys.exit("{}: {} is not a count database (*{}): a k-mer list holds no counts to verify an edit against - keep the reads' database "
                 "with find-unique-kmers --keep-databases".format(PROG, args.database, fu.DATABASE_SUFFIX))
    try:
        args.info = kmers.database_file_info(args.database)
    except (IOError, ValueError) as exc:
        sys.exit("{}: {}: {}".format(PROG, args.database, exc))
    if args.info["compressed"]:
        sys.exit("{}: {} holds homopolymer-compressed k-mers (find-unique-kmers --compress): an edit of the sequence is not defined in "
                 "compressed space. Give a plain database.".format(PROG, args.database))
    if presence and args.info["floor"] != 1:
        parser.error("--min-count 1: need 2 <= N <= 255 with this database, which was kept without the k-mers seen once; keep it "
                     "with find-unique-kmers --keep-databases --keep-singletons to count presence")
    if args.min_support is None:
        args.min_support = (args.info["k"] + 1) // 2
    return args


def verdict(record) -> str:
    """mended, ambiguous, unmended or long: what one ``kmers.REPAIR`` record says of its stretch"""
    if int(record["kind"]) == kmers.REPAIR_LONG:
        return "long"
    accepted = int(record["accepted"])
    return "unmended" if accepted == 0 else "mended" if accepted == 1 else "ambiguous"


def edit_line(name: str, sequence, record) -> str:
    """One --edits line (``EDIT_COLUMNS``) of a record of the sequence whose bytes are ``sequence``."""
    kind = int(record["kind"])
    pos = ref = alt = "."
    if kind in (kmers.REPAIR_SUB, kmers.REPAIR_DEL, kmers.REPAIR_INS):
        pos = str(int(record["pos"]))
        if kind != kmers.REPAIR_INS:
            ref = chr(int(sequence[int(record["pos"])])).upper()
        if kind != kmers.REPAIR_DEL:
            alt = chr(int(record["base"]))
    return "\t".join([name, str(int(record["first"])), str(int(record["windows"])), verdict(record), KIND_NAMES[kind], pos, ref, alt,
                      str(int(record["accepted"])), str(int(record["support"])), str(int(record["depth"]))]) + "\n"


def apply_edits(sequence: bytes, records, k: int):
    """(mended sequence, applied, conflicting): the bytes of one sequence with the edits of its mended records - accepted == 1 -
    applied, new bases in upper case and every other byte as given.  A mended edit whose ``pos`` lies fewer than k positions from
    another mended edit's is left out, and so is that other one; both count as conflicting.  Nothing else of ``records`` (all
    of one sequence) is applied.  A pure function: no device."""
    edits = sorted((int(r["pos"]), int(r["kind"]), int(r["base"])) for r in records if int(r["accepted"]) == 1)
    keep = []
    for i, edit in enumerate(edits):
        near = (i > 0 and edit[0] - edits[i - 1][0] < k) or (i + 1 < len(edits) and edits[i + 1][0] - edit[0] < k)
        if not near:
            keep.append(edit)
    out = bytearray(sequence)
    for pos, kind, base in reversed(keep):  # from the right: the positions to the left stay what they were
        if kind == kmers.REPAIR_SUB:
            out[pos] = base
        elif kind == kmers.REPAIR_DEL:
            del out[pos]
        else:
            out[pos:pos] = bytes([base])
    return bytes(out), len(keep), len(edits) - len(keep)


def main(argv=None):
    """Main method of program"""
    args = parse_args(argv)
    import numpy as np

    k = args.info["k"]
    edits_tmp = args.edits + ".tmp" if args.edits else None  # written beside their places and renamed: a run that fails leaves no half a file
    apply_tmp = args.apply + ".tmp" if args.apply else None
    out = sys.stdout
    total = [0] * 8  # length, stretches, mended, ambiguous, unmended, long, applied, conflicting
    column = {"mended": 2, "ambiguous": 3, "unmended": 4, "long": 5}
    try:
        with kmers.KmerDatabase.load(args.database) as database, database.query() as query, seq.BatchReader(args.assembly) as reader, \
                open(edits_tmp or os.devnull, "w") as edits, open(apply_tmp or os.devnull, "wb") as mended:
            batch = seq.Batch()
            try:
                while reader.next_batch(batch, _BATCH_BASES, _BATCH_READS):
                    bases, base_off, names, name_off = batch.arrays()[:4]
                    n = batch.n_reads
                    records = query.repairs(bases, base_off, args.min_count, args.min_support)
                    text = bytes(names)
                    label = [text[int(name_off[i]):int(name_off[i + 1])].decode() for i in range(n)]
                    off = base_off.astype(np.int64)
                    bounds = np.searchsorted(records["read"], np.arange(n + 1, dtype=np.uint64))  # the records are ordered by (read, first)
                    lines = []
                    for i in range(n):
                        own = records[int(bounds[i]):int(bounds[i + 1])]
                        sequence = np.asarray(bases)[int(off[i]):int(off[i + 1])]
                        row = [int(off[i + 1] - off[i]), own.size, 0, 0, 0, 0]
                        for record in own:
                            row[column[verdict(record)]] += 1
                        if edits_tmp:
                            edits.write("".join(edit_line(label[i], sequence, record) for record in own))
                        if apply_tmp:
                            fixed, applied, conflicting = apply_edits(sequence.tobytes(), own, k)
                            mended.write(b">" + label[i].encode() + b"\n" + fixed + b"\n")
                            total[6] += applied; total[7] += conflicting
                        for j in range(6):
                            total[j] += row[j]
                        lines.append("\t".join([label[i]] + [str(v) for v in row]) + "\n")
                    out.write("".join(lines))
            finally:
                batch.close()
        out.write("\t".join(["#total"] + [str(v) for v in total[:6]] + [str(args.min_count), str(args.min_support)] +
                            ([str(total[6]), str(total[7])] if apply_tmp else [])) + "\n")
        out.flush()
        if edits_tmp:
            os.replace(edits_tmp, args.edits)
        if apply_tmp:
            os.replace(apply_tmp, args.apply)
    except BaseException:
        for tmp in (edits_tmp, apply_tmp):
            if tmp and os.path.exists(tmp):
                os.remove(tmp)
        raise


if __name__ == "__main__":
    main()
