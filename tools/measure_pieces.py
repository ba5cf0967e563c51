#!/usr/bin/env python3
"""What the read pieces cost beside the read evidence: DatabaseQuery.pieces() against DatabaseQuery.evidence() on one resident session,
for a batch of HiFi-like reads and a batch of short reads.

The database is measure_screen.py's: about --genome 21-mers counted by KmerCounter from a random genome added twice (every counter
is 2).  A batch is reads of --length (then of --short-length) bases cut from the genome in order, --bases of them, with one base in
--error-every replaced by another: every error breaks k windows, so a 15 kb read falls into about 15 covered pieces with a gap of
one base between them, and about one 150-base read in seven into two.

Every call starts from the batch in host memory and ends with its result in host memory, with the stream idle on either side.
One warm-up, then the median of --runs runs, the calls taking turns.  The kernel times are device events
(tbk_kmerdb_query_evidence_times_, tbk_kmerdb_query_pieces_times_): the lookup pass, the evidence kernel, and everything between
the evidence kernel and the last piece kernel - the side bitmap, three compactions and their scans, and the host's waits for the
three totals that size the lists.  One JSON line on stdout; --out writes it to a file too.

    python tools/measure_pieces.py [--genome 30000000] [--bases 60000000] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=30_000_000)
    ap.add_argument("--bases", type=int, default=60_000_000)
    ap.add_argument("--length", type=int, default=15000)
    ap.add_argument("--short-length", type=int, default=150)
    ap.add_argument("--error-every", type=int, default=1000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import __graft_entry__ as entry

    if not os.environ.get("TBK_LIBRARY"):
        entry.build()
    from trio_binning_amd import _lib, kmers
    from trio_binning_amd._lib import check, lib

    dev, k = 0, args.k
    rng = np.random.default_rng(17)
    t0 = time.perf_counter()
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    codes = rng.integers(0, 4, args.genome, dtype=np.uint8)
    genome = letters[codes]
    chunk = 1 << 24
    with kmers.KmerCounter(k, int(1.1 * genome.size) + 1024) as counter:
        for _ in range(2):
            for lo in range(0, genome.size, chunk):  # (chunks overlap by k - 1 bases: every window is counted once per round)
                part = genome[lo:min(genome.size, lo + chunk + k - 1)]
                counter.add(part, np.array([0, part.size], dtype=np.uint64))
        database = counter.database()

    def reads_of(length):
        """(bases, offsets): reads of `length` bases cut from the genome in order, one base in args.error_every replaced by the next letter"""
        n = args.bases // length
        own = np.resize(codes, n * length).copy()
        at = rng.choice(own.size, own.size // args.error_every, replace=False)
        own[at] = (own[at] + 1) & 3
        return letters[own], np.arange(n + 1, dtype=np.uint64) * np.uint64(length)

    result = {"device": _lib.device_name(dev), "k": k, "genome": args.genome, "database_kmers": len(database), "error_every": args.error_every,
              "method": "host batch in, host result out, stream idle either side; one warm-up, median of {} runs, the calls taking turns; the "
                        "kernels by device events".format(args.runs), "batches": {}}

    def sync():
        check(lib.tbk_device_sync(dev))

    with database.query() as query:
        for name, length in (("long", args.length), ("short", args.short_length)):
            bases, offs = reads_of(length)
            calls = {
                "evidence": lambda: query.evidence(bases, offs),
                "pieces_covered_longest_with_evidence": lambda: query.pieces(bases, offs, which="longest", evidence=True),
                "pieces_covered_all": lambda: query.pieces(bases, offs),
                "pieces_uncovered_all": lambda: query.pieces(bases, offs, side="uncovered"),
            }
            times = {call: [] for call in calls}
            kernels = {call: [] for call in calls}
            for run in range(args.runs + 1):  # run 0 warms up: buffers grown, pages touched
                for call, fn in calls.items():
                    sync()
                    t = time.perf_counter()
                    got = fn()
                    sync()
                    if run:
                        times[call].append((time.perf_counter() - t) * 1e3)
                        ms = (C.c_double * 3)()
                        if call == "evidence":
                            check(lib.tbk_kmerdb_query_evidence_times_(query._h, ms))
                        else:
                            check(lib.tbk_kmerdb_query_pieces_times_(query._h, ms))
                        kernels[call].append(tuple(ms))
            records = query.evidence(bases, offs)
            found, with_it = query.pieces(bases, offs, evidence=True)
            assert with_it.tobytes() == records.tobytes() and found.size == int(records["stretches"].sum())
            assert int((found["end"] - found["first"]).sum()) == int(records["covered"].sum())
            longest = query.pieces(bases, offs, which="longest")
            assert np.array_equal(longest["end"] - longest["first"], records["longest"][records["longest"] > 0])
            batch = {"reads": int(offs.size - 1), "read_length": length, "bases": int(bases.size), "covered": int(records["covered"].sum()),
                     "pieces_covered": int(found.size), "pieces_uncovered": int(query.pieces(bases, offs, side="uncovered").size), "calls": {}}
            for call in calls:
                split = [statistics.median(s[i] for s in kernels[call]) for i in range(3)]
                batch["calls"][call] = {"ms": round(statistics.median(times[call]), 3), "every_ms": [round(x, 3) for x in times[call]],
                                        "lookup_kernel_ms": round(split[0], 3), "evidence_kernel_ms": round(split[1], 3)}
                if call != "evidence":
                    batch["calls"][call]["piece_kernels_ms"] = round(split[2], 3)
                    batch["calls"][call]["over_evidence"] = round(batch["calls"][call]["ms"] / batch["calls"]["evidence"]["ms"], 3)
                    batch["calls"][call]["piece_kernels_over_lookup"] = round(split[2] / split[0], 3)
            result["batches"][name] = batch
    database.close()
    result["setup_and_run_s"] = round(time.perf_counter() - t0, 2)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
