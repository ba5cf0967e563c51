#!/usr/bin/env python3
"""What the repair candidates cost beside the pass that finds the broken windows: DatabaseQuery.repairs() against
DatabaseQuery.add(), on one resident session and one synthetic batch of assembly-like size.

The database and the batch are measure_copy_track.py's: about --genome 21-mers counted by KmerCounter from a random genome
added twice (every counter is 2), and contigs of --length bases cut from that genome in order, --bases of them in one batch,
with --error-rate planted one-base errors per base: a third substituted, a third missing, a third extra bases.  `add` is the
yardstick: the lookup pass of `repairs` reads what it reads and writes two bits per stream position where add sends atomics;
the heads of the stretches are then compacted, and the repair kernel's time is set by the number of stretches.

Every call starts from the batch in host memory and ends with its result in host memory, with the stream idle on either side.
One warm-up, then the median of --runs runs.  The split of `repairs` is the library's own host clock (tbk_kmerdb_query_repair_times_):
the copy in, the separation, the lookup and the compaction up to the stretch count; then the records and the repair kernel up to
the stream's end (the copy home of 40 bytes per stretch is in the whole call only).  One JSON line on stdout; --out writes it to
a file too.

    python tools/measure_repairs.py [--genome 100000000] [--bases 64000000] [--error-rate 1e-4] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--bases", type=int, default=64_000_000)
    ap.add_argument("--length", type=int, default=15000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--error-rate", type=float, default=1e-4)
    ap.add_argument("--min-support", type=int, default=None)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import __graft_entry__ as entry

    if not os.environ.get("TBK_LIBRARY"):
        entry.build()
    from trio_binning_amd import _lib, kmers
    from trio_binning_amd._lib import check, lib

    dev, k, L = 0, args.k, args.length
    support = args.min_support or (k + 1) // 2
    rng = np.random.default_rng(13)
    t0 = time.perf_counter()
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, args.genome, dtype=np.uint8)]
    chunk = 1 << 24
    with kmers.KmerCounter(k, int(1.1 * args.genome)) as counter:
        for _ in range(2):
            for lo in range(0, args.genome, chunk):  # (chunks overlap by k - 1 bases: every window is counted once per round)
                part = genome[lo:min(args.genome, lo + chunk + k - 1)]
                counter.add(part, np.array([0, part.size], dtype=np.uint64))
        database = counter.database()
    n = args.bases // L
    bases = np.concatenate([genome] * (n * L // args.genome) + [genome[:n * L % args.genome]]) if n * L > args.genome else genome[:n * L].copy()
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    # the planted errors: distinct positions, dealt in turn to the three kinds
    planted = np.unique(rng.integers(0, bases.size, int(bases.size * args.error_rate)))
    sub, missing, extra = planted[0::3], planted[1::3], planted[2::3]
    bases[sub] = np.frombuffer(b"CGTA", dtype=np.uint8)[((bases[sub] >> 1) ^ (bases[sub] >> 2)) & 3]  # A -> C -> G -> T -> A
    copies = np.ones(bases.size, dtype=np.uint8)
    copies[missing] = 0
    copies[extra] = 2  # the base twice, and the first of the two made another base below
    ends = np.zeros(bases.size + 1, dtype=np.int64)
    np.cumsum(copies, out=ends[1:])
    first_of_two = ends[extra]
    bases = np.repeat(bases, copies)
    bases[first_of_two] = np.frombuffer(b"CGTA", dtype=np.uint8)[((bases[first_of_two] >> 1) ^ (bases[first_of_two] >> 2)) & 3]
    offs = ends[offs.astype(np.int64)].astype(np.uint64)
    result = {"device": _lib.device_name(dev), "k": k, "genome": args.genome, "database_kmers": len(database), "contigs": n, "bases": int(bases.size),
              "contig_length": L, "error_rate": args.error_rate, "planted": {"sub": int(sub.size), "missing": int(missing.size), "extra": int(extra.size)},
              "min_count": 2, "min_support": support, "setup_s": round(time.perf_counter() - t0, 2),
              "method": "host batch in, host result out, stream idle either side; add on a reset session (reset not timed); one warm-up, median of "
                        "{} runs; the split is the library's host clock around the stretch count".format(args.runs)}

    def sync():
        check(lib.tbk_device_sync(dev))

    split = []

    def median_ms(call, before=None, after=None):
        times = []
        for run in range(args.runs + 1):  # run 0 warms up: buffers grown, pages touched
            if before:
                before()
            sync()
            t = time.perf_counter()
            call()
            sync()
            if run:
                times.append((time.perf_counter() - t) * 1e3)
                if after:
                    after()
        return statistics.median(times), times

    with database.query() as query:
        add_ms, every = median_ms(lambda: query.add(bases, offs), query.reset)
        result["add_ms"], result["add_every_ms"] = round(add_ms, 3), [round(x, 3) for x in every]
        result["add_gbases_per_s"] = round(bases.size / add_ms / 1e6, 3)
        query.reset()
        per_read = query.add(bases, offs)
        result["clean"], result["found"] = int(per_read[:, 0].sum()), int(per_read[:, 1].sum())
        records = query.repairs(bases, offs, 2, support)
        result["stretches"] = int(records.size)
        result["mended"] = int((records["accepted"] == 1).sum())
        result["ambiguous"] = int((records["accepted"] > 1).sum())
        result["unmended"] = int((records["kind"] == kmers.REPAIR_NONE).sum())
        result["long"] = int((records["kind"] == kmers.REPAIR_LONG).sum())
        result["kinds"] = {name: int((records["kind"] == kind).sum()) for name, kind in (("sub", 1), ("del", 2), ("ins", 3))}

        def keep_split():
            ms = (C.c_double * 2)()
            check(lib.tbk_kmerdb_query_repair_times_(query._h, ms))
            split.append((ms[0], ms[1]))

        ms, every = median_ms(lambda: query.repairs(bases, offs, 2, support), after=keep_split)
        lookup_ms, repair_ms = statistics.median(s[0] for s in split), statistics.median(s[1] for s in split)
        result.update({"repairs_ms": round(ms, 3), "repairs_every_ms": [round(x, 3) for x in every], "repairs_over_add": round(ms / add_ms, 3),
                       "lookup_and_compaction_ms": round(lookup_ms, 3), "lookup_and_compaction_over_add": round(lookup_ms / add_ms, 3),
                       "records_and_repair_kernel_ms": round(repair_ms, 3),
                       "stretches_per_s": round(records.size / repair_ms * 1e3) if repair_ms else None,
                       "repairs_gbases_per_s": round(bases.size / ms / 1e6, 3)})
    database.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
