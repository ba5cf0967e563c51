#!/usr/bin/env python3
"""What the copy-number track costs beside the pass that feeds it: DatabaseQuery.track() against DatabaseQuery.add() of a
session made with copies, on one resident session and one synthetic batch of assembly-like size.

The database and the batch are measure_db_query.py's: about --genome 21-mers counted by KmerCounter from a random genome
added twice (every counter is 2, so the one-copy depth --peak is 2), and contigs of --length bases cut from that genome in
order with --error-rate substitutions, --bases of them in one batch.  `add` is the yardstick: the track's lookup pass repeats
its staging, rolling and bisection, gathers the copy counter beside the counter, writes two bytes and five bits per stream
position where add sends atomics, and the bin pass reduces them.

Every call starts from the batch in host memory and ends with its result in host memory, with the stream idle on either side.
`add` is timed on a session that was reset (not timed); `track` on the session as one add left it.  One warm-up, then the median
of --runs runs, for every window size of --windows.  One JSON line on stdout; --out writes it to a file too.

    python tools/measure_copy_track.py [--genome 100000000] [--bases 64000000] [--windows 10000,64] [--out FILE]"""
import argparse
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
    ap.add_argument("--error-rate", type=float, default=0.001)
    ap.add_argument("--windows", default="10000,64")
    ap.add_argument("--peak", type=int, default=2)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import __graft_entry__ as entry

    if not os.environ.get("TBK_LIBRARY"):
        entry.build()
    from trio_binning_amd import _lib, kmers
    from trio_binning_amd._lib import check, lib

    dev, k, L = 0, args.k, args.length
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
    flip = rng.integers(0, bases.size, int(bases.size * args.error_rate))
    bases[flip] = np.frombuffer(b"CGTA", dtype=np.uint8)[(bases[flip] >> 1) & 3]  # A -> C, C -> G, G -> A, T -> T: a substitution for three bases of four
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    result = {"device": _lib.device_name(dev), "k": k, "genome": args.genome, "database_kmers": len(database), "contigs": n, "bases": int(bases.size),
              "contig_length": L, "error_rate": args.error_rate, "peak": args.peak, "setup_s": round(time.perf_counter() - t0, 2),
              "method": "host batch in, host result out, stream idle either side; add on a reset session (reset not timed), track on the session one add "
                        "left; one warm-up, median of {} runs".format(args.runs)}

    def sync():
        check(lib.tbk_device_sync(dev))

    def median_ms(call, before=None):
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
        return statistics.median(times), times

    with database.query(copies=True) as query:
        add_ms, every = median_ms(lambda: query.add(bases, offs), query.reset)
        result["add_copies_ms"], result["add_copies_every_ms"] = round(add_ms, 3), [round(x, 3) for x in every]
        result["add_copies_gbases_per_s"] = round(bases.size / add_ms / 1e6, 3)
        query.reset()
        per_read = query.add(bases, offs)
        result["clean"], result["found"] = int(per_read[:, 0].sum()), int(per_read[:, 1].sum())
        result["track"] = []
        for window in (int(x) for x in args.windows.split(",")):
            bins, _ = query.track(bases, offs, window, args.peak)
            assert int(bins["clean"].sum(dtype=np.uint64)) == result["clean"], "the track counts other clean windows than add"
            ms, every = median_ms(lambda: query.track(bases, offs, window, args.peak))
            result["track"].append({"window": window, "bins": int(bins.size), "collapsed": int(bins["collapsed"].sum(dtype=np.uint64)),
                                    "expanded": int(bins["expanded"].sum(dtype=np.uint64)), "track_ms": round(ms, 3),
                                    "track_gbases_per_s": round(bases.size / ms / 1e6, 3), "track_over_add": round(ms / add_ms, 3),
                                    "track_every_ms": [round(x, 3) for x in every]})
    database.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
