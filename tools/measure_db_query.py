#!/usr/bin/env python3
"""Rate of the database query: DatabaseQuery.add() on batches of synthetic contigs against a count database of about
--genome 21-mers.  The database is counted here, by KmerCounter, from a random genome added twice (every k-mer's counter
is 2); the r10/r11 measurements crafted theirs from random ranks, but a sequence looked up in random ranks finds
nothing, and the lookup's cost lies in the windows it finds (the bucket search, the counter, the seen bit, the copy).
A batch is contigs of --length bases cut from the genome in order, wrapping round (a 300 Mbase batch of a 100 Mbase
genome holds every k-mer three times), with --error-rate substitutions, so that some windows are absent.

Every call starts from the batch in host memory and ends with its result in host memory; the session is reset (not
timed) before each call; each leg is warmed up once and the median of --runs runs is reported.  Legs per batch:

  add          add() without counts, a session without copies
  add_counts   add() that brings one byte per base home
  add_copies   add() of a session made with copies (a 32-bit atomic add per found window more)

--no-directory-library names a variant of the library whose lookup bisects the whole database for every window
(VARIANT_SRC=tbk_query tools/build_variant.sh query_nodir -DTBK_LOOKUP_NO_DIRECTORY): the `add` leg is repeated with it
in a fresh process, after this one's database is closed, and joins the record as "no_directory".  One JSON line on
stdout; --out writes it to a file too.

    python tools/measure_db_query.py [--genome 100000000] [--batches 60000000,300000000] [--length 15000] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--batches", default="60000000,300000000")
    ap.add_argument("--length", type=int, default=15000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--error-rate", type=float, default=0.001)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--legs", default="add,add_counts,add_copies")
    ap.add_argument("--no-directory-library", default="")
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
    result = {"device": _lib.device_name(dev), "library": os.path.basename(os.environ.get("TBK_LIBRARY", "")), "k": k, "genome": args.genome,
              "database_kmers": len(database), "contig_length": L, "error_rate": args.error_rate, "setup_s": round(time.perf_counter() - t0, 2),
              "method": "host batch in, host result out; session reset before each call, not timed; one warm-up, median of {} runs".format(args.runs),
              "batches": []}

    def sync():
        check(lib.tbk_device_sync(dev))

    def median_seconds(query, call):
        times = []
        for run in range(args.runs + 1):  # run 0 warms up: buffers grown, pages touched
            query.reset()
            sync()
            t = time.perf_counter()
            call()
            if run:
                times.append(time.perf_counter() - t)
        return statistics.median(times), times

    legs = args.legs.split(",")
    for total in (int(x) for x in args.batches.split(",")):
        n = total // L
        bases = np.concatenate([genome] * (n * L // args.genome) + [genome[:n * L % args.genome]]) if n * L > args.genome else genome[:n * L].copy()
        flip = rng.integers(0, bases.size, int(bases.size * args.error_rate))
        bases[flip] = np.frombuffer(b"CGTA", dtype=np.uint8)[(bases[flip] >> 1) & 3]  # A -> C, C -> G, G -> A, T -> T: a substitution for three bases of four
        offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
        row = {"contigs": n, "bases": int(bases.size)}
        with database.query() as plain, database.query(copies=True) as with_copies:
            per_read = plain.add(bases, offs)
            row["clean"], row["found"] = int(per_read[:, 0].sum()), int(per_read[:, 1].sum())
            row["seen"], row["solid"] = plain.completeness()
            for leg in legs:
                call = {"add": lambda: plain.add(bases, offs), "add_counts": lambda: plain.add(bases, offs, return_counts=True),
                        "add_copies": lambda: with_copies.add(bases, offs)}[leg]
                t, every = median_seconds(with_copies if leg == "add_copies" else plain, call)
                row[leg + "_ms"] = round(t * 1e3, 3)
                row[leg + "_gbases_per_s"] = round(bases.size / t / 1e9, 3)
                row[leg + "_seconds"] = [round(x, 5) for x in every]
        result["batches"].append(row)
        del bases
    database.close()
    if args.no_directory_library:
        cmd = [sys.executable, os.path.abspath(__file__), "--genome", str(args.genome), "--batches", args.batches, "--length", str(L), "--k", str(k),
               "--error-rate", str(args.error_rate), "--runs", str(args.runs), "--legs", "add"]
        done = subprocess.run(cmd, env=dict(os.environ, TBK_LIBRARY=os.path.abspath(args.no_directory_library)), stdout=subprocess.PIPE, timeout=900)
        result["no_directory"] = json.loads(done.stdout.decode().strip().splitlines()[-1]) if done.returncode == 0 else {"returncode": done.returncode}
        if done.returncode == 0:
            for mine, other in zip(result["batches"], result["no_directory"]["batches"]):
                assert (mine["clean"], mine["found"], mine["seen"]) == (other["clean"], other["found"], other["seen"]), "the variant answers differently"
                mine["no_directory_over_directory"] = round(other["add_ms"] / mine["add_ms"], 2)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
