#!/usr/bin/env python3
"""What the read evidence costs beside the project's own lookup pass: DatabaseQuery.evidence() and its two kernels against
DatabaseQuery.add(), on one resident session and one synthetic batch of HiFi-like reads; then the screen_reads command end to end
beside classify_by_kmers on one FASTQ file.

The database is measure_repairs.py's: about --genome 21-mers counted by KmerCounter from a random genome added twice (every
counter is 2).  The batch is reads of --length bases, --bases of them: all but one in --foreign of them are cut from the genome
in order, the others are random (their windows are absent).  `add` is the yardstick: the lookup pass of `evidence` does the same
searches and writes two bits per stream position where add sends atomics; the evidence kernel then reads the two bitmaps once.

Every call starts from the batch in host memory and ends with its result in host memory, with the stream idle on either side.
One warm-up, then the median of --runs runs.  The two kernel times are device events around each kernel
(tbk_kmerdb_query_evidence_times_).

With --e2e-bases N the same kind of reads are written as a FASTQ file of N bases; python -m trio_binning_amd.screen_reads and
python -m trio_binning_amd.classify_by_kmers (the database against a second one of the foreign reads' k-mers) run on it as child
processes, each --e2e-runs times in turns, the bins gzip'ed by the GPU writer: wall-clock seconds of the whole process, and the
bases per second that makes.  One JSON line on stdout; --out writes it to a file too.

    python tools/measure_screen.py [--genome 100000000] [--bases 64000000] [--e2e-bases 1000000000] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--bases", type=int, default=64_000_000)
    ap.add_argument("--length", type=int, default=15000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--foreign", type=int, default=4, help="one read in this many is random")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--e2e-bases", type=int, default=0)
    ap.add_argument("--e2e-runs", type=int, default=2)
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
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = letters[rng.integers(0, 4, args.genome, dtype=np.uint8)]
    chunk = 1 << 24

    def count(sequence):
        with kmers.KmerCounter(k, int(1.1 * sequence.size) + 1024) as counter:
            for _ in range(2):
                for lo in range(0, sequence.size, chunk):  # (chunks overlap by k - 1 bases: every window is counted once per round)
                    part = sequence[lo:min(sequence.size, lo + chunk + k - 1)]
                    counter.add(part, np.array([0, part.size], dtype=np.uint64))
            return counter.database()

    database = count(genome)

    def reads_of(total):
        """(bases, offsets, foreign bases): reads of L bases cut from the genome in order, every args.foreign-th one random"""
        n = total // L
        own = np.concatenate([genome] * (n * L // args.genome) + [genome[:n * L % args.genome]]) if n * L > args.genome else genome[:n * L].copy()
        rows = own.reshape(n, L)
        strangers = np.arange(args.foreign - 1, n, args.foreign)
        rows[strangers] = letters[rng.integers(0, 4, (strangers.size, L), dtype=np.uint8)]
        return own, np.arange(n + 1, dtype=np.uint64) * np.uint64(L), rows[strangers].reshape(-1)

    bases, offs, _ = reads_of(args.bases)
    n = offs.size - 1
    result = {"device": _lib.device_name(dev), "k": k, "genome": args.genome, "database_kmers": len(database), "reads": n, "bases": int(bases.size),
              "read_length": L, "foreign_one_in": args.foreign, "min_count": 1, "max_count": 255, "setup_s": round(time.perf_counter() - t0, 2),
              "method": "host batch in, host result out, stream idle either side; add on a reset session (reset not timed); one warm-up, median of "
                        "{} runs; the kernels by device events around each".format(args.runs)}

    def sync():
        check(lib.tbk_device_sync(dev))

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
        records = query.evidence(bases, offs)
        assert np.array_equal(records["clean"], per_read[:, 0]) and np.array_equal(records["held"], per_read[:, 1])
        result.update({"clean": int(records["clean"].sum()), "held": int(records["held"].sum()), "covered": int(records["covered"].sum()),
                       "reads_with_a_hit": int((records["held"] > 0).sum()), "reads_held_throughout": int((records["longest"] == L).sum())})
        split = []

        def keep_split():
            ms = (C.c_double * 2)()
            check(lib.tbk_kmerdb_query_evidence_times_(query._h, ms))
            split.append((ms[0], ms[1]))

        ms, every = median_ms(lambda: query.evidence(bases, offs), after=keep_split)
        lookup_ms, evidence_ms = statistics.median(s[0] for s in split), statistics.median(s[1] for s in split)
        result.update({"evidence_ms": round(ms, 3), "evidence_every_ms": [round(x, 3) for x in every], "evidence_over_add": round(ms / add_ms, 3),
                       "lookup_kernel_ms": round(lookup_ms, 3), "lookup_kernel_over_add": round(lookup_ms / add_ms, 3),
                       "evidence_kernel_ms": round(evidence_ms, 3), "evidence_kernel_over_add": round(evidence_ms / add_ms, 4),
                       "evidence_gbases_per_s": round(bases.size / ms / 1e6, 3)})

    if args.e2e_bases:
        with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR")) as tmp:
            reads, offsets, foreign = reads_of(args.e2e_bases)
            m = offsets.size - 1
            fastq = os.path.join(tmp, "reads.fastq")
            quality = b"+\n" + b"I" * L + b"\n"
            with open(fastq, "wb") as fh:
                for i in range(m):
                    fh.write(b"@m64011_%d/%d/ccs\n" % (i // 1000, i))
                    fh.write(reads[i * L:(i + 1) * L].tobytes())
                    fh.write(b"\n" + quality)
            own_path, other_path = os.path.join(tmp, "own.tbkdb"), os.path.join(tmp, "other.tbkdb")
            database.save(own_path)
            other = count(foreign[:min(foreign.size, 16 * chunk)])  # (a second parent for classify_by_kmers: the foreign reads' k-mers)
            other.save(other_path)
            other.close()
            database.close()
            commands = {
                "screen_reads": [sys.executable, "-m", "trio_binning_amd.screen_reads", fastq, own_path, "--min-share", "0.5"],
                "classify_by_kmers": [sys.executable, "-m", "trio_binning_amd.classify_by_kmers", fastq, own_path, other_path, "--min-count-a", "2",
                                      "--max-count-a", "255", "--min-count-b", "2", "--max-count-b", "255"],
            }
            e2e = {"fastq_bytes": os.path.getsize(fastq), "reads": m, "bases": int(reads.size), "seconds": {name: [] for name in commands}}
            env = dict(os.environ, PYTHONPATH=ROOT)
            for _ in range(args.e2e_runs):
                for name, argv in commands.items():
                    t = time.perf_counter()
                    done = subprocess.run(argv, cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
                    e2e["seconds"][name].append(round(time.perf_counter() - t, 3))
                    if done.returncode:
                        raise RuntimeError("{} failed: {}".format(name, done.stderr.decode()[-2000:]))
                    if name == "screen_reads":
                        e2e["screen_reads_stdout"] = done.stdout.decode().splitlines()
            for name in commands:
                best = min(e2e["seconds"][name])
                e2e[name + "_gbases_per_s"] = round(reads.size / best / 1e9, 3)
            e2e["bins_bytes"] = {f: os.path.getsize(os.path.join(tmp, f)) for f in sorted(os.listdir(tmp)) if f.endswith(".gz")}
            result["end_to_end"] = e2e
    else:
        database.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
