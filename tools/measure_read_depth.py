#!/usr/bin/env python3
"""What the read depth costs beside the read evidence and the project's own lookup pass: DatabaseQuery.read_depth() and its two
kernels against DatabaseQuery.evidence() and DatabaseQuery.add(), on one resident session per database and synthetic batches of
HiFi-like (--length, 15 kb) and Illumina-like (--short-length, 150) reads; then the read_depth command end to end beside
screen_reads on one FASTQ file.

Each batch is measured in two forms, which differ in the database alone.  ONE COUNTER: the random genome was counted --depth
times, so every window of every read carries that counter and every lane of the per-read kernel adds to the same row of its
wave's LDS histogram - a real library's reads, whose counters cluster at its depth.  SPREAD: the genome was counted in blocks
of 64 bases, block j (j mod 255) + 1 times, so a 15 kb read carries every counter from 2 to 255 (the blocks seen once are left
out of a solid database: absent) and its adds spread over the rows.  The yardstick of the per-read kernel is the evidence's lookup
kernel (tbk_screen_lookup_kernel) on the same batch in the same run: the rule of profiles/r28 is that the per-read kernel on the
one-counter batch may not take longer than that.

Every call starts from the batch in host memory and ends with its result in host memory, with the stream idle on either side.
One warm-up, then the median of --runs runs.  The kernel times are device events around each kernel
(tbk_kmerdb_query_read_depth_times_, tbk_kmerdb_query_evidence_times_).  TBK_LIBRARY selects a variant library
(tools/build_variant.sh, e.g. VARIANT_SRC=tbk_read_depth with -DTBK_READ_DEPTH_COMBINE).

With --e2e-bases N the 15 kb reads are written as a FASTQ file of N bases; python -m trio_binning_amd.read_depth --target and
python -m trio_binning_amd.screen_reads run on it against the one-counter database as child processes, each --e2e-runs times in
turns, the bins gzip'ed by the GPU writer: wall-clock seconds of the whole process.  One JSON line on stdout; --out writes it to
a file too.

    python tools/measure_read_depth.py [--genome 4000000] [--bases 64000000] [--e2e-bases 1000000000] [--out FILE]"""
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

BLOCK = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=4_000_000)
    ap.add_argument("--bases", type=int, default=64_000_000)
    ap.add_argument("--length", type=int, default=15000)
    ap.add_argument("--short-length", type=int, default=150)
    ap.add_argument("--depth", type=int, default=30, help="the counter of the one-counter database")
    ap.add_argument("--k", type=int, default=21)
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

    dev, k = 0, args.k
    rng = np.random.default_rng(28)
    t0 = time.perf_counter()
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    size = args.genome // BLOCK * BLOCK
    genome = letters[rng.integers(0, 4, size + k - 1, dtype=np.uint8)]  # (k - 1 bases behind the last block: its windows)
    chunk = 1 << 24

    def one_counter():
        with kmers.KmerCounter(k, int(1.1 * genome.size) + 1024) as counter:
            for _ in range(args.depth):
                for lo in range(0, size, chunk):  # (chunks overlap by k - 1 bases: every window is counted once per round)
                    part = genome[lo:min(genome.size, lo + chunk + k - 1)]
                    counter.add(part, np.array([0, part.size], dtype=np.uint64))
            return counter.database()

    def spread():
        """block j of 64 window starts is counted (j mod 255) + 1 times: in round t, the blocks with t rounds or more, each as a
        sequence of its own with the k - 1 bases behind it"""
        pieces = np.lib.stride_tricks.sliding_window_view(genome, BLOCK + k - 1)[::BLOCK]
        times = np.arange(pieces.shape[0]) % 255 + 1
        with kmers.KmerCounter(k, int(1.1 * genome.size) + 1024) as counter:
            for t in range(1, 256):
                rows = np.ascontiguousarray(pieces[times >= t]).reshape(-1)
                counter.add(rows, np.arange(rows.size // (BLOCK + k - 1) + 1, dtype=np.uint64) * np.uint64(BLOCK + k - 1))
            return counter.database()

    def reads_of(total, length):
        """(bases, offsets): reads of `length` bases cut from the genome in order, again from its start when it is used up"""
        n = total // length
        own = np.concatenate([genome[:size]] * (n * length // size) + [genome[:n * length % size]]) if n * length > size else genome[:n * length].copy()
        return own, np.arange(n + 1, dtype=np.uint64) * np.uint64(length)

    batches = {"long": reads_of(args.bases, args.length), "short": reads_of(args.bases, args.short_length)}
    result = {"device": _lib.device_name(dev), "library": os.environ.get("TBK_LIBRARY", "libtbk_hip.so"), "k": k, "genome": size, "depth": args.depth,
              "bases": args.bases, "lengths": {"long": args.length, "short": args.short_length}, "min_count": 1,
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
        return statistics.median(times)

    def measure(database, form):
        with database.query() as query:
            for name, (bases, offs) in batches.items():
                out = {"reads": int(offs.size - 1)}
                out["add_ms"] = round(median_ms(lambda: query.add(bases, offs), query.reset), 3)
                query.reset()
                per_read = query.add(bases, offs, 1)
                records = query.read_depth(bases, offs)
                assert np.array_equal(records["clean"], per_read[:, 0]) and np.array_equal(records["present"], per_read[:, 1])
                out.update({"clean": int(records["clean"].sum()), "present": int(records["present"].sum()),
                            "medians": {str(v): int(c) for v, c in zip(*np.unique(records["median"], return_counts=True))} if form == "one_counter" else
                            {"lowest": int(records["median"].min()), "highest": int(records["median"].max())},
                            "distinct_depths_of_read_0": int(np.unique(query.add(bases[:int(offs[1])], offs[:2], 1, True)[1]).size)})
                split = {"read_depth": [], "evidence": []}

                def keep(which, hook):
                    ms = (C.c_double * 2)()
                    check(hook(query._h, ms))
                    split[which].append((ms[0], ms[1]))

                out["read_depth_ms"] = round(median_ms(lambda: query.read_depth(bases, offs),
                                                       after=lambda: keep("read_depth", lib.tbk_kmerdb_query_read_depth_times_)), 3)
                out["evidence_ms"] = round(median_ms(lambda: query.evidence(bases, offs), after=lambda: keep("evidence", lib.tbk_kmerdb_query_evidence_times_)), 3)
                for which, names in (("read_depth", ("read_depth_lookup_kernel_ms", "read_depth_kernel_ms")),
                                     ("evidence", ("screen_lookup_kernel_ms", "screen_evidence_kernel_ms"))):
                    for i, field in enumerate(names):
                        out[field] = round(statistics.median(s[i] for s in split[which]), 4)
                out["read_depth_kernel_over_screen_lookup_kernel"] = round(out["read_depth_kernel_ms"] / out["screen_lookup_kernel_ms"], 4)
                out["read_depth_over_evidence"] = round(out["read_depth_ms"] / out["evidence_ms"], 3)
                out["read_depth_over_add"] = round(out["read_depth_ms"] / out["add_ms"], 3)
                out["read_depth_gbases_per_s"] = round(bases.size / out["read_depth_ms"] / 1e6, 3)
                result[form + "_" + name] = out

    uniform = one_counter()
    result["one_counter_database_kmers"] = len(uniform)
    measure(uniform, "one_counter")
    other = spread()
    result["spread_database_kmers"] = len(other)
    result["setup_s"] = round(time.perf_counter() - t0, 2)
    measure(other, "spread")
    other.close()

    if args.e2e_bases:
        with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR")) as tmp:
            L = args.length
            reads, offsets = reads_of(args.e2e_bases, L)
            m = offsets.size - 1
            fastq = os.path.join(tmp, "reads.fastq")
            quality = b"+\n" + b"I" * L + b"\n"
            with open(fastq, "wb") as fh:
                for i in range(m):
                    fh.write(b"@m64011_%d/%d/ccs\n" % (i // 1000, i))
                    fh.write(reads[i * L:(i + 1) * L].tobytes())
                    fh.write(b"\n" + quality)
            own_path = os.path.join(tmp, "own.tbkdb")
            uniform.save(own_path)
            uniform.close()
            commands = {
                "read_depth": [sys.executable, "-m", "trio_binning_amd.read_depth", fastq, own_path, "--target", str(max(args.depth // 2, 1))],
                "screen_reads": [sys.executable, "-m", "trio_binning_amd.screen_reads", fastq, own_path, "--min-share", "0.5"],
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
                    e2e[name + "_stdout"] = done.stdout.decode().splitlines()
            for name in commands:
                e2e[name + "_gbases_per_s"] = round(reads.size / min(e2e["seconds"][name]) / 1e9, 3)
            result["end_to_end"] = e2e
    else:
        uniform.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
