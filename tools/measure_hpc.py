#!/usr/bin/env python3
"""Rates of homopolymer compression (tbk_hpc, csrc/tbk_hpc.hip) and of what it is put in front of.

The sequence is random with homopolymer runs of geometric length (mean --mean-run, 1.4: a run of n bases has probability
(1 - p) p^(n - 1), p = 1 - 1 / mean, and neighbouring runs differ), cut into reads of --length bases.

  compress   HomopolymerCompressor.compress_device on one batch of --bases bases resident in HBM: wall time of the call (it
             returns when the result is complete), one warm-up and the median of --runs runs; the bytes the kernels move
             per base (the input twice - once to mark, once to scatter -, the output once, the two bitmaps written and read:
             4 x 1/8); the GB/s that is, beside tbk_calib_stream measured in the same process
  counter    KmerCounter.add_device of the same batch, plain and compressing: the counting kernel's own time
             (kernel_timing), and for the compressing counter the compress time beside it
  e2e        classify-by-kmers on one FASTA file of --e2e-bases bases (reads cut from two haplotypes whose parents were
             counted by find-unique-kmers with and without --compress), with and without --compress: wall time of the
             whole command, and the compressed loop's own account of where its time went (TBK_STATS)

One JSON line on stdout; --out writes it to a file too.

    python tools/measure_hpc.py [--bases 268435456] [--length 15000] [--legs compress,counter,e2e] [--out FILE]"""
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


def runny(rng, n, mean_run):
    """n bases in runs of geometric length with that mean; neighbouring runs differ."""
    symbols = int(n / mean_run * 1.02) + 16
    step = rng.integers(1, 4, symbols, dtype=np.uint8)
    codes = (np.cumsum(step, dtype=np.uint8) & 3)
    out = np.repeat(np.frombuffer(b"ACGT", dtype=np.uint8)[codes], rng.geometric(1.0 / mean_run, symbols))
    assert out.size >= n
    return out[:n].copy()


def write_fasta(path, genomes, n_reads, length, rng):
    """n_reads reads of `length` bases cut from the genomes in turn, as FASTA; returns the bases written."""
    per = 4096
    with open(path, "wb") as fh:
        for first in range(0, n_reads, per):
            m = min(per, n_reads - first)
            rows = np.empty((m, 10 + length + 1), dtype=np.uint8)
            rows[:, 0] = ord(">")
            number = np.arange(first, first + m)
            for digit in range(8):
                rows[:, 8 - digit] = ord("0") + (number // 10 ** digit) % 10
            rows[:, 9] = rows[:, -1] = ord("\n")
            for i in range(m):
                g = genomes[(first + i) % len(genomes)]
                p = int(rng.integers(0, g.size - length))
                rows[i, 10:10 + length] = g[p:p + length]
            fh.write(rows.tobytes())
    return n_reads * length


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=256 << 20)
    ap.add_argument("--length", type=int, default=15000)
    ap.add_argument("--mean-run", type=float, default=1.4)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--legs", default="compress,counter,e2e")
    ap.add_argument("--e2e-bases", type=int, default=1_500_000_000)
    ap.add_argument("--e2e-genome", type=int, default=2_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import __graft_entry__ as entry

    entry.build()
    from trio_binning_amd import _lib, kmers
    from trio_binning_amd._lib import check, lib

    dev, legs = 0, args.legs.split(",")
    rng = np.random.default_rng(14)
    result = {"device": _lib.device_name(dev), "read_length": args.length, "mean_run": args.mean_run, "k": args.k,
              "method": "one warm-up, median of {} runs".format(args.runs)}

    if "compress" in legs or "counter" in legs:
        n_reads = args.bases // args.length
        total = n_reads * args.length
        bases = runny(rng, total, args.mean_run)
        offsets = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(args.length)
        d_bases, d_offsets = C.c_void_p(), C.c_void_p()
        check(lib.tbk_device_alloc(dev, total + 64, C.byref(d_bases)))
        check(lib.tbk_device_alloc(dev, offsets.nbytes, C.byref(d_offsets)))
        check(lib.tbk_memcpy_h2d(dev, d_bases, bases.ctypes.data, total))
        check(lib.tbk_memcpy_h2d(dev, d_offsets, offsets.ctypes.data, offsets.nbytes))
        result.update({"bases": total, "reads": n_reads})
        compress_ms = None
        if "compress" in legs:
            with kmers.HomopolymerCompressor(dev) as comp:
                times, kept = [], 0
                for run in range(args.runs + 1):
                    check(lib.tbk_device_sync(dev))
                    t = time.perf_counter()
                    kept = comp.compress_device(d_bases.value, d_offsets.value, n_reads, total, True)[2]
                    if run:
                        times.append(time.perf_counter() - t)
            t = statistics.median(times)
            compress_ms = t * 1e3
            per_base = 2.0 + kept / total + 4 / 8
            rate = C.c_double()
            check(lib.tbk_calib_stream(dev, 1 << 30, 5, C.byref(rate)))
            result["compress"] = {"ms": round(t * 1e3, 3), "gbases_per_s": round(total / t / 1e9, 2), "seconds": [round(x, 5) for x in times],
                                  "kept_bases": kept, "shrink": round(kept / total, 4), "bytes_per_base": round(per_base, 3),
                                  "gb_per_s": round(per_base * total / t / 1e9, 1), "calib_stream_gb_per_s": round(rate.value / 1e9, 1),
                                  "of_stream": round(per_base * total / t / rate.value, 3)}
        if "counter" in legs:
            row = {}
            for name, compress in (("plain", False), ("compressing", True)):
                with kmers.KmerCounter(args.k, int(1.1 * total), dev, compress=compress) as counter:
                    counter.add_device(d_bases.value, d_offsets.value, n_reads, total)
                    launches, windows, ms = counter.kernel_timing()
                    st = counter.stats()
                    row[name] = {"count_kernel_ms": round(ms, 3), "launches": launches, "window_starts": windows, "bases_added": st["bases_added"],
                                 "distinct": st["distinct"], "gbases_in_per_s": round(total / ms / 1e6, 2)}
            if compress_ms is not None:
                row["compressing"]["compress_ms"] = round(compress_ms, 3)
                row["compress_over_count"] = round(compress_ms / row["compressing"]["count_kernel_ms"], 3)
            result["counter"] = row
        lib.tbk_device_free(dev, d_bases)
        lib.tbk_device_free(dev, d_offsets)
        del bases

    if "e2e" in legs:
        work = tempfile.mkdtemp(prefix="measure_hpc_")
        genomes = [runny(rng, args.e2e_genome, args.mean_run) for _ in range(2)]
        parents = []
        for i, g in enumerate(genomes):  # 30 x of exact 150-base reads, as FASTA
            path = os.path.join(work, "parent%d.fa" % i)
            write_fasta(path, [g], g.size * 30 // 150, 150, rng)
            parents.append(path)
        reads = os.path.join(work, "reads.fa")
        n_bases = write_fasta(reads, genomes, args.e2e_bases // args.length, args.length, rng)
        env = dict(os.environ, PYTHONPATH=ROOT, TBK_STATS="1")
        cuts = ["--min-count-a", "5", "--max-count-a", "200", "--min-count-b", "5", "--max-count-b", "200"]
        row = {"bases": n_bases, "reads": args.e2e_bases // args.length}
        for name, flag in (("plain", []), ("compress", ["--compress"])):
            out = os.path.join(work, name)
            os.makedirs(out)
            subprocess.run([sys.executable, "-m", "trio_binning_amd.find_unique_kmers", "-k", str(args.k), "-o", out, "-s", out] + cuts + flag + parents,
                           env=env, check=True, stderr=subprocess.DEVNULL, timeout=600)
            lists = [os.path.join(out, "hap%s_only_kmers.txt" % h) for h in "AB"]
            prefixes = ["--haplotype-a-out-prefix", os.path.join(out, "hapA"), "--haplotype-b-out-prefix", os.path.join(out, "hapB"),
                        "--unclassified-out-prefix", os.path.join(out, "unclassified")]
            t = time.perf_counter()
            done = subprocess.run([sys.executable, "-m", "trio_binning_amd.classify_by_kmers", reads] + lists + flag + prefixes, env=env, check=True,
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
            wall = time.perf_counter() - t
            stats = [line for line in done.stderr.decode().splitlines() if line.startswith("tbk-stats ")]
            tsv = done.stdout.decode().splitlines()
            row[name] = {"wall_s": round(wall, 3), "gbases_per_s": round(n_bases / wall / 1e9, 3), "list_lines": [sum(1 for _ in open(p)) for p in lists],
                         "bins": {b: sum(1 for line in tsv if line.split("\t")[1] == b) for b in "ABU"},
                         "stats": json.loads(stats[-1][len("tbk-stats "):]) if stats else None}
            for f in os.listdir(out):
                os.remove(os.path.join(out, f))
        for p in parents + [reads]:
            os.remove(p)
        result["e2e"] = row

    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
