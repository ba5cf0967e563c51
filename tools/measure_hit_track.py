#!/usr/bin/env python3
"""Rate of the hit tracker: HitTracker.runs() on a batch of synthetic haplotype reads against haplotype-shaped lists
(tbk_synth_hap_keys_device / tbk_synth_hap_reads_device), with Classifier.classify_batch on the same batch and tables
beside it as the yardstick.  Both calls start from a batch in host memory and end with their result in host memory; each
is warmed up once and the median of three runs is reported, in Gbases/s.  One JSON object on stdout:

    python tools/measure_hit_track.py [--genome 60000000] [--reads 4000] [--length 15000] [--k 21] [--out FILE]

The marking kernel asks two standalone tables (A, then B where A missed): two dependent random 64-byte lines per clean
window; the probe kernel reads one line that both lists share, and re-uses it along a minimizer's run."""
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
    ap.add_argument("--genome", type=int, default=60_000_000)
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--length", type=int, default=15000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--snp-rate", type=float, default=1 / 500)
    ap.add_argument("--error-rate", type=float, default=0.002)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import __graft_entry__ as entry

    entry.build()
    from trio_binning_amd import _lib, kmers
    from trio_binning_amd._lib import check, lib

    dev, k, R, L = 0, args.k, args.reads, args.length
    snp24 = int(round(args.snp_rate * (1 << 24)))
    cap = int(2.2 * args.genome * args.snp_rate * k) + (1 << 16)

    def dalloc(n):
        p = C.c_void_p()
        check(lib.tbk_device_alloc(dev, n, C.byref(p)))
        return p.value

    d_keys = dalloc(2 * cap * 8)
    got = C.c_uint64()
    check(lib.tbk_synth_hap_keys_device(dev, 0x5EED0001, args.genome, snp24, k, C.c_void_p(d_keys), C.c_void_p(d_keys + cap * 8), cap, C.byref(got)))
    n = got.value
    keys = np.empty(2 * cap, dtype=np.uint64)
    check(lib.tbk_memcpy_d2h(dev, keys.ctypes.data, C.c_void_p(d_keys), keys.nbytes))
    d_bases, d_offs = dalloc(R * L + 32), dalloc((R + 1) * 8)
    check(lib.tbk_synth_hap_reads_device(dev, 0x5EED0001, args.genome, snp24, 0x5EED0002, 0, R, L, int(args.error_rate * (1 << 24)),
                                         C.c_void_p(d_bases), C.c_void_p(d_offs)))
    bases, offs = np.empty(R * L, dtype=np.uint8), np.empty(R + 1, dtype=np.uint64)
    check(lib.tbk_memcpy_d2h(dev, bases.ctypes.data, C.c_void_p(d_bases), bases.nbytes))
    check(lib.tbk_memcpy_d2h(dev, offs.ctypes.data, C.c_void_p(d_offs), offs.nbytes))
    for p in (d_keys, d_bases, d_offs):
        check(lib.tbk_device_free(dev, C.c_void_p(p)))

    def median_seconds(call):
        call()  # warm-up: buffers grown, tables hashed, pages touched
        times = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
        return statistics.median(times), times

    a, b = kmers.HashSet.from_keys(keys[:n], k), kmers.HashSet.from_keys(keys[cap:cap + n], k)
    with kmers.Classifier(a, b) as cls, kmers.HitTracker(a, b) as tracker:
        runs, counts = tracker.runs(bases, offs)
        same = bool(np.array_equal(counts, cls.classify_batch(bases, offs)))
        t_runs, all_runs = median_seconds(lambda: tracker.runs(bases, offs))
        t_marks, all_marks = median_seconds(lambda: tracker.marks(bases, offs))
        t_cls, all_cls = median_seconds(lambda: cls.classify_batch(bases, offs))
    total = R * L
    result = {
        "device": _lib.device_name(dev), "k": k, "list_keys_each": int(n), "reads": R, "read_length": L, "bases": total,
        "markers": int(counts.sum()), "raw_runs": int(runs.size), "counts_equal_classify_batch": same,
        "runs_gbases_per_s": round(total / t_runs / 1e9, 3), "marks_gbases_per_s": round(total / t_marks / 1e9, 3),
        "classify_batch_gbases_per_s": round(total / t_cls / 1e9, 3),
        "runs_seconds": [round(t, 5) for t in all_runs], "marks_seconds": [round(t, 5) for t in all_marks],
        "classify_batch_seconds": [round(t, 5) for t in all_cls],
        "method": "host batch in, host result out; one warm-up, median of {} runs".format(args.runs),
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    a.close()
    b.close()


if __name__ == "__main__":
    main()
