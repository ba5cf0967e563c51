#!/usr/bin/env python3
"""Rate of the hit tracker: HitTracker.runs() on a batch of synthetic haplotype reads against haplotype-shaped lists
(tbk_synth_hap_keys_device / tbk_synth_hap_reads_device), with Classifier.classify_batch on the same batch and tables
beside it as the yardstick.  Both calls start from a batch in host memory and end with their result in host memory; each
is warmed up once and the median of three runs is reported, in Gbases/s.  One JSON object on stdout:

    python tools/measure_hit_track.py [--genome 60000000] [--reads 4000] [--length 15000] [--k 21] [--out FILE]

With --compress the legs are run in homopolymer-compressed space instead (one JSON object, "mode": "compress"): the synthetic
reads are compressed once (batch P), the lists are made of P's own k-mers (one site per 500 bases, k neighbouring windows each,
A and B in turn), and batch S is P with every base written a geometric number of times (mean 1.4), so S compresses to P.
Timed: runs() and marks() on P (the plain calls), runs(compress=True) and marks(compress=True) on S with the same tables,
compress_host on S alone, and the lift launch of S's run endpoints alone, by HIP events around the launch.

    python tools/measure_hit_track.py --compress [--out FILE]

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
    ap.add_argument("--compress", action="store_true", help="the legs in homopolymer-compressed space (see above)")
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

    if args.compress:
        result = compressed_legs(args, bases, offs, median_seconds)
        result["device"] = _lib.device_name(dev)
        finish(args, result)
        return

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
    finish(args, result)
    a.close()
    b.close()


def finish(args, result):
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def own_keys(cb, co, k, rng, every=500):
    """canonical keys of the compressed batch's own windows, shaped like haplotype lists: one site per `every` bases, the k
    neighbouring windows over it, the sites given to A and B in turn (a key both would hold stays in A)"""
    code = np.zeros(256, dtype=np.uint64)
    for i, c in enumerate(b"ACGT"):
        code[c] = i
    lengths = np.diff(co.astype(np.int64))
    starts, hap, n_sites = [], [], 0
    for r in np.flatnonzero(lengths >= 2 * k):
        sites = rng.integers(0, lengths[r] - 2 * k + 1, max(int(lengths[r]) // every, 1))
        starts.append(int(co[r]) + (sites[:, None] + np.arange(k)[None, :]).ravel())
        hap.append(np.repeat((n_sites + np.arange(sites.size)) % 2, k))
        n_sites += sites.size
    starts, hap = np.concatenate(starts), np.concatenate(hap)
    c = code[cb]
    fwd, rc = np.zeros(starts.size, dtype=np.uint64), np.zeros(starts.size, dtype=np.uint64)
    for j in range(k):
        fwd |= c[starts + j] << np.uint64(2 * j)
        rc |= (np.uint64(3) - c[starts + k - 1 - j]) << np.uint64(2 * j)
    keys = np.minimum(fwd, rc)
    keys_a = np.unique(keys[hap == 0])
    return keys_a, np.setdiff1d(keys[hap == 1], keys_a)


def compressed_legs(args, bases, offs, median_seconds):
    from trio_binning_amd import kmers
    from trio_binning_amd._lib import check, lib

    k, rng = args.k, np.random.default_rng(0x5EED0003)
    hip = C.CDLL("libamdhip64.so")
    with kmers.HomopolymerCompressor(0) as comp:
        cb, co = comp.compress(bases, offs, False)  # batch P
        times = rng.geometric(1 / 1.4, cb.size)
        big = np.repeat(cb, times)  # batch S
        big_off = np.concatenate([[0], np.cumsum(times)])[co.astype(np.int64)].astype(np.uint64)
        keys_a, keys_b = own_keys(cb, co, k, rng)
        a, b = kmers.HashSet.from_keys(keys_a, k), kmers.HashSet.from_keys(keys_b, k)
        with kmers.HitTracker(a, b) as tracker:
            runs, counts = tracker.runs(cb, co)
            lifted, counts_c = tracker.runs(big, big_off, compress=True)
            same = bool(np.array_equal(counts, counts_c) and runs.size == lifted.size and np.array_equal(runs["markers"], lifted["markers"]))
            legs = {}
            for name, call in (("plain_runs", lambda: tracker.runs(cb, co)), ("compressed_runs", lambda: tracker.runs(big, big_off, compress=True)),
                               ("plain_marks", lambda: tracker.marks(cb, co)), ("compressed_marks", lambda: tracker.marks(big, big_off, compress=True)),
                               ("compress_host", lambda: comp.compress_host(big, big_off, False))):
                legs[name] = median_seconds(call)
        # the lift launch alone: the endpoints of P's runs as stream positions of S's compressed form, already in HBM
        comp.compress_host(big, big_off, False)
        at = co[runs["read"].astype(np.int64)]
        positions = np.stack([at + runs["first"], at + runs["last"], at + runs["last"] + np.uint64(k)], axis=1).ravel().astype(np.uint64)
        d_in, d_out = C.c_void_p(), C.c_void_p()
        check(lib.tbk_device_alloc(0, max(positions.nbytes, 8), C.byref(d_in)))
        check(lib.tbk_device_alloc(0, max(positions.nbytes, 8), C.byref(d_out)))
        check(lib.tbk_memcpy_h2d(0, d_in, positions.ctypes.data, positions.nbytes))
        lib.tbk_hpc_lift_device_.restype = C.c_int
        lib.tbk_hpc_lift_device_.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        e0, e1, ms = C.c_void_p(), C.c_void_p(), C.c_float()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
        lift_ms = []
        for _ in range(args.runs + 1):  # the first is the warm-up
            assert hip.hipEventRecord(e0, None) == 0
            check(lib.tbk_hpc_lift_device_(comp._h, d_in, positions.size, d_out, None))
            assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
            assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            lift_ms.append(ms.value)
        got = np.empty(positions.size, dtype=np.uint64)
        check(lib.tbk_memcpy_d2h(0, got.ctypes.data, d_out, got.nbytes))
        starts = np.concatenate([[0], np.cumsum(times)]).astype(np.uint64)
        same = same and bool(np.array_equal(got, starts[positions.astype(np.int64)]))
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
        for p in (d_in, d_out):
            check(lib.tbk_device_free(0, p))
        a.close()
        b.close()
    result = {"mode": "compress", "k": k, "list_keys": [int(keys_a.size), int(keys_b.size)], "reads": int(co.size - 1),
              "bases_given": int(big.size), "bases_compressed": int(cb.size), "markers": int(counts.sum()), "raw_runs": int(runs.size),
              "compressed_legs_agree_with_plain": same, "lift_positions": int(positions.size),
              "lift_launch_ms": [round(t, 4) for t in lift_ms[1:]], "lift_launch_ms_median": round(statistics.median(lift_ms[1:]), 4),
              "method": "host batch in, host result out; one warm-up, median of {} runs; the lift launch by HIP events".format(args.runs)}
    for name, (median, every) in legs.items():
        result[name + "_ms"] = round(median * 1e3, 3)
        result[name + "_seconds"] = [round(t, 5) for t in every]
    return result


if __name__ == "__main__":
    main()
