"""Time tbk_kmerdb_union on two synthetic full databases beside the baseline it replaces, a sort of their concatenation.

    python tools/measure_union.py [--n 100000000] [--k 21] [--runs 7] [--out PATH]

A and B hold `n` entries each; half of B's keys are A's.  The keys are tbk_synth_keys_device's (distinct by construction),
turned into ranks and sorted with their counters by the path tbk_counter_export takes (tbk_launch_db_rank,
tbk_launch_sort_u64_u8), and adopted as databases where they lie.  Both legs run in this process, one after the other: HIP
events on the null stream around the call, one warm-up, then the median of `runs`.  The union's time is the whole call -
its allocations, the copy of the duplicate count to the host and the histogram's included - since that is what a caller
waits for; the sort's is tbk_launch_sort_u64_u8 over the 2n concatenated pairs, its temporary storage included.  `bytes` is
what the result needs at the least: each input read once, the output written once, 9 bytes an entry.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from trio_binning_amd import _lib, kmers  # noqa: E402
from trio_binning_amd._lib import check, lib  # noqa: E402

hip = C.CDLL("libamdhip64.so")
_vp = C.c_void_p
for name, argtypes in (("hipEventCreate", [C.POINTER(_vp)]), ("hipEventRecord", [_vp, _vp]), ("hipEventSynchronize", [_vp]),
                       ("hipEventElapsedTime", [C.POINTER(C.c_float), _vp, _vp]), ("hipEventDestroy", [_vp]),
                       ("hipMemset", [_vp, C.c_int, C.c_size_t]), ("hipMemcpy", [_vp, _vp, C.c_size_t, C.c_int]), ("hipMalloc", [C.POINTER(_vp), C.c_size_t]),
                       ("hipFree", [_vp])):
    getattr(hip, name).argtypes, getattr(hip, name).restype = argtypes, C.c_int
lib.tbk_launch_db_rank.argtypes, lib.tbk_launch_db_rank.restype = [_vp, _vp, C.c_uint64, C.c_int, _vp, _vp, _vp], C.c_int
lib.tbk_launch_sort_u64_u8.argtypes, lib.tbk_launch_sort_u64_u8.restype = [_vp, _vp, _vp, _vp, C.c_uint64, C.c_int, _vp], C.c_int
lib.tbk_kmerdb_adopt_device_.argtypes, lib.tbk_kmerdb_adopt_device_.restype = [_vp, _vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)], C.c_int
D2D = 3  # hipMemcpyDeviceToDevice


def ok(status, what):
    if status != 0:
        raise RuntimeError("{}: HIP error {}".format(what, status))


def dalloc(nbytes):
    p = _vp()
    ok(hip.hipMalloc(C.byref(p), max(nbytes, 16)), "hipMalloc")
    return p.value


def sorted_pairs(dev, first, n, k, counter):
    """(d_keys, d_counts): n ascending ranks of the synthetic keys first .. first + n - 1, every counter `counter`"""
    d_raw, d_rank, d_keys = dalloc(8 * n), dalloc(8 * n), dalloc(8 * n)
    d_c0, d_c1, d_counts = dalloc(n), dalloc(n), dalloc(n)
    check(lib.tbk_synth_keys_device(dev, 0x5EED0001, first, n, k, _vp(d_raw)))
    ok(hip.hipMemset(d_c0, counter, n), "hipMemset")
    ok(lib.tbk_launch_db_rank(d_raw, d_c0, n, k, d_rank, d_c1, None), "tbk_launch_db_rank")
    ok(lib.tbk_launch_sort_u64_u8(d_rank, d_keys, d_c1, d_counts, n, 2 * k, None), "tbk_launch_sort_u64_u8")
    check(lib.tbk_device_sync(dev))
    for p in (d_raw, d_rank, d_c0, d_c1):
        ok(hip.hipFree(p), "hipFree")
    return d_keys, d_counts


def timed(runs, call, after=lambda: None):
    """milliseconds between two events around `call`: one warm-up, then `runs`"""
    e0, e1 = _vp(), _vp()
    ok(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    times = []
    for run in range(runs + 1):
        ok(hip.hipEventRecord(e0, None), "hipEventRecord")
        call()
        ok(hip.hipEventRecord(e1, None), "hipEventRecord")
        ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
        after()
        if run:
            times.append(ms.value)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    return times


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, n, k = 0, args.n, args.k
    ceiling = json.load(open(os.path.join(ROOT, "profiles", "calibration.json")))["stream_tuned_GBps"]
    # A: keys 0 .. n - 1 of the sequence; B: n / 2 .. 3n / 2 - 1, so half of B's keys are A's
    a_keys, a_counts = sorted_pairs(dev, 0, n, k, 1)
    b_keys, b_counts = sorted_pairs(dev, n // 2, n, k, 200)
    # the baseline's input before the databases take the arrays over: both pair lists one behind the other
    cat_keys, cat_counts, out_keys, out_counts = dalloc(16 * n), dalloc(2 * n), dalloc(16 * n), dalloc(2 * n)
    for dst, src, size in ((cat_keys, a_keys, 8 * n), (cat_keys + 8 * n, b_keys, 8 * n), (cat_counts, a_counts, n), (cat_counts + n, b_counts, n)):
        ok(hip.hipMemcpy(dst, src, size, D2D), "hipMemcpy")
    ha, hb = _vp(), _vp()
    check(lib.tbk_kmerdb_adopt_device_(a_keys, a_counts, n, k, dev, 1, C.byref(ha)))
    check(lib.tbk_kmerdb_adopt_device_(b_keys, b_counts, n, k, dev, 1, C.byref(hb)))
    da, db = kmers.KmerDatabase(ha), kmers.KmerDatabase(hb)
    made = []

    def union():
        made.append(da.union(db))

    def drop():
        made.pop().close()

    with da.union(db) as first:
        n_out = len(first)
        hist = first.histogram()
        assert n_out == n + n - (n - n // 2) and int(hist[201]) == n - n // 2 and int(hist[1]) + int(hist[200]) == n_out - int(hist[201])
    union_ms = timed(args.runs, union, drop)
    sort_ms = timed(args.runs, lambda: ok(lib.tbk_launch_sort_u64_u8(cat_keys, out_keys, cat_counts, out_counts, 2 * n, 2 * k, None), "sort"))
    da.close()
    db.close()
    for p in (cat_keys, cat_counts, out_keys, out_counts):
        hip.hipFree(p)
    moved = 9 * (2 * n + n_out)
    um, sm = statistics.median(union_ms), statistics.median(sort_ms)
    result = {"device": _lib.device_name(dev), "k": k, "n_a": n, "n_b": n, "n_union": n_out, "runs": args.runs,
              "union_ms": round(um, 3), "union_ms_all": [round(x, 3) for x in union_ms],
              "sort_concatenation_ms": round(sm, 3), "sort_ms_all": [round(x, 3) for x in sort_ms],
              "bytes_at_least": moved, "union_GBps": round(moved / um / 1e6, 1), "stream_ceiling_GBps": ceiling,
              "union_fraction_of_ceiling": round(moved / um / 1e6 / ceiling, 3), "sort_over_union": round(sm / um, 2)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
