"""Time tbk_kmerdb_import_text and tbk_kmerdb_dump_text on a synthetic counted dump beside the parent's yardsticks.

    python tools/measure_dump.py [--n 100000000] [--k 21] [--runs 5] [--dir DIR] [--out PATH]

`n` synthetic k-mers (tbk_synth_keys_device: distinct and canonical by construction) with counters drawn from 1..255 are
ranked, sorted and adopted as a full database, which is dumped: canonical k-mers in ascending order, what kmc_dump and meryl
print write ("sorted").  Importing it must not sort, which is asserted through tbk_dump_import_stats.  The same pairs written
with numpy in pieces of 4 M lines, the lines of a piece permuted, the pieces in random order and every other k-mer as its
reverse complement (counters zero-padded to three digits, so that the rows have one width) are the "shuffled" dump, which takes
the sort path.  Every figure is the median of `runs` after one warm-up, wall clock around the whole call (mapping the file,
staging, launches, the header) - what a caller waits for; the files lie in the page cache.  parse_ms is the HIP-event time of
the newline and parse kernels alone, from the same counter.  The export is split by the library's own clock into selection,
copy home, and format + write.  Yardsticks, in the same process: tbk_table_create_from_file on a list of as many lines (the
fixed-length text parse), tbk_launch_sort_u64_u8 on as many pairs, tbk_calib_stream.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from trio_binning_amd import _lib, kmers  # noqa: E402
from trio_binning_amd._lib import check, lib  # noqa: E402

hip = C.CDLL("libamdhip64.so")
_vp = C.c_void_p
for name, argtypes in (("hipMemcpy", [_vp, _vp, C.c_size_t, C.c_int]), ("hipMalloc", [C.POINTER(_vp), C.c_size_t]), ("hipFree", [_vp])):
    getattr(hip, name).argtypes, getattr(hip, name).restype = argtypes, C.c_int
lib.tbk_launch_db_rank.argtypes, lib.tbk_launch_db_rank.restype = [_vp, _vp, C.c_uint64, C.c_int, _vp, _vp, _vp], C.c_int
lib.tbk_launch_sort_u64_u8.argtypes, lib.tbk_launch_sort_u64_u8.restype = [_vp, _vp, _vp, _vp, C.c_uint64, C.c_int, _vp], C.c_int
lib.tbk_kmerdb_adopt_device_.argtypes, lib.tbk_kmerdb_adopt_device_.restype = [_vp, _vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)], C.c_int
H2D = 1  # hipMemcpyHostToDevice


def ok(status, what):
    if status != 0:
        raise RuntimeError("{}: HIP error {}".format(what, status))


def dalloc(nbytes):
    p = _vp()
    ok(hip.hipMalloc(C.byref(p), max(nbytes, 16)), "hipMalloc")
    return p.value


def wall(runs, call, after=lambda r: None):
    """seconds of `call`: one warm-up, then `runs`"""
    times = []
    for run in range(runs + 1):
        t0 = time.perf_counter()
        r = call()
        t1 = time.perf_counter()
        after(r)
        if run:
            times.append(t1 - t0)
    return times


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the dumps are written (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, n, k = 0, args.n, args.k
    work = tempfile.TemporaryDirectory(dir=args.dir)
    mixed, ordered, listed = (os.path.join(work.name, name) for name in ("shuffled.txt", "sorted.txt", "list.txt"))

    # n pairs as tbk_counter_export orders them, counters 1..255, kept for the sort yardstick and adopted as a database
    d_raw, d_rank, d_keys = dalloc(8 * n), dalloc(8 * n), dalloc(8 * n)
    d_c0, d_c1, d_counts = dalloc(n), dalloc(n), dalloc(n)
    check(lib.tbk_synth_keys_device(dev, 0x5EED0016, 0, n, k, _vp(d_raw)))
    counters = np.random.default_rng(16).integers(1, 256, n).astype(np.uint8)
    ok(hip.hipMemcpy(d_c0, counters.ctypes.data, n, H2D), "hipMemcpy")
    ok(lib.tbk_launch_db_rank(d_raw, d_c0, n, k, d_rank, d_c1, None), "tbk_launch_db_rank")
    ok(lib.tbk_launch_sort_u64_u8(d_rank, d_keys, d_c1, d_counts, n, 2 * k, None), "tbk_launch_sort_u64_u8")
    check(lib.tbk_device_sync(dev))
    sort_s = wall(args.runs, lambda: ok(lib.tbk_launch_sort_u64_u8(d_rank, d_raw, d_c1, d_c0, n, 2 * k, None), "sort"))  # (it waits for its stream itself)
    for p in (d_raw, d_c0):
        hip.hipFree(p)
    h = _vp()
    check(lib.tbk_kmerdb_adopt_device_(d_keys, d_counts, n, k, dev, 1, C.byref(h)))
    export_ms = []
    with kmers.KmerDatabase(h) as db0:
        def export():
            assert db0.dump(ordered) == n
            ms = (C.c_double * 3)()
            check(lib.tbk_dump_export_timing_(ms))
            export_ms.append(list(ms))

        export_s = wall(args.runs, export)
        export_ms = export_ms[1:]
        keys, counts = db0.entries()
    for p in (d_rank, d_c1):
        hip.hipFree(p)
    n_canon = n

    # the list of as many lines for the fixed-length parse (the same k-mers without their counters) and the shuffled dump
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    rng = np.random.default_rng(17)
    piece = 1 << 22
    with open(listed, "wb") as fl:
        for lo in range(0, n, piece):
            part = keys[lo:lo + piece]
            rows = np.full((part.size, k + 1), 10, dtype=np.uint8)
            for j in range(k):
                rows[:, j] = lut[((part >> np.uint64(2 * (k - 1 - j))) & np.uint64(3)).astype(np.intp)]
            fl.write(rows.tobytes())
    with open(mixed, "wb") as fm:
        for lo in rng.permutation(np.arange(0, n, piece)):
            part, cnt = keys[lo:lo + piece], counts[lo:lo + piece].astype(np.uint32)
            rows = np.full((part.size, k + 5), 10, dtype=np.uint8)
            flip = np.arange(part.size) % 2 == 1
            for j in range(k):
                fwd = ((part >> np.uint64(2 * (k - 1 - j))) & np.uint64(3)).astype(np.intp)
                rev = 3 - ((part >> np.uint64(2 * j)) & np.uint64(3)).astype(np.intp)
                rows[:, j] = lut[np.where(flip, rev, fwd)]
            rows[:, k] = 9
            for j, div in enumerate((100, 10, 1)):
                rows[:, k + 1 + j] = 48 + cnt // div % 10
            fm.write(rows[rng.permutation(part.size)].tobytes())
    del keys, counts

    def stats():
        return kmers.dump_import_stats()

    s0 = stats()
    mixed_s = wall(args.runs, lambda: kmers.KmerDatabase.from_dump(mixed, k=k, floor=1), lambda db: db.close())
    s1 = stats()
    assert s1["sorts"] - s0["sorts"] == args.runs + 1, "the shuffled dump must take the sort path"
    with kmers.KmerDatabase.from_dump(mixed, k=k, floor=1) as again:
        assert len(again) == n, "the shuffled dump holds the same k-mers"
    s2 = stats()
    sorted_s = wall(args.runs, lambda: kmers.KmerDatabase.from_dump(ordered, k=k, floor=1), lambda db: db.close())
    s3 = stats()
    assert s3["sorts"] == s2["sorts"], "the sorted dump must not be sorted again"
    assert s3["lines"] - s2["lines"] == (args.runs + 1) * n_canon
    list_s = wall(args.runs, lambda: kmers.HashSet.from_file(listed, dev), lambda hs: hs.close())
    bps = C.c_double()
    check(lib.tbk_calib_stream(dev, 4 << 30, 5, C.byref(bps)))

    def med(xs):
        return statistics.median(xs)

    mixed_bytes, sorted_bytes, list_bytes = (os.path.getsize(p) for p in (mixed, ordered, listed))
    result = {
        "device": _lib.device_name(dev), "k": k, "n": n, "n_canonical": n_canon, "runs": args.runs,
        "import_sorted_s": round(med(sorted_s), 4), "import_sorted_GBps": round(sorted_bytes / med(sorted_s) / 1e9, 3),
        "import_sorted_Mlines_per_s": round(n_canon / med(sorted_s) / 1e6, 1), "import_sorted_sorts": s3["sorts"] - s2["sorts"],
        "import_sorted_parse_kernels_ms": round((s3["parse_ms"] - s2["parse_ms"]) / (args.runs + 1), 3),
        "import_sorted_parse_kernels_GBps": round(sorted_bytes / ((s3["parse_ms"] - s2["parse_ms"]) / (args.runs + 1)) / 1e6, 1),
        "import_shuffled_s": round(med(mixed_s), 4), "import_shuffled_GBps": round(mixed_bytes / med(mixed_s) / 1e9, 3),
        "import_shuffled_Mlines_per_s": round(n / med(mixed_s) / 1e6, 1),
        "import_shuffled_parse_kernels_ms": round((s1["parse_ms"] - s0["parse_ms"]) / (args.runs + 1), 3),
        "export_s": round(med(export_s), 4), "export_GBps_text": round(sorted_bytes / med(export_s) / 1e9, 3),
        "export_select_ms": round(med([m[0] for m in export_ms]), 3), "export_copy_home_ms": round(med([m[1] for m in export_ms]), 3),
        "export_format_write_ms": round(med([m[2] for m in export_ms]), 3),
        "yardstick_list_parse_s": round(med(list_s), 4), "yardstick_list_parse_GBps": round(list_bytes / med(list_s) / 1e9, 3),
        "yardstick_list_parse_Mlines_per_s": round(n_canon / med(list_s) / 1e6, 1),
        "yardstick_sort_pairs_ms": round(med(sort_s) * 1e3, 3), "yardstick_stream_GBps": round(bps.value / 1e9, 1),
        "host_threads": kmers.host_threads(), "text_bytes_sorted": sorted_bytes, "text_bytes_shuffled": mixed_bytes,
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    work.cleanup()


if __name__ == "__main__":
    main()
