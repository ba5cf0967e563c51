#!/usr/bin/env python3
"""The k-mer counter in passes (KmerCounter(passes=P)) on synthetic short reads generated in HBM, as
measure_count.py makes them: wall seconds of adding and of finishing, the counting kernel's summed ms, the kept
reads' bytes per base, the largest table and the databases.  --passes 0 asks find_unique_kmers.choose_passes.
--tree runs another checkout's package (its own libtbk_hip.so) with this script: the yardstick leg of an A/B
(--passes 1 or 0 where that checkout has no passes).  --sample N also counts the first N reads of the first batch
on the CPU (oracle count_kmers_np) and holds the whole counter's dumps to those counts."""
import argparse, ctypes as C, json, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--genome", type=int, default=200_000_000)
ap.add_argument("--coverage", type=float, default=20.0)
ap.add_argument("--read-len", type=int, default=150)
ap.add_argument("--error-rate", type=float, default=0.002)
ap.add_argument("--batch-bases", type=int, default=1_000_000_000)
ap.add_argument("-k", type=int, default=21)
ap.add_argument("--passes", type=int, default=1)
ap.add_argument("--capacity", type=int, default=0, help="distinct k-mers expected (default: genome + error k-mers)")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--sample", type=int, default=0)
ap.add_argument("--tmp", default="/tmp")
a = ap.parse_args()
sys.path.insert(0, a.tree)
import numpy as np
from trio_binning_amd import kmers
from trio_binning_amd._lib import check, lib

dev, k, L = 0, a.k, a.read_len
R = a.batch_bases // L
n_batches = max(1, int(a.genome * a.coverage / (R * L)))
bases_total = n_batches * R * L
def dalloc(n):
    p = C.c_void_p(); check(lib.tbk_device_alloc(dev, n, C.byref(p))); return p.value
d_bases, d_offs = dalloc(R * L + 64), dalloc((R + 1) * 8)
err24 = int(a.error_rate * (1 << 24))
capacity = a.capacity or int(a.genome * 1.05 + bases_total * a.error_rate * k * 1.1) + (1 << 20)
passes = a.passes
if not passes:
    # as the command line plans: the passes choose_passes asks for when all that is known is the number of bases; one pass
    # gets what estimate_capacity grants a table of the free HBM (a checkout without choose_passes always counts in one)
    from trio_binning_amd import find_unique_kmers as fu
    free = kmers.device_mem_info()[0]
    passes = fu.choose_passes(max(1 << 16, bases_total), bases_total, free) if hasattr(fu, "choose_passes") else 1
    if not a.capacity:
        capacity = bases_total if passes > 1 else max(1 << 16, min(bases_total, int(0.35 * free / 16 * 0.6)))
out = {"k": k, "genome": a.genome, "gbases": bases_total / 1e9, "batches": n_batches, "capacity": capacity, "passes": passes}
try:
    ctr = kmers.KmerCounter(k, capacity, passes=passes) if passes != 1 else kmers.KmerCounter(k, capacity)
    add_s = 0.0
    sample = None
    for b in range(n_batches):
        check(lib.tbk_synth_hap_reads_device(dev, 0x5EED0001, a.genome, 0, 0x5EED0003, b * R, R, L, err24, C.c_void_p(d_bases), C.c_void_p(d_offs)))
        check(lib.tbk_device_sync(dev))
        if b == 0 and a.sample:
            n = min(R, a.sample)
            sample = np.empty(n * L, dtype=np.uint8)
            check(lib.tbk_memcpy_d2h(dev, sample.ctypes.data, C.c_void_p(d_bases), sample.size))
        t = time.time()
        ctr.add_device(d_bases, d_offs, R, R * L)
        check(lib.tbk_device_sync(dev))
        add_s += time.time() - t
    before = ctr.stats()
    t = time.time(); hist = ctr.histogram(); finish_s = time.time() - t
    launches, windows, ms = ctr.kernel_timing(reset=False)
    st = ctr.stats()
    out.update({"add_s": round(add_s, 3), "finish_and_histogram_s": round(finish_s, 3), "wall_s": round(add_s + finish_s, 3),
                "kernel_ms": round(ms, 1), "kernel_launches": launches, "window_starts": windows,
                "store_bytes_per_base": round(before.get("store_used_bytes", 0) / bases_total, 4), "store_bytes": before.get("store_bytes", 0),
                "peak_table_bytes": st.get("peak_table_bytes"), "table_bytes_at_end": st["table_bytes"], "database_bytes": st.get("database_bytes"),
                "distinct": int(hist[0]), "singletons": int(hist[1]), "seen_twice_or_more": int(hist[2:].sum()),
                "hist_2_to_6": [int(x) for x in hist[2:7]]})
    # every window of every read is counted once, in exactly one class: while no counter reaches 255 the rows add up to the windows
    if not int(hist[255]):
        out["windows_counted"] = int((hist[1:] * np.arange(1, 256, dtype=np.uint64)).sum())
        out["windows_in_the_reads"] = n_batches * R * (L - k + 1)
    if sample is not None:
        # The sample's own counts against the whole run's, read from dumps of the k-mers the run counted exactly 2, 3, 4
        # and 5 or more times.  A k-mer the sample saw c times the run saw at least c times; where no other read holds it -
        # the k-mers the sample pins down - exactly c times: "same".  "lower" or "missing" would be wrong counts.
        from oracle import unique_oracle as uo
        n = sample.size // L
        keys, counts = uo.count_kmers_np(sample, np.arange(n + 1, dtype=np.uint64) * np.uint64(L), k)
        with (kmers.KmerCounter(k, 1 << 16, passes=passes) if passes != 1 else kmers.KmerCounter(k, 1 << 16)) as nothing:
            dumps = {}
            for c, hi in ((2, 2), (3, 3), (4, 4), (5, 255)):
                path = os.path.join(a.tmp, "tbk_passes_dump_%d_%d.txt" % (os.getpid(), c))
                ctr.unique(nothing, c, hi, path)
                dumps[c] = uo.read_list_np(path, k)
                os.remove(path)
        tally = {"same": 0, "higher": 0, "lower": 0, "missing": 0}
        for c in (2, 3, 4):
            mine = keys[counts == c]
            at = {d: int(np.isin(mine, dumps[d], assume_unique=True).sum()) for d in dumps}
            tally["same"] += at[c]
            tally["higher"] += sum(v for d, v in at.items() if d > c)
            tally["lower"] += sum(v for d, v in at.items() if d < c)
            tally["missing"] += mine.size - sum(at.values())
        out["sample"] = dict(tally, reads=n, dump_sizes={str(c): int(v.size) for c, v in dumps.items()})
    ctr.close()
except MemoryError as exc:
    out["error"] = "MemoryError: " + str(exc)
print(json.dumps(out))
