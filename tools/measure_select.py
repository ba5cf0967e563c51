"""Time tbk_kmerdb_select - the hap-mer selection - beside tbk_kmerdb_inherited_table, the three-database selection that ends
in a key list, on the crafted databases of tools/measure_db_handoff.py --inherited.

    python tools/measure_select.py [--n 100000000] [-k 21] [--runs 7] [--tmp /dev/shm] [--out-dir profiles/r20]
    python tools/measure_select.py --only-inherited --name measure_select_parent.json   # under TBK_LIBRARY: another build's list call
    python tools/measure_select.py --name measure_select_sparse.json   # under TBK_LIBRARY: the variant -DTBK_SELECT_SPARSE_SCATTER
    python tools/measure_select.py --render-only [--regs FILE] [--kernel-stats FILE] [--bench-parent FILE... --bench-change FILE...]

Three databases of --n k-mers each: A (ascending random ranks, counters uniform in 2..40), B (every fourth key of A and as many
keys A lacks) and a child that holds every second k-mer of A with a counter in [5, 35] that B lacks and, in place of every other
entry of A, the rank above it.  Every leg runs in this process and the legs take turns: HIP events on the null stream around the
whole call - its allocations, the scan's copy home and the tally included, since that is what a caller waits for - one warm-up
round, then the median of --runs rounds; tbk_calib_stream in the same process.  The legs:

  inherited_table    A.unique_set(B, 5, 35, child=child, child_min=2): flag with two partners, scan, scatter of 8-byte keys;
  select_base        A.select(5, 35, exclude=[B], require=[(child, 2, 255)], counter="base"): the same bisections, 9 bytes a
                     kept k-mer and the tally of the result's counters;
  select_min, _sum   the same selection with the counter made of A's and the child's: one more bisection per kept k-mer;
  select_from_child  child.select(2, 255, require=[(A, 5, 35)], exclude=[B]): the shape the hapmers command uses.

Every result is checked against the construction (keys and counters, entry for entry) before it is timed.  `bytes_at_least` is
each input's keys read once, the counters of base and of the REQUIRE partner, and the output.  Writes measure_select.json (or
--name) and README.md into --out-dir."""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from trio_binning_amd import _lib, kmers  # noqa: E402
from trio_binning_amd._lib import check, lib  # noqa: E402

hip = C.CDLL("libamdhip64.so")
_vp = C.c_void_p
for name, argtypes in (("hipEventCreate", [C.POINTER(_vp)]), ("hipEventRecord", [_vp, _vp]), ("hipEventSynchronize", [_vp]),
                       ("hipEventElapsedTime", [C.POINTER(C.c_float), _vp, _vp]), ("hipEventDestroy", [_vp])):
    getattr(hip, name).argtypes, getattr(hip, name).restype = argtypes, C.c_int
LO, HI = 5, 35


def ok(status, what):
    if status != 0:
        raise RuntimeError("{}: HIP error {}".format(what, status))


def write_db(path, k, keys, counts):
    """The *.tbkdb layout of INTEGRATION.md: header, keys, counters (a floor-2 file)."""
    hist = np.bincount(counts, minlength=256).astype("<u8")
    hist[0] = keys.size
    body = b"TBKKMDB1" + struct.pack("<IIQQQ", 2096, k, keys.size, 0, 0) + hist.tobytes()
    with open(path, "wb") as fh:
        fh.write(body + struct.pack("<II", zlib.crc32(body) & 0xFFFFFFFF, 0))
        keys.astype("<u8").tofile(fh)
        counts.tofile(fh)


def timed(runs, calls):
    """{name: milliseconds between two events around calls[name]()}, the result closed outside them.  The legs take turns:
    one warm-up round, then `runs` rounds of every leg in order, so that what else the box does meets all of them alike."""
    e0, e1 = _vp(), _vp()
    ok(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    times = {name: [] for name in calls}
    for run in range(runs + 1):
        for name, call in calls.items():
            ok(hip.hipEventRecord(e0, None), "hipEventRecord")
            made = call()
            ok(hip.hipEventRecord(e1, None), "hipEventRecord")
            ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            ms = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
            made.close()
            if run:
                times[name].append(ms.value)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    return times


def leg(times, nbytes, stream_gbps):
    med = statistics.median(times)
    return {"ms": round(med, 4), "ms_all": [round(t, 4) for t in times], "bytes_at_least": nbytes, "GBps": round(nbytes / med / 1e6, 1),
            "fraction_of_stream": round(nbytes / med / 1e6 / stream_gbps, 3)}


def bench_line(path):
    line = json.loads(open(path).read().strip().splitlines()[-1])
    return {key: line[key] for key in ("value", "unit", "ms_per_step", "table_build_s") if key in line}


def kernel_rows(path):
    """| kernel | calls | average, min and max ms | of the tbk_kmerdb kernels in a rocprofv3 kernel_stats CSV"""
    import csv

    rows = []
    for row in csv.DictReader(open(path)):
        name = row["Name"].split("(")[0].replace("void ", "")
        if name.startswith("tbk_kmerdb_"):
            rows.append("| `{}` | {} | {:.3f} | {:.3f} | {:.3f} |".format(name, row["Calls"], float(row["AverageNs"]) / 1e6, float(row["MinNs"]) / 1e6,
                                                                 float(row["MaxNs"]) / 1e6))
    return sorted(rows)


def readme(result, parent, sparse, regs, benches, kernel_stats):
    legs = result["legs"]
    base = legs["inherited_table"]["ms"]
    rows = ["| `{}` | {} | {} | {} | {:.3f} |".format(name, rec["ms"], rec["GBps"], rec["fraction_of_stream"], rec["ms"] / base) for name, rec in legs.items()]
    if parent:
        rec = parent["legs"]["inherited_table"]
        rows.insert(1, "| `inherited_table`, the parent commit's library | {} | {} | {} | {:.3f} |".format(rec["ms"], rec["GBps"], rec["fraction_of_stream"], rec["ms"] / base))
    if sparse:  # (the time over that run's own inherited_table)
        for name in ("select_min", "select_sum"):
            rec = sparse["legs"][name]
            rows.append("| `{}`, scatter with a lane per entry of the tile (variant build, a run of its own) | {} | {} | {} | {:.3f} |".format(
                name, rec["ms"], rec["GBps"], rec["fraction_of_stream"], rec["ms"] / sparse["legs"]["inherited_table"]["ms"]))
    text = """# r20 - a selection from count databases that stays a database (hap-mer databases)

What this directory is for: the register figures of the kernels of `csrc/tbk_select.hip` and the times of `tbk_kmerdb_select`
beside `tbk_kmerdb_inherited_table`, the call that does the same bisections and ends in a key list (DESIGN §9, "A selection that
stays a database").  Written by `tools/measure_select.py`; `measure_select.json` has every run.

## Measurement

{device}; k = {k}; three crafted databases of {n} entries each (`tools/measure_db_handoff.py --inherited`'s): A, B (every fourth key
of A and as many keys A lacks) and a child holding every second k-mer of A in [{lo}, {hi}] that B lacks; {kept} k-mers are kept.
HIP events around each whole call (allocations, the scan's copy home, the tally included); the legs take turns, one warm-up
round, median of {runs}.
`tbk_calib_stream` in the same process: **{stream} GB/s**.  GB/s is over the bytes a result needs at the least - the keys of every
input read once, the counters of the base and of the partner asked for them, the output - and "of stream" is that rate over the
stream figure; the last column is the time over this build's `inherited_table`.

| leg | ms | GB/s | of stream | over inherited_table |
|---|---:|---:|---:|---:|
{rows}

Every result was checked entry for entry against the construction before timing.
""".format(device=result["device"], k=result["k"], n=result["n"], lo=LO, hi=HI, kept=result["kept"], runs=result["runs"], stream=result["stream_GBps"],
           rows="\n".join(rows))
    if regs:
        text += ("\n## Registers (`tools/kernel_regs.sh trio_binning_amd/csrc/build/tbk_select.o tbk_kmerdb`; SGPRs and scratch from the same notes)\n\n"
                 + regs.strip() + "\n\nNo scratch, no spills.\n")
    if kernel_stats:
        text += ("\n## Kernel times (`rocprofv3 --kernel-trace --stats -- python3 tools/measure_select.py --runs 5`, a run of its own)\n\n"
                 "| kernel | calls | average ms | min | max |\n|---|---:|---:|---:|---:|\n" + "\n".join(kernel_rows(kernel_stats)) + "\n")
    if benches:
        text += "\n## `bench.py --gpus 1 --steps 5 --warmup 2`, parent and change taking turns, in the order they ran (two pairs a job)\n\n| build | " + " | ".join(benches[0][1]) + " |\n"
        text += "|---|" + "---:|" * len(benches[0][1]) + "\n"
        for build, line in benches:
            text += "| {} | ".format(build) + " | ".join(str(v) for v in line.values()) + " |\n"
        text += "\nThe parent's line is the parent commit's library under this tree's Python (`TBK_LIBRARY`); the classify stage runs no code this change touches.\n"
    return text


def render(args, result):
    parent_path = os.path.join(args.out_dir, "measure_select_parent.json")
    parent = json.loads(open(parent_path).read()) if os.path.exists(parent_path) else None
    sparse_path = os.path.join(args.out_dir, "measure_select_sparse.json")
    sparse = json.loads(open(sparse_path).read()) if os.path.exists(sparse_path) else None
    regs = open(args.regs).read() if args.regs else None
    benches = [(build, bench_line(path)) for pair in zip(args.bench_parent, args.bench_change) for build, path in zip(("parent", "change"), pair)]
    with open(os.path.join(args.out_dir, "README.md"), "w") as fh:
        fh.write(readme(result, parent, sparse, regs, benches, args.kernel_stats))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--tmp", default="/dev/shm")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r20"))
    ap.add_argument("--name", default="measure_select.json")
    ap.add_argument("--only-inherited", action="store_true", help="time the list call alone: for another build of the library under TBK_LIBRARY")
    ap.add_argument("--regs", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--bench-parent", nargs="*", default=[])
    ap.add_argument("--bench-change", nargs="*", default=[])
    ap.add_argument("--render-only", action="store_true")
    args = ap.parse_args()
    if args.render_only:
        render(args, json.loads(open(os.path.join(args.out_dir, "measure_select.json")).read()))
        return
    k, n, dev = args.k, args.n, 0
    rng = np.random.default_rng(10)
    max_gap = max(3, min(40_000, (1 << (2 * k)) // n - 1))
    t = time.time()
    keys_a = np.cumsum(rng.integers(2, max_gap + 1, n, dtype=np.uint64), dtype=np.uint64)
    assert int(keys_a[-1]) < 1 << (2 * k), "4^k is too small for --n"
    fourth = np.arange(n, dtype=np.uint64) % np.uint64(4) != 0
    keys_b = keys_a + fourth.astype(np.uint64)  # every fourth key shared; gaps >= 2 keep it ascending
    counts_a, counts_b, counts_c = (rng.integers(2, 41, n).astype(np.uint8) for _ in range(3))
    selected = (counts_a >= LO) & (counts_a <= HI) & fourth
    held = selected & (np.cumsum(selected) % 2 == 1)  # the 1st, 3rd, ... selected entry of A
    keys_c = keys_a + (~held).astype(np.uint64)
    paths = [os.path.join(args.tmp, "tbk_select_%d_%s.tbkdb" % (os.getpid(), h)) for h in "abc"]
    dbs = []
    try:
        for path, keys, counts in zip(paths, (keys_a, keys_b, keys_c), (counts_a, counts_b, counts_c)):
            write_db(path, k, keys, counts)
            dbs.append(kmers.KmerDatabase.load(path))
            os.remove(path)
    finally:
        for path in paths:
            if os.path.exists(path):
                os.remove(path)
    da, db, dc = dbs
    want_keys, want_a, want_c = keys_a[held], counts_a[held].astype(np.int64), counts_c[held].astype(np.int64)
    held_in_child = np.flatnonzero(held)  # the child's entry i stands where A's entry i does
    kept = int(want_keys.size)
    del keys_a, keys_b, keys_c, selected, held, fourth
    craft_s = round(time.time() - t, 2)
    rate = C.c_double()
    check(lib.tbk_calib_stream(dev, 1 << 30, 10, C.byref(rate)))
    stream = round(rate.value / 1e9, 1)
    result = {"device": _lib.device_name(dev), "library": os.path.basename(os.environ.get("TBK_LIBRARY", "")), "k": k, "n": n, "runs": args.runs,
              "cutoffs": [LO, HI], "kept": kept, "craft_and_load_s": craft_s, "stream_GBps": stream, "legs": {}}

    def listed():
        return da.unique_set(db, LO, HI, child=dc, child_min=2, child_max=255)

    with listed() as hs:
        assert hs.num_kmers == kept
    calls, nbytes = {"inherited_table": listed}, {"inherited_table": 8 * 3 * n + n + n + 8 * kept}
    if not args.only_inherited:
        for name, rule, want in (("select_base", "base", want_a), ("select_min", "min", np.minimum(want_a, want_c)),
                                 ("select_sum", "sum", np.minimum(want_a + want_c, 255))):
            call = lambda rule=rule: da.select(LO, HI, exclude=[db], require=[(dc, 2, 255)], counter=rule)
            with call() as got:
                keys, counts = got.entries()
                assert np.array_equal(keys, want_keys) and np.array_equal(counts, want.astype(np.uint8)), name
                assert np.array_equal(got.histogram()[1:], np.bincount(want, minlength=256)[1:].astype(np.uint64)), name
            calls[name], nbytes[name] = call, 8 * 3 * n + n + n + 9 * kept
        call = lambda: dc.select(2, 255, require=[(da, LO, HI)], exclude=[db])
        with call() as got:
            keys, counts = got.entries()
            assert np.array_equal(keys, want_keys) and np.array_equal(counts, counts_c[held_in_child]), "select_from_child"
        calls["select_from_child"], nbytes["select_from_child"] = call, 8 * 3 * n + n + n + 9 * kept
    for name, times in timed(args.runs, calls).items():
        result["legs"][name] = leg(times, nbytes[name], stream)
    base = result["legs"]["inherited_table"]["ms"]
    result["over_inherited_table"] = {name: round(rec["ms"] / base, 3) for name, rec in result["legs"].items()}
    for d in dbs:
        d.close()
    os.makedirs(args.out_dir, exist_ok=True)
    line = json.dumps(result)
    print(line)
    with open(os.path.join(args.out_dir, args.name), "w") as fh:
        fh.write(line + "\n")
    if args.name == "measure_select.json":
        render(args, result)


if __name__ == "__main__":
    main()
