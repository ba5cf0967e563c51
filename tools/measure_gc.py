"""Time tbk_kmerdb_gc_spectrum with both of its LDS layouts beside tbk_kmerdb_origin_spectrum, the tally over the same bytes
that exists already, and beside the streaming-read figure of the device.

    python tools/measure_gc.py [--n 20000000] [--k 21 32] [--runs 9] [--out-dir profiles/r25] [--regs FILE]
    python tools/measure_gc.py --n 100000000 --k 21 [--out-dir profiles/r25]           # a database the Infinity Cache does not hold
    python tools/measure_gc.py --render-only [--out-dir profiles/r25] [--regs FILE]    # README.md again from measure_gc*.json, no device

One full database of `n` entries per k, made as tools/measure_compare.py makes its own (tbk_synth_keys_device's keys, ranked and
sorted on the device, adopted where they lie) with that tool's counters: 94 % Poisson around 30, 4 % counter 1 or 2, 2 % spread
evenly over 64..255.  The keys are uniform over the 4^k ranks, so their GC is binomial around k / 2.  Every leg runs in this
process, one after the other, HIP events on the null stream around it, one warm-up, then the median of `runs`:

  gc, whole matrix   tbk_launch_kmerdb_gc_spectrum with layout 1: the (k + 1) x 256 cells of a block in dynamic LDS
  gc, corner         the same launch with layout 2: the counters below 64 in LDS, the others straight to global atomics
  - in 2048, 1024, 512, 256 blocks   each of the two again under a grid of that many blocks (tbk_kmerdb_gc_set_grid_; the first
                     line of each layout is the build's own grid)
  origin             tbk_launch_kmerdb_origin_spectrum with the database as base and as both partners: the launch the parent
                     commit has over the same 9 n bytes (every entry finds itself twice, within its own tile's bounds)
  gc call, origin call   tbk_kmerdb_gc_spectrum and tbk_kmerdb_origin_spectrum whole: allocation, memset, launch (the build's
                     layout) and the copy of the matrix home - what a caller waits for
  stream             tbk_calib_stream over 9 n bytes, and over 1 GiB as the other tools report it

The launches write into one device matrix, zeroed outside the timed span; each layout's matrix is brought home once and held
against the call's before anything is timed.  `bytes` is what a result needs at the least: 9 bytes an entry, read once.  Writes
measure_gc.json (measure_gc_n<N>.json for another --n) into --out-dir and README.md from every such file there; --regs (the text of tools/kernel_regs.sh on build/tbk_compare.o) is copied into
the README when given."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import measure_compare as mc  # noqa: E402  (the synthetic database, the event timer and the figures of a leg)
from trio_binning_amd import _lib  # noqa: E402
from trio_binning_amd._lib import check, lib  # noqa: E402

hip, _vp = mc.hip, C.c_void_p
hip.hipMemset.argtypes, hip.hipMemset.restype = [_vp, C.c_int, C.c_size_t], C.c_int
lib.tbk_kmerdb_arrays_.argtypes, lib.tbk_kmerdb_arrays_.restype = [_vp, C.POINTER(_vp), C.POINTER(_vp)], C.c_int
lib.tbk_launch_kmerdb_gc_spectrum.argtypes = [_vp, _vp, C.c_uint64, C.c_int, C.c_int, _vp, _vp]
lib.tbk_launch_kmerdb_gc_spectrum.restype = C.c_int
lib.tbk_launch_kmerdb_origin_spectrum.argtypes = [_vp, _vp, C.c_uint64, _vp, _vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp, _vp, C.c_uint64, C.c_uint32,
                                                  C.c_uint32, C.c_uint32, _vp, _vp]
lib.tbk_launch_kmerdb_origin_spectrum.restype = C.c_int
D2H = 2  # hipMemcpyDeviceToHost
LAYOUTS = {1: "whole matrix in LDS", 2: "counters below 64 in LDS"}
CELLS = 33 * 256
GRIDS = (2048, 1024, 512, 256)  # through the measurement hook tbk_kmerdb_gc_set_grid_; the build's is GC_GRID of csrc/tbk_compare.hip
lib.tbk_kmerdb_gc_set_grid_.argtypes, lib.tbk_kmerdb_gc_set_grid_.restype = [C.c_uint32], C.c_int


def measure(dev, n, k, runs, rng):
    db = mc.database(dev, 0, n, k, mc.spectrum_counters(rng, n))
    d_keys, d_counts = _vp(), _vp()
    check(lib.tbk_kmerdb_arrays_(db._h, C.byref(d_keys), C.byref(d_counts)))
    d_spec = mc.dalloc(8 * CELLS)
    zero = lambda: mc.ok(hip.hipMemset(d_spec, 0, 8 * CELLS), "hipMemset")
    want = db.gc_spectrum()
    assert int(want.sum()) == n and np.array_equal(want.sum(axis=0)[1:], db.histogram()[1:])
    rate = C.c_double()
    check(lib.tbk_calib_stream(dev, 9 * n, 10, C.byref(rate)))
    stream = round(rate.value / 1e9, 1)
    check(lib.tbk_calib_stream(dev, 1 << 30, 10, C.byref(rate)))
    out = {"k": k, "lds_bytes": {"1": (k + 1) * 256 * 4, "2": (k + 1) * 64 * 4}, "stream_GBps": stream, "stream_1GiB_GBps": round(rate.value / 1e9, 1),
           "rows_held": int((want.sum(axis=1) > 0).sum()), "counters_from_64": int(want[:, 64:].sum()), "legs": {}}
    for layout in LAYOUTS:
        launch = lambda: mc.ok(lib.tbk_launch_kmerdb_gc_spectrum(d_keys, d_counts, n, k, layout, d_spec, None), "tbk_launch_kmerdb_gc_spectrum")
        zero()
        launch()
        got = np.zeros((33, 256), dtype=np.uint64)
        mc.ok(hip.hipMemcpy(got.ctypes.data, d_spec, 8 * CELLS, D2H), "hipMemcpy")
        assert np.array_equal(got[:k + 1], want) and not got[k + 1:].any(), layout
        zero()
        out["legs"]["gc_layout{}".format(layout)] = mc.leg(mc.timed(runs, launch, zero), 9 * n, stream)
        try:  # fewer blocks, each over more tiles: less to zero and to flush, fewer waves to hide the loads behind
            for cap in GRIDS:
                check(lib.tbk_kmerdb_gc_set_grid_(cap))
                out["legs"]["gc_layout{}_grid{}".format(layout, cap)] = mc.leg(mc.timed(runs, launch, zero), 9 * n, stream)
        finally:
            check(lib.tbk_kmerdb_gc_set_grid_(0))
    origin = lambda: mc.ok(lib.tbk_launch_kmerdb_origin_spectrum(d_keys, d_counts, n, d_keys, d_counts, n, 1, 255, d_keys, d_counts, n, 1, 255, 15, d_spec,
                                                                 None), "tbk_launch_kmerdb_origin_spectrum")
    zero()
    out["legs"]["origin"] = mc.leg(mc.timed(runs, origin, zero), 9 * n, stream)
    table = db.origin_spectrum(db, db)
    assert np.array_equal(table[3][1:], db.histogram()[1:]) and not table[:3].any()
    out["legs"]["gc_call"] = mc.leg(mc.timed(runs, db.gc_spectrum), 9 * n, stream)
    out["legs"]["origin_call"] = mc.leg(mc.timed(runs, lambda: db.origin_spectrum(db, db)), 9 * n, stream)
    mc.ok(hip.hipFree(d_spec), "hipFree")
    db.close()
    return out


def section(result):
    """the part of the README one measure_gc*.json is: a paragraph and the table"""
    rows, kept = [], []
    for part in result["by_k"]:
        legs, k = part["legs"], part["k"]
        faster = min(LAYOUTS, key=lambda layout: legs["gc_layout{}".format(layout)]["ms"])
        kept.append((k, faster))
        for layout, name in LAYOUTS.items():
            leg = legs["gc_layout{}".format(layout)]
            rows.append("| {} | gc launch, {} ({} B), the build's grid | {} | {} | {} |".format(k, name, part["lds_bytes"][str(layout)], leg["ms"], leg["GBps"],
                                                                                          leg["fraction_of_stream"]))
            for cap in GRIDS:
                leg = legs.get("gc_layout{}_grid{}".format(layout, cap))
                if leg:
                    rows.append("| {} | - the same in {} blocks | {} | {} | {} |".format(k, cap, leg["ms"], leg["GBps"], leg["fraction_of_stream"]))
        for key, name in (("origin", "origin launch, the database as both partners"), ("gc_call", "`tbk_kmerdb_gc_spectrum`, the whole call"),
                          ("origin_call", "`tbk_kmerdb_origin_spectrum`, the whole call")):
            rows.append("| {} | {} | {} | {} | {} |".format(k, name, legs[key]["ms"], legs[key]["GBps"], legs[key]["fraction_of_stream"]))
    streams = "; ".join("k = {}: **{} GB/s** over 9 n bytes, {} GB/s over 1 GiB".format(p["k"], p["stream_GBps"], p["stream_1GiB_GBps"]) for p in result["by_k"])
    return """## {n} entries ({mb} MB of keys and counters)

{device}; one full database per k, uniform keys (GC binomial around k / 2: {rows}), counters 94 % Poisson around 30, 4 %
counter 1 or 2, 2 % spread evenly over 64..255 ({far} of the entries at k = {k0} have a counter from 64 on).  Median of {runs}.
`tbk_calib_stream` in the same process - {streams}.

| k | leg | ms | GB/s | of stream |
|---|---|---:|---:|---:|
{table}

Faster layout under the build's grid: {kept}.
""".format(device=result["device"], n=result["n"], mb=9 * result["n"] // 1000000, runs=result["runs"], streams=streams, table="\n".join(rows),
           rows=", ".join("{} of the {} rows hold entries at k = {}".format(p["rows_held"], p["k"] + 1, p["k"]) for p in result["by_k"]),
           far=result["by_k"][0]["counters_from_64"], k0=result["by_k"][0]["k"],
           kept=", ".join("k = {}: {} ({})".format(k, layout, LAYOUTS[layout]) for k, layout in kept))


def readme(results, regs):
    text = """# r25 - the GC x count matrix of a count database

What this directory is for: the times of the one launch behind `tbk_kmerdb_gc_spectrum` with each of the two LDS layouts its kernel
is written for and under four grids, beside the origin spectrum's launch over the same bytes and beside `tbk_calib_stream` (DESIGN
§9, "K-mer multiplicity against GC").  Written by `tools/measure_gc.py`, one run per database size; the `measure_gc*.json` files
have every run.

HIP events on the null stream around each leg, one warm-up, then the median; the launches tally into a device matrix zeroed
outside the timed span, the calls include their allocation, memset and the copy of the matrix home.  GB/s is over 9 bytes an
entry, read once; "of stream" is that rate over the stream figure of the same footprint.  A database of 2e7 entries fits the
256 MB Infinity Cache and is warm in it, its stream figure likewise; one of 1e8 is read from HBM.

The build keeps layout **{layout}** (`GC_LAYOUT` in `csrc/tbk_compare.hip`: {name}) in **{grid}** blocks (`GC_GRID`).

""".format(layout=results[0]["build_layout"], name=LAYOUTS[results[0]["build_layout"]], grid=results[0].get("build_grid", "?"))
    text += "\n".join(section(result) for result in results)
    if regs:
        fence = "" if regs.lstrip().startswith("|") else "```\n"
        text += "\n## Registers (`tools/kernel_regs.sh trio_binning_amd/csrc/build/tbk_compare.o tbk_kmerdb_gc`)\n\n" + fence + regs.strip() + "\n" + fence
        text += "\nLDS is dynamic: (k + 1) x 256 or (k + 1) x 64 words, the bytes in the tables above.  No scratch, no spills.\n"
    return text


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=20_000_000)
    ap.add_argument("--k", type=int, nargs="+", default=[21, 32])
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--build-layout", type=int, default=1, help="the layout the loaded library was built with (GC_LAYOUT), for the README")
    ap.add_argument("--build-grid", type=int, default=1024, help="the grid the loaded library was built with (GC_GRID), for the README")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r25"))
    ap.add_argument("--regs", default=None)
    ap.add_argument("--render-only", action="store_true")
    args = ap.parse_args()
    if not args.render_only:
        dev = 0
        rng = np.random.default_rng(25)
        result = {"device": _lib.device_name(dev), "n": args.n, "runs": args.runs, "build_layout": args.build_layout, "build_grid": args.build_grid,
                  "by_k": []}
        os.makedirs(args.out_dir, exist_ok=True)
        path = os.path.join(args.out_dir, "measure_gc.json" if args.n == 20_000_000 else "measure_gc_n{}.json".format(args.n))
        for k in args.k:  # (what is measured is on disk before the next database is made)
            result["by_k"].append(measure(dev, args.n, k, args.runs, rng))
            with open(path, "w") as fh:
                fh.write(json.dumps(result) + "\n")
        print(json.dumps(result))
    import glob

    results = sorted((json.loads(open(path).read()) for path in glob.glob(os.path.join(args.out_dir, "measure_gc*.json"))), key=lambda r: r["n"])
    with open(os.path.join(args.out_dir, "README.md"), "w") as fh:
        fh.write(readme(results, open(args.regs).read() if args.regs else None))


if __name__ == "__main__":
    main()
