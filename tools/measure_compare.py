"""Time tbk_kmerdb_joint_spectrum and tbk_kmerdb_origin_spectrum on synthetic full databases beside tbk_kmerdb_union, the
join over the same bytes that exists already, and beside the streaming-read figure of the device.

    python tools/measure_compare.py [--n 20000000] [--k 21] [--runs 7] [--out-dir profiles/r19]
                                    [--regs FILE] [--kernel-stats FILE] [--bench-parent FILE... --bench-change FILE...]
    python tools/measure_compare.py --render-only [--out-dir profiles/r19] [...]    # README.md again from measure_compare.json, no device

Three databases of `n` entries each: A, B (half of its keys are A's) and C (disjoint from both).  The keys are
tbk_synth_keys_device's (distinct by construction), turned into ranks and sorted with their counters by the path
tbk_counter_export takes, and adopted as databases where they lie (tools/measure_union.py's way).  The counters are a
sequenced library's spectrum in the small: 94 % Poisson around 30, 4 % error k-mers with counter 1 or 2, 2 % repeats spread
evenly over 64..255.  Every leg runs in this process, one after the other: HIP events on the null stream around the whole
call - its allocation, its memset and the copy of the spectrum to the host included, since that is what a caller waits for -
one warm-up, then the median of `runs`, on the half-shared pair and on the disjoint one.  The side of the joint kernel's LDS
corner is a constant of the build: the other sides tried are variant libraries (`VARIANT_SRC=tbk_compare tools/build_variant.sh
corner32 -DTBK_JOINT_CORNER=32`), each measured by a run of this tool under TBK_LIBRARY with --corner 32, which times the joint
spectrum alone and writes measure_compare_corner32.json; the README lists every such file beside the default's.  `bytes` is
what a result needs at the least:
each input read once, 9 bytes an entry (the union also writes its output).  Every spectrum is checked against what the
construction implies before it is timed.  Writes measure_compare.json and README.md into --out-dir; --regs (the text of
tools/kernel_regs.sh on build/tbk_compare.o), --kernel-stats (the kernel_stats CSV of a `rocprofv3 --kernel-trace --stats` run of
this tool, a run of its own) and the bench.py lines of parent and change (one file per run, in the order they ran) are copied
into the README when given."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from trio_binning_amd import _lib, kmers  # noqa: E402
from trio_binning_amd._lib import check, lib  # noqa: E402

hip = C.CDLL("libamdhip64.so")
_vp = C.c_void_p
for name, argtypes in (("hipEventCreate", [C.POINTER(_vp)]), ("hipEventRecord", [_vp, _vp]), ("hipEventSynchronize", [_vp]),
                       ("hipEventElapsedTime", [C.POINTER(C.c_float), _vp, _vp]), ("hipEventDestroy", [_vp]),
                       ("hipMemcpy", [_vp, _vp, C.c_size_t, C.c_int]), ("hipMalloc", [C.POINTER(_vp), C.c_size_t]), ("hipFree", [_vp])):
    getattr(hip, name).argtypes, getattr(hip, name).restype = argtypes, C.c_int
lib.tbk_launch_db_rank.argtypes, lib.tbk_launch_db_rank.restype = [_vp, _vp, C.c_uint64, C.c_int, _vp, _vp, _vp], C.c_int
lib.tbk_launch_sort_u64_u8.argtypes, lib.tbk_launch_sort_u64_u8.restype = [_vp, _vp, _vp, _vp, C.c_uint64, C.c_int, _vp], C.c_int
lib.tbk_kmerdb_adopt_device_.argtypes, lib.tbk_kmerdb_adopt_device_.restype = [_vp, _vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)], C.c_int
H2D = 1  # hipMemcpyHostToDevice
DEFAULT_CORNER = 64


def ok(status, what):
    if status != 0:
        raise RuntimeError("{}: HIP error {}".format(what, status))


def dalloc(nbytes):
    p = _vp()
    ok(hip.hipMalloc(C.byref(p), max(nbytes, 16)), "hipMalloc")
    return p.value


def spectrum_counters(rng, n):
    """a library's spectrum in the small: 94 % Poisson(30), 4 % errors (1 or 2), 2 % repeats (64..255, evenly)"""
    u = rng.random(n)
    out = np.clip(rng.poisson(30, n), 1, 255)
    out = np.where(u < 0.04, rng.integers(1, 3, n), out)
    out = np.where(u > 0.98, rng.integers(64, 256, n), out)
    return out.astype(np.uint8)


def database(dev, first, n, k, counters):
    """the full database of the synthetic keys first .. first + n - 1 with `counters`, dealt to the keys as they come"""
    d_raw, d_rank, d_keys = dalloc(8 * n), dalloc(8 * n), dalloc(8 * n)
    d_c0, d_c1, d_counts = dalloc(n), dalloc(n), dalloc(n)
    check(lib.tbk_synth_keys_device(dev, 0x5EED0001, first, n, k, _vp(d_raw)))
    ok(hip.hipMemcpy(d_c0, counters.ctypes.data, n, H2D), "hipMemcpy")
    ok(lib.tbk_launch_db_rank(d_raw, d_c0, n, k, d_rank, d_c1, None), "tbk_launch_db_rank")
    ok(lib.tbk_launch_sort_u64_u8(d_rank, d_keys, d_c1, d_counts, n, 2 * k, None), "tbk_launch_sort_u64_u8")
    check(lib.tbk_device_sync(dev))
    for p in (d_raw, d_rank, d_c0, d_c1):
        ok(hip.hipFree(p), "hipFree")
    h = _vp()
    check(lib.tbk_kmerdb_adopt_device_(d_keys, d_counts, n, k, dev, 1, C.byref(h)))
    return kmers.KmerDatabase(h)


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


def leg(times, nbytes, stream_gbps):
    med = statistics.median(times)
    return {"ms": round(med, 4), "ms_all": [round(t, 4) for t in times], "bytes_at_least": nbytes, "GBps": round(nbytes / med / 1e6, 1),
            "fraction_of_stream": round(nbytes / med / 1e6 / stream_gbps, 3)}


def bench_line(path):
    """the figures of a bench.py line that say where the classify stage is"""
    line = json.loads(open(path).read().strip().splitlines()[-1])
    keep = ("value", "unit", "ms_per_step", "table_build_s")
    return {key: line[key] for key in keep if key in line}


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


def readme(result, variants, regs, benches, kernel_stats=None):
    n, pairs = result["n"], result["pairs"]
    rows = []
    for pair in ("half_shared", "disjoint"):
        p = pairs[pair]
        for corner, joint in sorted([(DEFAULT_CORNER, p["joint"])] + [(v["corner"], v["pairs"][pair]["joint"]) for v in variants]):
            rows.append("| {} | joint spectrum, corner {}{} | {} | {} | {} |".format(pair, corner, " (the build's)" if corner == DEFAULT_CORNER else " (variant)",
                                                                                  joint["ms"], joint["GBps"], joint["fraction_of_stream"]))
        rows.append("| {} | `tbk_kmerdb_union` | {} | {} | {} |".format(pair, p["union"]["ms"], p["union"]["GBps"], p["union"]["fraction_of_stream"]))
    o = result["origin"]
    text = """# r19 - count databases held against each other: joint and origin spectrum

What this directory is for: the register figures of the two kernels of `csrc/tbk_compare.hip` and the times of
`tbk_kmerdb_joint_spectrum` and `tbk_kmerdb_origin_spectrum` beside `tbk_kmerdb_union` - the join over the same bytes the
parent commit has - and beside `tbk_calib_stream` (DESIGN §9, "Databases held against each other").  Written by
`tools/measure_compare.py`; `measure_compare.json` has every run.

## Measurement

{device}; k = {k}; three full databases of {n} entries each: A, B (half of its keys are A's) and C (disjoint).  Counters: 94 %
Poisson around 30, 4 % counter 1 or 2, 2 % spread evenly over 64..255.  HIP events around each whole call (allocation, memset
and the copy of the spectrum home included), one warm-up, median of {runs}.  `tbk_calib_stream` in the same process:
**{stream} GB/s**.  GB/s is over the bytes a result needs at the least - each input read once, 9 bytes an entry; the union's
figure adds its output - and "of stream" is that rate over the stream figure.

| pair | call | ms | GB/s | of stream |
|---|---|---:|---:|---:|
{rows}
| A against B and C | origin spectrum | {oms} | {ogb} | {ofr} |

Shared k-mers found: {shared} of {n} (half-shared pair), {zero} (disjoint pair); every spectrum's row and column sums were
checked against the databases' histograms before timing.

The joint kernel's LDS corner is **{default}**; the table has every side tried, the others as variant builds in the same job.
""".format(device=result["device"], k=result["k"], n=n, runs=result["runs"], stream=result["stream_GBps"], rows="\n".join(rows),
           oms=o["ms"], ogb=o["GBps"], ofr=o["fraction_of_stream"], shared=result["shared_half"], zero=result["shared_disjoint"],
           default=DEFAULT_CORNER)
    if regs:
        fence = "" if regs.lstrip().startswith("|") else "```\n"  # (a table is given as it is)
        text += ("\n## Registers (`tools/kernel_regs.sh trio_binning_amd/csrc/build/tbk_compare.o tbk_kmerdb`; SGPRs and scratch from the same notes)\n\n"
                 + fence + regs.strip() + "\n" + fence + "\nNo scratch, no spills.\n")
    if kernel_stats:
        text += ("\n## Kernel times (`rocprofv3 --kernel-trace --stats -- python3 tools/measure_compare.py --runs 5`, a run of its own)\n\n"
                 "The origin kernel's calls are the origin spectrum's (the slowest ones: two partners) and the second launch of every joint\n"
                 "spectrum (one partner); the union's kernels are beside them.\n\n| kernel | calls | average ms | min | max |\n|---|---:|---:|---:|---:|\n")
        text += "\n".join(kernel_rows(kernel_stats)) + "\n"
    if benches:
        text += "\n## `bench.py --gpus 1 --steps 5 --warmup 2`, parent and change taking turns in one job\n\n| build | " + " | ".join(benches[0][1]) + " |\n"
        text += "|---|" + "---:|" * len(benches[0][1]) + "\n"
        for build, line in benches:
            text += "| {} | ".format(build) + " | ".join(str(v) for v in line.values()) + " |\n"
        text += "\nThe parent's line is the parent commit's library under this tree's Python (`TBK_LIBRARY`); the classify stage runs no code this change touches.\n"
    return text


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=20_000_000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--corner", type=int, default=DEFAULT_CORNER, help="the corner the loaded library was built with; another than the default: the joint spectrum alone")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r19"))
    ap.add_argument("--regs", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--bench-parent", nargs="*", default=[])
    ap.add_argument("--bench-change", nargs="*", default=[])
    ap.add_argument("--render-only", action="store_true")
    args = ap.parse_args()
    if args.render_only:
        render(args, json.loads(open(os.path.join(args.out_dir, "measure_compare.json")).read()))
        return
    dev, n, k = 0, args.n, args.k
    rng = np.random.default_rng(19)
    a, b, c = (database(dev, first, n, k, spectrum_counters(rng, n)) for first in (0, n // 2, 2 * n))
    hists = [db.histogram() for db in (a, b, c)]
    rate = C.c_double()
    check(lib.tbk_calib_stream(dev, 1 << 30, 10, C.byref(rate)))
    stream = round(rate.value / 1e9, 1)
    result = {"device": _lib.device_name(dev), "k": k, "n": n, "runs": args.runs, "stream_GBps": stream, "corner": args.corner, "pairs": {}}
    made = []
    for pair, (x, y, hx, hy) in (("half_shared", (a, b, hists[0], hists[1])), ("disjoint", (a, c, hists[0], hists[2]))):
        first = x.joint_spectrum(y)
        assert int(first[0, 0]) == 0 and np.array_equal(first.sum(axis=1)[1:], hx[1:]) and np.array_equal(first.sum(axis=0)[1:], hy[1:])
        legs = {"joint": leg(timed(args.runs, lambda: x.joint_spectrum(y)), 9 * 2 * n, stream)}
        shared = int(first[1:, 1:].sum())
        result["shared_" + ("half" if pair == "half_shared" else "disjoint")] = shared
        assert shared == (n - n // 2 if pair == "half_shared" else 0)
        assert int(first.sum()) == 2 * n - shared
        if args.corner == DEFAULT_CORNER:
            with x.union(y) as u:
                assert len(u) == 2 * n - shared
            legs["union"] = leg(timed(args.runs, lambda: made.append(x.union(y)), lambda: made.pop().close()), 9 * (2 * n + 2 * n - shared), stream)
        result["pairs"][pair] = legs
    if args.corner == DEFAULT_CORNER:
        table = a.origin_spectrum(b, c)
        assert np.array_equal(table.sum(axis=0)[1:], hists[0][1:]) and not table[2:].any() and int(table[1].sum()) == result["shared_half"]
        result["origin"] = leg(timed(args.runs, lambda: a.origin_spectrum(b, c)), 9 * 3 * n, stream)
    for db in (a, b, c):
        db.close()
    os.makedirs(args.out_dir, exist_ok=True)
    line = json.dumps(result)
    print(line)
    name = "measure_compare.json" if args.corner == DEFAULT_CORNER else "measure_compare_corner{}.json".format(args.corner)
    with open(os.path.join(args.out_dir, name), "w") as fh:
        fh.write(line + "\n")
    if args.corner == DEFAULT_CORNER:
        render(args, result)


def render(args, result):
    regs = open(args.regs).read() if args.regs else None
    benches = [(build, bench_line(path)) for pair in zip(args.bench_parent, args.bench_change) for build, path in zip(("parent", "change"), pair)]
    import glob

    variants = [json.loads(open(path).read()) for path in sorted(glob.glob(os.path.join(args.out_dir, "measure_compare_corner*.json")))]
    with open(os.path.join(args.out_dir, "README.md"), "w") as fh:
        fh.write(readme(result, variants, regs, benches, args.kernel_stats))


if __name__ == "__main__":
    main()
