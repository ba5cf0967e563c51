"""Time tbk_kmerdb_hetmers - the het-mer pairs inside one count database - on the crafted databases of
tools/measure_db_handoff.py --inherited (tools/measure_select.py's construction), and the query session's lookup beside it.

    python tools/measure_hetmers.py [--n 100000000] [-k 21] [--runs 7] [--tmp /dev/shm] [--out-dir profiles/r21]
    python tools/measure_hetmers.py --name measure_hetmers_nodir.json   # under TBK_LIBRARY: the variant -DTBK_LOOKUP_NO_DIRECTORY
    python tools/measure_hetmers.py --render-only [--regs FILE] [--bench-parent FILE... --bench-change FILE...]

Three databases of about --n k-mers: A (ascending random ranks made canonical - a database of anything else has no class
structure - with counters uniform in 2..40), B (every fourth key of A and as many keys A lacks) and a child that stands where
A's entries stand or one rank above.  Random ranks hold next to no middle partner of each other (1e8 of 4^21 ranks: a few
thousand by chance), so every --plant-th key of A also gets its variant key ^ (1 << (k - 1)) as an entry: where both counters
are in range they form a pair.  Every leg runs in this process and the
legs take turns: HIP events on the null stream around the whole call - its allocations, the directory, the copies home - one
warm-up round, then the median of --runs rounds; tbk_calib_stream in the same process.  The legs:

  tally            A.hetmers(5, 35)
  tally_and_pairs  A.hetmers(5, 35, pairs=True): flag, scan, scatter and the records' copy home on top
  with_partners    A.hetmers(5, 35, y=B, z=child): four bounded searches per pair more
  query_add        a query session on A taking a batch of random contigs (--query-bases): one lookup per window through the
                   same kind of directory; a random sequence finds nothing, so this is the cost of a window that is absent

`ns_per_lookup` is the call's time over 3 x candidates, `ns_per_window` the query's over its clean windows.  The tallies of the
three hetmers legs must agree with each other and with the class structure before anything is timed.  Writes
measure_hetmers.json (or --name) and README.md into --out-dir."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.measure_select import bench_line, hip, ok, write_db  # noqa: E402  (the events' signatures are set there)
from trio_binning_amd import _lib, kmers  # noqa: E402
from trio_binning_amd._lib import check, lib  # noqa: E402

_vp = C.c_void_p
LO, HI = 5, 35


def revcomp_ranks(x, k):
    """the reverse complements of lexicographic ranks (uint64 array): the complement's 2-bit groups in reverse order"""
    x = ~np.asarray(x, dtype=np.uint64)
    for shift, mask in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F)):
        x = ((x >> np.uint64(shift)) & np.uint64(mask)) | ((x & np.uint64(mask)) << np.uint64(shift))
    return x.byteswap() >> np.uint64(64 - 2 * k)


def timed(runs, calls):
    """{name: [milliseconds between two events around calls[name]()]}: one warm-up round, then `runs` rounds of every leg in order"""
    e0, e1 = _vp(), _vp()
    ok(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    times = {name: [] for name in calls}
    for run in range(runs + 1):
        for name, call in calls.items():
            ok(hip.hipEventRecord(e0, None), "hipEventRecord")
            call()
            ok(hip.hipEventRecord(e1, None), "hipEventRecord")
            ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            ms = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
            if run:
                times[name].append(ms.value)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    return times


def readme(result, nodir, regs, benches):
    rows = []
    for name, rec in result["legs"].items():
        per = rec.get("ns_per_lookup", rec.get("ns_per_window"))
        rows.append("| `{}` | {} | {} | {} |".format(name, rec["ms"], per, "window" if "ns_per_window" in rec else "lookup"))
    if nodir:
        for name in ("tally", "tally_and_pairs", "with_partners"):
            rec = nodir["legs"][name]
            rows.append("| `{}`, every lookup a bisection of the whole database (variant build, a run of its own) | {} | {} | lookup |".format(
                name, rec["ms"], rec["ns_per_lookup"]))
    text = """# r21 - het-mer pairs of a count database

What this directory is for: the register figures of the kernels of `csrc/tbk_hetmer.hip` and the times of `tbk_kmerdb_hetmers`
beside the query session's lookup on the same database (DESIGN §9, "Het-mer pairs").  Written by `tools/measure_hetmers.py`;
`measure_hetmers.json` has every run.

## Measurement

{device}; k = {k}; A holds {n} entries ({planted} of them planted variants), {candidates} candidates in [{lo}, {hi}], {pairs} pairs;
B and the child as `tools/measure_select.py` crafts them.  HIP events around each whole call; the legs take turns, one warm-up
round, median of {runs}.  `tbk_calib_stream` in the same process: **{stream} GB/s**.  The last column says what the nanoseconds are
per: a lookup is one of the 3 x candidates variants of a call (dropped variants included), a window one clean window start of
the query's batch of {query_bases} random bases (none of them found).

| leg | ms | ns per | |
|---|---:|---:|---|
{rows}
""".format(device=result["device"], k=result["k"], n=result["n"], planted=result["planted"], candidates=result["candidates"], pairs=result["pairs"],
           lo=LO, hi=HI, runs=result["runs"], stream=result["stream_GBps"], query_bases=result["query_bases"], rows="\n".join(rows))
    if regs:
        text += ("\n## Registers (`tools/kernel_regs.sh trio_binning_amd/csrc/build/tbk_hetmer.o hetmer`; SGPRs from the same notes)\n\n" + regs.strip() + "\n")
    if benches:
        text += "\n## `bench.py --gpus 1 --steps 5 --warmup 2`, parent and change taking turns, in the order they ran\n\n| build | " + " | ".join(benches[0][1]) + " |\n"
        text += "|---|" + "---:|" * len(benches[0][1]) + "\n"
        for build, line in benches:
            text += "| {} | ".format(build) + " | ".join(str(v) for v in line.values()) + " |\n"
        text += "\nThe parent's line is the parent commit's library under this tree's Python (`TBK_LIBRARY`); the classify stage runs no code this change touches.\n"
    return text


def render(args, result):
    path = os.path.join(args.out_dir, "measure_hetmers_nodir.json")
    nodir = json.loads(open(path).read()) if os.path.exists(path) else None
    regs = open(args.regs).read() if args.regs else None
    benches = [(build, bench_line(p)) for pair in zip(args.bench_parent, args.bench_change) for build, p in zip(("parent", "change"), pair)]
    with open(os.path.join(args.out_dir, "README.md"), "w") as fh:
        fh.write(readme(result, nodir, regs, benches))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--plant", type=int, default=50, help="every this many keys of A gets its middle variant as an entry too")
    ap.add_argument("--query-bases", type=int, default=60_000_000)
    ap.add_argument("--tmp", default="/dev/shm")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r21"))
    ap.add_argument("--name", default="measure_hetmers.json")
    ap.add_argument("--regs", default=None)
    ap.add_argument("--bench-parent", nargs="*", default=[])
    ap.add_argument("--bench-change", nargs="*", default=[])
    ap.add_argument("--render-only", action="store_true")
    args = ap.parse_args()
    if args.render_only:
        render(args, json.loads(open(os.path.join(args.out_dir, "measure_hetmers.json")).read()))
        return
    k, n, dev = args.k, args.n, 0
    assert k % 2 == 1
    rng = np.random.default_rng(10)
    max_gap = max(3, min(40_000, (1 << (2 * k)) // n - 1))
    t = time.time()
    keys_a = np.cumsum(rng.integers(2, max_gap + 1, n, dtype=np.uint64), dtype=np.uint64)
    assert int(keys_a[-1]) < 1 << (2 * k), "4^k is too small for --n"
    keys_a = np.unique(np.minimum(keys_a, revcomp_ranks(keys_a, k)))  # canonical: the class structure holds for such entries alone
    n = int(keys_a.size)
    fourth = np.arange(n, dtype=np.uint64) % np.uint64(4) != 0
    keys_b = np.unique(keys_a + fourth.astype(np.uint64))  # every fourth key shared
    keys_c = np.unique(keys_a + (np.arange(n, dtype=np.uint64) % np.uint64(3) == 0).astype(np.uint64))
    planted = keys_a[::args.plant] ^ np.uint64(1 << (k - 1))  # (the flanks decide the orientation: canonical again)
    assert np.array_equal(planted, np.minimum(planted, revcomp_ranks(planted, k)))
    keys_a = np.union1d(keys_a, planted)
    n_planted = int(keys_a.size) - n
    counts = [rng.integers(2, 41, keys.size).astype(np.uint8) for keys in (keys_a, keys_b, keys_c)]
    paths = [os.path.join(args.tmp, "tbk_hetmers_%d_%s.tbkdb" % (os.getpid(), h)) for h in "abc"]
    dbs = []
    try:
        for path, keys, cs in zip(paths, (keys_a, keys_b, keys_c), counts):
            write_db(path, k, keys, cs)
            dbs.append(kmers.KmerDatabase.load(path))
            os.remove(path)
    finally:
        for path in paths:
            if os.path.exists(path):
                os.remove(path)
    da, db, dc = dbs
    n_a = int(keys_a.size)
    del keys_a, keys_b, keys_c, planted, fourth
    craft_s = round(time.time() - t, 2)
    rate = C.c_double()
    check(lib.tbk_calib_stream(dev, 1 << 30, 10, C.byref(rate)))
    stream = round(rate.value / 1e9, 1)

    calls = {"tally": lambda: da.hetmers(LO, HI), "tally_and_pairs": lambda: da.hetmers(LO, HI, pairs=True),
             "with_partners": lambda: da.hetmers(LO, HI, y=db, z=dc)}
    first = {name: call() for name, call in calls.items()}
    base = first["tally"]
    parts = [int(v) for v in base["partners"]]
    assert sum(parts) == base["candidates"] and parts[1] == 2 * base["pairs"] and parts[2] % 3 == 0 and parts[3] % 4 == 0
    assert int(base["spec"].sum()) == base["pairs"] and first["tally_and_pairs"]["records"].size == base["pairs"]
    for other in (first["tally_and_pairs"], first["with_partners"]):
        assert other["candidates"] == base["candidates"] and np.array_equal(other["partners"], base["partners"]) and np.array_equal(other["spec"], base["spec"])
    assert int(first["with_partners"]["origin"].sum()) == base["pairs"] and int(base["origin"][0, 0]) == base["pairs"]
    result = {"device": _lib.device_name(dev), "library": os.path.basename(os.environ.get("TBK_LIBRARY", "")), "k": k, "n": n_a, "planted": n_planted,
              "runs": args.runs, "cutoffs": [LO, HI], "candidates": base["candidates"], "partners": parts, "pairs": base["pairs"],
              "origin": first["with_partners"]["origin"].tolist(), "craft_and_load_s": craft_s, "stream_GBps": stream, "query_bases": args.query_bases,
              "legs": {}}
    del first

    length = 15000
    contigs = args.query_bases // length
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, contigs * length, dtype=np.uint8)]
    offs = np.arange(contigs + 1, dtype=np.uint64) * np.uint64(length)
    with da.query() as session:
        per_read = session.add(bases, offs)
        clean = int(per_read[:, 0].sum())

        def query_add():
            session.reset()
            session.add(bases, offs)

        calls["query_add"] = query_add
        times = timed(args.runs, calls)
    for name, ts in times.items():
        med = statistics.median(ts)
        rec = {"ms": round(med, 4), "ms_all": [round(v, 4) for v in ts]}
        if name == "query_add":
            rec["clean_windows"] = clean
            rec["ns_per_window"] = round(med * 1e6 / clean, 4)
        else:
            rec["ns_per_lookup"] = round(med * 1e6 / (3 * base["candidates"]), 4)
        result["legs"][name] = rec
    for d in dbs:
        d.close()
    os.makedirs(args.out_dir, exist_ok=True)
    line = json.dumps(result)
    print(line)
    with open(os.path.join(args.out_dir, args.name), "w") as fh:
        fh.write(line + "\n")
    if args.name == "measure_hetmers.json":
        render(args, result)


if __name__ == "__main__":
    main()
