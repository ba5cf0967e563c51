#!/usr/bin/env python3
"""From two count databases to the k-mer list a classifier is built from: the route through text against the direct one.

Two databases of --n k-mers each are crafted (ascending random ranks; B holds every fourth key of A and as many keys A
lacks; counters uniform in 2..40, cut-offs [5,35]) and loaded.  In one process, one warm-up and --runs timed runs each,
bracketed with a device synchronisation:

  text    KmerDatabase.unique() to a file under --tmp (tbk_kmerdb_unique: select, sort, copy home, print), then
          create_kmer_hash_set() on that file with TBK_LIST_CACHE=0 (stage the text, parse it on the GPU);
  direct  KmerDatabase.unique_set() (tbk_kmerdb_unique_table: flag, scan, scatter in HBM).

Both must give the same keys; the record also says how many bytes of text the direct route never writes or reads.
Prints one JSON line; --out writes it to a file too.

--inherited measures the three-database selection instead (tbk_kmerdb_inherited_table), on the same A and B and a third
crafted database of --n ranks: the child holds every second k-mer of A that unique_set(b) selects and, in place of every
other entry of A, the rank above it; counters uniform in 2..40, the child's range [2,255].  Timed alternately after a warm-up:

  unique_set   today's KmerDatabase.unique_set(b) on A and B, the same-box yardstick;
  inherited    KmerDatabase.unique_set(b, child=child).

The inherited keys must be every second key of unique_set's.  --full-depth-library names a variant of the library whose
flag kernel bisects the whole of B and of the child for every entry (VARIANT_SRC=tbk_count_kernels tools/build_variant.sh
inherited_full -DTBK_INHERITED_FULL_DEPTH): the same measurement is repeated with it in a fresh process, after this one's
databases are closed, and joins the record as "full_depth"."""
import argparse, ctypes as C, json, os, struct, subprocess, sys, time, zlib
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100_000_000)
ap.add_argument("-k", type=int, default=21)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--tmp", default="/dev/shm")
ap.add_argument("--out", default="")
ap.add_argument("--inherited", action="store_true")
ap.add_argument("--full-depth-library", default="")
a = ap.parse_args()
os.environ["TBK_LIST_CACHE"] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from trio_binning_amd import kmers
from trio_binning_amd._lib import check, lib

k, n, dev = a.k, a.n, 0
LO, HI = 5, 35
rng = np.random.default_rng(10)
max_gap = max(3, min(40_000, (1 << (2 * k)) // n - 1))
assert max_gap >= 3, "4^k is too small for --n"


def write_db(path, keys, counts):
    """The *.tbkdb layout of INTEGRATION.md: header, keys, counters."""
    hist = np.bincount(counts, minlength=256).astype("<u8")
    hist[0] = keys.size
    body = b"TBKKMDB1" + struct.pack("<IIQQQ", 2096, k, keys.size, 0, 0) + hist.tobytes()
    with open(path, "wb") as fh:
        fh.write(body + struct.pack("<II", zlib.crc32(body) & 0xFFFFFFFF, 0))
        keys.astype("<u8").tofile(fh)
        counts.tofile(fh)


t = time.time()
keys_a = np.cumsum(rng.integers(2, max_gap + 1, n, dtype=np.uint64), dtype=np.uint64)
assert int(keys_a[-1]) < 1 << (2 * k)
keys_b = keys_a + (np.arange(n, dtype=np.uint64) % np.uint64(4) != 0).astype(np.uint64)  # every fourth key shared, gaps >= 2 keep it ascending
paths = [os.path.join(a.tmp, "tbk_handoff_%d_%s.tbkdb" % (os.getpid(), h)) for h in "ab"]
text_path = os.path.join(a.tmp, "tbk_handoff_%d.txt" % os.getpid())
out = {"k": k, "n_per_database": n, "cutoffs": [LO, HI], "runs": a.runs}
try:
    counts_a = rng.integers(2, 41, n).astype(np.uint8)
    write_db(paths[0], keys_a, counts_a)
    write_db(paths[1], keys_b, rng.integers(2, 41, n).astype(np.uint8))
    if a.inherited:
        selected = (counts_a >= LO) & (counts_a <= HI) & (np.arange(n, dtype=np.uint64) % np.uint64(4) != 0)
        held = selected & (np.cumsum(selected) % 2 == 1)  # the 1st, 3rd, ... selected entry of A
        paths.append(paths[0].replace("_a.tbkdb", "_child.tbkdb"))
        write_db(paths[2], keys_a + (~held).astype(np.uint64), rng.integers(2, 41, n).astype(np.uint8))
        out["selected"], out["held_by_child"] = int(selected.sum()), int(held.sum())
        del selected, held
    del keys_a, keys_b, counts_a
    out["craft_s"] = round(time.time() - t, 2)
    t = time.time()
    da, db = kmers.KmerDatabase.load(paths[0]), kmers.KmerDatabase.load(paths[1])
    out["load_both_s"] = round(time.time() - t, 2)
    for p in paths[:2]:
        os.remove(p)

    def sync():
        check(lib.tbk_device_sync(dev))

    if a.inherited:
        dc = kmers.KmerDatabase.load(paths[2])
        os.remove(paths[2])
        legs = {"unique_set": [], "inherited": []}
        for run in range(a.runs + 1):  # run 0 warms up
            for name, child in (("unique_set", {}), ("inherited", {"child": dc, "child_min": 2, "child_max": 255})):
                sync(); t0 = time.time()
                hs = da.unique_set(db, LO, HI, **child)
                sync(); t1 = time.time()
                if run == 0:
                    legs[name + "_keys"] = hs.keys()
                else:
                    legs[name].append(round(t1 - t0, 5))
                hs.close()
        two, three = legs.pop("unique_set_keys"), legs.pop("inherited_keys")
        same = two.size == out["selected"] and np.array_equal(three, two[::2])
        del two, three
        da.close(); db.close(); dc.close()
        med = lambda rows: sorted(rows)[len(rows) // 2]
        out.update({"same_keys": bool(same), "library": os.path.basename(os.environ.get("TBK_LIBRARY", "")), "device": kmers._lib.device_name(dev),
                    "unique_set_s": med(legs["unique_set"]), "inherited_s": med(legs["inherited"]),
                    "unique_set_all_s": legs["unique_set"], "inherited_all_s": legs["inherited"]})
        out["inherited_over_unique_set"] = round(out["inherited_s"] / out["unique_set_s"], 2)
        if a.full_depth_library and same:
            cmd = [sys.executable, os.path.abspath(__file__), "--inherited", "--n", str(n), "-k", str(k), "--runs", str(a.runs), "--tmp", a.tmp]
            done = subprocess.run(cmd, env=dict(os.environ, TBK_LIBRARY=os.path.abspath(a.full_depth_library)), stdout=subprocess.PIPE, timeout=600)
            out["full_depth"] = json.loads(done.stdout.decode().strip().splitlines()[-1]) if done.returncode == 0 else {"returncode": done.returncode}
            if done.returncode == 0:
                out["full_depth_over_bounded"] = round(out["full_depth"]["inherited_s"] / out["inherited_s"], 2)
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        sys.exit(0 if same and out.get("full_depth", {}).get("same_keys", True) else 1)

    def text_route():
        sync(); t0 = time.time()
        lines = da.unique(db, LO, HI, text_path)
        sync(); t1 = time.time()
        hs = kmers.HashSet.from_file(text_path)
        sync(); t2 = time.time()
        return hs, {"dump_s": t1 - t0, "load_s": t2 - t1, "total_s": t2 - t0, "lines": lines}

    def direct_route():
        sync(); t0 = time.time()
        hs = da.unique_set(db, LO, HI)
        sync(); t1 = time.time()
        return hs, {"total_s": t1 - t0, "lines": hs.num_kmers}

    legs = {"text": [], "direct": []}
    for run in range(a.runs + 1):  # run 0 warms up
        for name, route in (("text", text_route), ("direct", direct_route)):
            hs, rec = route()
            if run == 0:
                rec["origin"] = hs.origin
                legs[name + "_warm_up"] = rec
                legs[name + "_keys"] = hs.keys()
            else:
                legs[name].append(rec)
            hs.close()
    same = np.array_equal(legs.pop("text_keys"), legs.pop("direct_keys"))
    lines = legs["direct"][0]["lines"]
    med = lambda rows, f: round(sorted(r[f] for r in rows)[len(rows) // 2], 4)
    out.update({
        "lines": lines, "same_keys": bool(same), "text_bytes_avoided": lines * (k + 1),
        "text_dump_s": med(legs["text"], "dump_s"), "text_load_s": med(legs["text"], "load_s"), "text_total_s": med(legs["text"], "total_s"),
        "direct_total_s": med(legs["direct"], "total_s"),
        "text_total_all_s": [round(r["total_s"], 4) for r in legs["text"]], "direct_total_all_s": [round(r["total_s"], 4) for r in legs["direct"]],
        "warm_up": {"text_s": round(legs["text_warm_up"]["total_s"], 4), "direct_s": round(legs["direct_warm_up"]["total_s"], 4),
                    "text_origin": legs["text_warm_up"]["origin"], "direct_origin": legs["direct_warm_up"]["origin"]},
        "device": kmers._lib.device_name(dev),
    })
    out["speedup"] = round(out["text_total_s"] / out["direct_total_s"], 1) if out["direct_total_s"] > 0 else None
    da.close(); db.close()
finally:
    for p in paths + [text_path]:
        if os.path.exists(p):
            os.remove(p)
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
sys.exit(0 if out.get("same_keys") else 1)
