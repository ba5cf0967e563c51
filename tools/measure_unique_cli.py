#!/usr/bin/env python3
"""End-to-end timing of the find-unique-kmers CLI on synthetic parents (two haplotypes of one random
genome, short reads with errors written as FASTQ), then of classify-by-kmers on long reads of both
haplotypes with the lists it made: the whole pipeline on files."""
import argparse, json, os, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--genome", type=int, default=20_000_000)
ap.add_argument("--coverage", type=float, default=30.0)
ap.add_argument("--read-len", type=int, default=150)
ap.add_argument("--split", type=int, default=1, help="files per parent library")
ap.add_argument("--gzip", action="store_true", help="gzip the parents' FASTQ files")
ap.add_argument("--passes", type=int, default=0, help="find-unique-kmers --passes (0: it chooses)")
ap.add_argument("--from-databases", action="store_true",
                help="also: a --keep-databases run, a re-dump from the two *.tbkdb files at the first run's cut-offs, and the seconds "
                     "of export, save, load and unique on their own; the legs alternate --repeat times")
ap.add_argument("--tree", default="", help="with --from-databases: a checkout of the parent commit (built) whose full counting run is timed beside the re-dump")
ap.add_argument("--repeat", type=int, default=3)
a = ap.parse_args()
k = 21
rng = np.random.default_rng(5)
lut = np.frombuffer(b"ACGT", dtype=np.uint8)
base = rng.integers(0, 4, a.genome, dtype=np.uint8)
def mutate():
    h = base.copy(); pos = np.nonzero(rng.random(a.genome) < 1 / 500)[0]
    h[pos] = (h[pos] + rng.integers(1, 4, pos.size)) % 4
    return h
haps = [mutate(), mutate()]
tmp = tempfile.mkdtemp(prefix="tbk_unique_")
import gzip as _gzip
def write_fastq(path, codes2d, prefix):
    n, L = codes2d.shape
    text = lut[codes2d]
    qual = b"I" * L
    with (_gzip.open(path, "wb", compresslevel=1) if path.endswith(".gz") else open(path, "wb")) as fh:
        for i in range(n):
            fh.write(b"@%s%d\n" % (prefix, i)); fh.write(text[i].tobytes()); fh.write(b"\n+\n"); fh.write(qual); fh.write(b"\n")
files = []
n_reads = int(a.genome * a.coverage / a.read_len)
for h, name in zip(haps, ("mother", "father")):
    starts = rng.integers(0, a.genome - a.read_len, n_reads)
    reads = h[starts[:, None] + np.arange(a.read_len)[None, :]]
    err = rng.random(reads.shape) < 0.003
    reads[err] = (reads[err] + rng.integers(1, 4, int(err.sum()))) % 4
    parts = []
    for j in range(a.split):
        path = os.path.join(tmp, "%s_%d.fastq%s" % (name, j, ".gz" if a.gzip else ""))
        write_fastq(path, reads[j * n_reads // a.split:(j + 1) * n_reads // a.split], name.encode()); parts.append(path)
    files.append(",".join(parts))
    del reads
env = dict(os.environ, PYTHONPATH=ROOT)
t = time.time()
p = subprocess.run([sys.executable, "-m", "trio_binning_amd.find_unique_kmers", "-k", str(k), "-o", tmp, "-s", tmp, "--passes", str(a.passes), files[0], files[1]], env=env, capture_output=True)
t_unique = time.time() - t
assert p.returncode == 0, p.stderr.decode()[-2000:]
err = p.stderr.decode()
lists = [os.path.join(tmp, "hapA_only_kmers.txt"), os.path.join(tmp, "hapB_only_kmers.txt")]
n_list = [os.path.getsize(f) // (k + 1) for f in lists]
# offspring long reads: one haplotype each
L, n_long = 15000, 2000
starts = rng.integers(0, a.genome - L, n_long)
long_reads = np.stack([haps[i % 2][s:s + L] for i, s in enumerate(starts)])
fq = os.path.join(tmp, "child.fastq"); write_fastq(fq, long_reads, b"child")
t = time.time()
p2 = subprocess.run([sys.executable, "-m", "trio_binning_amd.classify_by_kmers", fq, lists[0], lists[1], "--no-gzip-output",
                     "--haplotype-a-out-prefix", os.path.join(tmp, "A"), "--haplotype-b-out-prefix", os.path.join(tmp, "B"),
                     "--unclassified-out-prefix", os.path.join(tmp, "U")], env=env, capture_output=True)
t_classify = time.time() - t
assert p2.returncode == 0, p2.stderr.decode()[-2000:]
bins = [l.split("\t")[1] for l in p2.stdout.decode().splitlines()]
right = sum(1 for i, b in enumerate(bins) if b == "AB"[i % 2])
print(json.dumps({"genome": a.genome, "parent_reads": n_reads, "parent_gbases_each": round(n_reads * a.read_len / 1e9, 3),
                  "files_per_parent": a.split, "passes": a.passes, "gzip": a.gzip, "file_GB_each_parent": round(sum(os.path.getsize(f) for f in files[0].split(",")) / 1e9, 2), "find_unique_s": round(t_unique, 2),
                  "cutoffs": [l for l in err.splitlines() if "Using counts" in l], "list_sizes": n_list,
                  "classify_s": round(t_classify, 2), "child_reads": n_long, "binned_to_the_right_parent": right}))
if a.from_databases:
    import re, shutil
    cut = [int(x) for l in err.splitlines() if "Using counts" in l for x in re.findall(r"\d+", l.split("range")[1])]
    assert len(cut) == 4, err
    want = [open(f, "rb").read() for f in lists]
    def cli(tree, out, extra, parents):
        os.makedirs(out, exist_ok=True)
        t = time.time()
        q = subprocess.run([sys.executable, "-m", "trio_binning_amd.find_unique_kmers", "-k", str(k), "-o", out, "-s", out] + extra + parents,
                           env=dict(os.environ, PYTHONPATH=tree), capture_output=True)
        dt = time.time() - t
        assert q.returncode == 0, q.stderr.decode()[-2000:]
        got = [open(os.path.join(out, n), "rb").read() for n in ("hapA_only_kmers.txt", "hapB_only_kmers.txt")]
        assert got == want, "the lists differ from the first run's"
        return round(dt, 2)
    keep = os.path.join(tmp, "keep")
    dbs = [os.path.join(keep, "haplotypeA.tbkdb"), os.path.join(keep, "haplotypeB.tbkdb")]
    cuts = ["--min-count-a", str(cut[0]), "--max-count-a", str(cut[1]), "--min-count-b", str(cut[2]), "--max-count-b", str(cut[3])]
    legs = {"plain_s": [], "keep_databases_s": [], "redump_from_files_s": [], "parent_commit_plain_s": []}
    for _ in range(a.repeat):  # the legs alternate
        if a.tree:
            legs["parent_commit_plain_s"].append(cli(a.tree, os.path.join(tmp, "parent"), ["--passes", str(a.passes)], files))
        legs["plain_s"].append(cli(ROOT, os.path.join(tmp, "plain"), ["--passes", str(a.passes)], files))
        legs["keep_databases_s"].append(cli(ROOT, keep, ["--passes", str(a.passes), "--keep-databases"], files))
        legs["redump_from_files_s"].append(cli(ROOT, os.path.join(tmp, "redump"), cuts, dbs))
    # the four steps on their own, in this process
    sys.path.insert(0, ROOT)
    from trio_binning_amd import find_unique_kmers as fu, kmers
    steps = {"export_s": [], "save_s": [], "load_s": [], "unique_s": []}
    n_kept = []
    for files_string, hap in zip(files, "AB"):
        paths = files_string.split(",")
        counter = fu.count_library(paths, k, fu.estimate_capacity(paths), 1)
        t = time.time(); db = counter.database(); steps["export_s"].append(round(time.time() - t, 3))
        counter.close()
        path = os.path.join(tmp, "step%s.tbkdb" % hap)
        t = time.time(); db.save(path); steps["save_s"].append(round(time.time() - t, 3))
        n_kept.append(len(db)); db.close()
    loaded = []
    for hap in "AB":
        t = time.time(); loaded.append(kmers.KmerDatabase.load(os.path.join(tmp, "step%s.tbkdb" % hap))); steps["load_s"].append(round(time.time() - t, 3))
    for x, y, lo, hi in ((0, 1, cut[0], cut[1]), (1, 0, cut[2], cut[3])):
        t = time.time(); loaded[x].unique(loaded[y], lo, hi, os.path.join(tmp, "step.txt")); steps["unique_s"].append(round(time.time() - t, 3))
    for d in loaded: d.close()
    sizes = [os.path.getsize(os.path.join(tmp, "step%s.tbkdb" % hap)) for hap in "AB"]
    print(json.dumps({"from_databases": True, "legs": legs, "steps_per_parent": steps, "kept_kmers": n_kept, "file_bytes": sizes,
                      "file_bytes_per_kept_kmer": [round(sz / max(1, n), 4) for sz, n in zip(sizes, n_kept)]}))
    for d in ("keep", "plain", "redump", "parent"):
        shutil.rmtree(os.path.join(tmp, d), ignore_errors=True)
for f in os.listdir(tmp): os.remove(os.path.join(tmp, f))
os.rmdir(tmp)
