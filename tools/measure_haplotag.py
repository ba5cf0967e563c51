#!/usr/bin/env python3
"""Haplotag output measured: unaligned BAM records rewritten with their HP, ka and kb tags
  per shape  HiFi-like records of --read-len bases without kinetics, the same with kinetics (fi / ri B arrays), and short records
             (150 bases), each with an HP tag to lose, --mb megabytes of records per shape:
               write kernel   alone between HIP events, as GB/s of record bytes (tbk_bam_haplotag_bench_device);
               kernels        measure + scan + size home + write on the resident run, by the wall clock;
               device call    what the writer pays per batch with warm buffers: copy in, kernels, records home;
               host           tbk_bam_haplotag on TBK_HOST_THREADS threads (16 unless set), in the same process;
  cli        classify-by-kmers --haplotag-output on a generated uBAM of --cli-reads reads, beside --bam-output and the default
             gzip FASTQ bins, with the rewrite on the host's threads and (TBK_HAPLOTAG_REWRITE=gpu) on the device.
Medians of --reps runs after a warm-up.  One JSON line."""
import argparse, ctypes as C, json, os, statistics, struct, subprocess, sys, tempfile, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TBK_HOST_THREADS", "16")
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mb", type=int, default=96, help="megabytes of records per shape")
ap.add_argument("--read-len", type=int, default=15_000)
ap.add_argument("--cli-reads", type=int, default=40_000, help="reads of the file the command line classifies (0: skip)")
ap.add_argument("--kmers", type=int, default=2_000_000, help="k-mers per list for the command line")
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
rng = np.random.default_rng(19)
k = 21
CODE = np.array([1, 2, 4, 8], dtype=np.uint8)   # A C G T in BAM's 4-bit codes


def hifi_qual(n):
    qv = np.clip(rng.normal(60, 15, n), 2, 93).astype(np.uint8)
    qv[rng.random(n) < 0.6] = 93
    return qv


def tags(n, kinetics):
    out = b"zmi" + struct.pack("<i", 4711) + b"HPC\x01" + b"rqf" + struct.pack("<f", 0.9995) + b"npi" + struct.pack("<i", 12) + b"RGZ0a1b2c3d\0"
    if kinetics:
        for name in (b"fi", b"ri"):
            out += name + b"BC" + struct.pack("<i", n) + rng.integers(5, 60, n, dtype=np.uint8).tobytes()
    return out


def record(i, two_bit, qual, kinetics=False):
    n = len(two_bit)
    name = b"m64011_190830_220126/%d/ccs\0" % i
    c = CODE[two_bit]
    if n & 1:
        c = np.append(c, 0)
    body = name + ((c[0::2] << 4) | c[1::2]).astype(np.uint8).tobytes() + qual.tobytes() + tags(n, kinetics)
    fixed = struct.pack("<iiBBHHHIiii", -1, -1, len(name), 255, 4680, 0, 4, n, -1, -1, 0)
    return struct.pack("<I", 32 + len(body)) + fixed + body


def bgzf(data, block=0xFF00):
    out = bytearray()
    for at in range(0, len(data), block):
        piece = data[at:at + block]
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        body = co.compress(piece) + co.flush()
        out += struct.pack("<BBBBIBBHBBHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, len(body) + 25) + body + struct.pack("<II", zlib.crc32(piece), len(piece))
    return bytes(out) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


from trio_binning_amd._lib import check, lib

res = {"host_threads": int(lib.tbk_host_threads()), "shapes": {}}
for shape, (n_bases, kinetics) in {"hifi": (a.read_len, False), "hifi_kinetics": (a.read_len, True), "short_150": (150, False)}.items():
    recs, size = [], 0
    while size < a.mb << 20:
        recs.append(record(len(recs), rng.integers(0, 4, n_bases), hifi_qual(n_bases), kinetics))
        size += len(recs[-1])
    n = len(recs)
    offsets = np.cumsum([0] + [len(r) for r in recs[:-1]], dtype=np.uint64)
    run = b"".join(recs)
    del recs
    offs = offsets.ctypes.data_as(C.POINTER(C.c_uint64))
    bins = bytes(rng.choice(np.frombuffer(b"ABU", dtype=np.uint8), n))
    counts = rng.integers(0, 500, (n, 2), dtype=np.int32)
    cnt = counts.ctypes.data_as(C.POINTER(C.c_int32))
    out_len = C.c_uint64()
    whole, write, call = (C.c_double * a.reps)(), (C.c_double * a.reps)(), (C.c_double * a.reps)()
    check(lib.tbk_bam_haplotag_bench_device(0, run, len(run), offs, n, bins, cnt, a.reps, whole, write, call, C.byref(out_len)))
    cap = len(run) + 18 * n
    dst = C.create_string_buffer(cap)
    times = []
    for i in range(a.reps + 1):
        t = time.perf_counter()
        check(lib.tbk_bam_haplotag(run, len(run), offs, n, bins, cnt, dst, cap, None, C.byref(out_len)))
        times.append(time.perf_counter() - t)
    h, w, alone, c = statistics.median(times[1:]), statistics.median(whole), statistics.median(write), statistics.median(call)
    res["shapes"][shape] = {"records": n, "record_MB": round(len(run) / 1e6, 1), "tagged_MB": round(out_len.value / 1e6, 1),
                            "write_kernel_ms": round(alone * 1e3, 3), "write_kernel_GB_per_s": round(len(run) / alone / 1e9, 1),
                            "kernels_ms": round(w * 1e3, 3), "kernels_GB_per_s": round(len(run) / w / 1e9, 1),
                            "device_call_ms": round(c * 1e3, 2), "device_call_GB_per_s": round(len(run) / c / 1e9, 2),
                            "host_ms": round(h * 1e3, 2), "host_GB_per_s": round(len(run) / h / 1e9, 2), "device_call_over_host": round(c / h, 2)}
    del dst, run

if a.cli_reads:
    L = a.read_len
    tmp = tempfile.mkdtemp(prefix="tbk_haplotag_")
    keys = np.unique(rng.integers(0, 4**k, 2 * a.kmers + a.kmers // 20, dtype=np.uint64))
    rng.shuffle(keys)
    keys = keys[: 2 * a.kmers]
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    def decode(v):
        out = np.empty((v.size, k + 1), dtype=np.uint8)
        for i in range(k):
            out[:, i] = lut[((v >> np.uint64(2 * i)) & np.uint64(3)).astype(np.int64)]
        out[:, k] = 10
        return out
    la, lb = decode(keys[: a.kmers]), decode(keys[a.kmers:])
    fa, fb = os.path.join(tmp, "hapA.txt"), os.path.join(tmp, "hapB.txt")
    la.tofile(fa); lb.tofile(fb)
    inv = np.zeros(256, dtype=np.uint8)
    inv[lut] = np.arange(4, dtype=np.uint8)
    parts = [b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", 0)]
    for r in range(a.cli_reads):
        two = rng.integers(0, 4, L).astype(np.uint8)
        src = la if r % 2 == 0 else lb
        for j in range(20):  # plant 20 list k-mers per read
            p = j * (L // 20) + 5
            two[p:p + k] = inv[src[(r * 20 + j) % a.kmers, :k]]
        parts.append(record(r, two, hifi_qual(L)))
    path = os.path.join(tmp, "reads.hifi_reads.bam")
    open(path, "wb").write(bgzf(b"".join(parts)))
    del parts
    gbases = a.cli_reads * L / 1e9
    res["cli"] = {"reads": a.cli_reads, "gbases": gbases, "kmers_per_list": a.kmers, "file_MB": round(os.path.getsize(path) / 1e6, 1)}
    tagged = os.path.join(tmp, "tagged.bam")
    runs = [("haplotag_host_rewrite", ["--haplotag-output", tagged], {"TBK_HAPLOTAG_REWRITE": "cpu"}),
            ("haplotag_device_rewrite", ["--haplotag-output", tagged], {"TBK_HAPLOTAG_REWRITE": "gpu"}), ("bam_output", ["--bam-output"], {}), ("gzip_fastq", [], {})]
    walls = {name: [] for name, _, _ in runs}
    tsv = {}
    for i in range(a.reps + 1):   # the modes take turns
        for name, extra, more in runs:
            out = os.path.join(tmp, "%s%d" % (name, i)); os.makedirs(out)
            t = time.time()
            p = subprocess.run([sys.executable, "-m", "trio_binning_amd.classify_by_kmers", path, fa, fb, "--haplotype-a-out-prefix", os.path.join(out, "hapA"),
                                "--haplotype-b-out-prefix", os.path.join(out, "hapB"), "--unclassified-out-prefix", os.path.join(out, "unc")] + extra,
                               env=dict(os.environ, PYTHONPATH=ROOT, **more), capture_output=True)
            walls[name].append(time.time() - t)
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            tsv[name] = p.stdout
            sizes = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) + (os.path.getsize(tagged) if extra[:1] == ["--haplotag-output"] else 0)
            for f in os.listdir(out):
                os.remove(os.path.join(out, f))
            res["cli"].setdefault(name, {})["output_MB"] = round(sizes / 1e6, 1)
    for name, _, _ in runs:
        m = statistics.median(walls[name][1:])
        res["cli"][name].update({"wall_s": round(m, 2), "gbases_per_s": round(gbases / m, 3), "walls": [round(x, 2) for x in walls[name]]})
    res["cli"]["same_tsv"] = len(set(tsv.values())) == 1
print(json.dumps(res))
