#!/usr/bin/env python3
"""BAM input measured (profiles/r17/): one window of 15 kb HiFi-like reads as unaligned BAM records
  kernels   the transcode kernels on the resident window (tbk_bam_bench_device: the write kernel alone between HIP events,
            and measure + scan + size home + write by the wall clock) beside tbk_calib_stream in the same process;
  host      tbk_bam_fastq (csrc/tbk_bam.h on TBK_HOST_THREADS threads, 16 unless set) on the same window;
  cli       classify-by-kmers from the reads as BAM and from the same reads as bgzf FASTQ, with --no-gzip-output.
Medians of three runs after a warm-up.  One JSON line."""
import argparse, ctypes as C, json, os, statistics, struct, subprocess, sys, tempfile, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TBK_HOST_THREADS", "16")
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=4000, help="reads of the resident window")
ap.add_argument("--read-len", type=int, default=15_000)
ap.add_argument("--cli-reads", type=int, default=8000, help="reads of the files the command line classifies (0: skip)")
ap.add_argument("--kmers", type=int, default=2_000_000, help="k-mers per list for the command line")
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
rng = np.random.default_rng(17)
L, k = a.read_len, 21
CODE = np.array([1, 2, 4, 8], dtype=np.uint8)   # A C G T in BAM's 4-bit codes
TAGS = b"rqf" + struct.pack("<f", 0.9995) + b"npi" + struct.pack("<i", 12)


def hifi_qual(n):
    qv = np.clip(rng.normal(60, 15, n), 2, 93).astype(np.uint8)
    qv[rng.random(n) < 0.6] = 93
    return qv


def record(i, two_bit, qual):
    name = b"m64011_190830_220126/%d/ccs\0" % i
    c = CODE[two_bit]
    if L & 1:
        c = np.append(c, 0)
    body = name + ((c[0::2] << 4) | c[1::2]).astype(np.uint8).tobytes() + qual.tobytes() + TAGS
    fixed = struct.pack("<iiBBHHHIiii", -1, -1, len(name), 255, 4680, 0, 4, L, -1, -1, 0)
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

res = {"reads": a.reads, "read_len": L, "host_threads": int(lib.tbk_host_threads())}
recs = [record(i, rng.integers(0, 4, L), hifi_qual(L)) for i in range(a.reads)]
offsets = np.cumsum([0] + [len(r) for r in recs[:-1]], dtype=np.uint64)
window = b"".join(recs)
offs = offsets.ctypes.data_as(C.POINTER(C.c_uint64))
text_len = C.c_uint64()

# the kernels
whole, write = (C.c_double * a.reps)(), (C.c_double * a.reps)()
check(lib.tbk_bam_bench_device(0, window, len(window), offs, a.reads, 0x900, a.reps, whole, write, C.byref(text_len)))
stream = C.c_double()
check(lib.tbk_calib_stream(0, 1 << 30, 20, C.byref(stream)))
moved = len(window) + text_len.value   # (bytes read + bytes written; tags are read by nobody, but they lie in the lines that are)
w, alone = statistics.median(whole), statistics.median(write)
res["kernels"] = {"window_MB": round(len(window) / 1e6, 1), "text_MB": round(text_len.value / 1e6, 1), "write_kernel_ms": round(alone * 1e3, 3),
                  "write_kernel_GB_per_s": round(moved / alone / 1e9, 1), "whole_ms": round(w * 1e3, 3), "whole_GB_per_s": round(moved / w / 1e9, 1),
                  "gbases_per_s_whole": round(a.reads * L / w / 1e9, 1), "calib_stream_GB_per_s": round(stream.value / 1e9, 1),
                  "write_kernel_fraction_of_stream": round(moved / alone / stream.value, 3), "whole_fraction_of_stream": round(moved / w / stream.value, 3)}

# the host's transcoder on the same window
dst = C.create_string_buffer(text_len.value)
n_w, n_s = C.c_uint64(), C.c_uint64()
times = []
for i in range(a.reps + 1):
    t = time.perf_counter()
    check(lib.tbk_bam_fastq(window, len(window), offs, a.reads, 0x900, dst, text_len.value, C.byref(text_len), C.byref(n_w), C.byref(n_s)))
    times.append(time.perf_counter() - t)
h = statistics.median(times[1:])
res["host"] = {"ms": round(h * 1e3, 1), "GB_per_s": round(moved / h / 1e9, 2), "gbases_per_s": round(a.reads * L / h / 1e9, 2)}
del dst

# the command line: BAM against the same reads as bgzf FASTQ
if a.cli_reads:
    tmp = tempfile.mkdtemp(prefix="tbk_bam_")
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
    bam_parts, fq_parts = [b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", 0)], []
    for r in range(a.cli_reads):
        two = rng.integers(0, 4, L).astype(np.uint8)
        src = la if r % 2 == 0 else lb
        for j in range(20):  # plant 20 list k-mers per read
            p = j * (L // 20) + 5
            two[p:p + k] = inv[src[(r * 20 + j) % a.kmers, :k]]
        q = hifi_qual(L)
        bam_parts.append(record(r, two, q))
        fq_parts.append(b"@m64011_190830_220126/%d/ccs\n" % r + lut[two].tobytes() + b"\n+\n" + (q + 33).astype(np.uint8).tobytes() + b"\n")
    files = {"bam": os.path.join(tmp, "reads.hifi_reads.bam"), "bgzf_fastq": os.path.join(tmp, "reads.fastq.gz")}
    open(files["bam"], "wb").write(bgzf(b"".join(bam_parts)))
    open(files["bgzf_fastq"], "wb").write(bgzf(b"".join(fq_parts)))
    del bam_parts, fq_parts
    gbases = a.cli_reads * L / 1e9
    res["cli"] = {"reads": a.cli_reads, "gbases": gbases, "kmers_per_list": a.kmers}
    env = dict(os.environ, PYTHONPATH=ROOT, TBK_STATS="1")
    tsv = {}
    for name, path in files.items():
        walls = []
        for i in range(a.reps + 1):
            out = os.path.join(tmp, "%s%d" % (name, i)); os.makedirs(out)
            t = time.time()
            p = subprocess.run([sys.executable, "-m", "trio_binning_amd.classify_by_kmers", path, fa, fb, "--no-gzip-output",
                                "--haplotype-a-out-prefix", os.path.join(out, "hapA"), "--haplotype-b-out-prefix", os.path.join(out, "hapB"),
                                "--unclassified-out-prefix", os.path.join(out, "unc")], env=env, capture_output=True)
            walls.append(time.time() - t)
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            tsv[name] = p.stdout
            st = [l for l in p.stderr.decode().splitlines() if l.startswith("tbk-stats ")]
            for f in os.listdir(out):
                os.remove(os.path.join(out, f))
        m = statistics.median(walls[1:])
        res["cli"][name] = {"file_MB": round(os.path.getsize(path) / 1e6, 1), "wall_s": round(m, 2), "gbases_per_s": round(gbases / m, 3), "walls": [round(x, 2) for x in walls],
                            "stages": json.loads(st[-1][10:]) if st else None}
    res["cli"]["same_tsv"] = tsv["bam"] == tsv["bgzf_fastq"]
    res["cli"]["bam_over_bgzf_fastq"] = round(res["cli"]["bam"]["gbases_per_s"] / res["cli"]["bgzf_fastq"]["gbases_per_s"], 3)
print(json.dumps(res))
