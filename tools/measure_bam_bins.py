#!/usr/bin/env python3
"""BAM bins measured (DESIGN section 9 addendum, profiles/r18/): tools/measure_bam.py's synthetic HiFi-like records, once as they
are ("plain": rq and np tags) and once with kinetics-sized B tags ("kinetics": fi, ri, fp, rp of one byte a base)
  size      bytes out over bytes in of the bgzf coder with the writer's four hints per record and with fixed cuts (host twin: the
            same cuts as the device), and of zlib at levels 1 and 6 in blocks of 65280 bytes on the same bytes;
  host      tbk_bgzf_members on 16 threads;
  kernels   the bgzf mode of csrc/tbk_gdeflate.hip (tbk_bgzf_members_bench_device: one job's kernels between HIP events, and the wall
            time per job through the three-deep ring, link included) beside tbk_calib_stream in the same process;
  cli       classify-by-kmers from a BAM of --cli-reads reads three ways - --bam-output, the default gzip FASTQ bins,
            --no-gzip-output - and, with --parent DIR (a built checkout of the parent commit), the latter two by the parent too.
Medians of --reps runs after a warm-up.  One JSON line.  --no-device: size and host only."""
import argparse, ctypes as C, json, os, statistics, struct, subprocess, sys, tempfile, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TBK_HOST_THREADS", "16")
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1500, help="reads of the encoder's window")
ap.add_argument("--read-len", type=int, default=15_000)
ap.add_argument("--cli-reads", type=int, default=40_000, help="reads of the file the command line classifies (0: skip)")
ap.add_argument("--kmers", type=int, default=2_000_000, help="k-mers per list for the command line")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its command line runs the FASTQ-bin modes too")
ap.add_argument("--no-device", action="store_true")
a = ap.parse_args()
rng = np.random.default_rng(17)
L, k = a.read_len, 21
CODE = np.array([1, 2, 4, 8], dtype=np.uint8)   # A C G T in BAM's 4-bit codes
TAGS = b"rqf" + struct.pack("<f", 0.9995) + b"npi" + struct.pack("<i", 12)
PAYLOAD = 65280


def hifi_qual(n):
    qv = np.clip(rng.normal(60, 15, n), 2, 93).astype(np.uint8)
    qv[rng.random(n) < 0.6] = 93
    return qv


def kinetics_tags(n):
    """fi / ri / fp / rp as HiFi kinetics are stored: B,C arrays of one codec byte a base (inter-pulse durations and pulse widths, skewed low)"""
    out = b""
    for tag, mean in ((b"fi", 18), (b"ri", 18), (b"fp", 11), (b"rp", 11)):
        v = np.clip(rng.gamma(2.0, mean / 2.0, n), 0, 255).astype(np.uint8)
        out += tag + b"BC" + struct.pack("<i", n) + v.tobytes()
    return out


def record(i, two_bit, qual, tags=TAGS):
    name = b"m64011_190830_220126/%d/ccs\0" % i
    c = CODE[two_bit]
    if L & 1:
        c = np.append(c, 0)
    body = name + ((c[0::2] << 4) | c[1::2]).astype(np.uint8).tobytes() + qual.tobytes() + tags
    fixed = struct.pack("<iiBBHHHIiii", -1, -1, len(name), 255, 4680, 0, 4, L, -1, -1, 0)
    return struct.pack("<I", 32 + len(body)) + fixed + body


def hints_of(recs):
    """the writer's four per record: start of seq, of qual, of the tags, the record's end"""
    out, at = [], 0
    for r in recs:
        seq_at = 36 + r[12]
        out += [at + seq_at, at + seq_at + (L + 1) // 2, at + seq_at + (L + 1) // 2 + L, at + len(r)]
        at += len(r)
    return out


def zlib_bgzf_size(data, level):
    n = 0
    for at in range(0, len(data), PAYLOAD):
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        n += len(co.compress(data[at:at + PAYLOAD])) + len(co.flush()) + 26
    return n


from trio_binning_amd._lib import check, lib

lib.tbk_calib_stream.restype = C.c_int
res = {"reads": a.reads, "read_len": L, "host_threads": 16}
stream = C.c_double()
if not a.no_device:
    check(lib.tbk_calib_stream(0, 1 << 30, 20, C.byref(stream)))
    res["calib_stream_GB_per_s"] = round(stream.value / 1e9, 1)
for shape in ("plain", "kinetics"):
    recs = [record(i, rng.integers(0, 4, L), hifi_qual(L), TAGS + (kinetics_tags(L) if shape == "kinetics" else b"")) for i in range(a.reads)]
    data = b"".join(recs)
    hints = hints_of(recs)
    del recs
    h = (C.c_uint64 * len(hints))(*hints)
    cap = len(data) + 128 * (len(data) // PAYLOAD + 1)
    buf = C.create_string_buffer(cap)
    need, nm = C.c_uint64(), C.c_uint64()
    out = {"MB_in": round(len(data) / 1e6, 1)}
    times = []
    for i in range(a.reps + 1):
        t = time.perf_counter()
        check(lib.tbk_bgzf_members_threads_(data, len(data), h, len(hints), buf, cap, C.byref(need), C.byref(nm), 16))
        times.append(time.perf_counter() - t)
    hinted = need.value
    check(lib.tbk_bgzf_members_threads_(data, len(data), None, 0, buf, cap, C.byref(need), C.byref(nm), 16))
    fixed = need.value
    t = statistics.median(times[1:])
    out["size"] = {"hinted_over_in": round(hinted / len(data), 4), "fixed_cuts_over_in": round(fixed / len(data), 4), "hinted_over_fixed": round(hinted / fixed, 4),
                   "zlib1_over_in": round(zlib_bgzf_size(data, 1) / len(data), 4), "zlib6_over_in": round(zlib_bgzf_size(data, 6) / len(data), 4), "members": nm.value}
    out["host_16_threads"] = {"ms": round(t * 1e3, 1), "GB_per_s_in": round(len(data) / t / 1e9, 2)}
    if not a.no_device:
        lib.tbk_host_alloc.restype = C.c_void_p
        pinned = lib.tbk_host_alloc(len(data))
        assert pinned
        C.memmove(pinned, data, len(data))
        pipelined, kernels, made = C.c_double(), C.c_double(), C.c_uint64()
        ring, alone = [], []
        for i in range(a.reps):
            check(lib.tbk_bgzf_members_bench_device(0, pinned, len(data), h, len(hints), 8, C.byref(pipelined), C.byref(kernels), C.byref(made)))
            ring.append(pipelined.value); alone.append(kernels.value)
        dev_hinted = made.value
        check(lib.tbk_bgzf_members_bench_device(0, pinned, len(data), None, 0, 4, C.byref(pipelined), C.byref(kernels), C.byref(made)))
        lib.tbk_host_free(C.c_void_p(pinned))
        kt, rt = statistics.median(alone), statistics.median(ring)
        out["device"] = {"kernels_ms": round(kt * 1e3, 3), "kernels_GB_per_s_in": round(len(data) / kt / 1e9, 1), "kernels_fraction_of_stream": round(len(data) / kt / stream.value, 4),
                         "ring_ms_per_job": round(rt * 1e3, 3), "ring_GB_per_s_in": round(len(data) / rt / 1e9, 2), "hinted_over_in": round(dev_hinted / len(data), 4),
                         "fixed_cuts_over_in": round(made.value / len(data), 4), "fixed_kernels_ms": round(kernels.value * 1e3, 3)}
    res[shape] = out
    del data, buf

# the command line: BAM bins, gzip FASTQ bins, plain FASTQ bins - and the parent's FASTQ bins
if a.cli_reads and not a.no_device:
    tmp = tempfile.mkdtemp(prefix="tbk_bam_bins_")
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
    path = os.path.join(tmp, "reads.hifi_reads.bam")
    with open(path, "wb") as fh:
        pending = bytearray(b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", 0))
        def drain(everything):
            while len(pending) >= PAYLOAD or (everything and pending):
                piece = bytes(pending[:PAYLOAD]); del pending[:PAYLOAD]
                co = zlib.compressobj(1, zlib.DEFLATED, -15)
                body = co.compress(piece) + co.flush()
                fh.write(struct.pack("<BBBBIBBHBBHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, len(body) + 25) + body + struct.pack("<II", zlib.crc32(piece), len(piece)))
        for r in range(a.cli_reads):
            two = rng.integers(0, 4, L).astype(np.uint8)
            src = la if r % 2 == 0 else lb
            for j in range(20):  # plant 20 list k-mers per read
                p = j * (L // 20) + 5
                two[p:p + k] = inv[src[(r * 20 + j) % a.kmers, :k]]
            pending += record(r, two, hifi_qual(L))
            drain(False)
        drain(True)
        fh.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    gbases = a.cli_reads * L / 1e9
    res["cli"] = {"reads": a.cli_reads, "gbases": gbases, "kmers_per_list": a.kmers, "file_MB": round(os.path.getsize(path) / 1e6, 1)}
    runs = [("bam_output", ROOT, ["--bam-output"]), ("gzip_fastq", ROOT, []), ("plain_fastq", ROOT, ["--no-gzip-output"])]
    if a.parent:
        runs += [("parent_gzip_fastq", a.parent, []), ("parent_plain_fastq", a.parent, ["--no-gzip-output"])]
    # the modes take turns, round after round, so that none of them has the warm file cache or the settled clocks to itself
    tsv, walls, stages, sizes = {}, {name: [] for name, _, _ in runs}, {}, {}
    for i in range(a.reps + 1):
        for name, root, extra in runs:
            env = dict(os.environ, PYTHONPATH=root, TBK_STATS="1")
            out = os.path.join(tmp, "%s%d" % (name, i)); os.makedirs(out)
            t = time.time()
            p = subprocess.run([sys.executable, "-m", "trio_binning_amd.classify_by_kmers", path, fa, fb, "--haplotype-a-out-prefix", os.path.join(out, "hapA"),
                                "--haplotype-b-out-prefix", os.path.join(out, "hapB"), "--unclassified-out-prefix", os.path.join(out, "unc")] + extra,
                               env=env, capture_output=True, cwd=root)
            walls[name].append(time.time() - t)
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            tsv[name] = p.stdout
            st = [l for l in p.stderr.decode().splitlines() if l.startswith("tbk-stats ")]
            stages[name] = json.loads(st[-1][10:]) if st else None
            sizes[name] = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
            for f in os.listdir(out):
                os.remove(os.path.join(out, f))
    for name, _, _ in runs:
        m = statistics.median(walls[name][1:])
        res["cli"][name] = {"wall_s": round(m, 3), "gbases_per_s": round(gbases / m, 3), "walls": [round(x, 2) for x in walls[name]], "bins_MB": round(sizes[name] / 1e6, 1),
                            "stages": stages[name]}
    res["cli"]["same_tsv"] = len(set(tsv.values())) == 1
    if a.parent:
        for mode in ("gzip_fastq", "plain_fastq"):
            res["cli"][mode + "_over_parent"] = round(res["cli"][mode]["wall_s"] / res["cli"]["parent_" + mode]["wall_s"], 3)
print(json.dumps(res))
