"""End-to-end CLI on the reference's toy inputs (BASELINE.json configs[0] inputs, run on
the GPU path): stdout TSV and decompressed bins must equal what the real reference
produced (tests/golden/toy_cli.json, diff_vectors.json)."""
import gzip
import hashlib
import io
import os
from unittest.mock import patch

import pytest

from conftest import DATA, load_golden

pytestmark = pytest.mark.gpu


def _run(argv, capsys):
    from trio_binning_amd.classify_by_kmers import main

    with patch("sys.argv", ["classify-by-kmers"] + argv):
        main()
    out, _ = capsys.readouterr()
    return out


@pytest.mark.parametrize("reads_name", ["test.ccs.fastq.gz", "test.fa", "test.fastq"])
def test_toy_cli_gzip_mode(gpu, capsys, tmp_path, reads_name):
    g = load_golden("toy_cli.json")[reads_name]
    pa, pb, pu = (str(tmp_path / x) for x in ("hapA", "hapB", "unclassified"))
    out = _run([os.path.join(DATA, reads_name), os.path.join(DATA, "hapA.txt"), os.path.join(DATA, "hapB.txt"),
                "--haplotype-a-out-prefix", pa, "--haplotype-b-out-prefix", pb, "--unclassified-out-prefix", pu], capsys)
    assert out == g["stdout"]
    assert sorted(os.listdir(tmp_path)) == sorted(g["files"])
    for fn, meta in g["files"].items():
        body = gzip.open(os.path.join(tmp_path, fn), "rb").read()
        assert len(body) == meta["size"], fn
        assert hashlib.sha256(body).hexdigest() == meta["sha256"], fn
        if "text" in meta:
            assert body.decode() == meta["text"]


def test_reference_cli_test_shape(gpu, capsys, tmp_path):
    """The reference's own CLI test (tests/test_classify_by_kmers.py:19-57) with the
    --no-gzip-output defect fixed: the hapA file holds exactly the A read."""
    from trio_binning_amd.seq import readfq

    pa, pb, pu = (str(tmp_path / x) for x in ("hapA", "hapB", "hapU"))
    out = _run([os.path.join(DATA, "test.ccs.fastq.gz"), os.path.join(DATA, "hapA.txt"), os.path.join(DATA, "hapB.txt"),
                "--haplotype-a-out-prefix", pa, "--haplotype-b-out-prefix", pb, "--unclassified-out-prefix", pu,
                "--no-gzip-output"], capsys)
    assert out == load_golden("toy_cli.json")["test.ccs.fastq.gz"]["stdout"]
    names = {fn: [r.name for r in readfq(open(os.path.join(tmp_path, fn)))] for fn in sorted(os.listdir(tmp_path))}
    assert names == {"hapA.fastq": ["m64234e_220609_193909/2/ccs"], "hapB.fastq": ["m64234e_220609_193909/3/ccs"],
                     "hapU.fastq": ["m64234e_220609_193909/6/ccs"]}
    # each bin equals the corresponding gzip-mode bin of the reference
    g = load_golden("toy_cli.json")["test.ccs.fastq.gz"]["files"]
    for ours, theirs in (("hapA.fastq", "hapA.fastq.gz"), ("hapB.fastq", "hapB.fastq.gz"), ("hapU.fastq", "unclassified.fastq.gz")):
        assert hashlib.sha256(open(os.path.join(tmp_path, ours), "rb").read()).hexdigest() == g[theirs]["sha256"]


@pytest.mark.parametrize("k", [21, 32])
def test_differential_cli(gpu, capsys, tmp_path, k):
    """150 reads with planted hits through the CLI: TSV text and the three bins equal the
    real reference's (recorded in diff_vectors.json)."""
    v = next(x for x in load_golden("diff_vectors.json") if x["k"] == k)
    fa, fb, fq = tmp_path / "la.txt", tmp_path / "lb.txt", tmp_path / f"reads{k}.fa"
    fa.write_text("".join(x + "\n" for x in v["list_a"]))
    fb.write_text("".join(x + "\n" for x in v["list_b"]))
    with open(fq, "w") as fh:
        for i, s in enumerate(v["reads"]):
            fh.write(f">r{i} some comment\n{s}\n")
    od = tmp_path / "out"
    od.mkdir()
    out = _run([str(fq), str(fa), str(fb), "--haplotype-a-out-prefix", str(od / "hapA"),
                "--haplotype-b-out-prefix", str(od / "hapB"), "--unclassified-out-prefix", str(od / "unclassified")], capsys)
    assert out == v["cli_stdout"]
    assert sorted(os.listdir(od)) == sorted(v["cli_bins"])
    for fn, digest in v["cli_bins"].items():
        assert hashlib.sha256(gzip.open(od / fn, "rb").read()).hexdigest() == digest, fn


@pytest.mark.parametrize("k,wide", [(21, 0), (21, 1), (32, 1), (21, 2)])
def test_differential_cli_through_the_entry_layouts(gpu, capsys, tmp_path, monkeypatch, k, wide):
    """The same recorded reference output with the table in entry layout (narrow entries, and the 16-byte ones k = 32
    needs) and in short keys (wide = 2): the native loop, its packed batches and short reads' multi-read passes over
    tbk_probe_entry_kernel."""
    import trio_binning_amd.classify_by_kmers as cbk

    monkeypatch.setenv("TBK_SHORT" if wide == 2 else "TBK_ENTRY", "1")
    if wide == 1:
        monkeypatch.setenv("TBK_ENTRY_WIDE", "1")
    monkeypatch.setattr(cbk, "_BATCH_BASES", 2000)
    monkeypatch.setattr(cbk, "_BATCH_READS", 40)
    test_differential_cli(gpu, capsys, tmp_path, k)


def test_stats_line_goes_to_stderr_only(gpu, capsys, tmp_path, monkeypatch):
    import json

    monkeypatch.setenv("TBK_STATS", "1")
    g = load_golden("toy_cli.json")["test.fastq"]
    from trio_binning_amd.classify_by_kmers import main

    with patch("sys.argv", ["classify-by-kmers", os.path.join(DATA, "test.fastq"), os.path.join(DATA, "hapA.txt"),
                            os.path.join(DATA, "hapB.txt"), "--haplotype-a-out-prefix", str(tmp_path / "a"),
                            "--haplotype-b-out-prefix", str(tmp_path / "b"), "--unclassified-out-prefix", str(tmp_path / "u")]):
        main()
    out, err = capsys.readouterr()
    assert out == g["stdout"]
    line = [l for l in err.splitlines() if l.startswith("tbk-stats ")][-1]
    st = json.loads(line[len("tbk-stats "):])
    assert st["reads"] == 4 and st["bases"] == 220 and st["batches"] == 1


def test_small_batches_keep_input_order(gpu, capsys, tmp_path, monkeypatch):
    """Force many tiny batches through the streaming ring: outputs identical."""
    import trio_binning_amd.classify_by_kmers as cbk

    monkeypatch.setattr(cbk, "_BATCH_BASES", 300)
    monkeypatch.setattr(cbk, "_BATCH_READS", 7)
    test_differential_cli(gpu, capsys, tmp_path, 21)


def test_synthetic_prefix_through_the_file_path(gpu, capsys, tmp_path):
    """a prefix of the synthetic bench workload goes through files — text k-mer lists,
    a FASTQ of GPU-generated reads — and the CLI must report exactly the counts that the
    device-resident path (bench.py's path) gets on the same bytes."""
    import ctypes as C

    import numpy as np

    from trio_binning_amd import kmers
    from trio_binning_amd._lib import check, lib

    dev, k, n_list, R, L = 0, 21, 20000, 256, 3000

    def dalloc(n):
        p = C.c_void_p()
        check(lib.tbk_device_alloc(dev, n, C.byref(p)))
        return p.value

    d_keys = dalloc(2 * n_list * 8)
    check(lib.tbk_synth_keys_device(dev, 0x5EED0001, 0, 2 * n_list, k, C.c_void_p(d_keys)))
    h_keys = np.empty(2 * n_list, dtype=np.uint64)
    check(lib.tbk_memcpy_d2h(dev, h_keys.ctypes.data, C.c_void_p(d_keys), h_keys.nbytes))
    a = kmers.HashSet.from_device_keys(d_keys, n_list, k)
    b = kmers.HashSet.from_device_keys(d_keys + n_list * 8, n_list, k)
    total = R * L
    d_bases, d_offs, d_counts = dalloc(total + 32), dalloc((R + 1) * 8), dalloc(R * 8)
    check(lib.tbk_synth_reads_device(dev, 0x5EED0002, 0, R, L, 0x5EED0001, n_list, n_list, k, 30, 3, C.c_void_p(d_bases), C.c_void_p(d_offs)))
    with kmers.Classifier(a, b) as cls:
        cls.classify_device(d_bases, d_offs, R, total, d_counts)
        cls.sync()
    counts = np.zeros((R, 2), dtype=np.int32)
    check(lib.tbk_memcpy_d2h(dev, counts.ctypes.data, C.c_void_p(d_counts), counts.nbytes))
    bases = np.empty(total, dtype=np.uint8)
    check(lib.tbk_memcpy_d2h(dev, bases.ctypes.data, C.c_void_p(d_bases), total))
    for p in (d_keys, d_bases, d_offs, d_counts):
        check(lib.tbk_device_free(dev, C.c_void_p(p)))

    def decode(keys):
        lut = np.frombuffer(b"ACGT", dtype=np.uint8)
        out = np.empty((keys.size, k + 1), dtype=np.uint8)
        for i in range(k):
            out[:, i] = lut[((keys >> np.uint64(2 * i)) & np.uint64(3)).astype(np.int64)]
        out[:, k] = 10
        return out.tobytes()

    (tmp_path / "hapA.txt").write_bytes(decode(h_keys[:n_list]))
    (tmp_path / "hapB.txt").write_bytes(decode(h_keys[n_list:]))
    with open(tmp_path / "reads.fastq", "wb") as fh:
        for r in range(R):
            fh.write(b"@s%d\n" % r + bases[r * L:(r + 1) * L].tobytes() + b"\n+\n" + b"I" * L + b"\n")
    od = tmp_path / "out"
    od.mkdir()
    out = _run([str(tmp_path / "reads.fastq"), str(tmp_path / "hapA.txt"), str(tmp_path / "hapB.txt"),
                "--haplotype-a-out-prefix", str(od / "hapA"), "--haplotype-b-out-prefix", str(od / "hapB"),
                "--unclassified-out-prefix", str(od / "unc")], capsys)
    lines = out.splitlines()
    assert len(lines) == R
    sa, sb, bins = kmers.score_and_bin(counts, n_list, n_list)
    for r, line in enumerate(lines):
        name, bin_, x, y = line.split("\t")
        assert (name, bin_, float(x), float(y)) == (f"s{r}", chr(bins[r]), float(sa[r]), float(sb[r]))
    n_in_bins = sum(len(list(readfq_names(od / f))) for f in ("hapA.fastq.gz", "hapB.fastq.gz", "unc.fastq.gz"))
    assert n_in_bins == R and counts.sum() > 20 * R


def readfq_names(path):
    import gzip

    from trio_binning_amd.seq import readfq

    with gzip.open(path, "rt") as fh:
        for rec in readfq(fh):
            yield rec.name


def _rc(s: bytes) -> bytes:
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


@pytest.fixture(scope="module")
def uneven_workload(tmp_path_factory):
    """k = 21; two 5 Mb haplotypes (B is A with 1 % of its positions changed) and 2 x 10^5 k-mers of each that the other lacks;
    ~3000 FASTQ reads with HiFi-like qualities from either haplotype (either strand) or from neither: log-normal lengths around
    8 kb, four of 2-5 Mb, some shorter than k.  Written as bgzf, as one ordinary gzip member and plain.  Expected: the oracle's
    counts, scores and bins, the TSV the reference prints from them, and each bin's text as the Python mirror writes it."""
    import numpy as np

    import oracle
    from trio_binning_amd import seq
    from test_gpu_inflate import bgzf

    d = tmp_path_factory.mktemp("uneven")
    rng = np.random.default_rng(2024)
    k, G = 21, 5_000_000
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    ha = rng.integers(0, 4, G).astype(np.uint8)
    hb = ha.copy()
    snp = np.unique(rng.integers(0, G, G // 100))
    hb[snp] = (hb[snp] + rng.integers(1, 4, snp.size)) % 4
    A, B = lut[ha].tobytes(), lut[hb].tobytes()
    near = np.zeros(G, dtype=bool)   # k-mer starts whose window holds a changed position: present in one haplotype only
    for o in range(k):
        near[np.clip(snp - o, 0, G - k)] = True
    starts = np.flatnonzero(near)
    for name, hap in (("la.txt", A), ("lb.txt", B)):
        pick = np.sort(rng.choice(starts, 200_000, replace=False))
        (d / name).write_bytes(b"".join(hap[p:p + k] + b"\n" for p in pick))
    lens = np.clip(rng.lognormal(np.log(8000), 0.6, 3000), 1, 60_000).astype(np.int64)
    short = rng.random(lens.size) < 0.02
    lens[short] = rng.integers(1, k, int(short.sum()))
    lens[[400, 1100, 1900, 2600]] = [2_000_000, 4_900_000, 3_100_000, 2_500_000]
    recs = []
    for i, L in enumerate(lens):
        L = int(L)
        src = rng.integers(0, 3)
        if src == 2:
            s = lut[rng.integers(0, 4, L)].tobytes()
        else:
            p = int(rng.integers(0, G - L))
            s = (A, B)[src][p:p + L]
            if rng.random() < 0.5:
                s = _rc(s)
        qv = np.clip(rng.normal(60, 15, L), 2, 93).astype(np.uint8)
        qv[rng.random(L) < 0.6] = 93
        recs.append(b"@r%d/ccs len=%d\n" % (i, L) + s + b"\n+\n" + (qv + 33).tobytes() + b"\n")
    text = b"".join(recs)
    del recs
    (d / "reads.fastq").write_bytes(text)
    (d / "reads.fastq.gz").write_bytes(gzip.compress(text, 1))
    (d / "reads.bgzf.fastq.gz").write_bytes(bgzf(text, level=1))
    del text
    reads = list(seq.open_fastx_read(str(d / "reads.fastq")))
    assert len(reads) == 3000 and 30e6 < sum(len(r.seq) for r in reads) < 50e6
    orc = oracle.load()
    ta, tb = orc.table_from_file(str(d / "la.txt")), orc.table_from_file(str(d / "lb.txt"))
    bases = np.frombuffer(b"".join(r.seq.encode() for r in reads), dtype=np.uint8)
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r.seq) for r in reads], out=offsets[1:])
    counts = orc.count_batch(bases, offsets, ta, tb, threads=16)
    sa, sb, bins = orc.score_and_bin(counts, ta.num_kmers, tb.num_kmers)
    assert {"A", "B", "U"} <= set(bins) and bins.count("A") > 500 and bins.count("B") > 500
    tsv = "".join("\t".join(map(str, [r.name, c, float(x), float(y)])) + "\n" for r, c, x, y in zip(reads, bins, sa, sb))
    want = {}
    for letter, fn in (("A", "hapA.fastq.gz"), ("B", "hapB.fastq.gz"), ("U", "unc.fastq.gz")):
        buf = io.StringIO()
        for r, c in zip(reads, bins):
            if c == letter:
                r.print(file=buf)
        want[fn] = buf.getvalue().encode()
    return d, tsv, want


@pytest.mark.parametrize("encoder", ["gpu", "cpu"])
@pytest.mark.parametrize("sizes", ["default", "small"])
@pytest.mark.parametrize("reads_name", ["reads.bgzf.fastq.gz", "reads.fastq.gz", "reads.fastq"])
def test_default_cli_on_uneven_reads(gpu, capsys, tmp_path, monkeypatch, uneven_workload, reads_name, sizes, encoder):
    """The default command line (gzip'ed bins) on ~42 Mbases of uneven reads, from bgzf (the device inflater), one gzip member (the
    host inflater) and plain text; with the default sizes and with small inflater windows and batches (remnant batches, flushes of
    changing size); the members coded on the device or on the host.  stdout and the decompressed bins equal the oracle's."""
    import trio_binning_amd.classify_by_kmers as cbk

    d, tsv, want = uneven_workload
    monkeypatch.setenv("TBK_GZIP_ENCODER", encoder)
    if sizes == "small":
        monkeypatch.setenv("TBK_BGZF_GPU_WINDOW", str(1 << 20))
        monkeypatch.setattr(cbk, "_BATCH_BASES", 1_500_000)
        monkeypatch.setattr(cbk, "_BATCH_READS", 300)
    od = tmp_path / "out"
    od.mkdir()
    out = _run([str(d / reads_name), str(d / "la.txt"), str(d / "lb.txt"), "--haplotype-a-out-prefix", str(od / "hapA"),
                "--haplotype-b-out-prefix", str(od / "hapB"), "--unclassified-out-prefix", str(od / "unc")], capsys)
    assert out == tsv
    assert sorted(os.listdir(od)) == sorted(want)
    for fn, body in want.items():
        assert gzip.open(od / fn, "rb").read() == body, fn
