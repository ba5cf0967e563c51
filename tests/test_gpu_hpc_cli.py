"""Homopolymer-compressed k-mers end to end on the command lines: find-unique-kmers --compress --keep-databases, then
classify-by-kmers from the two databases (which switch the mode on by themselves) and from the two lists with --compress.
The TSV must be the one computed from tests/hpc_ref.compress_np(..., fold_case=False) of the reads, the oracle's counts
against the dumped lists and score_and_bin; the bins must hold the reads as they came.  Last, the case the feature exists
for: reads whose every homopolymer run is off by one base score (0, 0) in plain space and are binned in compressed space."""
import contextlib
import gzip
import io
import itertools
import os
from unittest.mock import patch

import numpy as np
import pytest

import hpc_ref

pytestmark = pytest.mark.gpu

K = 21
COMP = str.maketrans("ACGT", "TGCA")
CUTS = ["--min-count-a", "3", "--max-count-a", "200", "--min-count-b", "3", "--max-count-b", "200"]


def _runny_genome(rng, n, max_gap=6):
    """n bases in which homopolymer runs of two or three bases lie at most max_gap bases apart."""
    out, last, since = [], "", 0
    while sum(map(len, out)) < n:
        base = "ACGT"[int(rng.integers(0, 4))]
        if base == last:
            continue
        length = int(rng.integers(2, 4)) if since >= max_gap - 1 or rng.random() < 0.3 else 1
        since = 0 if length > 1 else since + 1
        out.append(base * length)
        last = base
    return "".join(out)[:n]


def _off_by_one(rng, s):
    """Every run of two or more equal bases one base longer or one shorter; single bases as they are."""
    out = []
    for ch, run in itertools.groupby(s):
        n = len(list(run))
        out.append(ch * (n + (1 if rng.random() < 0.5 else -1) if n >= 2 else n))
    return "".join(out)


def _short_reads(rng, genome, coverage=25, length=150):
    reads = []
    for _ in range(len(genome) * coverage // length):
        p = int(rng.integers(0, len(genome) - length + 1))
        r = genome[p:p + length]
        reads.append(r.translate(COMP)[::-1] if rng.random() < 0.5 else r)
    return reads


def _fastq(path, reads, gz=False):
    text = "".join(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads))
    with (gzip.open if gz else open)(path, "wt") as fh:
        fh.write(text)
    return str(path)


def _find(out, argv):
    from trio_binning_amd import find_unique_kmers as fu

    out.mkdir()
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        fu.main(["-k", str(K), "-o", str(out), "-s", str(out), "--capacity", "400000"] + CUTS + argv)
    return [str(out / name) for name in ("hapA_only_kmers.txt", "hapB_only_kmers.txt")]


def _classify(argv, out_dir, capsys):
    """One run of the driver: (stdout, stderr, {bin: decompressed text})."""
    from trio_binning_amd.classify_by_kmers import main

    out_dir.mkdir()
    prefixes = ["--haplotype-a-out-prefix", str(out_dir / "hapA"), "--haplotype-b-out-prefix", str(out_dir / "hapB"),
                "--unclassified-out-prefix", str(out_dir / "unclassified")]
    capsys.readouterr()
    with patch("sys.argv", ["classify-by-kmers"] + argv + prefixes):
        main()
    out, err = capsys.readouterr()
    bins = {name[0].upper() if name.startswith("u") else name[3]: gzip.open(out_dir / name, "rt").read() for name in sorted(os.listdir(out_dir))}
    return out, err, bins


def _oracle_counts_of(reads, k, compressed):
    from oracle import unique_oracle as uo

    bases, offsets = uo.pack(reads)
    if compressed:
        bases, offsets = hpc_ref.compress_np(bases, offsets, True)
    return uo.count_kmers_np(bases, offsets, k)


def _expected(orc, reads, lists, compressed):
    """(counts, score_a, score_b, bins) of the reads against the two list files: the oracle's counter on the reads, compressed
    as the classifier compresses them (case as it came) or as they are; the scores and bins of kmers.score_and_bin."""
    from oracle import unique_oracle as uo
    from trio_binning_amd import kmers

    bases, offsets = uo.pack(reads)
    if compressed:
        bases, offsets = hpc_ref.compress_np(bases, offsets, False)
    counts = orc.count_batch(np.ascontiguousarray(bases), offsets, orc.table_from_file(lists[0]), orc.table_from_file(lists[1]))
    lines = [sum(1 for _ in open(p)) for p in lists]
    score_a, score_b, bins = kmers.score_and_bin(counts, lines[0], lines[1])
    return counts, score_a, score_b, bins.decode()


def _check_run(run, reads, expected):
    out, _, bins = run
    counts, score_a, score_b, want_bins = expected
    rows = [line.split("\t") for line in out.splitlines()]
    assert len(rows) == len(reads)
    for i, row in enumerate(rows):
        assert row[0] == f"r{i}" and row[1:] == [want_bins[i], str(float(score_a[i])), str(float(score_b[i]))], (i, row, counts[i])
    # the three bins hold the reads as they came, uncompressed, in input order
    for which in "ABU":
        want = "".join(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads) if want_bins[i] == which)
        assert bins[which] == want, which


@pytest.fixture(scope="module")
def family(gpu, tmp_path_factory):
    """Two parents (haplotypes of one random genome, 25x of exact 150-base reads each) counted with --compress, their
    databases kept; a child's long reads from both, every one with its runs lengthened or shortened at random."""
    root = tmp_path_factory.mktemp("hpc_cli")
    rng = np.random.default_rng(1234)
    ga = "".join("ACGT"[c] for c in rng.integers(0, 4, 12_000))
    gb = list(ga)
    for i in np.flatnonzero(rng.random(len(ga)) < 1 / 120):
        gb[int(i)] = "ACGT"[("ACGT".index(gb[int(i)]) + int(rng.integers(1, 4))) % 4]
    gb = "".join(gb)
    parents = {"a": _short_reads(rng, ga), "b": _short_reads(rng, gb)}
    child = []
    for i in range(60):
        g = (ga, gb)[i % 2]
        length = int(rng.integers(100, 3000))
        p = int(rng.integers(0, len(g) - length))
        r = "".join(ch * max(len(list(run)) + int(rng.integers(-1, 2)), 1) for ch, run in itertools.groupby(g[p:p + length]))
        child.append(r.translate(COMP)[::-1] if i % 3 == 0 else r)
    child += [ga[:400].lower(), ga[400:700] + "NNNN" + gb[700:1000], "ACGT" * 10, "N" * 50, "A" * 300, "AaAaCcGgTt" * 30]
    files = {"a": _fastq(root / "a.fastq", parents["a"]), "b": _fastq(root / "b.fastq.gz", parents["b"], gz=True),
             "child": _fastq(root / "child.fastq", child)}
    lists = _find(root / "counted", ["--compress", "--keep-databases", files["a"], files["b"]])
    return {"root": root, "parents": parents, "child": child, "files": files, "lists": lists,
            "dbs": [str(root / "counted" / name) for name in ("haplotypeA.tbkdb", "haplotypeB.tbkdb")]}


def test_find_unique_kmers_compress_leaves_compressed_lists_and_databases(family):
    from oracle import unique_oracle as uo
    from trio_binning_amd import kmers

    na, nb = (_oracle_counts_of(family["parents"][name], K, True) for name in "ab")
    for path, want in zip(family["lists"], (uo.unique_np(na, nb, 3, 200), uo.unique_np(nb, na, 3, 200))):
        assert want.size > 300 and np.array_equal(uo.read_list_np(path, K), want)
        assert all(x != y for line in open(path) for x, y in zip(line.strip(), line.strip()[1:]))
    for path in family["dbs"]:
        assert open(path, "rb").read(8) == b"TBKKMDH1" and kmers.database_file_info(path)["compressed"]


def test_classify_from_compressed_databases_and_from_compressed_lists(family, orc, capsys, tmp_path):
    expected = _expected(orc, family["child"], family["lists"], True)
    assert expected[3].count("A") >= 20 and expected[3].count("B") >= 20 and expected[3].count("U") >= 3
    by_db = _classify([family["files"]["child"]] + family["dbs"] + CUTS, tmp_path / "dbs", capsys)
    assert "homopolymer-compressed space" in by_db[1]
    _check_run(by_db, family["child"], expected)
    by_list = _classify([family["files"]["child"]] + family["lists"] + ["--compress"], tmp_path / "lists", capsys)
    assert "homopolymer-compressed space" in by_list[1]
    _check_run(by_list, family["child"], expected)
    assert by_list[0] == by_db[0] and by_list[2] == by_db[2]
    # several batches, taking turns on the two sessions: the same output
    with patch("trio_binning_amd.classify_by_kmers._BATCH_READS", 7):
        small = _classify([family["files"]["child"]] + family["lists"] + ["--compress"], tmp_path / "small", capsys)
    assert small[0] == by_db[0] and small[2] == by_db[2]
    # a compressed database beside a list is refused as any database beside a list is
    from trio_binning_amd.classify_by_kmers import main

    with patch("sys.argv", ["classify-by-kmers", family["files"]["child"], family["dbs"][0], family["lists"][1]]):
        with pytest.raises(SystemExit):
            main()


def test_reads_whose_every_run_is_off_by_one_are_binned_only_in_compressed_space(gpu, orc, capsys, tmp_path):
    from oracle import unique_oracle as uo

    rng = np.random.default_rng(4321)
    ga, gb = _runny_genome(rng, 6_000), _runny_genome(rng, 6_000)
    longest_gap = max(len(piece) for piece in "".join("x" if len(list(run)) > 1 else "." for _, run in itertools.groupby(ga)).split("x"))
    assert longest_gap <= K // 2  # runs of two or more lie at most k/2 bases apart
    parents = {"a": _short_reads(rng, ga), "b": _short_reads(rng, gb)}
    child = []
    for _ in range(30):
        length = int(rng.integers(600, 2000))
        p = int(rng.integers(0, len(ga) - length))
        child.append(_off_by_one(rng, ga[p:p + length]))
    files = {"a": _fastq(tmp_path / "a.fastq", parents["a"]), "b": _fastq(tmp_path / "b.fastq", parents["b"]), "child": _fastq(tmp_path / "child.fastq", child)}
    plain_lists = _find(tmp_path / "plain", [files["a"], files["b"]])
    hpc_lists = _find(tmp_path / "hpc", ["--compress", files["a"], files["b"]])
    # in plain space no window of these reads survives: the plain oracle says so, of the lists the plain run dumped
    na, nb = (_oracle_counts_of(parents[name], K, False) for name in "ab")
    assert np.array_equal(uo.read_list_np(plain_lists[0], K), uo.unique_np(na, nb, 3, 200)) and uo.unique_np(na, nb, 3, 200).size > 1000
    plain = _expected(orc, child, plain_lists, False)
    assert not plain[0].any()
    run = _classify([files["child"]] + plain_lists, tmp_path / "plain_bins", capsys)
    assert [line.split("\t")[2:] for line in run[0].splitlines()] == [["0.0", "0.0"]] * len(child)
    _check_run(run, child, plain)
    # in compressed space every one of them is binned A, with the counts the oracle gives
    hpc = _expected(orc, child, hpc_lists, True)
    assert hpc[3] == "A" * len(child) and (hpc[0][:, 0] > 50).all() and not hpc[0][:, 1].any()
    run = _classify([files["child"]] + hpc_lists + ["--compress"], tmp_path / "hpc_bins", capsys)
    _check_run(run, child, hpc)
    assert run[2]["B"] == "" and run[2]["U"] == ""
