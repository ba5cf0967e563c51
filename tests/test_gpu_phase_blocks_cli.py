"""python -m trio_binning_amd.phase_blocks on three "contigs" built from two synthetic haplotypes - pure A, pure B, and A-then-B
with one isolated single-window B-marker planted inside the A part - from text lists and from count databases.

Haplotype B is haplotype A with a SNP every 100 bases.  The parents' count databases (crafted files: tests/kmerdb_files.py)
hold every k-mer of their haplotype as its lexicographically smaller strand; the lists are what find-unique-kmers' selection
dumps from them, and a list line hits only where that strand is also the smaller packed key, so about half the k windows
over a SNP are markers.  The TSV and the BED are compared byte for byte with what the test works out itself: marks from numpy,
runs and blocks from a Python loop (tests/hit_track_ref.py), and the lines formatted here."""
import gzip
import os
from unittest.mock import patch

import numpy as np
import pytest

import hit_track_ref as ref
import kmerdb_files as kf

pytestmark = pytest.mark.gpu

K = 21
CUTS = ["--min-count-a", "2", "--max-count-a", "255", "--min-count-b", "2", "--max-count-b", "255"]


def _lex_rank(kmer):
    return sum("ACGT".index(c) << (2 * (len(kmer) - 1 - i)) for i, c in enumerate(kmer))


def _smaller_strand(kmer):
    return min(kmer, ref.revcomp(kmer))


def _kmers(s):
    return {_smaller_strand(s[i:i + K]) for i in range(len(s) - K + 1)}


def _write_db(path, kmer_set):
    ranks = np.array(sorted(_lex_rank(x) for x in kmer_set), dtype=np.uint64)
    counts = np.full(ranks.size, 9, dtype=np.uint8)
    hist = np.bincount(counts, minlength=256).astype(np.uint64)
    hist[1] = 3
    hist[0] = ranks.size + 3
    with open(path, "wb") as fh:
        fh.write(kf.file_bytes(K, ranks, counts, hist, reads=1, bases=K))
    return str(path)


def _fasta(path, records, gz=False, width=70):
    text = "".join(">{} made up\n{}\n".format(name, "\n".join(s[i:i + width] for i in range(0, len(s), width))) for name, s in records)
    with (gzip.open if gz else open)(path, "wb") as fh:
        fh.write(text.encode())
    return str(path)


@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    from trio_binning_amd import kmers

    root = tmp_path_factory.mktemp("phase")
    rng = np.random.default_rng(31)
    hap_a = "".join("ACGT"[c] for c in rng.integers(0, 4, 3000))
    hap_b = list(hap_a)
    for p in range(50, 3000, 100):
        hap_b[p] = "ACGT"[("ACGT".index(hap_b[p]) + 1 + int(rng.integers(0, 3))) % 4]
    hap_b = "".join(hap_b)
    # the third contig: A, then B from 1500 on, and in the A part a base of its own at 700 (50 bases from either SNP): of the
    # windows over it, one whose smaller strand is also its smaller packed key goes into parent B's database as an "error" k-mer
    mixed = list(hap_a[:1500] + hap_b[1500:])
    mixed[700] = "ACGT"[("ACGT".index(mixed[700]) + 2) % 4]
    mixed = "".join(mixed)
    error_at = next(w for w in range(690, 700) if ref.pack(_smaller_strand(mixed[w:w + K])) == ref.canonical(mixed[w:w + K]))
    error = _smaller_strand(mixed[error_at:error_at + K])
    contigs = [("pureA", hap_a), ("pureB", hap_b), ("switch", mixed)]
    db_a, db_b = _write_db(root / "hapA.tbkdb", _kmers(hap_a)), _write_db(root / "hapB.tbkdb", _kmers(hap_b) | {error})
    # the child holds what its contigs hold, but nothing over the SNPs at 250 and 2350: the parents' k-mers there are not inherited
    child = _kmers(mixed) | _kmers(hap_a) | _kmers(hap_b)
    child -= _kmers(hap_a[230:271]) | _kmers(hap_b[230:271]) | _kmers(hap_a[2330:2371]) | _kmers(hap_b[2330:2371])
    db_child = _write_db(root / "child.tbkdb", child)
    lists = {}
    with kmers.KmerDatabase.load(db_a) as da, kmers.KmerDatabase.load(db_b) as db, kmers.KmerDatabase.load(db_child) as dc:
        for name, third in (("plain", {}), ("child", {"child": dc, "child_min": 2, "child_max": 255})):
            lists[name] = (str(root / f"{name}_A.txt"), str(root / f"{name}_B.txt"))
            assert da.unique(db, 2, 255, lists[name][0], **third) > 0 and db.unique(da, 2, 255, lists[name][1], **third) > 0
    assert open(lists["child"][0]).read().count("\n") < open(lists["plain"][0]).read().count("\n")
    soft = [(name, "".join(c.lower() if (i // 40) % 3 == 0 else c for i, c in enumerate(s))) for name, s in contigs]
    return {"root": root, "contigs": contigs, "soft": soft, "lists": lists, "db_a": db_a, "db_b": db_b, "db_child": db_child,
            "error_at": error_at, "hap_a": hap_a, "hap_b": hap_b,
            "fa": _fasta(root / "contigs.fa", contigs), "fa_gz": _fasta(root / "contigs.fa.gz", contigs, gz=True),
            "fa_soft": _fasta(root / "soft.fa", soft)}


def _list_keys(path):
    return np.array([ref.pack(line.strip()) for line in open(path)], dtype=np.uint64)


def _expected(records, list_paths, min_run, ignore_case=False):
    """(TSV, BED, blocks) as the command must write them, from the reference alone"""
    from trio_binning_amd import kmers

    bases, offsets = kmers.pack_reads([s for _, s in records])
    mk = ref.marks(bases, offsets, _list_keys(list_paths[0]), _list_keys(list_paths[1]), K, ignore_case)
    counts = ref.counts_of(mk, offsets)
    blocks = ref.blocks(ref.runs(mk, offsets), min_run)
    tsv, bed = [], []
    for r, (name, s) in enumerate(records):
        mine = blocks[blocks["read"] == r]
        extent = [int(b["last"]) + K - int(b["first"]) for b in mine]
        in_hap = [sum(e for e, b in zip(extent, mine) if int(b["hap"]) == h) for h in (0, 1)]
        tsv.append("\t".join(str(x) for x in (name, len(s), counts[r, 0], counts[r, 1], len(mine), max(len(mine) - 1, 0), in_hap[0], in_hap[1],
                                              max(extent, default=0))) + "\n")
        bed += ["{}\t{}\t{}\t{}\t{}\n".format(name, int(b["first"]), int(b["last"]) + K, "AB"[int(b["hap"])], int(b["markers"])) for b in mine]
    return "".join(tsv), "".join(bed), blocks


def _run(argv, bed, capsys):
    from trio_binning_amd import phase_blocks

    capsys.readouterr()
    phase_blocks.main(argv + ["--bed", str(bed)])
    out = capsys.readouterr().out
    assert not os.path.exists(str(bed) + ".tmp")
    return out, open(bed).read()


def test_text_lists_the_isolated_marker_splits_the_block(world, capsys, tmp_path):
    lists = list(world["lists"]["plain"])
    tsv, bed, blocks = _expected(world["contigs"], lists, 1)
    assert _run([world["fa"]] + lists + ["--min-run", "1"], tmp_path / "one.bed", capsys) == (tsv, bed)
    assert _run([world["fa"]] + lists, tmp_path / "default.bed", capsys) == (tsv, bed)  # (--min-run 1 is the default)
    # what the expectation itself must look like: one block per pure contig, A B A B in the third, the B in the middle one marker
    assert [(int(b["read"]), int(b["hap"])) for b in blocks] == [(0, 0), (1, 1), (2, 0), (2, 1), (2, 0), (2, 1)]
    assert (int(blocks[3]["first"]), int(blocks[3]["last"]), int(blocks[3]["markers"])) == (world["error_at"], world["error_at"], 1)
    assert tsv.splitlines()[2].split("\t")[4:6] == ["4", "3"]
    tsv2, bed2, blocks2 = _expected(world["contigs"], lists, 2)
    assert _run([world["fa"]] + lists + ["--min-run", "2"], tmp_path / "two.bed", capsys) == (tsv2, bed2)
    assert [(int(b["read"]), int(b["hap"])) for b in blocks2] == [(0, 0), (1, 1), (2, 0), (2, 1)]
    assert tsv2.splitlines()[2].split("\t")[4:6] == ["2", "1"] and tsv2.splitlines()[2].split("\t")[:4] == tsv.splitlines()[2].split("\t")[:4]


@pytest.mark.parametrize("with_child", [False, True])
def test_databases_give_the_blocks_of_their_dumped_lists(world, capsys, tmp_path, with_child):
    lists = list(world["lists"]["child" if with_child else "plain"])
    third = ["--child-database", world["db_child"], "--min-count-child", "2"] if with_child else []
    for min_run in (1, 2):
        want = _expected(world["contigs"], lists, min_run)[:2]
        assert _run([world["fa"], world["db_a"], world["db_b"], "--min-run", str(min_run)] + CUTS + third, tmp_path / f"db{min_run}.bed", capsys) == want
        assert _run([world["fa"]] + lists + ["--min-run", str(min_run)], tmp_path / f"list{min_run}.bed", capsys) == want
    if with_child:
        assert want != _expected(world["contigs"], list(world["lists"]["plain"]), 2)[:2]


def test_gzipped_fasta(world, capsys, tmp_path):
    lists = list(world["lists"]["plain"])
    assert _run([world["fa_gz"]] + lists, tmp_path / "gz.bed", capsys) == _expected(world["contigs"], lists, 1)[:2]


def test_ignore_case_on_a_soft_masked_copy(world, capsys, tmp_path):
    lists = list(world["lists"]["plain"])
    plain = _expected(world["contigs"], lists, 1)[:2]
    assert _run([world["fa_soft"]] + lists + ["--ignore-case"], tmp_path / "ic.bed", capsys) == plain
    masked = _expected(world["soft"], lists, 1, ignore_case=False)[:2]
    assert masked != plain
    assert _run([world["fa_soft"]] + lists, tmp_path / "masked.bed", capsys) == masked


def test_fastq_marker_columns_are_what_classify_by_kmers_counts(world, capsys, tmp_path):
    from trio_binning_amd import classify_by_kmers as cbk

    rng = np.random.default_rng(32)
    reads = []
    for i in range(40):
        g = (world["hap_a"], world["hap_b"])[i % 2]
        n = int(rng.integers(10, 1200))
        p = int(rng.integers(0, len(g) - n))
        s = g[p:p + n]
        reads.append(("read{}".format(i), ref.revcomp(s) if i % 3 == 0 else s))
    reads += [("chimera", world["hap_a"][:800] + world["hap_b"][800:1600]), ("short", "ACGT"), ("noisy", "N" * 60)]
    fq = tmp_path / "reads.fastq"
    fq.write_text("".join("@{}\n{}\n+\n{}\n".format(name, s, "I" * len(s)) for name, s in reads))
    lists = list(world["lists"]["plain"])
    tsv, _ = _run([str(fq)] + lists, tmp_path / "reads.bed", capsys)
    assert tsv == _expected(reads, lists, 1)[0]
    bins = tmp_path / "bins"
    bins.mkdir()
    argv = [str(fq)] + lists + ["--haplotype-a-out-prefix", str(bins / "hapA"), "--haplotype-b-out-prefix", str(bins / "hapB"),
                                "--unclassified-out-prefix", str(bins / "unclassified")]
    with patch("sys.argv", ["classify-by-kmers"] + argv):
        cbk.main()
    scored = [line.split("\t") for line in capsys.readouterr().out.splitlines()]
    n_a, n_b = (open(p).read().count("\n") for p in lists)
    scale = (max(n_a, n_b) / n_a, max(n_a, n_b) / n_b)
    mine = [line.split("\t") for line in tsv.splitlines()]
    assert [row[0] for row in scored] == [row[0] for row in mine] == [name for name, _ in reads]
    for row, got in zip(scored, mine):
        assert (round(float(row[2]) / scale[0]), round(float(row[3]) / scale[1])) == (int(got[2]), int(got[3])), row[0]
    assert sum(int(row[2]) for row in mine) > 0 and sum(int(row[3]) for row in mine) > 0
