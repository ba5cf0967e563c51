"""python -m trio_binning_amd.phase_blocks --compress on three "contigs" - pure A, pure B, and A-then-B with one isolated
single-window B-marker planted inside the A part - whose homopolymer runs have been stretched: the markers are found in compressed
space, and TSV and BED speak the coordinates of the contigs as given.

The two haplotypes are made in compressed space (no two equal neighbours); B is A with a SNP every 100 letters that keeps it
so.  A contig is a haplotype with every letter written a random number of times, differently for every contig.  The parents are
crafted TBKKMDH1 count databases (tests/kmerdb_files.py) that hold every k-mer of their compressed haplotype as its
lexicographically smaller strand; the lists are what the selection dumps from them.  TSV and BED are compared byte for byte with
what the test works out itself (tests/hpc_lift_ref.py: numpy compression, reference marks and runs, lifted through the keep
bits) and formats here."""
import os
from unittest.mock import patch

import numpy as np
import pytest

import hit_track_ref as ref
import hpc_lift_ref as lref
import hpc_ref
import kmerdb_files as kf

pytestmark = pytest.mark.gpu

K = 21
MAGIC_HPC = b"TBKKMDH1"
CUTS = ["--min-count-a", "2", "--max-count-a", "255", "--min-count-b", "2", "--max-count-b", "255"]


def _lex_rank(kmer):
    return sum("ACGT".index(c) << (2 * (len(kmer) - 1 - i)) for i, c in enumerate(kmer))


def _kmers(s):
    return {min(s[i:i + K], ref.revcomp(s[i:i + K])) for i in range(len(s) - K + 1)}


def _write_db(path, kmer_set):
    ranks = np.array(sorted(_lex_rank(x) for x in kmer_set), dtype=np.uint64)
    counts = np.full(ranks.size, 9, dtype=np.uint8)
    hist = np.bincount(counts, minlength=256).astype(np.uint64)
    hist[1] = 3
    hist[0] = ranks.size + 3
    with open(path, "wb") as fh:
        fh.write(kf.file_bytes(K, ranks, counts, hist, reads=1, bases=K, magic=MAGIC_HPC))
    return str(path)


def _fasta(path, records, width=70):
    with open(path, "w") as fh:
        fh.write("".join(">{} made up\n{}\n".format(name, "\n".join(s[i:i + width] for i in range(0, len(s), width))) for name, s in records))
    return str(path)


def _contigs(small, seed):
    """the three compressed contigs with their runs stretched by seeded random amounts, one run of each longer than a tile"""
    rng = np.random.default_rng(seed)
    out = []
    for name, s in small:
        lengths = rng.geometric(0.4, len(s))
        lengths[int(rng.integers(100, len(s) - 100))] = 4096 + int(rng.integers(1, 900))
        lengths[-1] = int(rng.integers(2, 12))  # the contig ends in a run
        out.append((name, lref.stretch(s, lengths)))
    return out


@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    from trio_binning_amd import kmers

    root = tmp_path_factory.mktemp("phase_hpc")
    rng = np.random.default_rng(41)
    hap_a = lref.compressed_sequence(rng, 3000)
    hap_b = list(hap_a)
    for p in range(50, 3000, 100):  # a SNP that leaves no two equal neighbours
        hap_b[p] = next(c for c in "ACGT" if c not in (hap_a[p - 1], hap_a[p], hap_a[p + 1]))
    hap_b = "".join(hap_b)
    # the third contig: A, then B from 1500 on, and in the A part a letter of its own at 700 (50 letters from either SNP); one
    # window over it goes into parent B's database as an "error" k-mer
    mixed = list(hap_a[:1500] + hap_b[1500:])
    mixed[700] = next(c for c in "ACGT" if c not in (hap_a[699], hap_a[700], hap_a[701]))
    mixed = "".join(mixed)
    error_at = 693
    error = min(mixed[error_at:error_at + K], ref.revcomp(mixed[error_at:error_at + K]))
    for s in (hap_a, hap_b, mixed):
        assert all(x != y for x, y in zip(s, s[1:]))
    small = [("pureA", hap_a), ("pureB", hap_b), ("switch", mixed)]
    db_a, db_b = _write_db(root / "hapA.tbkdb", _kmers(hap_a)), _write_db(root / "hapB.tbkdb", _kmers(hap_b) | {error})
    lists = (str(root / "A.txt"), str(root / "B.txt"))
    with kmers.KmerDatabase.load(db_a) as da, kmers.KmerDatabase.load(db_b) as db:
        assert da.compressed and db.compressed
        assert da.unique(db, 2, 255, lists[0]) > 0 and db.unique(da, 2, 255, lists[1]) > 0
    contigs, other = _contigs(small, 42), _contigs(small, 43)
    return {"root": root, "small": small, "error_at": error_at, "contigs": contigs, "other": other, "lists": lists, "db_a": db_a, "db_b": db_b,
            "fa": _fasta(root / "contigs.fa", contigs), "fa_other": _fasta(root / "other.fa", other)}


def _list_keys(path):
    return np.array([ref.pack(line.strip()) for line in open(path)], dtype=np.uint64)


def _expected(records, list_paths, min_run, ignore_case=False):
    """(TSV, BED, blocks) as the command must write them under --compress, from the reference alone"""
    from trio_binning_amd import kmers

    bases, offsets = kmers.pack_reads([s for _, s in records])
    want = lref.Lifted(bases, offsets, _list_keys(list_paths[0]), _list_keys(list_paths[1]), K, ignore_case)
    blocks = lref.blocks(want.runs, min_run)
    tsv, bed = [], []
    for r, (name, s) in enumerate(records):
        mine = blocks[blocks["read"] == r]
        extent = [int(b["end"]) - int(b["first"]) for b in mine]
        in_hap = [sum(e for e, b in zip(extent, mine) if int(b["hap"]) == h) for h in (0, 1)]
        tsv.append("\t".join(str(x) for x in (name, len(s), want.counts[r, 0], want.counts[r, 1], len(mine), max(len(mine) - 1, 0), in_hap[0],
                                              in_hap[1], max(extent, default=0))) + "\n")
        bed += ["{}\t{}\t{}\t{}\t{}\n".format(name, int(b["first"]), int(b["end"]), "AB"[int(b["hap"])], int(b["markers"])) for b in mine]
    return "".join(tsv), "".join(bed), blocks


def _run(argv, bed, capsys):
    from trio_binning_amd import phase_blocks

    capsys.readouterr()
    phase_blocks.main(argv + ["--bed", str(bed)])
    out = capsys.readouterr().out
    assert not os.path.exists(str(bed) + ".tmp")
    return out, open(bed).read()


@pytest.mark.parametrize("min_run", [1, 2])
def test_lists_and_databases_give_the_lifted_blocks(world, capsys, tmp_path, min_run):
    lists = list(world["lists"])
    tsv, bed, blocks = _expected(world["contigs"], lists, min_run)
    assert _run([world["fa"]] + lists + ["--compress", "--min-run", str(min_run)], tmp_path / "lists.bed", capsys) == (tsv, bed)
    assert _run([world["fa"], world["db_a"], world["db_b"], "--compress", "--min-run", str(min_run)] + CUTS, tmp_path / "dbs.bed", capsys) == (tsv, bed)
    # what the expectation itself must look like: one block per pure contig; A B A B in the third, the B in the middle one
    # marker that --min-run 2 drops; each block from its first marker window's first base to its last one's end
    assert [(int(b["read"]), int(b["hap"])) for b in blocks] == [(0, 0), (1, 1)] + [(2, 0), (2, 1)] * (2 if min_run == 1 else 1)
    lengths = [len(s) for _, s in world["contigs"]]
    assert int(blocks[1]["end"]) - int(blocks[1]["first"]) > 0.9 * lengths[1] and int(blocks[-1]["end"]) <= lengths[2]
    if min_run == 1:
        from trio_binning_amd import kmers

        bases, offsets = kmers.pack_reads([s for _, s in world["contigs"]])
        co = hpc_ref.compress_np(bases, offsets, False)[1]
        start = int(lref.lift_np(bases, offsets, False)[int(co[2]) + world["error_at"]]) - int(offsets[2])  # the error window's first base
        assert (int(blocks[3]["first"]), int(blocks[3]["last"]), int(blocks[3]["markers"])) == (start, start, 1)
        assert int(blocks[3]["end"]) > start + K  # (at least one of the window's 21 letters is written more than once)
    rows = [line.split("\t") for line in tsv.splitlines()]
    assert [row[1] for row in rows] == [str(n) for n in lengths]  # length is the length as given
    assert int(rows[0][8]) > 4096 and int(rows[0][6]) == int(blocks[0]["end"]) - int(blocks[0]["first"]) and rows[0][7] == "0"


def test_without_the_switch_the_stretched_contigs_hold_next_to_nothing(world, capsys, tmp_path):
    """(why the switch matters: the lists' k-mers have no two equal neighbours, the stretched contigs hardly a window without)"""
    lists = list(world["lists"])
    tsv, _ = _run([world["fa"]] + lists, tmp_path / "plain.bed", capsys)
    with_switch = _expected(world["contigs"], lists, 1)[0]
    markers = lambda text: sum(int(line.split("\t")[2]) + int(line.split("\t")[3]) for line in text.splitlines())  # noqa: E731
    assert markers(tsv) * 20 < markers(with_switch)


def test_other_stretch_factors_move_the_coordinates_and_nothing_else(world, capsys, tmp_path):
    lists = list(world["lists"])
    one = _run([world["fa"]] + lists + ["--compress"], tmp_path / "one.bed", capsys)
    two = _run([world["fa_other"]] + lists + ["--compress"], tmp_path / "two.bed", capsys)
    assert two == _expected(world["other"], lists, 1)[:2]
    rows = [[line.split("\t") for line in text.splitlines()] for text in (one[0], two[0])]
    assert [row[:1] + row[2:6] for row in rows[0]] == [row[:1] + row[2:6] for row in rows[1]]  # names, markers, blocks, switches
    assert [row[1] for row in rows[0]] != [row[1] for row in rows[1]]
    beds = [[line.split("\t") for line in text.splitlines()] for text in (one[1], two[1])]
    assert [(b[0], b[3], b[4]) for b in beds[0]] == [(b[0], b[3], b[4]) for b in beds[1]]
    assert [(b[1], b[2]) for b in beds[0]] != [(b[1], b[2]) for b in beds[1]]
    # the same compressed contigs unstretched: the same again, at compressed coordinates
    flat = _run([_fasta(tmp_path / "small.fa", world["small"])] + lists + ["--compress"], tmp_path / "flat.bed", capsys)
    assert flat == _expected(world["small"], lists, 1)[:2]
    rows.append([line.split("\t") for line in flat[0].splitlines()])
    assert [row[:1] + row[2:6] for row in rows[2]] == [row[:1] + row[2:6] for row in rows[0]]


def test_fastq_marker_columns_are_what_classify_by_kmers_counts_in_compressed_mode(world, capsys, tmp_path):
    from trio_binning_amd import classify_by_kmers as cbk

    rng = np.random.default_rng(44)
    reads = []
    for i in range(30):
        g = world["contigs"][i % 3][1]
        n = int(rng.integers(10, 2500))
        p = int(rng.integers(0, len(g) - n))
        s = g[p:p + n]
        reads.append(("read{}".format(i), ref.revcomp(s) if i % 3 == 0 else s))
    reads += [("short", "AACCGGTT"), ("noisy", "N" * 60), ("one_run", "A" * 500)]
    fq = tmp_path / "reads.fastq"
    fq.write_text("".join("@{}\n{}\n+\n{}\n".format(name, s, "I" * len(s)) for name, s in reads))
    lists = list(world["lists"])
    tsv, _ = _run([str(fq)] + lists + ["--compress"], tmp_path / "reads.bed", capsys)
    assert tsv == _expected(reads, lists, 1)[0]
    bins = tmp_path / "bins"
    bins.mkdir()
    argv = [str(fq)] + lists + ["--compress", "--haplotype-a-out-prefix", str(bins / "hapA"), "--haplotype-b-out-prefix", str(bins / "hapB"),
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
