"""python -m trio_binning_amd.assembly_qv on four "contigs" cut from one synthetic genome - a perfect one, one with a single
substitution, one with an N, a soft-masked stretch and a tail the reads never saw, and a short one - against a crafted count
database of the genome's k-mers (tests/kmerdb_files.py).  The TSV, the #total line, the --spectrum table and the --absent-bed file
are compared byte for byte with what the test works out itself: the loop of tests/db_query_ref.py, kmers.qv and the formats the
module's docstring states."""
import gzip
import os

import numpy as np
import pytest

import db_query_ref as ref

pytestmark = pytest.mark.gpu

K = 21


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _fasta(path, records, gz=False, width=70):
    text = "".join(">{} made up\n{}\n".format(name, "\n".join(s[i:i + width] for i in range(0, len(s), width))) for name, s in records)
    with (gzip.open if gz else open)(path, "wb") as fh:
        fh.write(text.encode())
    return str(path)


@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    root = tmp_path_factory.mktemp("qv")
    rng = np.random.default_rng(77)
    genome = _seq(rng, 4000)
    unseen = _seq(rng, 300)
    db = {km: 2 + ref.lex_rank(km) % 254 for km in ref.window_kmers(genome, K)}
    assert len(db) == len(genome) - K + 1  # (every 21-mer of the genome is unique: a substitution costs exactly k windows)
    planted = list(genome[1000:2500])
    planted[700] = "ACGT"[("ACGT".index(planted[700]) + 2) % 4]
    rough = genome[2400:2900] + "N" + genome[2901:3200].lower() + genome[3200:3500] + unseen
    contigs = [("perfect", genome[:1500]), ("planted", "".join(planted)), ("rough", rough), ("short", genome[10:10 + K - 1]),
               ("reverse", ref.revcomp(genome[3000:3900]))]
    path = root / "reads.tbkdb"
    path.write_bytes(ref.database_bytes(db, K))
    return {"root": root, "db": db, "db_path": str(path), "contigs": contigs, "fa": _fasta(root / "asm.fa", contigs),
            "fa_gz": _fasta(root / "asm.fa.gz", contigs, gz=True), "perfect_fa": _fasta(root / "perfect.fa", contigs[:1] + contigs[4:])}


def _expected(db, records, min_count=2, max_count=255):
    """(TSV with the #total line, spectrum table, BED) as the command must write them, from the reference alone"""
    from trio_binning_amd import kmers

    tally = ref.Tally(db)
    tsv, bed, total = [], [], [0, 0, 0]
    for name, s in records:
        per_read, counts = tally.add([s], K, min_count)
        clean, found = int(per_read[0, 0]), int(per_read[0, 1])
        tsv.append("{}\t{}\t{}\t{}\t{:.4f}\n".format(name, len(s), clean, found, kmers.qv(found, clean, K)))
        total = [total[0] + len(s), total[1] + clean, total[2] + found]
        is_clean = [km is not None for km in ref.window_kmers(s, K)]
        bed += ["{}\t{}\t{}\t{}\n".format(name, a, b + K, b - a + 1) for a, b in ref.absent_stretches(counts, is_clean)]
    seen, solid = tally.completeness(min_count, max_count)
    rate = 1.0 - (total[2] / total[1]) ** (1.0 / K) if total[2] < total[1] else 0.0
    tsv.append("#total\t{}\t{}\t{}\t{:.4f}\t{}\t{}\t{:.6f}\t{:.5e}\n".format(total[0], total[1], total[2], kmers.qv(total[2], total[1], K), seen, solid,
                                                                         seen / solid, rate))
    spec = tally.spectrum()
    labels = ["0", "1", "2", "3", "4", ">4"]
    spectrum = "".join("{}\t{}\t{}\n".format(c, labels[m], int(spec[m, c])) for c in range(256) for m in range(6) if spec[m, c])
    return "".join(tsv), spectrum, "".join(bed)


def _run(argv, tmp_path, capsys, tag):
    from trio_binning_amd import assembly_qv

    spectrum, bed = tmp_path / (tag + ".spectrum"), tmp_path / (tag + ".bed")
    capsys.readouterr()
    assembly_qv.main(argv + ["--spectrum", str(spectrum), "--absent-bed", str(bed)])
    out = capsys.readouterr().out
    assert not os.path.exists(str(bed) + ".tmp") and not os.path.exists(str(spectrum) + ".tmp")
    return out, spectrum.read_text(), bed.read_text()


def test_the_tables_byte_for_byte(world, capsys, tmp_path):
    want = _expected(world["db"], world["contigs"])
    assert _run([world["fa"], world["db_path"]], tmp_path, capsys, "plain") == want
    assert _run([world["fa_gz"], world["db_path"]], tmp_path, capsys, "gz") == want
    # what the expectation itself must look like
    rows = [line.split("\t") for line in want[0].splitlines()]
    assert [r[0] for r in rows] == ["perfect", "planted", "rough", "short", "reverse", "#total"]
    assert rows[0][2] == rows[0][3] == str(1500 - K + 1) and rows[0][4] == "inf"
    assert rows[3][1:] == [str(K - 1), "0", "0", "nan"] and rows[4][4] == "inf"
    assert int(rows[2][2]) == len(world["contigs"][2][1]) - K + 1 - K and int(rows[2][3]) == int(rows[2][2]) - 300  # the N costs k windows, the tail 300
    assert int(rows[5][5]) < int(rows[5][6]) == len(world["db"]) and rows[5][7].startswith("0.")
    assert want[1].splitlines()[0].split("\t")[0] == "2" and {line.split("\t")[1] for line in want[1].splitlines()} == {"0", "1", "2"}


def test_without_the_optional_files(world, capsys, tmp_path, monkeypatch):
    from trio_binning_amd import assembly_qv

    monkeypatch.chdir(tmp_path)
    capsys.readouterr()
    assembly_qv.main([world["fa"], world["db_path"]])
    assert capsys.readouterr().out == _expected(world["db"], world["contigs"])[0]
    assert os.listdir(tmp_path) == []


def test_cut_offs_change_found_and_solid(world, capsys, tmp_path):
    want = _expected(world["db"], world["contigs"], 50, 200)
    assert _run([world["fa"], world["db_path"], "--min-count", "50", "--max-count", "200"], tmp_path, capsys, "cuts") == want
    plain = _expected(world["db"], world["contigs"])
    assert want[0] != plain[0] and want[1] == plain[1] and want[2] == plain[2]  # found and solid move; the spectrum and the absent loci do not
    assert int(want[0].splitlines()[-1].split("\t")[6]) < len(world["db"])


def test_a_perfect_assembly_gives_inf(world, capsys, tmp_path):
    out, _, bed = _run([world["perfect_fa"], world["db_path"]], tmp_path, capsys, "perfect")
    rows = [line.split("\t") for line in out.splitlines()]
    assert [r[4] for r in rows] == ["inf", "inf", "inf"] and rows[2][8] == "0.00000e+00" and bed == ""
    assert (out, bed) == _expected(world["db"], world["contigs"][:1] + world["contigs"][4:])[::2]


def test_one_substitution_is_k_absent_windows_in_one_bed_line(world, capsys, tmp_path):
    fa = _fasta(tmp_path / "planted.fa", world["contigs"][1:2])
    out, _, bed = _run([fa, world["db_path"]], tmp_path, capsys, "planted")
    assert bed == "planted\t{}\t{}\t{}\n".format(700 - K + 1, 700 + K, K)
    row = out.splitlines()[0].split("\t")
    assert int(row[2]) - int(row[3]) == K and (out, bed) == _expected(world["db"], world["contigs"][1:2])[::2]
