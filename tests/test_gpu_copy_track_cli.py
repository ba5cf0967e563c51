"""python -m trio_binning_amd.copy_track on "contigs" cut from one synthetic genome - a plain one, one that holds a stretch of the
first again (a duplication), one with an N, a soft-masked stretch and a tail the reads never saw, a short one and a reverse
strand - against a crafted count database (tests/db_query_ref.database_bytes) in which a stretch is read twice as deep as the
rest (a collapse).  stdout and the --track file are compared byte for byte with what tests/copy_track_ref.py formats from its
loop reference."""
import gzip
import os

import numpy as np
import pytest

import copy_track_ref as ctr
import db_query_ref as ref

pytestmark = pytest.mark.gpu

K = 21
ERRORS = {2: 60, 3: 30, 4: 10, 5: 4, 6: 5, 7: 6, 8: 8, 9: 10, 10: 12, 11: 14, 14: 3}


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _fasta(path, records, gz=False, width=70):
    text = "".join(">{} made up\n{}\n".format(name, "\n".join(s[i:i + width] for i in range(0, len(s), width))) for name, s in records)
    with (gzip.open if gz else open)(path, "wb") as fh:
        fh.write(text.encode())
    return str(path)


@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    root = tmp_path_factory.mktemp("copy_track")
    rng = np.random.default_rng(78)
    genome = _seq(rng, 4000)
    unseen = _seq(rng, 300)
    windows = ref.window_kmers(genome, K)
    assert len(set(windows)) == len(windows)
    # one-copy depth 12; windows 500..799 read twice as deep; 900..909 capped
    db = {km: 255 if 900 <= i < 910 else 24 if 500 <= i < 800 else 12 + (i % 3 == 0) for i, km in enumerate(windows)}
    # k-mers of sequencing errors, which no contig holds: the falling head of the histogram and the valley in front of the peak
    for counter, n in ERRORS.items():
        for _ in range(n):
            db[ref.canonical(_seq(rng, K))] = counter
    assert len(db) == len(windows) + sum(ERRORS.values())
    rough = genome[2400:2900] + "N" + genome[2901:3200].lower() + genome[3200:3500] + unseen
    contigs = [("plain", genome[:1500]), ("again", genome[1450:2500] + genome[100:400]), ("rough", rough), ("short", genome[10:10 + K - 1]),
               ("reverse", ref.revcomp(genome[3000:3900]))]
    path = root / "reads.tbkdb"
    path.write_bytes(ref.database_bytes(db, K))
    return {"root": root, "db": db, "db_path": str(path), "contigs": contigs, "fa": _fasta(root / "asm.fa", contigs),
            "fa_gz": _fasta(root / "asm.fa.gz", contigs, gz=True)}


def _expected(db, records, window, peak):
    tally = ref.Tally(db)
    sequences = [s for _, s in records]
    tally.add(sequences, K)
    return ctr.command_tables([name for name, _ in records], [len(s) for s in sequences], ctr.track(tally, sequences, K, window, peak), window, peak)


def _run(argv, tmp_path, capsys, tag):
    from trio_binning_amd import copy_track

    track = tmp_path / (tag + ".track")
    capsys.readouterr()
    copy_track.main(argv + ["--track", str(track)])
    got = capsys.readouterr()
    assert not os.path.exists(str(track) + ".tmp")
    return got.out, track.read_text(), got.err


def test_the_tables_byte_for_byte(world, capsys, tmp_path):
    want = _expected(world["db"], world["contigs"], 100, 12)
    for tag, fa in (("plain", world["fa"]), ("gz", world["fa_gz"])):
        out, track, err = _run([fa, world["db_path"], "--window", "100", "--peak", "12"], tmp_path, capsys, tag)
        assert (out, track) == want and "one-copy read depth" not in err
    # what the expectation itself must look like
    rows = {r[0]: [int(x) for x in r[1:]] for r in (line.split("\t") for line in want[0].splitlines())}
    assert list(rows) == ["plain", "again", "rough", "short", "reverse", "#total"]
    assert rows["plain"][:3] == [1500, 1480, 0] and rows["plain"][3] == 10  # clean, nothing absent, the ten capped windows
    assert rows["plain"][4] >= 300 and rows["plain"][5] >= 280  # the stretch read twice as deep; the stretch `again` repeats
    assert rows["again"][5] >= 280 + 30 and rows["short"] == [K - 1, 0, 0, 0, 0, 0]
    assert 280 <= rows["rough"][2] <= 300 and rows["#total"][-2:] == [12, 100]
    lines = [line.split("\t") for line in want[1].splitlines()]
    assert [line[:3] for line in lines[:2]] == [["plain", "0", "100"], ["plain", "100", "200"]]
    assert lines[14][:3] == ["plain", "1400", "1500"] and lines[15][0] == "again"  # the last bin ends with the sequence
    assert lines[5][6:8] == ["24", "1"] and lines[2][6:8] == ["12", "2"]  # depth and copies: the collapse, the duplication
    assert not any(line[0] == "short" for line in lines)


def test_the_default_window_and_no_track_file(world, capsys, tmp_path, monkeypatch):
    from trio_binning_amd import copy_track

    monkeypatch.chdir(tmp_path)
    capsys.readouterr()
    copy_track.main([world["fa"], world["db_path"], "--peak", "12"])
    assert capsys.readouterr().out == _expected(world["db"], world["contigs"], 10000, 12)[0]
    assert os.listdir(tmp_path) == []


def test_the_default_peak_is_chosen_and_printed(world, capsys, tmp_path):
    """The header's rows fall from 2 to 5 (4 k-mers) and rise from 6: lo = 5.  Row 14 (3) is the first behind it below 4: hi = 14.
    Rows 12 and 13 hold most of the database and 12 holds more; row 24, the stretch read twice, lies outside."""
    from trio_binning_amd import kmers

    hist = kmers.database_file_info(world["db_path"])["histogram"]
    assert int(hist[12]) > int(hist[13]) > int(hist[24]) > 0
    out, track, err = _run([world["fa"], world["db_path"], "--window", "64"], tmp_path, capsys, "default")
    assert "Using 12 as the one-copy read depth" in err
    assert (out, track) == _expected(world["db"], world["contigs"], 64, 12)


def test_many_records_in_small_batches(world, capsys, tmp_path, monkeypatch):
    """A multi-record file read in several batches: pass 1 has counted every batch before pass 2 reads the first one back."""
    from trio_binning_amd import copy_track

    rng = np.random.default_rng(5)
    records = [("r{}".format(i), world["contigs"][i % 5][1][int(rng.integers(0, 40)):]) for i in range(23)] + [("none", ""), ("n", "N" * 30)]
    fa = _fasta(tmp_path / "many.fa.gz", [r for r in records if r[1]], gz=True)
    records = [r for r in records if r[1]]
    monkeypatch.setattr(copy_track, "_BATCH_BASES", 3000)
    monkeypatch.setattr(copy_track, "_BATCH_READS", 4)
    out, track, _ = _run([fa, world["db_path"], "--window", "333", "--peak", "12"], tmp_path, capsys, "many")
    want = _expected(world["db"], records, 333, 12)
    assert (out, track) == want
    assert int(want[0].splitlines()[-1].split("\t")[6]) > 1000  # five copies of everything: expanded all over


def test_a_failing_run_leaves_no_tmp_file(world, capsys, tmp_path, monkeypatch):
    from trio_binning_amd import copy_track, kmers

    def broken(self, *args, **kwargs):
        raise RuntimeError("made to fail")

    track = tmp_path / "fails.track"
    monkeypatch.setattr(kmers.DatabaseQuery, "track", broken)
    with pytest.raises(RuntimeError, match="made to fail"):
        copy_track.main([world["fa"], world["db_path"], "--peak", "12", "--track", str(track)])
    assert not track.exists() and not os.path.exists(str(track) + ".tmp")
