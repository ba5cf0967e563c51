"""python -m trio_binning_amd.repair_candidates on an "assembly" of a synthetic genome with planted one-base errors, against a
database made from the true genome (tests/db_query_ref.database_bytes): stdout and the --edits file byte for byte with what this
file formats from tests/repair_ref.py, the --apply output byte for byte the true genome, and assembly_qv's word on it."""
import gzip
import os

import numpy as np
import pytest

import db_query_ref as ref
import repair_ref as rr

pytestmark = pytest.mark.gpu

K = 21
SUPPORT = (K + 1) // 2  # the command's default
KIND = {rr.NONE: ".", rr.SUB: "sub", rr.DEL: "del", rr.INS: "ins", rr.LONG: "."}


def _genome(rng, n):
    """random, no two equal neighbouring bases: no homopolymer run, so every planted error has one left-aligned spelling"""
    out = ["ACGT"[int(rng.integers(0, 4))]]
    while len(out) < n:
        out.append([c for c in "ACGT" if c != out[-1]][int(rng.integers(0, 3))])
    return "".join(out)


def _fasta(path, records, gz=False, width=70):
    text = "".join(">{}\n{}\n".format(name, "\n".join(s[i:i + width] for i in range(0, len(s), width))) for name, s in records)
    with (gzip.open if gz else open)(path, "wb") as fh:
        fh.write(text.encode())
    return str(path)


def _plant(genome, errors):
    """the genome with (pos, kind, base) errors in its own coordinates - a substituted, a missing, an extra base - from the right"""
    s = list(genome)
    for pos, kind, base in sorted(errors, reverse=True):
        if kind == "sub":
            s[pos] = base
        elif kind == "missing":
            del s[pos]
        else:
            s.insert(pos, base)
    return "".join(s)


def _verdict(rec):
    return "long" if rec[5] == rr.LONG else "unmended" if rec[4] == 0 else "mended" if rec[4] == 1 else "ambiguous"


def _expected(db, contigs, min_count=2, min_support=SUPPORT):
    """(stdout, edits, [mended sequences], applied, conflicting) from the reference's records, formatted here"""
    names, sequences = [n for n, _ in contigs], [s for _, s in contigs]
    records = rr.repairs(db, sequences, K, min_count, min_support)
    out, edits, mended, total = [], [], [], [0] * 8
    for read, (name, s) in enumerate(contigs):
        own = [r for r in records if r[0] == read]
        row = [len(s), len(own)] + [sum(_verdict(r) == v for r in own) for v in ("mended", "ambiguous", "unmended", "long")]
        out.append("\t".join([name] + [str(v) for v in row]))
        for r in own:
            edit = r[5] in (rr.SUB, rr.DEL, rr.INS)
            edits.append("\t".join([name, str(r[1]), str(r[3]), _verdict(r), KIND[r[5]], str(r[2]) if edit else ".",
                                    s[r[2]].upper() if edit and r[5] != rr.INS else ".", chr(r[6]) if edit and r[5] != rr.DEL else ".",
                                    str(r[4]), str(r[7]), str(r[8])]))
        sure = sorted((r[2], r[5], chr(r[6]) if r[6] else "") for r in own if r[4] == 1)
        apart = [e for e in sure if all(o is e or abs(o[0] - e[0]) >= K for o in sure)]
        mended.append(rr.apply_edits(s, [(kind, pos, base) for pos, kind, base in apart]))
        total[6] += len(apart)
        total[7] += len(sure) - len(apart)
        for j in range(6):
            total[j] += row[j]
    out.append("\t".join(["#total"] + [str(v) for v in total[:6]] + [str(min_count), str(min_support)]))
    return "\n".join(out) + "\n", "".join(e + "\n" for e in edits), mended, total[6], total[7], records


@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    root = tmp_path_factory.mktemp("repair_candidates")
    rng = np.random.default_rng(2024)
    genome = _genome(rng, 6000)
    assert all(a != b for a, b in zip(genome, genome[1:]))
    db = {km: 12 for km in ref.window_kmers(genome, K)}
    errors = []
    for i in range(25):  # 230 >= 3 k apart
        pos, kind = 100 + 230 * i, ("sub", "missing", "extra")[i % 3]
        others = [c for c in "ACGT" if c != genome[pos] and (kind != "extra" or c != genome[pos - 1])]  # (an extra base makes no run)
        errors.append((pos, kind, others[int(rng.integers(0, len(others)))]))
    path = root / "reads.tbkdb"
    path.write_bytes(ref.database_bytes(db, K))
    return {"root": root, "genome": genome, "db": db, "db_path": str(path), "errors": errors, "assembly": _plant(genome, errors)}


def _run(argv, tmp_path, capsys, tag, apply=True):
    from trio_binning_amd import repair_candidates

    edits, mended = tmp_path / (tag + ".tsv"), tmp_path / (tag + ".fa")
    capsys.readouterr()
    repair_candidates.main(argv + ["--edits", str(edits)] + (["--apply", str(mended)] if apply else []))
    got = capsys.readouterr()
    assert not os.path.exists(str(edits) + ".tmp") and not os.path.exists(str(mended) + ".tmp")
    return got.out, edits.read_text(), mended.read_bytes() if apply else None


def test_every_planted_error_is_mended(world, capsys, tmp_path):
    from trio_binning_amd import assembly_qv

    genome, contigs = world["genome"], [("ctg1", world["assembly"])]
    out, edits, mended, applied, conflicting, records = _expected(world["db"], contigs)
    # the reference itself mends every planted error, and nothing else, without ambiguity: the inputs hide no failure
    assert len(records) == 25 and all(r[4] == 1 for r in records) and (applied, conflicting) == (25, 0) and mended == [genome]
    assert sorted({r[5] for r in records}) == [rr.SUB, rr.DEL, rr.INS] and all(r[7] == (K - 1 if r[5] == rr.DEL else K) for r in records)
    for tag, gz in (("plain", False), ("gz", True)):
        fa = _fasta(tmp_path / ("asm.fa" + (".gz" if gz else "")), contigs, gz=gz)
        got_out, got_edits, got_fa = _run([fa, world["db_path"]], tmp_path, capsys, tag)
        assert got_out == out[:-1] + "\t25\t0\n"  # with --apply the last line also says applied and conflicting
        assert got_out.splitlines()[0] == "ctg1\t{}\t25\t25\t0\t0\t0".format(len(world["assembly"]))  # every stretch is mended
        assert got_edits == edits and got_edits.count("\tmended\t") == 25
        assert got_fa == (">ctg1\n" + genome + "\n").encode()  # byte for byte the true genome
    # assembly_qv on the mended file: every clean window is found
    capsys.readouterr()
    assembly_qv.main([str(tmp_path / "gz.fa"), world["db_path"]])
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].split("\t")[4] == "inf" and lines[-1].split("\t")[4] == "inf"
    assembly_qv.main([_fasta(tmp_path / "before.fa", contigs), world["db_path"]])
    assert capsys.readouterr().out.splitlines()[0].split("\t")[4] not in ("inf", "nan")


def test_two_errors_five_bases_apart_and_other_contigs(world, capsys, tmp_path, monkeypatch):
    from trio_binning_amd import repair_candidates

    genome = world["genome"]
    near = _plant(genome[:1500], [(700, "sub", [c for c in "ACGT" if c != genome[700]][0]), (705, "sub", [c for c in "ACGT" if c != genome[705]][0])])
    soft = _plant(genome[1500:3000], [(400, "missing", "")])
    soft = soft[:380] + soft[380:420].lower() + soft[420:]  # lower case around the missing base: the inserted base is upper case, the rest stays
    contigs = [("near", near), ("soft_masked", soft), ("short", genome[10:10 + K - 1]), ("unseen", _genome(np.random.default_rng(3), 90)),
               ("reverse", ref.revcomp(_plant(genome[3000:4000], [(500, "extra", [c for c in "ACGT" if c not in genome[499:501]][0])])))]
    out, edits, mended, applied, conflicting, records = _expected(world["db"], contigs, 2, 3)
    verdicts = [_verdict(r) for r in records]
    assert verdicts.count("long") == 2 and verdicts.count("mended") == 2 and (applied, conflicting) == (2, 0)  # near and unseen are long
    assert mended[1] == genome[1500:1880] + genome[1880:1900].lower() + genome[1900] + genome[1901:1921].lower() + genome[1921:3000] and mended[4] == ref.revcomp(genome[3000:4000])
    fa = _fasta(tmp_path / "asm.fa", contigs)
    monkeypatch.setattr(repair_candidates, "_BATCH_BASES", 1600)  # several batches: the records' reads are those of their batch
    monkeypatch.setattr(repair_candidates, "_BATCH_READS", 2)
    got_out, got_edits, got_fa = _run([fa, world["db_path"], "--min-support", "3"], tmp_path, capsys, "several")
    assert got_out == out[:-1] + "\t{}\t{}\n".format(applied, conflicting) and got_edits == edits
    assert got_fa == "".join(">{}\n{}\n".format(name, s) for (name, _), s in zip(contigs, mended)).encode()
    # without --apply the last line ends with min_support
    got_out, got_edits, _ = _run([fa, world["db_path"], "--min-support", "3"], tmp_path, capsys, "tables", apply=False)
    assert got_out == out and got_edits == edits and not os.path.exists(tmp_path / "tables.fa")


def test_a_failing_run_leaves_no_tmp_file(world, capsys, tmp_path, monkeypatch):
    from trio_binning_amd import kmers, repair_candidates

    def broken(self, *args, **kwargs):
        raise RuntimeError("made to fail")

    fa = _fasta(tmp_path / "asm.fa", [("ctg1", world["assembly"])])
    edits, mended = tmp_path / "fails.tsv", tmp_path / "fails.fa"
    monkeypatch.setattr(kmers.DatabaseQuery, "repairs", broken)
    with pytest.raises(RuntimeError, match="made to fail"):
        repair_candidates.main([fa, world["db_path"], "--edits", str(edits), "--apply", str(mended)])
    for path in (edits, mended):
        assert not path.exists() and not os.path.exists(str(path) + ".tmp")
