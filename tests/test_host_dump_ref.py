"""Counted k-mer dumps without a device: tests/dump_ref.py (the rule the GPU tests hold the importer and exporter to) against
the oracle's counter, tbk_dump_file_k, the argument refusals of import_database and dump_database, and the host pieces of
csrc/tbk_dump_text.h in a stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dump_ref as ref
import kmerdb_files as kf
from conftest import ROOT
from oracle import unique_oracle as uo


def _reads(rng, n=60):
    """reads over a few repeated sequences, so that counts spread from 1 to well past 255; some N and lower case"""
    units = ["".join("ACGT"[c] for c in rng.integers(0, 4, int(rng.integers(5, 40)))) for _ in range(6)]
    reads = []
    for i in range(n):
        s = "".join(units[int(u)] for u in rng.integers(0, len(units), int(rng.integers(1, 30))))
        if i % 7 == 0:
            s = s[:len(s) // 2] + "N" + s[len(s) // 2:]
        reads.append(s.lower() if i % 11 == 0 else s)
    reads += ["".join("ACGT"[c] for c in rng.integers(0, 4, 80)) for _ in range(5)]  # (k-mers seen once)
    return reads + ["A" * 400, "ACGT" * 90]


@pytest.mark.parametrize("k", [1, 2, 5, 15, 21, 31, 32])
def test_reference_equals_the_oracles_counter(k):
    rng = np.random.default_rng(100 + k)
    reads = _reads(rng)
    counted = uo.count_kmers(reads, k)
    keys, counts = uo.count_kmers_np(*uo.pack(reads), k)
    assert {ref.rank(s): c for s, c in counted.items()} == dict(zip(keys.tolist(), counts.tolist()))
    assert counts.max() > 255 and (counts.min() == 1 or k < 8)
    # the full dump of the oracle's counts, as kmc -ci1 -cs255 and kmc_dump would print it
    text = ref.format(keys, np.minimum(counts, 255), k)
    assert text == "".join("{}\t{}\n".format(s, min(c, 255)) for s, c in sorted(counted.items())).encode()
    pk, pc = ref.parse(text, k)
    assert np.array_equal(pk, keys) and np.array_equal(pc, np.minimum(counts, 255))
    want_keys, want_counts, want_hist = kf.database_of(keys, counts)
    got = ref.database(pk, pc, 2)
    assert np.array_equal(got[0], want_keys) and np.array_equal(got[1], want_counts) and np.array_equal(got[2], want_hist)
    assert dict(zip(uo.kmer_strings(got[0], k), got[1].tolist())) == uo.database(counted)
    full = ref.database(pk, pc, 1)
    assert np.array_equal(full[0], keys) and np.array_equal(full[1], np.minimum(counts, 255).astype(np.uint8))
    assert full[2][0] == keys.size and full[2][1:].sum() == keys.size and np.array_equal(full[2][1:], want_hist[1:])
    assert ref.database(pk, pc)[3] == (1 if (counts == 1).any() else 2)
    # both strands with the counter split, shuffled: the same database
    lines = []
    for s, c in counted.items():
        c = min(c, 255)
        rc = ref.revcomp(s)
        lines += [(s, c)] if c == 1 or rc == s else [(s, c // 2), (rc, c - c // 2)]
    order = rng.permutation(len(lines))
    split = "".join("{} {}\n".format(*lines[i]) for i in order).encode()
    again = ref.database(*ref.parse(split, k), 1)
    assert all(np.array_equal(a, b) for a, b in zip(again[:3], full[:3]))
    # ranges of the export
    for lo, hi in ((2, 255), (3, 7), (255, 255), (7, 3)):
        want = "".join("{}\t{}\n".format(s, min(c, 255)) for s, c in sorted(counted.items()) if lo <= min(c, 255) <= hi).encode()
        assert ref.format(full[0], full[1], k, lo, hi) == want


def test_reference_refusals():
    k = 4
    ok = b"ACGT\t3\n"
    cases = {
        b"ACGT\t\t3\n": ref.NOT_DIGITS, b"ACGT3\n": ref.NO_SEPARATOR, b"ACGT\n": ref.NO_COUNTER, b"ACG\t3\n": ref.SHORT_KMER,
        b"ACGTA\t3\n": ref.LONG_KMER, b"ACNT\t3\n": ref.NOT_ACGT, b"ACgT\t3\n": ref.NOT_ACGT, b"ACGT\t3\r\n": ref.NOT_DIGITS,
        b"\n": ref.EMPTY, b"ACGT\t0\n": ref.ZERO, b"ACGT\t000\n": ref.ZERO, b"ACGT\t-1\n": ref.NOT_DIGITS, b"ACGT\t\n": ref.EMPTY_COUNTER,
        b"ACGT\t" + b"1" * 33 + b"\n": ref.TOO_MANY_DIGITS, b"ACGT\t" + b"1" * 40 + b"\n": ref.TOO_LONG, b"AC\n": ref.SHORT_KMER,
    }
    for line, reason in cases.items():
        with pytest.raises(ref.DumpError) as exc:
            ref.parse(ok * 3 + line + ok, k)
        assert (exc.value.line_no, exc.value.reason) == (4, reason), line
    assert ref.parse(ok + b"AACG 9", k)[1].tolist() == [3, 9]
    with pytest.raises(ref.DumpError) as exc:
        ref.parse(ok + b"AACG 9\n", k, compressed=True)
    assert (exc.value.line_no, exc.value.reason) == (2, ref.NOT_COMPRESSED)
    assert ref.parse(b"", k)[0].size == 0
    assert ref.parse(b"TTTT\t" + b"9" * 32 + b"\n" + b"ACGT 007\n", k)[1].tolist() == [255, 7]
    assert ref.parse(b"TTTT\t1\n", k)[0].tolist() == [0]  # (canonical: AAAA)


def _write(tmp_path, name, data):
    path = tmp_path / name
    path.write_bytes(data)
    return str(path)


def test_dump_file_k(built, tmp_path):
    from trio_binning_amd import _lib, kmers

    assert _lib.HAS_DUMP
    assert kmers.dump_file_k(_write(tmp_path, "tab.txt", b"ACGTACGTACGTACGTACGTA\t17\nAC\t1\n")) == 21
    assert kmers.dump_file_k(_write(tmp_path, "space.txt", b"ACGTA 17")) == 5
    assert kmers.dump_file_k(_write(tmp_path, "k32.txt", b"A" * 32 + b"\t1\n")) == 32
    with pytest.raises(ValueError, match="empty"):
        kmers.dump_file_k(_write(tmp_path, "empty.txt", b""))
    with pytest.raises(ValueError, match="line 1"):
        kmers.dump_file_k(_write(tmp_path, "nosep.txt", b"ACGTACGT\nACGT\t1\n"))
    with pytest.raises(ValueError, match="1..32"):
        kmers.dump_file_k(_write(tmp_path, "k33.txt", b"A" * 33 + b"\t1\n"))
    with pytest.raises(ValueError, match="1..32"):
        kmers.dump_file_k(_write(tmp_path, "k0.txt", b"\t1\n"))
    with pytest.raises(IOError):
        kmers.dump_file_k(str(tmp_path / "missing.txt"))


def test_import_database_refuses_arguments(built, tmp_path, capsys):
    from trio_binning_amd import import_database as cli

    dump = _write(tmp_path, "a.txt", b"ACGT\t3\n")
    out = str(tmp_path / "a.tbkdb")
    args = cli.parse_args(["-o", out, "--floor", "2", "--reads", "5", "--bases", "50", dump + "," + dump])
    assert (args.floor, args.k, args.reads, args.bases, args.dumps) == (2, None, 5, 50, [dump, dump])
    assert cli.parse_args(["-o", out, "-k", "32", dump]).floor == "auto"
    for argv, words in (
        (["-o", out, str(tmp_path / "missing.txt")], "does not exist"),
        (["-o", out, "--floor", "3", dump], "--floor 3"),
        (["-o", out, "-k", "33", dump], "-k 33"),
        (["-o", out, "-k", "0", dump], "-k 0"),
        (["-o", out, "--reads", "5", dump], "--reads and --bases"),
        (["-o", out, "--bases", "5", dump], "--reads and --bases"),
        (["-o", str(tmp_path / "a.db"), dump], ".tbkdb"),
    ):
        with pytest.raises(SystemExit) as exc:
            cli.parse_args(argv)
        assert exc.value.code not in (0, None)
        assert words in capsys.readouterr().err + str(exc.value.code), argv


def test_dump_database_refuses_arguments(built, tmp_path, capsys):
    from trio_binning_amd import dump_database as cli

    data, _keys, _counts, _hist = kf.sound()
    db = _write(tmp_path, "a.tbkdb", data)
    out = str(tmp_path / "a.txt")
    args = cli.parse_args([db, "-o", out, "--min-count", "3"])
    assert (args.min_count, args.max_count, args.info["k"]) == (3, 255, 21)
    for argv, words in (
        ([str(tmp_path / "missing.tbkdb"), "-o", out], "does not exist"),
        ([_write(tmp_path, "bad.tbkdb", data[:1000]), "-o", out], "bad.tbkdb"),
        ([db, "-o", out, "--min-count", "-1"], "not negative"),
        ([db], "-o"),
    ):
        with pytest.raises(SystemExit) as exc:
            cli.parse_args(argv)
        assert exc.value.code not in (0, None)
        assert words in capsys.readouterr().err + str(exc.value.code), argv


def test_host_pieces_under_sanitizers(tmp_path):
    """Window cutting over a mapped file, k of the first line, the export's length prefix sum and formatter: a stand-alone
    program with its own main, built with AddressSanitizer and UBSan for the CPU."""
    exe = str(tmp_path / "dump_text_check")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                            os.path.join(ROOT, "trio_binning_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "native", "dump_text_check.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, str(tmp_path / "scratch.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
