"""The searched order of the canonical 4-mers that mod-sampling ranks at t = 4 (csrc/tbk_tmer_order.h, written by
tools/tmer_order_search.cpp): the table's format, tbk_tmer_rank and the strand symmetry of the buckets a key may select
(tests/native/tmer_order_check.cpp over csrc/tbk_common.h), and the sampling density the order was searched for.  No GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trio_binning_amd", "csrc")


def _table():
    text = open(os.path.join(CSRC, "tbk_tmer_order.h")).read()
    body = text[text.index("tbk_tmer4_ranks[256] = {"):]
    return [int(v, 16) for v in re.findall(r"0x([0-9A-Fa-f]+)u", body[: body.index("};")])]


def _rc4(x):
    y = 0
    for i in range(4):
        y |= (3 - ((x >> (2 * i)) & 3)) << (2 * (3 - i))
    return y


def test_table_is_a_function_of_the_canonical_4mer():
    r = _table()
    assert len(r) == 256
    assert all(r[x] == r[_rc4(x)] for x in range(256))
    assert all(v & 31 == 0 for v in r)
    canon = [x for x in range(256) if x <= _rc4(x)]
    assert len(canon) == 136 and len({r[x] for x in canon}) == 136   # one rank per canonical 4-mer: no ties between different ones


def test_rank_and_strand_flips(tmp_path):
    exe = str(tmp_path / "tmer_order_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "tmer_order_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "ok table" in r.stdout and "ok rank" in r.stdout and r.stdout.count("ok strands") == 4, r.stdout


@pytest.fixture(scope="module")
def search_tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tmer_order_search") / "tmer_order_search")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tools", "tmer_order_search.cpp")], check=True)
    return exe


def test_compiled_order_samples_fewer_lines_than_the_hash_order(search_tool):
    # no search (--iters 0): the tool scores the hash order on held-out sequence, and the order compiled into tbk_common.h
    # through tbk_tmer_rank / tbk_bucket_candidates on the same bases
    r = subprocess.run([search_tool, "--iters", "0", "--train", "100000", "--test", "2000000", "--distinct", "2000000"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    held = re.search(r"held-out \d+ random bases: lanes ([0-9.]+) -> ([0-9.]+).*continuous ([0-9.]+) -> ([0-9.]+), tie rate ([0-9.]+)", r.stdout)
    comp = re.search(r"compiled-in order .*: lanes ([0-9.]+), continuous ([0-9.]+), tie rate ([0-9.]+)", r.stdout)
    assert held and comp, r.stdout
    hash_lanes, hash_cont, hash_ties = float(held.group(1)), float(held.group(3)), float(held.group(5))
    lanes, cont, ties = (float(comp.group(i)) for i in (1, 2, 3))
    assert 0.215 < hash_lanes < 0.231, r.stdout                       # the hash order: 4 / (3w + 1) = 0.2105 plus the lanes' first windows
    assert lanes <= 0.975 * hash_lanes and cont <= 0.975 * hash_cont, r.stdout
    assert ties <= 1.05 * hash_ties, r.stdout
