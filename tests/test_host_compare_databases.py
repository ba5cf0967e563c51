"""compare-databases without a GPU: the numpy restatement of the two spectra (tests/db_compare_ref.py) against the properties
they have by construction, the arithmetic from spectra to the report's lines on hand-written spectra, the --matrix and
--spectra files there and back, and every refusal of the command line from crafted headers alone, with the library's device
entry points patched to raise."""
import contextlib
from unittest.mock import patch

import numpy as np
import pytest

import db_compare_ref as ref
import kmerdb_files as kf
from test_host_kmerdb_full import FULL_HPC, full_file

DEVICE_ENTRIES = ("tbk_kmerdb_load", "tbk_kmerdb_solid", "tbk_kmerdb_joint_spectrum", "tbk_kmerdb_origin_spectrum", "tbk_kmerdb_read",
                  "tbk_kmerdb_unique_table", "tbk_kmerdb_inherited_table")


@contextlib.contextmanager
def no_device():
    """every device entry point a comparison could reach raises"""
    from trio_binning_amd import _lib

    with contextlib.ExitStack() as stack:
        for name in DEVICE_ENTRIES:
            stack.enter_context(patch.object(_lib.lib, name, side_effect=AssertionError("the device was touched: " + name)))
        yield


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def _random_db(rng, n, floor, top=4000):
    keys = np.sort(rng.choice(top, size=n, replace=False)).astype(np.uint64)
    return keys, rng.integers(floor, 256, n).astype(np.uint8)


@pytest.mark.parametrize("seed", range(6))
def test_the_reference_has_the_properties_of_its_definition(seed):
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 700, 2500]
    (x, cx), (y, cy), (z, cz) = (_random_db(rng, sizes[int(rng.integers(0, 4))] if seed else 700, floor) for floor in (1, 2, 1))
    spec = ref.joint_spectrum(x, cx, y, cy)
    ref.check_joint_invariants(spec, cx, cy, np.union1d(x, y).size)
    assert np.array_equal(ref.joint_spectrum(y, cy, x, cx), spec.T)
    shared = np.intersect1d(x, y)
    assert int(spec[1:, 1:].sum()) == shared.size and int(spec[1:, 0].sum()) == x.size - shared.size
    for y_range, z_range in (((1, 255), (1, 255)), ((2, 255), (2, 255)), ((7, 7), (100, 255))):
        table = ref.origin_spectrum(x, cx, y, cy, y_range, z, cz, z_range)
        ref.check_origin_invariants(table, cx)
        in_y = np.isin(x, y[(cy >= y_range[0]) & (cy <= y_range[1])])
        in_z = np.isin(x, z[(cz >= z_range[0]) & (cz <= z_range[1])])
        assert [int(t.sum()) for t in table] == [int((~in_y & ~in_z).sum()), int((in_y & ~in_z).sum()), int((~in_y & in_z).sum()), int((in_y & in_z).sum())]
    # the joint spectrum's columns are an origin spectrum's classes summed: entries of x that y holds at all
    table = ref.origin_spectrum(x, cx, y, cy, (1, 255), z[:0], cz[:0], (1, 255))
    assert np.array_equal(table[1, 1:], spec[1:, 1:].sum(axis=1)) and np.array_equal(table[0], spec[:, 0]) and not table[2:].any()


def test_the_reference_on_a_hand_made_pair():
    x, cx = np.array([3, 5, 9, 11], dtype=np.uint64), np.array([1, 2, 2, 255], dtype=np.uint8)
    y, cy = np.array([5, 9, 10], dtype=np.uint64), np.array([7, 2, 1], dtype=np.uint8)
    spec = ref.joint_spectrum(x, cx, y, cy)
    want = {(1, 0): 1, (2, 7): 1, (2, 2): 1, (255, 0): 1, (0, 1): 1}
    assert {(int(i), int(j)): int(spec[i, j]) for i, j in zip(*np.nonzero(spec))} == want
    table = ref.origin_spectrum(x, cx, y, cy, (2, 255), y, cy, (1, 2))
    assert {(int(i), int(j)): int(table[i, j]) for i, j in zip(*np.nonzero(table))} == {(0, 1): 1, (1, 2): 1, (3, 2): 1, (0, 255): 1}


# ---- from spectra to lines ----------------------------------------------------------------------------------------------------------
def test_report_two_on_a_hand_written_spectrum(built):
    from trio_binning_amd import compare_databases as cd

    spec = np.zeros((256, 256), dtype=np.uint64)
    spec[1, 0], spec[30, 31], spec[255, 255], spec[2, 0], spec[0, 1], spec[0, 40] = 5, 100, 3, 2, 10, 30
    # x: 5 + 100 + 3 + 2 = 110; y: 100 + 3 + 10 + 30 = 143; shared 103; union 150
    assert cd.report_two(spec, 21, False, 1, 2) == [
        "k\t21", "space\tplain", "floor_x\t1", "floor_y\t2", "kmers_x\t110", "kmers_y\t143", "shared\t103", "only_x\t7", "only_y\t40", "union\t150",
        "jaccard\t0.686667", "containment_x_in_y\t0.936364", "containment_y_in_x\t0.720280"]
    assert cd.report_two(spec.ravel(), 21, False, 1, 2) == cd.report_two(spec, 21, False, 1, 2)  # the C array's shape is taken too
    empty = np.zeros((256, 256), dtype=np.uint64)
    assert cd.report_two(empty, 32, True, 2, 2) == [
        "k\t32", "space\tcompressed", "floor_x\t2", "floor_y\t2", "kmers_x\t0", "kmers_y\t0", "shared\t0", "only_x\t0", "only_y\t0", "union\t0",
        "jaccard\tnan", "containment_x_in_y\tnan", "containment_y_in_x\tnan"]
    only_y = empty.copy()
    only_y[0, 9] = 4
    lines = cd.report_two(only_y, 21, False, 2, 2)
    assert lines[4:] == ["kmers_x\t0", "kmers_y\t4", "shared\t0", "only_x\t0", "only_y\t4", "union\t4", "jaccard\t0.000000", "containment_x_in_y\tnan",
                         "containment_y_in_x\t0.000000"]


def test_report_trio_on_hand_written_spectra(built):
    from trio_binning_amd import compare_databases as cd

    child, a, b = (np.zeros((4, 256), dtype=np.uint64) for _ in range(3))
    # the child: counters 2 (below its cut-off 3), 3 and 255
    child[0, 2], child[3, 2] = 1000, 7
    child[0, 3], child[1, 3], child[2, 3], child[3, 3] = 2, 30, 40, 500
    child[0, 255], child[3, 255] = 1, 27
    # A in [4, 6]: counter 3 and 7 lie outside
    a[0, 3], a[2, 3], a[0, 7], a[2, 7] = 900, 1, 50, 50
    a[0, 4], a[1, 4], a[2, 4], a[3, 4] = 10, 100, 9, 200
    a[0, 6], a[2, 6] = 30, 31
    # B in [2, 300]: everything it has, the upper bound clamped to 255
    b[0, 2], b[2, 2], b[1, 2] = 8, 2, 77
    b[2, 255], b[3, 255] = 5, 6
    assert cd.report_trio(child, a, b, 21, False, (4, 6), (2, 300), 3) == [
        "k\t21", "space\tplain", "range_a\t4,6", "range_b\t2,300", "min_count_child\t3",
        "child_solid\t600", "child_in_both\t527", "child_only_a\t30", "child_only_b\t40", "child_in_neither\t3", "child_in_neither_share\t0.005000",
        "unique_a\t80", "inherited_a\t40", "inherited_a_share\t0.500000",
        "unique_b\t15", "inherited_b\t7", "inherited_b_share\t0.466667"]
    zero = np.zeros((4, 256), dtype=np.uint64)
    assert cd.report_trio(zero, zero, zero, 16, True, (2, 255), (2, 255), 2) == [
        "k\t16", "space\tcompressed", "range_a\t2,255", "range_b\t2,255", "min_count_child\t2",
        "child_solid\t0", "child_in_both\t0", "child_only_a\t0", "child_only_b\t0", "child_in_neither\t0", "child_in_neither_share\tnan",
        "unique_a\t0", "inherited_a\t0", "inherited_a_share\tnan", "unique_b\t0", "inherited_b\t0", "inherited_b_share\tnan"]


# ---- the files ----------------------------------------------------------------------------------------------------------------------
def test_the_matrix_and_the_spectra_come_back_as_written(built, tmp_path):
    from trio_binning_amd import compare_databases as cd

    rng = np.random.default_rng(3)
    spec = rng.integers(0, 1 << 40, (256, 256)).astype(np.uint64)
    spec[0, 0], spec[255, 255], spec[0, 255] = 0, (1 << 64) - 1, 1 << 63
    path = str(tmp_path / "joint.tsv")
    cd.write_matrix(path, spec, "x.tbkdb", "dir/y.tbkdb", 1, 2)
    lines = open(path).read().split("\n")
    head = [l for l in lines if l.startswith("#")]
    assert lines[:len(head)] == head and "x = x.tbkdb (floor 1)" in head[1] and "y = dir/y.tbkdb (floor 2)" in head[2] and "row 0" in head[3] and "column 0" in head[3]
    body = lines[len(head):]
    assert body[-1] == "" and len(body) == 257 and all(len(l.split("\t")) == 256 for l in body[:-1])
    assert body[255].split("\t")[255] == str((1 << 64) - 1)
    assert np.array_equal(cd.read_matrix(path), spec)
    with open(path, "a") as fh:
        fh.write("\t".join(["0"] * 256) + "\n")
    with pytest.raises(ValueError, match="not 256 x 256"):
        cd.read_matrix(path)

    tables = [("base = child c.tbkdb; first = A a.tbkdb [2,255]; second = B b.tbkdb [2,255]", rng.integers(0, 1 << 50, (4, 256)).astype(np.uint64)),
              ("base = A a.tbkdb; first = B b.tbkdb [2,255]; second = child c.tbkdb [4,255]", np.zeros((4, 256), dtype=np.uint64)),
              ("base = B b.tbkdb; first = A a.tbkdb [2,255]; second = child c.tbkdb [4,255]", rng.integers(0, 3, (4, 256)).astype(np.uint64))]
    tables[0][1][3, 255] = (1 << 64) - 1
    path = str(tmp_path / "trio.tsv")
    cd.write_spectra(path, tables)
    lines = open(path).read().split("\n")
    assert len(lines) == 3 * 258 + 1 and lines[0] == "# " + tables[0][0] and lines[1] == "# counter\tneither\tfirst_only\tsecond_only\tboth"
    assert lines[2].split("\t")[0] == "0" and lines[257].split("\t") == ["255"] + [str(int(v)) for v in tables[0][1][:, 255]]
    back = cd.read_spectra(path)
    assert [t for t, _ in back] == [t for t, _ in tables] and all(np.array_equal(g, w) and g.dtype == np.uint64 for (_, g), (_, w) in zip(back, tables))


# ---- the command line ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def dbs(tmp_path):
    files = {
        "full": full_file(k=21, seed=2)[0],
        "full16": full_file(k=16, seed=2)[0],
        "fullh": full_file(k=21, seed=2, magic=FULL_HPC)[0],
        "solid": kf.sound(k=21, n=40, seed=3)[0],
        "solid2": kf.sound(k=21, n=30, seed=4)[0],
        "solid16": kf.sound(k=16, n=30, seed=4)[0],
        "damaged": kf.sound(k=21, n=40, seed=3)[0][:-3],
    }
    out = {}
    for name, data in files.items():
        out[name] = str(tmp_path / (name + ".tbkdb"))
        open(out[name], "wb").write(data)
    out["list"] = str(tmp_path / "hapA.txt")
    open(out["list"], "w").write("ACGTACGTACGTACGTACGTA\n")
    return out


def test_sound_command_lines_are_settled_from_the_headers(built, dbs):
    from trio_binning_amd import compare_databases as cd

    cut = ["--min-count-a", "3", "--max-count-a", "90", "--min-count-b", "2", "--max-count-b", "80"]
    with no_device():
        a = cd.parse_args([dbs["full"], dbs["solid"], "--matrix", "m.tsv"])
        assert a.databases is None and [i["floor"] for i in a.infos] == [1, 2] and a.matrix == "m.tsv" and a.infos[0]["k"] == 21
        a = cd.parse_args([dbs["solid"], dbs["solid2"], "--child-database", dbs["full"], "--spectra", "t.tsv", "--min-count-child", "4"] + cut)
        pair = a.databases
        assert (pair.ranges, pair.child_min, pair.child_path, pair.prog, pair.compressed, a.k) == ({"A": (3, 90), "B": (2, 80)}, 4, dbs["full"], "compare-databases", False, 21)
        assert cd.trio_titles(pair)[1] == "base = A {}; first = B {} [2,255]; second = child {} [4,255]".format(dbs["solid"], dbs["solid2"], dbs["full"])
        # and a sound command line goes on to the device
        with pytest.raises(AssertionError, match="the device was touched: tbk_kmerdb_load"):
            cd.main([dbs["full"], dbs["solid"]])
        with pytest.raises(AssertionError, match="the device was touched: tbk_kmerdb_load"):
            cd.main([dbs["solid"], dbs["solid2"], "--child-database", dbs["full"], "--min-count-child", "4"] + cut)


def test_every_refusal_comes_from_the_command_line_and_the_headers(built, dbs, capsys):
    from trio_binning_amd import compare_databases as cd

    cut = ["--min-count-a", "3", "--max-count-a", "90", "--min-count-b", "2", "--max-count-b", "80", "--min-count-child", "2"]
    child = ["--child-database", dbs["solid"]]
    cases = (
        # different k
        ([dbs["full"], dbs["full16"]], None, [dbs["full"], dbs["full16"], "21-mers", "16-mers"]),
        ([dbs["solid"], dbs["solid16"]] + child + cut, None, ["21-mers", "16-mers", "compare-databases"]),
        ([dbs["solid"], dbs["solid2"], "--child-database", dbs["solid16"]] + cut, None, [dbs["solid16"], "16-mers"]),
        # mixed spaces
        ([dbs["full"], dbs["fullh"]], None, [dbs["fullh"], "homopolymer-compressed", "plain"]),
        ([dbs["fullh"], dbs["solid"]], None, ["homopolymer-compressed", "plain"]),
        ([dbs["solid"], dbs["fullh"]] + child + cut, None, ["homopolymer-compressed", "plain", "compare-databases"]),
        ([dbs["solid"], dbs["solid2"], "--child-database", dbs["fullh"]] + cut, None, ["the child's", "homopolymer-compressed"]),
        # a path that is not *.tbkdb
        ([dbs["list"], dbs["solid"]], 2, [dbs["list"], "not a count database", ".tbkdb"]),
        ([dbs["solid"], dbs["list"]], 2, [dbs["list"], "not a count database"]),
        ([dbs["solid"], dbs["solid2"], "--child-database", dbs["list"]], 2, [dbs["list"], "not a count database"]),
        # the tables of the other mode
        ([dbs["solid"], dbs["solid2"], "--matrix", "m.tsv"] + child, 2, ["--matrix", "--spectra"]),
        ([dbs["solid"], dbs["solid2"], "--spectra", "t.tsv"], 2, ["--spectra", "--child-database"]),
        # the cut-off options without a child
        ([dbs["solid"], dbs["solid2"], "--min-count-a", "3", "--max-count-a", "9"], 2, ["--min-count-a", "--child-database"]),
        ([dbs["solid"], dbs["solid2"], "--max-count-b", "9"], 2, ["--max-count-b", "--child-database"]),
        ([dbs["solid"], dbs["solid2"], "--min-count-child", "3"], 2, ["--min-count-child", "--child-database"]),
        # cut-offs that cannot be
        ([dbs["solid"], dbs["solid2"], "--min-count-a", "3"] + child, 2, ["--min-count-a and --max-count-a go together"]),
        ([dbs["solid"], dbs["solid2"], "--min-count-a", "9", "--max-count-a", "3"] + child, 2, ["need 1 <= min <= max"]),
        ([dbs["solid"], dbs["solid2"], "--min-count-child", "256"] + child, 2, ["--min-count-child 256", "255"]),
        ([dbs["solid"], dbs["solid2"], "--min-count-child", "0"] + child, 2, ["--min-count-child 0"]),
        # files that are no databases, or are not there
        ([dbs["solid"], dbs["damaged"]], None, [dbs["damaged"], "compare-databases"]),
        ([dbs["solid"], dbs["solid"] + ".absent.tbkdb"], None, [".absent.tbkdb", "compare-databases"]),
        ([dbs["damaged"], dbs["solid"]] + child + cut, None, [dbs["damaged"], "compare-databases"]),
    )
    with no_device():
        for argv, code, words in cases:
            with pytest.raises(SystemExit) as ei:
                cd.main(argv)
            err = capsys.readouterr().err
            text = err if code == 2 else str(ei.value.code)
            assert (ei.value.code == 2) == (code == 2) and all(w in text for w in words), (argv, ei.value.code, err)
    assert capsys.readouterr().out == ""
