"""What of the hit tracker needs no device: kmers.phase_blocks on hand-written runs, the refusals python -m
trio_binning_amd.phase_blocks makes from its arguments alone (every one before anything loads a list, loads a database or makes
a tracker - those entry points are replaced by ones that fail the test), and the new symbols of the built library."""
import ctypes as C
import os

import numpy as np
import pytest

import kmerdb_files as kf
from conftest import DATA


def _runs(*rows):
    from trio_binning_amd import kmers

    return np.array(list(rows), dtype=kmers.HIT_RUN_DTYPE)


def _blocks(rows, min_run):
    from trio_binning_amd import kmers

    return kmers.phase_blocks(_runs(*rows), min_run).tolist()


# (read, first, last, markers, hap)
def test_a_drop_makes_two_neighbours_merge(built):
    rows = [(0, 0, 40, 12, 0), (0, 55, 55, 1, 1), (0, 70, 200, 30, 0), (0, 300, 420, 25, 1)]
    assert _blocks(rows, 1) == rows
    assert _blocks(rows, 2) == [(0, 0, 200, 42, 0), (0, 300, 420, 25, 1)]


def test_the_drop_is_one_pass_and_is_not_repeated(built):
    # dropping the single B-marker merges two A-runs of 2 into a block of 4; the runs are judged before that, so min_run 3 drops both
    rows = [(0, 0, 1, 2, 0), (0, 5, 5, 1, 1), (0, 9, 10, 2, 0), (0, 20, 30, 5, 1)]
    assert _blocks(rows, 2) == [(0, 0, 10, 4, 0), (0, 20, 30, 5, 1)]
    assert _blocks(rows, 3) == [(0, 20, 30, 5, 1)]


def test_a_drop_at_a_reads_end(built):
    rows = [(0, 0, 90, 20, 0), (0, 95, 95, 1, 1), (1, 3, 3, 1, 1), (1, 10, 60, 8, 0)]
    assert _blocks(rows, 2) == [(0, 0, 90, 20, 0), (1, 10, 60, 8, 0)]


def test_no_merge_across_reads(built):
    rows = [(0, 0, 90, 20, 0), (1, 5, 60, 9, 0), (1, 70, 70, 1, 1), (2, 0, 10, 4, 0)]
    assert _blocks(rows, 1) == rows
    assert _blocks(rows, 2) == [(0, 0, 90, 20, 0), (1, 5, 60, 9, 0), (2, 0, 10, 4, 0)]


def test_min_run_above_every_run_and_empty_input(built):
    from trio_binning_amd import kmers

    rows = [(0, 0, 90, 20, 0), (1, 5, 60, 9, 1)]
    got = kmers.phase_blocks(_runs(*rows), 21)
    assert got.size == 0 and got.dtype == np.dtype(kmers.HIT_RUN_DTYPE)
    for min_run in (1, 5):
        got = kmers.phase_blocks(np.zeros(0, dtype=kmers.HIT_RUN_DTYPE), min_run)
        assert got.size == 0 and got.dtype == np.dtype(kmers.HIT_RUN_DTYPE)
    with pytest.raises(ValueError):
        kmers.phase_blocks(_runs(*rows), 0)


# ---- the command line's refusals ---------------------------------------------------------------------------------------------
@pytest.fixture()
def files(built, tmp_path, monkeypatch):
    from trio_binning_amd import kmers

    paths = {}
    for name, seed in (("a21", 1), ("b21", 2)):
        paths[name] = str(tmp_path / (name + ".tbkdb"))
        with open(paths[name], "wb") as fh:
            fh.write(kf.sound(k=21, n=5, seed=seed)[0])
    paths["list_a"], paths["list_b"] = os.path.join(DATA, "hapA.txt"), os.path.join(DATA, "hapB.txt")
    paths["fa"] = os.path.join(DATA, "test.fa")
    paths["bed"] = str(tmp_path / "out.bed")

    def touched(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were refused")

    monkeypatch.setattr(kmers, "create_kmer_hash_set", touched)
    monkeypatch.setattr(kmers.HashSet, "from_file", touched)
    monkeypatch.setattr(kmers.KmerDatabase, "load", touched)
    monkeypatch.setattr(kmers.KmerDatabase, "unique_set", touched)
    monkeypatch.setattr(kmers.HitTracker, "__init__", touched)
    return paths


def _exit(files, argv):
    from trio_binning_amd import phase_blocks

    with pytest.raises(SystemExit) as ei:
        phase_blocks.main(argv + ["--bed", files["bed"]])
    assert not os.path.exists(files["bed"]) and not os.path.exists(files["bed"] + ".tmp")
    return ei.value.code


@pytest.mark.parametrize("order", ["list_first", "database_first"])
def test_a_list_beside_a_database_is_refused(files, capsys, order):
    pair = [files["list_a"], files["b21"]] if order == "list_first" else [files["a21"], files["list_b"]]
    code = _exit(files, [files["fa"]] + pair)
    assert isinstance(code, str) and code.startswith("phase_blocks: ") and pair[0] in code and pair[1] in code
    assert "k-mer list" in code and "count database" in code
    assert capsys.readouterr().out == ""


def test_count_options_with_lists_are_refused(files, capsys):
    code = _exit(files, [files["fa"], files["list_a"], files["list_b"], "--min-count-a", "3", "--max-count-a", "30"])
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and "choose from a count database" in err
    code = _exit(files, [files["fa"], files["list_a"], files["list_b"], "--child-database", files["a21"]])
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and "--child-database selects from two count databases" in err


@pytest.mark.parametrize("value", ["0", "-3"])
def test_min_run_below_one_is_refused(files, capsys, value):
    code = _exit(files, [files["fa"], files["list_a"], files["list_b"], "--min-run", value])
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and "--min-run" in err and "1 <= N" in err


@pytest.mark.parametrize("missing", ["sequences", "list", "database", "child"])
def test_a_missing_file_is_refused(files, capsys, tmp_path, missing):
    gone = str(tmp_path / ("nothing.tbkdb" if missing in ("database", "child") else "nothing.txt"))
    cuts = ["--min-count-a", "2", "--max-count-a", "9", "--min-count-b", "2", "--max-count-b", "9"]
    argv = {"sequences": [gone, files["list_a"], files["list_b"]], "list": [files["fa"], files["list_a"], gone],
            "database": [files["fa"], gone, files["b21"]] + cuts,
            "child": [files["fa"], files["a21"], files["b21"], "--child-database", gone, "--min-count-child", "2"] + cuts}[missing]
    code = _exit(files, argv)
    assert isinstance(code, str) and code.startswith("phase_blocks: ") and gone in code and "does not exist" in code
    assert capsys.readouterr().out == ""


def test_help_says_whose_rule_min_run_is(built, capsys):
    from trio_binning_amd import phase_blocks

    with pytest.raises(SystemExit) as ei:
        phase_blocks.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert ei.value.code == 0 and "not Merqury's short-range-switch rule" in text


# ---- the library ------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_and_their_signatures(built):
    from trio_binning_amd import _lib, kmers

    assert _lib.HAS_HIT_TRACKER and _lib.lib.tbk_abi_version() == 1
    vp, u64 = C.c_void_p, C.c_uint64
    want = {
        "tbk_hit_tracker_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
        "tbk_hit_tracker_destroy": (None, [vp]),
        "tbk_hit_tracker_runs": (C.c_int, [vp, vp, vp, u64, C.c_int, C.POINTER(vp), C.POINTER(u64), vp]),
        "tbk_hit_tracker_marks": (C.c_int, [vp, vp, vp, u64, C.c_int, vp]),
    }
    for name, (restype, argtypes) in want.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    # struct tbk_hit_run { uint64_t read, first, last; uint32_t markers, hap; }
    dt = np.dtype(kmers.HIT_RUN_DTYPE)
    assert dt.itemsize == 32 and [dt.fields[f][1] for f in ("read", "first", "last", "markers", "hap")] == [0, 8, 16, 24, 28]
    header = open(os.path.join(os.path.dirname(DATA), "..", "include", "tbk.h")).read()
    for name in want:
        assert name + "(" in header
    assert "typedef struct tbk_hit_run { uint64_t read, first, last; uint32_t markers, hap; } tbk_hit_run;" in header
    # NULL handles are refused without a device
    out = vp()
    assert _lib.lib.tbk_hit_tracker_create(None, None, C.byref(out)) == -1 and not out.value
    _lib.lib.tbk_hit_tracker_destroy(None)
    import trio_binning.phase_blocks as alias
    import trio_binning_amd.phase_blocks as impl

    assert alias is impl or alias.main is impl.main
