"""What of phase blocks in homopolymer-compressed space needs no device: the definition of the lift (tests/hpc_lift_ref.py) held to
its two properties against the slow restatement of compression (hpc_ref.compress_reads), kmers.phase_blocks and
phase_blocks.sequence_rows on lifted runs, what python -m trio_binning_amd.phase_blocks refuses or accepts under --compress from
its arguments and the files' headers alone (every entry point that loads a list, loads a database or makes a tracker is
replaced by one that fails the test), and the new symbols of the built library."""
import ctypes as C
import os

import numpy as np
import pytest

import hpc_lift_ref as lref
import hpc_ref
import kmerdb_files as kf
from conftest import DATA

MAGIC_HPC = b"TBKKMDH1"
CUTS = ["--min-count-a", "2", "--max-count-a", "9", "--min-count-b", "2", "--max-count-b", "9"]


# ---- the definition ----------------------------------------------------------------------------------------------------------
def _random_reads(rng):
    """reads of 0 to 60 bytes over a few symbols in mixed case, in runs of geometric length; empty reads anywhere"""
    alphabet = rng.choice(list("ACGTNacgtn"), int(rng.integers(2, 6)), replace=False)
    reads = []
    for _ in range(int(rng.integers(1, 9))):
        n = int(rng.integers(0, 61)) if rng.integers(0, 4) else 0
        symbols = alphabet[rng.integers(0, alphabet.size, n + 1)]
        reads.append("".join(np.repeat(symbols, rng.geometric(0.45, symbols.size))[:n]))
    return reads


def _pack(reads):
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer("".join(reads).encode(), dtype=np.uint8), offsets


@pytest.mark.parametrize("fold", [False, True])
def test_the_two_properties_of_the_lift(fold):
    rng = np.random.default_rng(40 + fold)
    windows = 0
    for _ in range(150):
        reads = _random_reads(rng)
        bases, offsets = _pack(reads)
        slow = hpc_ref.compress_reads(reads, fold)
        cb, co = hpc_ref.compress_np(bases, offsets, fold)
        assert bytes(cb).decode() == "".join(slow) and co.tolist() == np.cumsum([0] + [len(s) for s in slow]).tolist()
        lift = lref.lift_np(bases, offsets, fold)
        assert lift.size == cb.size + 1 and int(lift[-1]) == int(offsets[-1])
        # a read's compressed start lifts to its start, empty and trailing empty reads included
        assert np.array_equal(lift[co.astype(np.int64)], offsets)
        for r, (read, small) in enumerate(zip(reads, slow)):
            k = int(rng.integers(1, 8))
            for w in range(len(small) - k + 1):
                lo, hi = (int(lift[int(co[r]) + w + d]) - int(offsets[r]) for d in (0, k))
                assert 0 <= lo < hi <= len(read)
                assert hpc_ref.compress_reads([read[lo:hi]], fold) == [small[w:w + k]]  # the span compresses to exactly the window
                assert (hi == len(read)) == (w + k == len(small))  # the trailing run belongs to the last window
                windows += 1
    assert windows > 2000


def test_expand_np_puts_a_value_on_the_first_base_of_its_run():
    bases, offsets = _pack(["AAACCG", "", "GGT"])
    lift = lref.lift_np(bases, offsets, False)
    assert lift.tolist() == [0, 3, 5, 6, 8, 9]
    assert lref.expand_np(np.array([1, 2, 3, 4, 5], dtype=np.uint8), lift, 9).tolist() == [1, 0, 0, 2, 0, 3, 4, 0, 5]


# ---- the block rule on lifted runs --------------------------------------------------------------------------------------------
# (read, first, last, end, markers, hap)
LIFTED_ROWS = [(0, 0, 40, 75, 12, 0), (0, 80, 80, 130, 1, 1), (0, 140, 200, 260, 30, 0), (0, 300, 420, 500, 25, 1), (1, 3, 9, 41, 4, 1)]


def test_phase_blocks_carries_the_end_of_the_last_run(built):
    from trio_binning_amd import kmers

    runs = np.array(LIFTED_ROWS, dtype=kmers.HIT_RUN_LIFTED_DTYPE)
    one = kmers.phase_blocks(runs, 1)
    assert one.dtype == np.dtype(kmers.HIT_RUN_LIFTED_DTYPE) and one.tolist() == LIFTED_ROWS
    two = kmers.phase_blocks(runs, 2)
    assert two.dtype == np.dtype(kmers.HIT_RUN_LIFTED_DTYPE)
    assert two.tolist() == [(0, 0, 200, 260, 42, 0), (0, 300, 420, 500, 25, 1), (1, 3, 9, 41, 4, 1)]
    for min_run in (1, 2, 3, 13, 31):
        assert np.array_equal(kmers.phase_blocks(runs, min_run), lref.blocks(runs, min_run)), min_run
    none = kmers.phase_blocks(runs, 31)
    assert none.size == 0 and none.dtype == np.dtype(kmers.HIT_RUN_LIFTED_DTYPE)
    empty = kmers.phase_blocks(np.zeros(0, dtype=kmers.HIT_RUN_LIFTED_DTYPE), 1)
    assert empty.size == 0 and empty.dtype == np.dtype(kmers.HIT_RUN_LIFTED_DTYPE)


def test_phase_blocks_on_the_plain_dtype_is_unchanged(built):
    from trio_binning_amd import kmers

    rows = [(0, 0, 40, 12, 0), (0, 55, 55, 1, 1), (0, 70, 200, 30, 0), (0, 300, 420, 25, 1)]
    runs = np.array(rows, dtype=kmers.HIT_RUN_DTYPE)
    assert kmers.phase_blocks(runs, 1).dtype == np.dtype(kmers.HIT_RUN_DTYPE) and kmers.phase_blocks(runs, 1).tolist() == rows
    assert kmers.phase_blocks(runs, 2).tolist() == [(0, 0, 200, 42, 0), (0, 300, 420, 25, 1)]
    assert kmers.phase_blocks(rows, 2).tolist() == [(0, 0, 200, 42, 0), (0, 300, 420, 25, 1)]  # (a plain list of tuples, as before)


def test_sequence_rows_measure_a_lifted_block_from_first_to_end(built):
    from trio_binning_amd import kmers, phase_blocks

    blocks = np.array(LIFTED_ROWS, dtype=kmers.HIT_RUN_LIFTED_DTYPE)
    counts = np.array([[42, 26], [0, 4], [0, 0]], dtype=np.int32)
    k = 21  # (last + k would give other figures: 61, 71, ...)
    got = [c.tolist() for c in phase_blocks.sequence_rows(3, [600, 41, 7], counts, blocks, k)]
    assert got == [[600, 41, 7], [42, 0, 0], [26, 4, 0], [4, 1, 0], [3, 0, 0], [75 + 120, 0, 0], [50 + 200, 38, 0], [200, 38, 0]]
    assert phase_blocks.block_ends(blocks, k).tolist() == [75, 130, 260, 500, 41]
    plain = np.array([(0, 0, 40, 12, 0), (0, 80, 80, 1, 1)], dtype=kmers.HIT_RUN_DTYPE)
    assert phase_blocks.block_ends(plain, k).tolist() == [61, 101]
    got = [c.tolist() for c in phase_blocks.sequence_rows(1, [600], counts[:1], plain, k)]
    assert got == [[600], [42], [26], [2], [1], [61], [21], [61]]


# ---- the command line under --compress ----------------------------------------------------------------------------------------
@pytest.fixture()
def files(built, tmp_path, monkeypatch):
    """Sound plain and compressed databases of k = 21, text lists, and a driver in which touching the device is a failure."""
    import trio_binning_amd.classify_by_kmers as cbk
    from trio_binning_amd import kmers

    paths = {}
    for name, seed, magic in (("plain_a", 1, kf.MAGIC), ("plain_b", 2, kf.MAGIC), ("hpc_a", 1, MAGIC_HPC), ("hpc_b", 2, MAGIC_HPC)):
        _, keys, counts, hist = kf.sound(k=21, n=5, seed=seed)
        paths[name] = str(tmp_path / (name + ".tbkdb"))
        with open(paths[name], "wb") as fh:
            fh.write(kf.file_bytes(21, keys, counts, hist, reads=11, bases=1234, magic=magic))
    paths["list_a"], paths["list_b"] = os.path.join(DATA, "hapA.txt"), os.path.join(DATA, "hapB.txt")
    paths["hpc_list"] = str(tmp_path / "compressed_list.txt")
    with open(paths["hpc_list"], "w") as fh:
        fh.write("ACGTACGTACGTACGTACGTA\nTGCATGCATGCATGCATGCAT\n")
    paths["fa"] = os.path.join(DATA, "test.fa")
    paths["bed"] = str(tmp_path / "out.bed")

    def touched(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were refused")

    monkeypatch.setattr(kmers, "create_kmer_hash_set", touched)
    monkeypatch.setattr(kmers.HashSet, "from_file", touched)
    monkeypatch.setattr(kmers.KmerDatabase, "load", touched)
    monkeypatch.setattr(kmers.KmerDatabase, "unique_set", touched)
    monkeypatch.setattr(kmers, "HomopolymerCompressor", touched)
    monkeypatch.setattr(kmers.HitTracker, "__init__", touched)
    monkeypatch.setattr(cbk, "make_classifier", touched)
    monkeypatch.setattr(cbk, "classify_compressed", touched)
    return paths


def _exit(files, argv):
    from trio_binning_amd import phase_blocks

    with pytest.raises(SystemExit) as ei:
        phase_blocks.main(argv + ["--bed", files["bed"]])
    assert not os.path.exists(files["bed"]) and not os.path.exists(files["bed"] + ".tmp")
    assert isinstance(ei.value.code, str), ei.value.code
    return ei.value.code


def test_compressed_databases_without_the_switch_stay_refused_and_say_which_switch(files, capsys):
    code = _exit(files, [files["fa"], files["hpc_a"], files["hpc_b"]] + CUTS)
    assert code.startswith("phase_blocks:") and "homopolymer-compressed" in code and files["hpc_a"] in code and files["hpc_b"] in code
    assert "--compress" in code
    assert capsys.readouterr().out == ""


def test_plain_databases_under_the_switch_are_refused(files, capsys):
    code = _exit(files, [files["fa"], files["plain_a"], files["plain_b"], "--compress"] + CUTS)
    assert code.startswith("phase_blocks:") and "--compress" in code and "plain" in code
    assert files["plain_a"] in code and files["plain_b"] in code
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("pair", [("hpc_a", "plain_b"), ("plain_a", "hpc_b")])
def test_parents_that_disagree_are_refused_under_the_switch_too(files, capsys, pair):
    code = _exit(files, [files["fa"], files[pair[0]], files[pair[1]], "--compress"] + CUTS)
    assert code.startswith("phase_blocks:") and files[pair[0]] in code and files[pair[1]] in code
    assert "homopolymer-compressed" in code and "plain" in code
    assert capsys.readouterr().out == ""


def test_a_list_that_was_not_made_with_compress_is_refused_in_this_programs_name(files, capsys):
    for pair in ((files["list_a"], files["list_b"]), (files["hpc_list"], files["list_b"]), (files["list_a"], files["hpc_list"])):
        code = _exit(files, [files["fa"], pair[0], pair[1], "--compress"])
        culprit = pair[0] if pair[0] != files["hpc_list"] else pair[1]
        assert code.startswith("phase_blocks: --compress") and "this list was not made with --compress" in code and culprit in code
    assert capsys.readouterr().out == ""


def test_what_is_accepted_goes_on_to_the_device(files, capsys):
    from trio_binning_amd import phase_blocks

    args = phase_blocks.parse_args([files["fa"], files["hpc_a"], files["hpc_b"], "--compress"] + CUTS)
    assert args.compress is True and args.databases is not None and args.databases.compressed is True
    args = phase_blocks.parse_args([files["fa"], files["hpc_list"], files["hpc_list"], "--compress"])
    assert args.compress is True and args.databases is None
    args = phase_blocks.parse_args([files["fa"], files["plain_a"], files["plain_b"]] + CUTS)
    assert args.compress is False and args.databases.compressed is False
    args = phase_blocks.parse_args([files["fa"], files["list_a"], files["list_b"]])  # (a plain list is not looked into without the switch)
    assert args.compress is False and args.databases is None
    for argv in ([files["hpc_a"], files["hpc_b"], "--compress"] + CUTS, [files["hpc_list"], files["hpc_list"], "--compress"]):
        with pytest.raises(AssertionError, match="device was touched"):  # nothing refused: the lists or databases are loaded next
            phase_blocks.main([files["fa"]] + argv + ["--bed", files["bed"]])
    assert not os.path.exists(files["bed"]) and capsys.readouterr().out == ""


def test_help_says_what_the_coordinates_are(built, capsys):
    from trio_binning_amd import phase_blocks

    with pytest.raises(SystemExit) as ei:
        phase_blocks.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert ei.value.code == 0 and "--compress" in text and "coordinates of the sequence as given" in text


# ---- the library ------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_and_their_signatures(built):
    from trio_binning_amd import _lib, kmers

    vp, u64 = C.c_void_p, C.c_uint64
    want = {
        "tbk_hpc_lift": (C.c_int, [vp, vp, u64, vp]),
        "tbk_hpc_expand": (C.c_int, [vp, vp, vp]),
        "tbk_hit_tracker_runs_compressed": (C.c_int, [vp, vp, vp, u64, C.c_int, C.POINTER(vp), C.POINTER(u64), vp]),
        "tbk_hit_tracker_marks_compressed": (C.c_int, [vp, vp, vp, u64, C.c_int, vp]),
    }
    for name, (restype, argtypes) in want.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    dt = np.dtype(kmers.HIT_RUN_LIFTED_DTYPE)
    assert dt.itemsize == 40 and [dt.fields[f][1] for f in ("read", "first", "last", "end", "markers", "hap")] == [0, 8, 16, 24, 32, 36]
    assert dt == np.dtype(lref.LIFTED_DTYPE)
    header = open(os.path.join(os.path.dirname(DATA), "..", "include", "tbk.h")).read()
    for name in want:
        assert name + "(" in header
    assert "typedef struct tbk_hit_run_lifted { uint64_t read, first, last, end; uint32_t markers, hap; } tbk_hit_run_lifted;" in header
    # NULL handles are refused without a device
    out = np.zeros(1, dtype=np.uint64)
    assert _lib.lib.tbk_hpc_lift(None, out.ctypes.data, 1, out.ctypes.data) == -1
    assert _lib.lib.tbk_hpc_expand(None, out.ctypes.data, out.ctypes.data) == -1
    ptr, n = vp(), u64()
    assert _lib.lib.tbk_hit_tracker_runs_compressed(None, None, out.ctypes.data, 0, 0, C.byref(ptr), C.byref(n), None) == -1
    assert _lib.lib.tbk_hit_tracker_marks_compressed(None, None, out.ctypes.data, 0, 0, None) == -1
