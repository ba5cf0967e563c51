"""Homopolymer compression on the device (tbk_hpc, kmers.HomopolymerCompressor; kernels: csrc/tbk_hpc.hip) against the numpy
restatement of its contract (tests/hpc_ref.py), byte for byte - bases and offsets - at the smallest shapes at which the
kernels can go wrong: T = the kernels' tile (4096 bases), 16 = the vector a lane loads, 1024 = a wave's share of a tile."""
import ctypes as C

import numpy as np
import pytest

import hpc_ref

pytestmark = pytest.mark.gpu


def _tile():
    from trio_binning_amd._lib import lib

    lib.tbk_hpc_tile.restype = C.c_uint32
    return int(lib.tbk_hpc_tile())


def _pack(reads):
    """(bases, offsets) of reads given as bytes or str."""
    enc = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in reads]
    offsets = np.zeros(len(enc) + 1, dtype=np.uint64)
    if enc:
        offsets[1:] = np.cumsum([len(b) for b in enc], dtype=np.uint64)
    return np.frombuffer(b"".join(enc), dtype=np.uint8).copy(), offsets


def _check(comp, bases, offsets, folds=(False, True)):
    for fold in folds:
        want_b, want_o = hpc_ref.compress_np(bases, offsets, fold)
        got_b, got_o = comp.compress(bases, offsets, fold_case=fold)
        assert got_o.dtype == np.uint64 and got_b.dtype == np.uint8
        assert np.array_equal(got_o, want_o), (fold, np.flatnonzero(got_o != want_o)[:5])
        assert got_b.size == want_b.size and np.array_equal(got_b, want_b), (fold, np.flatnonzero(got_b != want_b)[:5])
    return want_b, want_o


def _background(n, phase=0):
    """n bytes without two equal neighbours and without an 'A': runs of 'A' planted in it keep their ends."""
    return np.frombuffer(b"CGT", dtype=np.uint8)[(np.arange(n) + phase) % 3].copy()


@pytest.fixture(scope="module")
def comp(gpu):
    from trio_binning_amd import kmers

    with kmers.HomopolymerCompressor() as c:
        yield c


def test_no_reads_and_empty_reads(comp):
    b, o = comp.compress(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    assert b.size == 0 and o.tolist() == [0]
    b, o = comp.compress(*_pack(["", "", ""]), fold_case=True)
    assert b.size == 0 and o.tolist() == [0, 0, 0, 0]
    want_b, want_o = _check(comp, *_pack(["", "", "ACCA", "", "GG", "", "", "TTTA", "", ""]))
    assert bytes(want_b) == b"ACAGTA" and want_o.tolist() == [0, 0, 0, 3, 3, 4, 4, 4, 6, 6, 6]


def test_one_base_and_nothing_to_drop(comp):
    T = _tile()
    want_b, want_o = _check(comp, *_pack(["A"]))
    assert bytes(want_b) == b"A" and want_o.tolist() == [0, 1]
    for n in (1, 15, 16, 17, T - 1, T, T + 37, 2 * T + 1):
        bases = _background(n)
        for offsets in ([0, n], [0, n // 3, n // 3, n]):
            want_b, want_o = _check(comp, bases, np.array(offsets, dtype=np.uint64))
            assert np.array_equal(want_b, bases) and want_o.tolist() == offsets


def test_one_long_run_becomes_one_base(comp):
    T = _tile()
    want_b, want_o = _check(comp, *_pack([b"A" * (3 * T + 5)]))
    assert bytes(want_b) == b"A" and want_o.tolist() == [0, 1]
    want_b, _ = _check(comp, *_pack([b"C" + b"a" * (3 * T + 5) + b"G"]))
    assert bytes(want_b) == b"CaG"


def test_runs_that_start_or_end_on_every_boundary(comp):
    T = _tile()
    n = T + 64
    for edge in (16, 1024, T):
        for delta in (-1, 0, 1):
            for run in ((edge + delta, edge + delta + 7), (edge + delta - 7, edge + delta), (edge + delta - 20, edge + delta + 20)):
                if run[0] < 0:
                    continue
                bases = _background(n)
                bases[run[0]:run[1]] = ord("A")
                want_b, _ = _check(comp, bases, np.array([0, n], dtype=np.uint64), folds=(False,))
                assert want_b.size == n - (run[1] - run[0]) + 1
                bases[run[0]:run[1]:2] = ord("a")  # the same run in mixed case: one base folded, none dropped unfolded
                _check(comp, bases, np.array([0, n], dtype=np.uint64))


def test_a_read_boundary_inside_equal_bytes_keeps_both_first_bases(comp):
    T = _tile()
    n = T + 64
    bases = np.full(n, ord("A"), dtype=np.uint8)
    for cut in (8, 15, 16, 17, 1023, 1024, 1025, T - 1, T, T + 1):
        want_b, want_o = _check(comp, bases, np.array([0, cut, n], dtype=np.uint64))
        assert bytes(want_b) == b"AA" and want_o.tolist() == [0, 1, 2]
    cuts = [0, 8, 16, 16, 1024, T, T + 1, n, n]
    want_b, want_o = _check(comp, bases, np.array(cuts, dtype=np.uint64))
    assert bytes(want_b) == b"A" * 6 and want_o.tolist() == [0, 1, 2, 2, 3, 4, 5, 6, 6]
    bases[1::2] = ord("a")
    _check(comp, bases, np.array(cuts, dtype=np.uint64))


def test_totals_beside_the_vector_and_the_tile(comp):
    T = _tile()
    rng = np.random.default_rng(5)
    for total in (1, 15, 17, 47, 48, 49, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1):
        bases = np.frombuffer(b"AC", dtype=np.uint8)[rng.integers(0, 2, total)].copy()
        cuts = np.sort(rng.integers(0, total + 1, 5)).tolist()
        _check(comp, bases, np.array([0] + cuts + [total], dtype=np.uint64))


def test_case_is_folded_only_on_request(comp):
    for text, plain, folded in (("AaAa", "AaAa", "A"), ("NNnn", "Nn", "N"), ("aAAa", "aAa", "a"), ("@`[{", "@`[{", "@`[{"), ("zZ\xfa\xda", "zZ\xfa\xda", "z\xfa\xda")):
        bases, offsets = _pack([text])
        got, _ = comp.compress(bases, offsets, fold_case=False)
        assert bytes(got) == plain.encode("latin-1"), text
        got, _ = comp.compress(bases, offsets, fold_case=True)
        assert bytes(got) == folded.encode("latin-1"), text
        _check(comp, bases, offsets)


def _random_batch(rng, T, max_reads=200, max_bytes=2 << 20, min_reads=1):
    """Reads of 0 to 3T bytes over two to five symbols in mixed case, in runs of geometric length (mean 2.2)."""
    alphabet = rng.choice(np.frombuffer(b"ACGTNacgtn", dtype=np.uint8), int(rng.integers(2, 6)), replace=False)
    lengths = rng.integers(0, 3 * T + 1, int(rng.integers(min_reads, max_reads + 1)))
    lengths = lengths[np.cumsum(lengths) <= max_bytes]
    total = int(lengths.sum())
    symbols = alphabet[rng.integers(0, alphabet.size, total + 1)]
    bases = np.repeat(symbols, rng.geometric(0.45, symbols.size))[:total].copy()
    assert bases.size == total
    offsets = np.zeros(lengths.size + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lengths)
    return bases, offsets


def test_a_session_shrinks_and_grows_and_refuses_bad_offsets(gpu):
    from trio_binning_amd import kmers

    T = _tile()
    rng = np.random.default_rng(11)
    with kmers.HomopolymerCompressor() as comp:
        for max_reads in (30, 3, 120, 1):
            _check(comp, *_random_batch(rng, T, max_reads, min_reads=max_reads))
        bases, offsets = _random_batch(rng, T, 10, min_reads=10)
        bad = offsets.copy()
        bad[2], bad[3] = offsets[3] + 1, offsets[2]
        with pytest.raises(ValueError):
            comp.compress(bases, bad)
        with pytest.raises(ValueError):
            comp.fetch(0)  # (a refused batch leaves no result)
        _check(comp, bases, offsets)


def test_compress_device_equals_compress_and_checks_its_offsets(gpu, comp):
    from trio_binning_amd._lib import check, lib

    T = _tile()
    rng = np.random.default_rng(12)
    bases, offsets = _random_batch(rng, T, 40, min_reads=40)
    d_bases, d_offsets = C.c_void_p(), C.c_void_p()
    check(lib.tbk_device_alloc(comp.device, bases.size + 64, C.byref(d_bases)))
    check(lib.tbk_device_alloc(comp.device, offsets.nbytes, C.byref(d_offsets)))
    try:
        check(lib.tbk_memcpy_h2d(comp.device, d_bases, bases.ctypes.data, bases.size))
        check(lib.tbk_memcpy_h2d(comp.device, d_offsets, offsets.ctypes.data, offsets.nbytes))
        for fold in (False, True):
            want_b, want_o = hpc_ref.compress_np(bases, offsets, fold)
            _, _, total = comp.compress_device(d_bases.value, d_offsets.value, offsets.size - 1, bases.size, fold)
            got_b, got_o = comp.fetch(total)
            assert np.array_equal(got_b, want_b) and np.array_equal(got_o, want_o)
        # the result of a session, compressed again by another: nothing is left to drop
        from trio_binning_amd import kmers

        d_cb, d_co, total = comp.compress_device(d_bases.value, d_offsets.value, offsets.size - 1, bases.size, True)
        with kmers.HomopolymerCompressor() as second:
            _, _, again = second.compress_device(d_cb, d_co, offsets.size - 1, total, True)
            got_b, got_o = second.fetch(again)
        assert again == total and np.array_equal(got_b, want_b) and np.array_equal(got_o, want_o)
        for damage in ("descends", "starts_late", "ends_early"):
            bad = offsets.copy()
            if damage == "descends":
                bad[5], bad[6] = offsets[6] + 3, offsets[5]
            elif damage == "starts_late":
                bad[0] = 1
            else:
                bad[-1] -= 1
            check(lib.tbk_memcpy_h2d(comp.device, d_offsets, bad.ctypes.data, bad.nbytes))
            with pytest.raises(ValueError):
                comp.compress_device(d_bases.value, d_offsets.value, offsets.size - 1, bases.size, False)
        check(lib.tbk_memcpy_h2d(comp.device, d_offsets, offsets.ctypes.data, offsets.nbytes))
        _, _, total = comp.compress_device(d_bases.value, d_offsets.value, offsets.size - 1, bases.size, False)
        want_b, want_o = hpc_ref.compress_np(bases, offsets, False)
        got_b, got_o = comp.fetch(total)
        assert np.array_equal(got_b, want_b) and np.array_equal(got_o, want_o)
    finally:
        lib.tbk_device_free(comp.device, d_bases)
        lib.tbk_device_free(comp.device, d_offsets)


@pytest.mark.parametrize("seed", range(40))
def test_fuzz(comp, seed):
    rng = np.random.default_rng(1000 + seed)
    bases, offsets = _random_batch(rng, _tile())
    assert bases.size <= 2 << 20
    _check(comp, bases, offsets)
