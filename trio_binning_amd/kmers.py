"""Counting parental k-mers in reads on an MI355X.

Host-side mirror of the reference's ``trio_binning.kmers`` (src/trio_binning/kmers.py):
the same five functions with the same argument meaning and error behaviour, bound to the
HIP library's C-ABI (include/tbk.h) instead of the reference's c/kmers.c, plus the batch
interface the GPU needs (``Classifier``).

>>> hapA = kmers.create_kmer_hash_set("tests/data/hapA.txt")
>>> hapB = kmers.create_kmer_hash_set("tests/data/hapB.txt")
>>> kmers.count_kmers_in_read("CTTATCATGTCTTTGTTTTCAAAGCTTC...", hapA, hapB)
(2, 1)

Every function that computes needs a visible MI355X; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from os.path import isfile
from typing import Iterable, Optional, Sequence, Tuple


class _LazyNumpy:
    """numpy, imported at first use: the command line's path (lists from files, the native loop) needs none of it,
    and its import is a quarter of a second of a run that takes under three."""

    def __getattr__(self, name):
        import numpy

        globals()["np"] = numpy
        return getattr(numpy, name)


np = _LazyNumpy()

from . import _lib
from ._lib import check, lib


def default_device() -> int:
    """Device index used when none is given: TBK_DEVICE, else the first of TBK_DEVICES, else
    LOCAL_RANK, else 0."""
    for var in ("TBK_DEVICE", "TBK_DEVICES", "LOCAL_RANK"):
        v = os.environ.get(var)
        if v not in (None, ""):
            return int(v.split(",")[0])
    return 0


class _Contents:
    """Stand-in for ``POINTER(_HashSet).contents`` (reference kmers.py:41-59,159)."""

    def __init__(self, hs):
        self._hs = hs

    @property
    def num_kmers(self) -> int:
        return self._hs.num_kmers

    @property
    def k(self) -> int:
        return self._hs.k


class HashSet:
    """A parental k-mer list resident in HBM (packed 64-bit keys).

    Plays the role of the reference's ``HashSet`` pointer type (kmers.py:96-101): what
    ``create_kmer_hash_set`` returns and ``count_kmers_in_read`` accepts.  Pairing two of
    them in a ``Classifier`` hashes them into the open-addressing tables the probe kernel
    reads; ``contains`` hashes this list on its own.
    """

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)

    # -- construction ---------------------------------------------------------------------
    @classmethod
    def from_file(cls, path: str, device: Optional[int] = None) -> "HashSet":
        h = C.c_void_p()
        check(lib.tbk_table_create_from_file(os.fsencode(path), default_device() if device is None else device, C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_keys(cls, keys, k: int, device: Optional[int] = None) -> "HashSet":
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        h = C.c_void_p()
        check(lib.tbk_table_create_from_keys(
            keys.ctypes.data, keys.size, k, default_device() if device is None else device, C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_device_keys(cls, d_keys: int, n: int, k: int, device: Optional[int] = None) -> "HashSet":
        h = C.c_void_p()
        check(lib.tbk_table_create_from_device_keys(
            C.c_void_p(d_keys), n, k, default_device() if device is None else device, C.byref(h)))
        return cls(h.value)

    # -- facts ----------------------------------------------------------------------------
    @property
    def num_kmers(self) -> int:
        """Number of list lines, duplicates included (reference: hash_set.num_kmers)."""
        return lib.tbk_table_num_kmers(self._h)

    @property
    def k(self) -> int:
        return lib.tbk_table_k(self._h)

    @property
    def device(self) -> int:
        return lib.tbk_table_device(self._h)

    @property
    def distinct(self) -> int:
        """Distinct keys in the list (hashes the list on its own on first use)."""
        n = C.c_uint64()
        check(lib.tbk_table_distinct(self._h, C.byref(n)))
        return n.value

    @property
    def nbytes(self) -> int:
        return lib.tbk_table_bytes(self._h)

    @property
    def device_keys(self) -> int:
        """Device pointer of the list's packed keys (num_kmers of them, read-only)."""
        return lib.tbk_table_device_keys(self._h)

    @property
    def contents(self) -> _Contents:
        return _Contents(self)

    @property
    def origin(self) -> str:
        """Where the keys came from: "keys" (the caller's, or the general host parser), "gpu-parser", "cache", "databases"
        (``KmerDatabase.unique_set``)."""
        return {0: "keys", 1: "gpu-parser", 2: "cache", 3: "databases"}.get(lib.tbk_table_origin(self._h), "?")

    def keys(self) -> np.ndarray:
        """The packed keys, one per list line, copied to the host."""
        out = np.empty(self.num_kmers, dtype=np.uint64)
        check(lib.tbk_table_keys(self._h, out.ctypes.data, out.size))
        return out

    def contains(self, keys) -> np.ndarray:
        """Membership of raw packed keys (no canonicalisation)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros(keys.size, dtype=np.uint8)
        check(lib.tbk_table_contains(self._h, keys.ctypes.data, keys.size, out.ctypes.data))
        return out.astype(bool)

    def close(self) -> None:
        if self._h is not None and self._h.value:
            lib.tbk_table_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- the reference's five functions ------------------------------------------------------
def kmer_to_int(kmer: str) -> int:
    """Convert a kmer to integer format (reference kmers.py:80-82 -> c/kmers.c:50-72)."""
    raw = bytes(kmer, "utf-8")
    return lib.tbk_kmer_to_int(raw, C.c_ubyte(len(kmer)))


def reverse_complement(kmer: str) -> str:
    """Reverse complement a k-mer (reference kmers.py:89-93 -> c/kmers.c:74-93).

    As in the reference, the output starts as ``"x" * k`` and positions whose source
    base is not one of ACGT keep the ``x``.
    """
    k = len(kmer)
    out = C.create_string_buffer(b"x" * k, k + 1)
    lib.tbk_reverse_complement(bytes(kmer, "utf-8"), out, k)
    return out.raw[:k].decode("utf-8")


def create_kmer_hash_set(kmer_file_path: str) -> HashSet:
    """Read a list of k-mers (one per line) into a searchable set in HBM.

    Same contract as the reference (kmers.py:104-122): ``IOError`` when the path is not
    a file, a progress line on stderr, a handle for ``count_kmers_in_read``.
    """
    if not isfile(kmer_file_path):
        raise IOError(f"Specified file {kmer_file_path} does not exist or is not file.")
    print(f"Reading k-mers in {kmer_file_path}...", file=sys.stderr)
    hs = HashSet.from_file(kmer_file_path)
    print(f"Found {hs.num_kmers} {hs.k}-mers in {kmer_file_path} (in HBM on device {hs.device}).", file=sys.stderr)
    return hs


def parse_kmer_list(kmer_file_path: str) -> Tuple[np.ndarray, int]:
    """Host-only: (packed keys, k) of a k-mer list file, exactly what ``create_kmer_hash_set``
    places in HBM (the reference's getline rules, c/kmers.c:124-146,204-221)."""
    keys, n, k = _lib._u64p(), C.c_uint64(), C.c_int()
    check(lib.tbk_list_parse_file(os.fsencode(kmer_file_path), C.byref(keys), C.byref(n), C.byref(k)))
    try:
        out = np.ctypeslib.as_array(keys, shape=(n.value,)).copy() if n.value else np.zeros(0, dtype=np.uint64)
    finally:
        lib.tbk_list_free(keys)
    return out, k.value


def count_kmers_in_read(read: str, kmers_hap_a: HashSet, kmers_hap_b: HashSet) -> Tuple[int, int]:
    """Count the k-mers of one read found in each of two sets (reference kmers.py:125-154).

    Returns ``(count_a, count_b)``; a k-mer present in both sets counts for A only.  One
    kernel launch per call: use ``Classifier`` for throughput.
    """
    raw = read.encode("utf-8")
    ca, cb = C.c_int(), C.c_int()
    check(lib.tbk_count_kmers_in_read(raw, len(raw), kmers_hap_a._h, kmers_hap_b._h, C.byref(ca), C.byref(cb)))
    return ca.value, cb.value


def get_number_kmers_in_set(kmer_hash_set: HashSet) -> int:
    """Look up the number of k-mers in a hash set (reference kmers.py:157-159)."""
    return kmer_hash_set.contents.num_kmers


# ---- batch interface ---------------------------------------------------------------------
def pack_reads(seqs: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """Concatenate read sequences into the batch layout of the C-ABI:
    ``bases`` (uint8, back to back) and ``offsets`` (uint64, n+1)."""
    lens = np.fromiter((len(s) for s in seqs), dtype=np.uint64, count=len(seqs))
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    raw = "".join(seqs).encode("utf-8")
    if len(raw) != int(offsets[-1]):
        # non-ASCII text: lengths must be byte lengths
        enc = [s.encode("utf-8") for s in seqs]
        lens = np.fromiter((len(b) for b in enc), dtype=np.uint64, count=len(enc))
        np.cumsum(lens, out=offsets[1:])
        raw = b"".join(enc)
    bases = np.frombuffer(raw, dtype=np.uint8)
    return bases, offsets


class PackedBatch:
    """A read batch in the packed transfer format (include/tbk.h): 2-bit code words, the exceptions
    (chunks holding a byte outside ACGT or positions past the end) and the reads' offsets."""

    def __init__(self, codes, exc_chunk, exc_mask, offsets):
        self.codes, self.exc_chunk, self.exc_mask, self.offsets = codes, exc_chunk, exc_mask, offsets

    @property
    def n_reads(self) -> int:
        return self.offsets.size - 1

    @property
    def nbytes(self) -> int:
        """Bytes that cross PCIe for this batch."""
        return self.codes.nbytes + self.exc_chunk.nbytes + self.exc_mask.nbytes + self.offsets.nbytes


def pack_bases(bases: np.ndarray, offsets: np.ndarray, pinned: bool = True) -> PackedBatch:
    """Pack a batch's ASCII bases on the host (all host threads; AVX2 when the CPU has it)."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    total = int(offsets[-1])
    n_chunks = int(lib.tbk_packed_chunks(total))
    alloc = pinned_empty if pinned else (lambda shape, dt: np.empty(shape, dtype=dt))
    codes = alloc((max(n_chunks, 1),), np.uint32)
    n_exc = C.c_uint64()
    cap = 1024
    while True:
        ec, em = np.empty(cap, dtype=np.uint32), np.empty(cap, dtype=np.uint16)
        rc = lib.tbk_pack_bases(bases.ctypes.data, total, codes.ctypes.data, ec.ctypes.data, em.ctypes.data, cap, C.byref(n_exc))
        if rc == _lib.TBK_ERR_NOMEM and n_exc.value > cap:
            cap = n_exc.value
            continue
        check(rc)
        break
    n = n_exc.value
    exc_chunk, exc_mask = alloc((max(n, 1),), np.uint32)[:n], alloc((max(n, 1),), np.uint16)[:n]
    exc_chunk[:] = ec[:n]
    exc_mask[:] = em[:n]
    if pinned:
        po = pinned_empty(offsets.shape, np.uint64)
        po[:] = offsets
        offsets = po
    return PackedBatch(codes[:n_chunks], exc_chunk, exc_mask, offsets)


class Options:
    """How a classifier is built (include/tbk.h: ``tbk_options``).  The reference configures itself through argparse alone
    (classify_by_kmers.py:14-54); this library's choices - which layout the paired table takes, the sampling rule, loads,
    the memory budget - are arguments too: ``Options(entries=1, entry_load=0.64)``, ``Options.layout("short_keys")``.
    No option changes a result.  ``Options.from_env()`` overlays the ``TBK_*`` variables of the process environment - the
    command-line tools' fallback, and what ``Classifier`` / ``MultiClassifier`` do when no options are given; the library's
    constructors themselves never read the environment, so two classifiers of one process can be built differently at the
    same time."""

    LAYOUTS = {
        "auto": {},
        "keys": {"short_keys": 0, "entries": 0, "full_keys": 0},
        "keys_front": {"short_keys": 0, "entries": 0, "full_keys": 0, "front": 1},
        "keys_whole_lines": {"short_keys": 0, "entries": 0, "full_keys": 0, "front": 0},
        "full_keys": {"short_keys": 0, "entries": 0, "full_keys": 1},
        "entries": {"entries": 1, "wide_entries": 0},
        "wide_entries": {"entries": 1, "wide_entries": 1},
        "short_keys": {"short_keys": 1},
    }

    def __init__(self, **fields):
        self.c = _lib.tbk_options()
        lib.tbk_options_init(C.byref(self.c))
        self.update(**fields)

    def update(self, **fields) -> "Options":
        names = {f[0] for f in _lib.tbk_options._fields_} - {"size"}
        for name, value in fields.items():
            if name not in names:
                raise TypeError(f"tbk_options has no field {name!r}")
            setattr(self.c, name, value)
        return self

    @classmethod
    def layout(cls, name: str, **fields) -> "Options":
        return cls(**dict(cls.LAYOUTS[name], **fields))

    @classmethod
    def from_env(cls, **fields) -> "Options":
        self = cls()
        check(lib.tbk_options_from_env(C.byref(self.c)))
        return self.update(**fields)

    def __repr__(self):
        dflt = _lib.tbk_options()
        lib.tbk_options_init(C.byref(dflt))
        diff = {f[0]: getattr(self.c, f[0]) for f in _lib.tbk_options._fields_ if getattr(self.c, f[0]) != getattr(dflt, f[0])}
        return f"Options({', '.join(f'{k}={v}' for k, v in diff.items())})"


def _options_ptr(options):
    """ctypes pointer for the *_opts calls: the given Options, or - none given - the TBK_* environment's (the fallback)"""
    if not _lib.HAS_OPTIONS:
        return None
    if options is None:
        options = Options.from_env()
    return C.byref(options.c)


class Classifier:
    """The batch hot path: per-read (hapA, hapB) k-mer hit counts for many reads at once.

    Replaces the per-read Python loop of the reference driver
    (classify_by_kmers.py:99-102).  ``submit``/``wait`` keep up to ``depth`` batches in
    flight so the host-to-device copy of the next batch overlaps the kernel of the
    current one.
    """

    def __init__(self, kmers_hap_a: HashSet, kmers_hap_b: HashSet, _handle: Optional[int] = None, options: Optional[Options] = None):
        if _handle is None:
            h = C.c_void_p()
            if _lib.HAS_OPTIONS:
                check(lib.tbk_classifier_create_opts(kmers_hap_a._h, kmers_hap_b._h, _options_ptr(options), C.byref(h)))
            else:
                check(lib.tbk_classifier_create(kmers_hap_a._h, kmers_hap_b._h, C.byref(h)))
        else:  # one of tbk_classifier_create_multi's classifiers
            h = C.c_void_p(_handle)
        self._h = h
        self._a, self._b = kmers_hap_a, kmers_hap_b  # keep the tables alive
        self._keep = {}
        self.device = lib.tbk_classifier_device(h)

    @property
    def depth(self) -> int:
        return lib.tbk_stream_depth(self._h)

    def stats(self) -> dict:
        """Distinct keys per list, bucket lines and bytes of the paired table in HBM."""
        da, db, nb, by = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib.tbk_classifier_stats(self._h, C.byref(da), C.byref(db), C.byref(nb), C.byref(by)))
        w, m, o = C.c_int(), C.c_int(), C.c_int()
        check(lib.tbk_classifier_layout(self._h, C.byref(w), C.byref(m), C.byref(o)))
        sh = C.c_uint64()
        check(lib.tbk_classifier_shared_keys(self._h, C.byref(sh)))
        nb_, past = C.c_int(), C.c_uint64()
        check(lib.tbk_classifier_build_info(self._h, C.byref(nb_), C.byref(past)))
        front, behind = C.c_int(), C.c_uint64()
        if hasattr(lib, "tbk_classifier_front"):
            check(lib.tbk_classifier_front(self._h, C.byref(front), C.byref(behind)))
        ent, ea, eb = C.c_int(), C.c_uint64(), C.c_uint64()
        if hasattr(lib, "tbk_classifier_entries"):
            check(lib.tbk_classifier_entries(self._h, C.byref(ent), C.byref(ea), C.byref(eb)))
        return {"entry_layout": ent.value in (1, 2), "wide_entries": ent.value == 2, "short_keys": ent.value == 3, "full_keys": ent.value == 4, "entries_a": ea.value, "entries_b": eb.value, "shared_keys": sh.value, "layout_builds": nb_.value, "keys_past_half": past.value, "front_layout": bool(front.value), "keys_behind_front": behind.value, "distinct_a": da.value, "distinct_b": db.value, "n_buckets": nb.value, "table_bytes": by.value,
                "minimizer_w": w.value, "minimizer_m": m.value, "span_offset": o.value,
                "sampling_t": lib.tbk_classifier_sampling_t(self._h)}

    def verified(self) -> dict:
        """What the constructor's own check did (``tbk_options.verify_build``: by default every table built by inserts that
        merge keys - entries, wide entries - is asked for every line of both lists before it is handed out, on every device):
        {"lines": list lines looked up again (0: not checked), "seconds"}.  A table that answers a line wrongly is never
        returned - the constructor fails."""
        lines, sec = C.c_uint64(), C.c_double()
        if not hasattr(lib, "tbk_classifier_verified"):
            return {"lines": 0, "seconds": 0.0}
        check(lib.tbk_classifier_verified(self._h, C.byref(lines), C.byref(sec)))
        return {"lines": lines.value, "seconds": sec.value}

    def table_id(self) -> tuple:
        """(where the table lies - equal ids share one table -, how it was made: 0 built first or shared, 1 a copy of a finished
        table, 2 built again on this device from the lists in the first one's geometry)"""
        tid, rep = C.c_uint64(), C.c_int()
        check(lib.tbk_classifier_table_id(self._h, C.byref(tid), C.byref(rep)))
        return tid.value, rep.value

    def verify(self, kmers_hap_a: Optional[HashSet] = None, kmers_hap_b: Optional[HashSet] = None) -> dict:
        """Every line of both lists through the finished table, against the lists' standalone tables of verbatim keys
        (``tbk_classifier_verify``): {"lines", "count_a", "count_b", "bad_lines", "first_bad"}; raises nothing - the caller decides."""
        a, b = kmers_hap_a or self._a, kmers_hap_b or self._b
        out = (C.c_uint64 * 5)()
        check(lib.tbk_classifier_verify(self._h, a._h, b._h, out))
        return {"lines": out[0], "count_a": out[1], "count_b": out[2], "bad_lines": out[3], "first_bad": None if out[4] == 2 ** 64 - 1 else out[4]}

    def classify_batch(self, bases: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        counts = np.zeros((n, 2), dtype=np.int32)
        check(lib.tbk_classify_batch(self._h, bases.ctypes.data, offsets.ctypes.data, n, counts.ctypes.data))
        return counts

    def classify_reads(self, seqs: Sequence[str]) -> np.ndarray:
        return self.classify_batch(*pack_reads(seqs))

    def count_read(self, read: str) -> Tuple[int, int]:
        """One read, one kernel launch (``tbk_classifier_count_read``): what ``count_kmers_in_read`` - the reference's per-read
        call, kmers.py:125-154 - does on its cached classifier."""
        raw = read.encode("utf-8")
        ca, cb = C.c_int(), C.c_int()
        check(lib.tbk_classifier_count_read(self._h, raw, len(raw), C.byref(ca), C.byref(cb)))
        return ca.value, cb.value

    def submit(self, bases: np.ndarray, offsets: np.ndarray) -> int:
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        counts = np.zeros((n, 2), dtype=np.int32)
        ticket = C.c_uint64()
        check(lib.tbk_stream_submit(self._h, bases.ctypes.data, offsets.ctypes.data, n, counts.ctypes.data, C.byref(ticket)))
        self._keep[ticket.value] = (bases, offsets, counts)
        return ticket.value

    def submit_packed(self, packed: PackedBatch) -> int:
        """Submit a batch packed ahead of time (``pack_bases``): 0.25 bytes per base cross PCIe."""
        counts = np.zeros((packed.n_reads, 2), dtype=np.int32)
        ticket = C.c_uint64()
        check(lib.tbk_stream_submit_packed(self._h, packed.codes.ctypes.data, packed.exc_chunk.ctypes.data, packed.exc_mask.ctypes.data,
                                           packed.exc_chunk.size, packed.offsets.ctypes.data, packed.n_reads, counts.ctypes.data, C.byref(ticket)))
        self._keep[ticket.value] = (packed, None, counts)
        return ticket.value

    @property
    def packed_transfer(self) -> bool:
        """Whether ``submit`` / ``classify_batch`` pack host batches before the copy (default; TBK_PACKED_H2D=0 turns it off)."""
        return bool(lib.tbk_classifier_transfer(self._h))

    @packed_transfer.setter
    def packed_transfer(self, on: bool) -> None:
        check(lib.tbk_classifier_set_transfer(self._h, int(bool(on))))

    def submit_batch(self, batch) -> int:
        """Submit a ``seq.Batch`` (its bases already lie in pinned memory: no staging copy)."""
        bases_ptr, off_ptr = batch.pointers()
        counts = np.zeros((batch.n_reads, 2), dtype=np.int32)
        ticket = C.c_uint64()
        check(lib.tbk_stream_submit(self._h, C.c_void_p(bases_ptr), C.c_void_p(off_ptr), batch.n_reads,
                                    counts.ctypes.data, C.byref(ticket)))
        self._keep[ticket.value] = (batch, None, counts)
        return ticket.value

    def wait(self, ticket: int) -> np.ndarray:
        check(lib.tbk_stream_wait(self._h, ticket))
        return self._keep.pop(ticket)[2]

    wait_ticket = wait

    # device-resident form (bench.py; inputs already in HBM)
    def classify_device(self, d_bases: int, d_offsets: int, n_reads: int, total_bases: int, d_counts: int) -> None:
        check(lib.tbk_classify_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_reads, total_bases,
                                      C.c_void_p(d_counts)))

    def submit_device(self, d_bases: int, d_offsets: int, n_reads: int, total_bases: int, counts: np.ndarray) -> int:
        """Ticketed form of ``classify_device``: ``counts`` (int32 [n_reads, 2], ideally a view
        of pinned memory from ``pinned_empty``) is filled when ``wait_ticket`` returns."""
        ticket = C.c_uint64()
        check(lib.tbk_stream_submit_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_reads, total_bases,
                                           counts.ctypes.data, C.byref(ticket)))
        self._keep[ticket.value] = (None, None, counts)
        return ticket.value

    def sync(self) -> None:
        check(lib.tbk_classifier_sync(self._h))

    def kernel_timing(self, on: bool) -> None:
        check(lib.tbk_kernel_timing_enable(self._h, int(on)))

    def kernel_timing_read(self) -> Tuple[int, float]:
        n, ms = C.c_uint64(), C.c_double()
        check(lib.tbk_kernel_timing_read(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def kernel_timing_read2(self) -> Tuple[int, float, float]:
        """Probes since enable, their summed milliseconds (pass index + both probe kernels) and those of
        the single-read kernel alone - on long reads the dominant kernel."""
        n, ms, single = C.c_uint64(), C.c_double(), C.c_double()
        check(lib.tbk_kernel_timing_read2(self._h, C.byref(n), C.byref(ms), C.byref(single)))
        return n.value, ms.value, single.value

    def calibrate(self) -> float:
        """Random 64-byte line reads per second over this table where it lies in HBM (a diagnostic)."""
        v = C.c_double()
        check(lib.tbk_classifier_calibrate(self._h, C.byref(v)))
        return v.value

    def calibrate_pairs(self, inflight: int = 4, waves_per_simd: int = 8, n_lines: int = 1 << 28) -> float:
        """The same in the entry kernels' own request shape (two lanes x 16 bytes of a line, one-wave blocks): random lines
        per second over this table - the ceiling of the window loop's line rate on this table, on this box, in this process."""
        v = C.c_double()
        check(lib.tbk_classifier_calibrate_pairs(self._h, inflight, waves_per_simd, n_lines, C.byref(v)))
        return v.value

    def last_passes(self) -> Tuple[int, int]:
        """(passes, passes that touch more than one read) of the most recent probe: 2048 window starts each; the
        latter went through the two-read or the multi-read kernel, the rest through the single-read kernel."""
        n, m = C.c_uint64(), C.c_uint64()
        check(lib.tbk_classifier_last_passes(self._h, C.byref(n), C.byref(m)))
        return n.value, m.value

    def close(self) -> None:
        if self._h is not None and self._h.value:
            lib.tbk_classifier_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# one raw run or phase block: tbk_hit_run (include/tbk.h), 32 bytes
HIT_RUN_DTYPE = [("read", "<u8"), ("first", "<u8"), ("last", "<u8"), ("markers", "<u4"), ("hap", "<u4")]
# the same found in homopolymer-compressed space, in the coordinates of the read as given: tbk_hit_run_lifted, 40 bytes
HIT_RUN_LIFTED_DTYPE = [("read", "<u8"), ("first", "<u8"), ("last", "<u8"), ("end", "<u8"), ("markers", "<u4"), ("hap", "<u4")]


class HitTracker:
    """WHERE along each read of a batch the haplotype k-mers lie (``tbk_hit_tracker``).

    A window start is a marker of hapA or hapB by the rule of ``count_kmers_in_read`` (hapA first); a raw run is a
    maximal sequence of one read's markers, in position order, of one haplotype.  The lists are borrowed, as a
    ``Classifier`` borrows them; the tracker owns its device buffers.

    With ``compress=True`` (lists of homopolymer-compressed k-mers) the batch is compressed on the device first, with
    ``fold_case = ignore_case``; markers, runs and counts are those of the compressed batch, and only the coordinates are
    lifted back to the batch as given: a run covers the bases ``[first, end)`` of its read."""

    def __init__(self, kmers_hap_a: HashSet, kmers_hap_b: HashSet):
        h = C.c_void_p()
        check(lib.tbk_hit_tracker_create(kmers_hap_a._h, kmers_hap_b._h, C.byref(h)))
        self._h = h
        self._a, self._b = kmers_hap_a, kmers_hap_b  # keep the tables alive
        self.k = kmers_hap_a.k

    def runs(self, bases: np.ndarray, offsets: np.ndarray, ignore_case: bool = False, compress: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """(runs, counts): the batch's raw runs ordered by (read, first) - a structured array with the fields read, first,
        last (window starts of the first and last marker within the read), markers and hap (0 = A, 1 = B) - and the
        markers per read and list, ``Classifier.classify_batch``'s (n_reads, 2) array.  With ``compress`` the runs have
        ``HIT_RUN_LIFTED_DTYPE``: first and last are the original positions of the first kept byte of the first and last
        marker's windows, ``end`` the original end of the last marker's window; counts are those of the compressed batch."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        counts = np.zeros((n, 2), dtype=np.int32)
        ptr, n_runs = C.c_void_p(), C.c_uint64()
        fn = lib.tbk_hit_tracker_runs_compressed if compress else lib.tbk_hit_tracker_runs
        check(fn(self._h, bases.ctypes.data, offsets.ctypes.data, n, int(bool(ignore_case)), C.byref(ptr), C.byref(n_runs), counts.ctypes.data))
        runs = np.zeros(n_runs.value, dtype=HIT_RUN_LIFTED_DTYPE if compress else HIT_RUN_DTYPE)
        if n_runs.value:
            C.memmove(runs.ctypes.data, ptr.value, runs.nbytes)
        lib.tbk_host_free(ptr)
        return runs, counts

    def marks(self, bases: np.ndarray, offsets: np.ndarray, ignore_case: bool = False, compress: bool = False) -> np.ndarray:
        """One byte per base of the batch: 0 none, 1 A, 2 B for the window that starts there (a read's last k - 1 bytes are 0).
        With ``compress`` the window is one of the compressed read and its mark sits on the first base of the window's
        first run, in the batch as given; every other base is 0."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        marks = np.zeros(int(offsets[-1]) if offsets.size else 0, dtype=np.uint8)
        fn = lib.tbk_hit_tracker_marks_compressed if compress else lib.tbk_hit_tracker_marks
        check(fn(self._h, bases.ctypes.data, offsets.ctypes.data, n, int(bool(ignore_case)), marks.ctypes.data))
        return marks

    def close(self) -> None:
        if self._h is not None and self._h.value:
            lib.tbk_hit_tracker_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def phase_blocks(runs: np.ndarray, min_run: int = 1) -> np.ndarray:
    """Raw runs -> phase blocks, on the host.  Every raw run with fewer than ``min_run`` markers is dropped, in one pass
    that is not repeated; surviving runs that are now neighbours in the same read and of the same haplotype merge into
    one block: ``first`` of the first, ``last`` of the last, the markers added up.  (This project's rule - an isolated
    hit of an error k-mer is one window, a real variant up to k neighbouring ones - not Merqury's short-range-switch rule.)
    Lifted runs (``HIT_RUN_LIFTED_DTYPE``: an ``end`` field) give lifted blocks, a block's ``end`` that of its last run."""
    if min_run < 1:
        raise ValueError("min_run must be at least 1")
    lifted = isinstance(runs, np.ndarray) and runs.dtype.names is not None and "end" in runs.dtype.names
    runs = np.asarray(runs, dtype=HIT_RUN_LIFTED_DTYPE if lifted else HIT_RUN_DTYPE)
    kept = runs[runs["markers"] >= min_run]
    if kept.size == 0:
        return kept.copy()
    head = np.ones(kept.size, dtype=bool)
    head[1:] = (kept["read"][1:] != kept["read"][:-1]) | (kept["hap"][1:] != kept["hap"][:-1])
    starts = np.nonzero(head)[0]
    ends = np.append(starts[1:], kept.size) - 1
    blocks = kept[starts].copy()
    blocks["last"] = kept["last"][ends]
    if lifted:
        blocks["end"] = kept["end"][ends]
    total = np.add.reduceat(kept["markers"].astype(np.uint64), starts)
    blocks["markers"] = np.minimum(total, 0xFFFFFFFF).astype(np.uint32)
    return blocks


def visible_devices() -> list:
    """Device indices a multi-device run uses: TBK_DEVICES ("0,1,2", a device may repeat), else
    every visible device."""
    spec = os.environ.get("TBK_DEVICES", "").strip()
    if spec:
        return [int(x) for x in spec.split(",") if x.strip() != ""]
    return list(range(_lib.device_count()))


class MultiClassifier:
    """Reads dealt over several devices behind ``Classifier``'s interface (tables replicated,
    no collective; the reference's loop, classify_by_kmers.py:99-102, has no cross-read state).

    A thin wrapper over the library's ``tbk_pipeline``: one feeder thread and one stream ring per entry of
    ``devices`` (a device may repeat), one ordered queue.  ``submit`` only queues a batch and returns a
    ticket; the next feeder whose ring has room takes it.  ``wait(ticket)`` returns that batch's counts
    whichever device computed them, so a caller that waits in submission order gets its results in input
    order.  ``depth`` batches may be in flight on the devices; ``depth + len(devices)`` may be submitted
    and not yet waited for.  Nothing per batch happens in Python.
    """

    def __init__(self, kmers_hap_a: HashSet, kmers_hap_b: HashSet, devices: Optional[Sequence[int]] = None, options: Optional[Options] = None):
        devices = list(visible_devices() if devices is None else devices)
        if not devices:
            raise _lib.TbkError(_lib.TBK_ERR_NO_DEVICE, "no HIP device visible; there is no CPU fallback")
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        if _lib.HAS_OPTIONS:
            check(lib.tbk_pipeline_create_opts(kmers_hap_a._h, kmers_hap_b._h, arr, len(devices), _options_ptr(options), C.byref(h)))
        else:
            check(lib.tbk_pipeline_create(kmers_hap_a._h, kmers_hap_b._h, arr, len(devices), C.byref(h)))
        self._h = h
        self._a, self._b = kmers_hap_a, kmers_hap_b  # keep the tables alive
        self._keep = {}
        self._stubs = None
        self.devices = devices
        self.device = devices[0]

    @classmethod
    def from_classifiers(cls, classifiers, ring_depth: Optional[int] = None) -> "MultiClassifier":
        """The same queue and feeder threads over classifier-like Python objects (``submit(bases, offsets)
        -> ticket``, ``wait(ticket) -> counts``): the library's testing hook, no GPU needed."""
        self = cls.__new__(cls)
        parts = list(classifiers)
        self._stubs = parts
        self._keep = {}
        self._a = self._b = None
        self.devices = [getattr(p, "device", None) for p in parts]
        self.device = self.devices[0]
        pending = {}  # (slot, stub ticket) -> (counts pointer, n_reads)

        def on_submit(user, slot, bases, offsets, n_reads, counts, ticket):
            try:
                off = np.ctypeslib.as_array(C.cast(offsets, C.POINTER(C.c_uint64)), (n_reads + 1,))
                total = int(off[n_reads])
                b = np.ctypeslib.as_array(C.cast(bases, C.POINTER(C.c_uint8)), (total,)) if total else np.zeros(0, dtype=np.uint8)
                t = parts[slot].submit(b, off)
                pending[(slot, t)] = (counts, n_reads)
                ticket[0] = t
                return 0
            except Exception as exc:  # reported through the job's status
                self._stub_error = exc
                return _lib.TBK_ERR_STATE

        def on_wait(user, slot, ticket):
            try:
                got = np.ascontiguousarray(parts[slot].wait(ticket), dtype=np.int32)
                ptr, n = pending.pop((slot, ticket))
                if n:
                    C.memmove(ptr, got.ctypes.data, n * 8)
                return 0
            except Exception as exc:
                self._stub_error = exc
                return _lib.TBK_ERR_STATE

        sub_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64))
        wait_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_uint64)
        self._callbacks = (sub_t(on_submit), wait_t(on_wait))  # kept alive with the pipeline
        lib.tbk_pipeline_create_test_.restype = C.c_int
        lib.tbk_pipeline_create_test_.argtypes = [C.c_int, C.c_int, sub_t, wait_t, C.c_void_p, C.POINTER(C.c_void_p)]
        h = C.c_void_p()
        depth = ring_depth if ring_depth is not None else min(getattr(p, "depth", 3) for p in parts)
        check(lib.tbk_pipeline_create_test_(len(parts), depth, self._callbacks[0], self._callbacks[1], None, C.byref(h)))
        self._h = h
        return self

    @property
    def depth(self) -> int:
        return lib.tbk_pipeline_depth(self._h)

    @property
    def dealt(self) -> list:
        """Batches each ring has taken so far."""
        n = lib.tbk_pipeline_devices(self._h)
        out = (C.c_uint64 * n)()
        check(lib.tbk_pipeline_batches(self._h, out, n))
        return [int(x) for x in out]

    def _part(self, slot: int) -> "Classifier":
        c = Classifier.__new__(Classifier)
        c._h = C.c_void_p(lib.tbk_pipeline_classifier(self._h, slot))
        c._a, c._b, c._keep = self._a, self._b, {}
        c.device = lib.tbk_classifier_device(c._h)
        c.close = lambda: None  # the pipeline owns it
        return c

    def stats(self) -> dict:
        st = dict(self._stubs[0].stats() if self._stubs is not None else self._part(0).stats())
        st["devices"] = list(self.devices)
        st["table_bytes_total"] = st.get("table_bytes", 0) * len(set(self.devices))  # the rings of one device share its table
        return st

    def kernel_timing(self, on: bool) -> None:
        for i in range(len(self.devices)):
            self._part(i).kernel_timing(on)

    def kernel_timing_read(self):
        """Summed over the rings: probes, their milliseconds, the single-read kernel's milliseconds."""
        tot = [0, 0.0, 0.0]
        for i in range(len(self.devices)):
            for j, v in enumerate(self._part(i).kernel_timing_read2()):
                tot[j] += v
        return tuple(tot)

    def submit(self, bases: np.ndarray, offsets: np.ndarray) -> int:
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        counts = np.zeros((n, 2), dtype=np.int32)
        ticket = C.c_uint64()
        check(lib.tbk_pipeline_submit(self._h, bases.ctypes.data, offsets.ctypes.data, n, counts.ctypes.data, C.byref(ticket)))
        self._keep[ticket.value] = (bases, offsets, counts)
        return ticket.value

    def submit_packed(self, packed: PackedBatch, counts: Optional[np.ndarray] = None) -> int:
        if counts is None:
            counts = np.zeros((packed.n_reads, 2), dtype=np.int32)
        ticket = C.c_uint64()
        check(lib.tbk_pipeline_submit_packed(self._h, packed.codes.ctypes.data, packed.exc_chunk.ctypes.data, packed.exc_mask.ctypes.data,
                                             packed.exc_chunk.size, packed.offsets.ctypes.data, packed.n_reads, counts.ctypes.data, C.byref(ticket)))
        self._keep[ticket.value] = (packed, None, counts)
        return ticket.value

    def submit_batch(self, batch) -> int:
        """Submit a ``seq.Batch``: in the packed transfer format when the reader made it, else its ASCII bases."""
        counts = np.zeros((batch.n_reads, 2), dtype=np.int32)
        ticket = C.c_uint64()
        bases_ptr, off_ptr = batch.pointers()
        packed = batch.packed_pointers() if self._stubs is None else None
        if packed is not None:
            codes, exc_chunk, exc_mask, n_exc = packed
            check(lib.tbk_pipeline_submit_packed(self._h, C.c_void_p(codes), C.c_void_p(exc_chunk), C.c_void_p(exc_mask), n_exc,
                                                 C.c_void_p(off_ptr), batch.n_reads, counts.ctypes.data, C.byref(ticket)))
        else:
            check(lib.tbk_pipeline_submit(self._h, C.c_void_p(bases_ptr), C.c_void_p(off_ptr), batch.n_reads, counts.ctypes.data, C.byref(ticket)))
        self._keep[ticket.value] = (batch, None, counts)
        return ticket.value

    def wait(self, ticket: int) -> np.ndarray:
        try:
            check(lib.tbk_pipeline_wait(self._h, ticket, None))
        except _lib.TbkError:
            exc, self._stub_error = getattr(self, "_stub_error", None), None
            if exc is not None:
                raise exc
            raise
        return self._keep.pop(ticket)[2]

    wait_ticket = wait

    def classify_batch(self, bases: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        return self.wait(self.submit(bases, offsets))

    def classify_reads(self, seqs: Sequence[str]) -> np.ndarray:
        return self.classify_batch(*pack_reads(seqs))

    def classify_file(self, reads_path: str, num_kmers_a: int, num_kmers_b: int, out_names: Sequence[str], gzip_output: bool,
                      gzip_level: int = -1, tsv_fd: int = 1, batch_bases: int = 0, batch_reads: int = 0) -> dict:
        """The whole read / classify / write loop of classify-by-kmers on native threads (``tbk_classify_file``);
        the TSV goes to ``tsv_fd``.  ``gzip_output`` 2: BAM bins from BAM input (``classify-by-kmers --bam-output``); 3: one BAM file,
        ``out_names[0]``, of every read's record tagged with its bin and counts (``--haplotag-output``).  Returns the run's statistics."""

        class Stats(C.Structure):
            _fields_ = [("reads", C.c_uint64), ("bases", C.c_uint64), ("batches", C.c_uint64), ("read_s", C.c_double),
                        ("gpu_wait_s", C.c_double), ("write_s", C.c_double), ("total_s", C.c_double), ("gzip_encoder", C.c_int32), ("_pad", C.c_int32)]

        st = Stats()
        a, b, u = [os.fsencode(n) for n in out_names]
        check(lib.tbk_classify_file(self._h, os.fsencode(reads_path), num_kmers_a, num_kmers_b, a, b, u, int(gzip_output) if gzip_output in (2, 3) else int(bool(gzip_output)), gzip_level,
                                    tsv_fd, batch_bases, batch_reads, C.byref(st)))
        out = {name: getattr(st, name) for name, _ in Stats._fields_ if name != "_pad"}
        out["gzip_encoder"] = {0: None, 1: "host", 2: "device"}.get(st.gzip_encoder)   # who coded the bins' gzip members
        return out

    def sync(self) -> None:
        pass  # every ticket that was waited for is complete; there is nothing else in flight to wait for

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value:
            lib.tbk_pipeline_destroy(h)
        if self._stubs is not None:
            for p in self._stubs:
                p.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


Pipeline = MultiClassifier


class _PinnedOwner:
    """Frees a tbk_host_alloc block when the array that views it is collected."""

    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        try:
            lib.tbk_host_free(C.c_void_p(self.ptr))
        except Exception:
            pass


def host_threads() -> int:
    """Host threads worth starting (hardware threads within the affinity mask and the cgroup quota)."""
    return int(lib.tbk_host_threads())


def device_mem_info(device: Optional[int] = None) -> Tuple[int, int]:
    """(free, total) bytes of HBM on the device."""
    free, total = C.c_uint64(), C.c_uint64()
    check(lib.tbk_device_mem_info(default_device() if device is None else device, C.byref(free), C.byref(total)))
    return free.value, total.value


class KmerCounter:
    """Counting table of canonical k-mers in HBM: the database `kmc` builds for the reference's
    find-unique-kmers step (find_unique_kmers.py:62-103), with the histogram, subtraction and dump
    `kmc_tools` / `kmc_dump` provide (find_unique_kmers.py:123-129,186-194,218-225).

    ``passes`` > 1 counts a library whose distinct k-mers outgrow one table: the k-mers fall into that many
    classes, the reads are kept on the device in packed form (0.5 bytes per base, at most ``store_limit`` bytes if
    given), and one class at a time goes through a table sized for a class (``tbk_counter_create_opts`` in
    include/tbk.h).  Results are those of one pass; ``unique`` needs both counters made with the same ``passes``.

    ``compress`` counts in homopolymer-compressed space: every batch goes through ``HomopolymerCompressor`` (case folded)
    before its k-mers are cut, ``bases_added`` counts the bases that are left, and the database says so (``KmerDatabase.compressed``);
    ``unique`` needs both counters to agree on it.

    ``keep_singletons`` makes ``database()`` a FULL database: the k-mers seen once are entries too (counters 1..255), so two
    such databases can be united exactly (``KmerDatabase.union``).  Histogram and ``unique`` answer as without it."""

    def __init__(self, k: int, capacity: int, device: Optional[int] = None, passes: int = 1, store_limit: int = 0, compress: bool = False,
                 keep_singletons: bool = False):
        self._h = C.c_void_p()
        self.k = k
        self.passes = passes
        self.compress = bool(compress)
        self.keep_singletons = bool(keep_singletons)
        self.device = default_device() if device is None else device
        if passes == 1 and not store_limit and not compress and not keep_singletons:
            check(lib.tbk_counter_create(k, capacity, self.device, C.byref(self._h)))
        else:
            opts = _lib.CounterOptions()
            lib.tbk_counter_options_init(C.byref(opts))
            opts.passes, opts.store_limit_bytes, opts.compress = passes, store_limit, int(self.compress)
            opts.keep_singletons = int(self.keep_singletons)
            check(lib.tbk_counter_create_opts(k, capacity, C.byref(opts), self.device, C.byref(self._h)))

    def add_reads(self, reads: Sequence[str]) -> None:
        bases, offsets = pack_reads(reads)
        self.add(bases, offsets)

    def add(self, bases: np.ndarray, offsets: np.ndarray) -> None:
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        check(lib.tbk_counter_add_batch(self._h, bases.ctypes.data, offsets.ctypes.data, offsets.size - 1))

    def add_batch(self, batch) -> None:
        """Count a ``seq.Batch`` straight from its (pinned) buffers."""
        bases_ptr, off_ptr = batch.pointers()
        check(lib.tbk_counter_add_batch(self._h, C.c_void_p(bases_ptr), C.c_void_p(off_ptr), batch.n_reads))

    def add_device(self, d_bases: int, d_offsets: int, n_reads: int, total_bases: int) -> None:
        check(lib.tbk_counter_add_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_reads, total_bases))

    def kernel_timing(self, reset: bool = True) -> Tuple[int, int, float]:
        """(launches, window starts, total ms) of the counting kernel since the last reset."""
        n, w, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        check(lib.tbk_counter_kernel_timing(self._h, C.byref(n), C.byref(w), C.byref(ms), int(reset)))
        return n.value, w.value, ms.value

    def finish(self) -> None:
        """No more reads.  With ``passes`` > 1 this counts the remaining classes and frees the kept reads and the
        table (``histogram`` and ``unique`` do it themselves when it has not been done)."""
        check(lib.tbk_counter_finish(self._h))

    def histogram(self) -> np.ndarray:
        """hist[c], c = 1..255: distinct k-mers whose counter (capped at 255) is c; hist[0]: all."""
        hist = np.zeros(256, dtype=np.uint64)
        check(lib.tbk_counter_histogram(self._h, hist.ctypes.data_as(C.POINTER(C.c_uint64))))
        return hist

    def stats(self) -> dict:
        v = [C.c_uint64() for _ in range(4)]
        check(lib.tbk_counter_stats(self._h, *[C.byref(x) for x in v]))
        info = _lib.CounterInfo(size=C.sizeof(_lib.CounterInfo))
        check(lib.tbk_counter_stats_ex(self._h, C.byref(info)))  # (its `distinct` never finishes a counter working in passes)
        p = [C.c_int() for _ in range(4)]
        check(lib.tbk_counter_params(self._h, *[C.byref(x) for x in p]))
        st = dict(zip(("n_slots", "table_bytes", "bases_added", "reads_added", "distinct", "w", "m", "o", "t"),
                      [x.value for x in v] + [info.distinct] + [x.value for x in p]))
        for name in ("passes", "finished", "store_bytes", "store_used_bytes", "peak_table_bytes", "database_bytes"):
            st[name] = int(getattr(info, name))
        return st

    def unique(self, other: "KmerCounter", min_count: int, max_count: int, out_path: str) -> int:
        """Write the k-mers this library saw at least twice, with a counter in [min_count,
        max_count], that `other` saw at most once; one per line, sorted.  Returns how many."""
        n = C.c_uint64()
        check(lib.tbk_counter_unique(self._h, other._h, min_count, max_count, os.fsencode(out_path), C.byref(n)))
        return n.value

    def database(self) -> "KmerDatabase":
        """The counter's database as an object of its own (``tbk_counter_export``): it outlives the counter, which
        takes no more reads afterwards.  A one-pass counter still answers ``histogram`` and ``unique`` as before."""
        h = C.c_void_p()
        check(lib.tbk_counter_export(self._h, C.byref(h)))
        return KmerDatabase(h)

    def close(self) -> None:
        if self._h is not None and self._h.value:
            h, self._h = self._h, None
            lib.tbk_counter_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def database_file_info(path: str) -> dict:
    """Header of a ``*.tbkdb`` file, checked (``tbk_kmerdb_file_info``); touches no device.  ``IOError`` for a file
    that cannot be read, ``ValueError`` for one that is not a sound database."""
    k, n, reads, bases = C.c_int(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    hist = np.zeros(256, dtype=np.uint64)
    check(lib.tbk_kmerdb_file_info(os.fsencode(path), C.byref(k), C.byref(n), hist.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   C.byref(reads), C.byref(bases)))
    flag = C.c_int()
    check(lib.tbk_kmerdb_file_compressed(os.fsencode(path), C.byref(flag)))
    floor = C.c_int()
    check(lib.tbk_kmerdb_file_floor(os.fsencode(path), C.byref(floor)))
    return {"k": k.value, "n": n.value, "histogram": hist, "reads_added": reads.value, "bases_added": bases.value,
            "compressed": bool(flag.value), "floor": floor.value}


def dump_file_k(path: str) -> int:
    """k of a counted k-mer dump (``KMER<tab or space>COUNT`` lines): the bytes before the first separator of line 1
    (``tbk_dump_file_k``); touches no device.  ``IOError`` for a file that cannot be read, ``ValueError`` for an empty one,
    a first line without a separator or a k outside 1..32."""
    k = C.c_int()
    check(lib.tbk_dump_file_k(os.fsencode(path), C.byref(k)))
    return k.value


def dump_import_stats() -> dict:
    """Running totals of this process's dump imports (``tbk_dump_import_stats``)."""
    imports, sorts, windows, lines, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
    check(lib.tbk_dump_import_stats(C.byref(imports), C.byref(sorts), C.byref(windows), C.byref(lines), C.byref(ms)))
    return {"imports": imports.value, "sorts": sorts.value, "windows": windows.value, "lines": lines.value, "parse_ms": ms.value}


def load_solid_database(path: str, device: Optional[int] = None) -> "KmerDatabase":
    """A ``*.tbkdb`` file for a consumer that works on k-mers seen at least twice (the list builders, the classifier's lists,
    the phase blocks): a full file is loaded, turned solid (``KmerDatabase.solid``) and freed, so what comes back is what the
    solid file of the same reads would have given."""
    db = KmerDatabase.load(path, device)
    if db.floor >= 2:
        return db
    try:
        return db.solid()
    finally:
        db.close()


# tbk_hetmer_pair (include/tbk.h): 24 bytes
HETMER_PAIR_DTYPE = np.dtype([("minor", "<u8"), ("major", "<u8"), ("c_minor", "u1"), ("c_major", "u1"), ("cls_minor", "u1"), ("cls_major", "u1"),
                              ("reserved", "u1", (4,))])


class KmerDatabase:
    """What a ``KmerCounter`` leaves behind, kept: the k-mers seen at least twice as ascending lexicographic ranks
    with their counters (2..255) in HBM, and the counter's whole histogram - the ``haplotypeA.*`` database `kmc`
    leaves under --outpath in the reference (find_unique_kmers.py:247).  It goes to a ``*.tbkdb`` file and comes
    back checked (include/tbk.h), and ``unique`` re-dumps from it at any cut-offs without counting again."""

    def __init__(self, handle):
        self._h = handle
        k, n, device = C.c_int(), C.c_uint64(), C.c_int()
        check(lib.tbk_kmerdb_info(self._h, C.byref(k), C.byref(n), C.byref(device), None))
        self.k, self._n, self.device = k.value, n.value, device.value
        flag = C.c_int()
        check(lib.tbk_kmerdb_compressed(self._h, C.byref(flag)))
        self.compressed = bool(flag.value)  # counted in homopolymer-compressed space: its file has another magic, and it mixes with no plain one
        floor = C.c_int()
        check(lib.tbk_kmerdb_floor(self._h, C.byref(floor)))
        self.floor = floor.value  # 2, or 1: a full database, which holds the k-mers seen once too (``KmerCounter(keep_singletons=True)``)

    @classmethod
    def load(cls, path: str, device: Optional[int] = None) -> "KmerDatabase":
        h = C.c_void_p()
        check(lib.tbk_kmerdb_load(os.fsencode(path), default_device() if device is None else device, C.byref(h)))
        return cls(h)

    @classmethod
    def from_dump(cls, paths, k: Optional[int] = None, floor="auto", compressed: bool = False, reads: int = 0, bases: int = 0,
                  device: Optional[int] = None, window_bytes: int = 0) -> "KmerDatabase":
        """The database of one or several counted dumps - ``kmc_dump``, ``meryl print``, ``jellyfish dump -c``: one
        ``KMER<tab or space>COUNT`` line per k-mer - parsed, made canonical, ordered and folded on the device
        (``tbk_kmerdb_import_text``; include/tbk.h has the line rule).  ``k`` None: taken from the first line.  ``floor``:
        1 keeps the k-mers seen once (a full database), 2 leaves them out, "auto" is 1 when the dump holds any.  ``ValueError``
        names the file and the first offending line."""
        if isinstance(paths, (str, bytes, os.PathLike)):
            paths = [paths]
        paths = [os.fsencode(p) for p in paths]
        if floor not in ("auto", 0, 1, 2):
            raise ValueError("floor = {!r}: one of 'auto', 1, 2".format(floor))
        o = _lib.DumpOptions()
        lib.tbk_dump_options_init(C.byref(o))
        o.k = 0 if k is None else int(k)
        o.floor = 0 if floor == "auto" else int(floor)
        o.compressed = 1 if compressed else 0
        o.reads, o.bases, o.window_bytes = int(reads), int(bases), int(window_bytes)
        arr = (C.c_char_p * len(paths))(*paths)
        h = C.c_void_p()
        check(lib.tbk_kmerdb_import_text(arr, len(paths), C.byref(o), default_device() if device is None else device, C.byref(h)))
        return cls(h)

    def dump(self, path: str, min_count: int = 1, max_count: int = 255) -> int:
        """What ``kmc_dump -ciMIN -cxMAX`` writes: ``KMER<tab>COUNT`` lines in lexicographic order for the entries whose
        counter lies in [max(floor, min_count), min(255, max_count)] (``tbk_kmerdb_dump_text``).  Returns the lines written."""
        n = C.c_uint64()
        check(lib.tbk_kmerdb_dump_text(self._h, max(0, min(int(min_count), 0xFFFFFFFF)), max(0, min(int(max_count), 0xFFFFFFFF)),
                                       os.fsencode(path), C.byref(n)))
        return n.value

    def __len__(self) -> int:
        return self._n

    def save(self, path: str) -> None:
        check(lib.tbk_kmerdb_save(self._h, os.fsencode(path)))

    def histogram(self) -> np.ndarray:
        """The histogram of the counter the database came from (``KmerCounter.histogram``), all 256 rows."""
        hist = np.zeros(256, dtype=np.uint64)
        check(lib.tbk_kmerdb_histogram(self._h, hist.ctypes.data_as(C.POINTER(C.c_uint64))))
        return hist

    def stats(self) -> dict:
        reads, bases, nbytes = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib.tbk_kmerdb_stats(self._h, C.byref(reads), C.byref(bases)))
        check(lib.tbk_kmerdb_info(self._h, None, None, None, C.byref(nbytes)))
        return {"reads_added": reads.value, "bases_added": bases.value, "bytes": nbytes.value}

    def entries(self, first: int = 0, count: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(keys uint64, counts uint8) of ``count`` entries from ``first`` on (default: all that follow)."""
        if count is None:
            count = max(0, self._n - first)
        keys, counts = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint8)
        check(lib.tbk_kmerdb_read(self._h, first, count, keys.ctypes.data, counts.ctypes.data))
        return keys, counts

    def unique(self, other: "KmerDatabase", min_count: int, max_count: int, out_path: str,
               child: Optional["KmerDatabase"] = None, child_min: int = 2, child_max: int = 255) -> int:
        """``KmerCounter.unique`` between two databases: the same file.  With ``child`` (a third database) only the k-mers
        that the child holds with a counter in [child_min, child_max] are written (``tbk_kmerdb_inherited``)."""
        n = C.c_uint64()
        if child is None:
            check(lib.tbk_kmerdb_unique(self._h, other._h, min_count, max_count, os.fsencode(out_path), C.byref(n)))
        else:
            check(lib.tbk_kmerdb_inherited(self._h, other._h, child._h, min_count, max_count, child_min, child_max,
                                           os.fsencode(out_path), C.byref(n)))
        return n.value

    def unique_set(self, other: "KmerDatabase", min_count: int, max_count: int,
                   child: Optional["KmerDatabase"] = None, child_min: int = 2, child_max: int = 255) -> HashSet:
        """The list ``unique`` would write, as the ``HashSet`` ``create_kmer_hash_set`` would make of that file - the same keys
        in the same order - without the text in between (``tbk_kmerdb_unique_table``): selected, compacted and packed where
        the databases lie.  ``ValueError`` ("empty k-mer list") when nothing is selected, as for an empty list file.  With
        ``child`` the list holds the inherited k-mers only, as ``unique`` does (``tbk_kmerdb_inherited_table``)."""
        h = C.c_void_p()
        if child is None:
            check(lib.tbk_kmerdb_unique_table(self._h, other._h, min_count, max_count, C.byref(h)))
        else:
            check(lib.tbk_kmerdb_inherited_table(self._h, other._h, child._h, min_count, max_count, child_min, child_max, C.byref(h)))
        return HashSet(h.value)

    def union(self, other: "KmerDatabase") -> "KmerDatabase":
        """The database of both read sets (``tbk_kmerdb_union``): exactly what one count of both would have left.  Both must
        be full (``floor == 1``), of one k, one device and one space; ``ValueError`` otherwise."""
        h = C.c_void_p()
        check(lib.tbk_kmerdb_union(self._h, other._h, C.byref(h)))
        return KmerDatabase(h)

    def solid(self) -> "KmerDatabase":
        """From a full database the one the same counter would have left without ``keep_singletons`` (``tbk_kmerdb_solid``):
        the entries seen at least twice, the histogram as it is."""
        h = C.c_void_p()
        check(lib.tbk_kmerdb_solid(self._h, C.byref(h)))
        return KmerDatabase(h)

    def joint_spectrum(self, other: "KmerDatabase") -> np.ndarray:
        """The joint k-mer spectrum of two databases (``tbk_kmerdb_joint_spectrum``), shape (256, 256), uint64: cell
        ``[cx, cy]`` is the number of distinct k-mers with counter ``cx`` here and ``cy`` in ``other``, 0 standing for "holds no
        entry" (below the floor, or never seen).  Either floor in either place; one k, one device and one space, ``ValueError``
        otherwise."""
        spec = np.zeros((256, 256), dtype=np.uint64)
        check(lib.tbk_kmerdb_joint_spectrum(self._h, other._h, spec.ctypes.data))
        return spec

    def origin_spectrum(self, y: "KmerDatabase", z: "KmerDatabase", y_range: Tuple[int, int] = (1, 255),
                        z_range: Tuple[int, int] = (1, 255)) -> np.ndarray:
        """This database's entries by counter and by which of two partners hold them (``tbk_kmerdb_origin_spectrum``), shape
        (4, 256), uint64: row ``cls`` has bit 0 set when ``y`` holds the k-mer with a counter in ``y_range`` (inclusive, taken
        literally: 1 <= min <= max <= 255), bit 1 the same for ``z``.  ``ValueError`` for a range outside that, or databases
        of different k, device or space."""
        bounds = [int(v) for v in (*y_range, *z_range)]
        if any(not 0 <= v <= 0xFFFFFFFF for v in bounds):
            raise ValueError("counter ranges {} and {}: need 1 <= min <= max <= 255".format(tuple(y_range), tuple(z_range)))
        spec = np.zeros((4, 256), dtype=np.uint64)
        check(lib.tbk_kmerdb_origin_spectrum(self._h, y._h, bounds[0], bounds[1], z._h, bounds[2], bounds[3], spec.ctypes.data))
        return spec

    def gc_spectrum(self) -> np.ndarray:
        """This database's entries by GC content and by counter (``tbk_kmerdb_gc_spectrum``), shape (k + 1, 256), uint64: cell
        ``[g, c]`` is the number of k-mers with ``g`` G-or-C bases and counter ``c`` - k-mer multiplicity against GC, the matrix
        ``kat gcp`` plots.  Column 0 is 0, column ``c >= 1`` sums to ``histogram()[c]`` from the floor on, and the whole matrix
        to ``len(self)``.  Either floor, either space; an empty database gives zeros."""
        spec = np.zeros((33, 256), dtype=np.uint64)
        check(lib.tbk_kmerdb_gc_spectrum(self._h, spec.ctypes.data))
        return spec[:self.k + 1].copy()

    def select(self, min_count: int = 1, max_count: int = 255, require=(), exclude=(), counter: str = "base",
               gc: Optional[Tuple[Optional[int], Optional[int]]] = None) -> "KmerDatabase":
        """A selection of this database's entries that is a database again (``tbk_kmerdb_select``): those with a counter in
        [min_count, max_count] that every partner of ``require`` holds with a counter in that partner's range and no partner
        of ``exclude`` does.  A partner is ``(KmerDatabase, min, max)`` or a bare ``KmerDatabase``, which means
        ``(db, 1, 255)``; ranges are taken literally, 1 <= min <= max <= 255; at most two partners in all (chain calls for
        more).  ``counter``: "base" keeps this database's counters, "min" takes the minimum with the ``require`` partners',
        "sum" adds them, capped at 255.  ``gc``: ``(lo, hi)`` keeps only the k-mers with lo..hi G-or-C bases (bases, not per
        cent; 0 <= lo <= hi <= 32, a bound above k never binds, and either may be None for "no bound"); the default is no
        bound.  The result is a full database (``floor == 1``) in this database's order, of its k and
        space, with ``reads_added == bases_added == 0``; it may be empty.  ``ValueError`` for a range, rule or number of
        partners outside that, or databases of different k, device or space."""
        if counter not in _lib.SELECT_COUNTERS:
            raise ValueError("counter = {!r}: one of 'base', 'min', 'sum'".format(counter))
        asked = []
        for mode, group in ((_lib.SELECT_REQUIRE, require), (_lib.SELECT_EXCLUDE, exclude)):
            for partner in group:
                db, lo, hi = (partner, 1, 255) if isinstance(partner, KmerDatabase) else partner
                asked.append((db, int(lo), int(hi), mode))
        if len(asked) > 2:
            raise ValueError("{} partners: a selection takes at most two (chain calls for more)".format(len(asked)))
        bounds = [int(min_count), int(max_count)] + [v for _, lo, hi, _ in asked for v in (lo, hi)]
        if any(not 0 <= v <= 0xFFFFFFFF for v in bounds):
            raise ValueError("counter ranges {}: need 1 <= min <= max <= 255".format(list(zip(bounds[::2], bounds[1::2]))))
        o = _lib.SelectOptions()
        lib.tbk_select_options_init(C.byref(o))
        o.min_count, o.max_count, o.counter = bounds[0], bounds[1], _lib.SELECT_COUNTERS[counter]
        if gc is not None:
            lo, hi = (0 if gc[0] is None else int(gc[0])), (32 if gc[1] is None else int(gc[1]))
            if not (0 <= lo <= 0xFFFFFFFF and 0 <= hi <= 0xFFFFFFFF):
                raise ValueError("GC range {}: need 0 <= min <= max <= 32".format((lo, hi)))
            o.min_gc, o.max_gc = lo, hi
        partners = (_lib.SelectPartner * max(1, len(asked)))()
        for slot, (db, lo, hi, mode) in zip(partners, asked):
            slot.db, slot.min_count, slot.max_count, slot.mode = (db._h.value if db._h is not None else None), lo, hi, mode
        h = C.c_void_p()
        check(lib.tbk_kmerdb_select(self._h, partners, len(asked), C.byref(o), C.byref(h)))
        return KmerDatabase(h)

    def hetmers(self, min_count: int, max_count: int, y: Optional["KmerDatabase"] = None, z: Optional["KmerDatabase"] = None,
                y_range: Tuple[int, int] = (1, 255), z_range: Tuple[int, int] = (1, 255), pairs: bool = False) -> dict:
        """The het-mer pairs inside this database (``tbk_kmerdb_hetmers``; include/tbk.h has the definitions): among the entries
        with a counter in [min_count, max_count] - the candidates - those that differ from exactly one other candidate in the
        middle base alone, which is what the two alleles of a heterozygous SNP leave.  k must be odd.  Returns a dict:
        ``candidates`` and ``pairs`` (int); ``partners``, shape (4,): candidates by number of middle partners among the
        candidates; ``spec``, shape (256, 256): pairs by the counter of the minor (row) and the major member (column);
        ``origin``, shape (4, 4): pairs by the class of the minor (row) and the major member, bit 0 of a class set when ``y``
        holds that k-mer with a counter in ``y_range``, bit 1 the same for ``z`` (a partner left out contributes 0).  All uint64.
        With ``pairs=True`` also ``records``: a structured array (``HETMER_PAIR_DTYPE``: minor, major as ranks, c_minor, c_major,
        cls_minor, cls_major), ascending by the rank of each pair's lower-ranked member.  ``ValueError`` for an even k, a range
        outside 1 <= min <= max <= 255, or partners of another k, device or space."""
        bounds = [int(v) for v in (min_count, max_count, *y_range, *z_range)]
        if any(not 0 <= v <= 0xFFFFFFFF for v in bounds):
            raise ValueError("counter ranges {}: need 1 <= min <= max <= 255".format(list(zip(bounds[::2], bounds[1::2]))))
        o, res = _lib.HetmerOptions(), _lib.HetmerResult()
        lib.tbk_hetmer_options_init(C.byref(o))
        lib.tbk_hetmer_result_init(C.byref(res))
        o.min_count, o.max_count, o.y_min, o.y_max, o.z_min, o.z_max = bounds
        o.y = None if y is None else y._h.value
        o.z = None if z is None else z._h.value
        o.want_pairs = int(bool(pairs))
        spec = np.zeros((256, 256), dtype=np.uint64)
        ptr = C.c_void_p()
        check(lib.tbk_kmerdb_hetmers(self._h, C.byref(o), C.byref(res), spec.ctypes.data, C.byref(ptr)))
        out = {"candidates": int(res.candidates), "pairs": int(res.pairs), "partners": np.array(list(res.partners), dtype=np.uint64),
               "spec": spec, "origin": np.array(list(res.origin), dtype=np.uint64).reshape(4, 4)}
        if pairs:
            records = np.zeros(int(res.pairs), dtype=HETMER_PAIR_DTYPE)
            if ptr.value:
                C.memmove(records.ctypes.data, ptr.value, records.nbytes)
            out["records"] = records
        lib.tbk_host_free(ptr)
        return out

    def query(self, copies: bool = False) -> "DatabaseQuery":
        """A session that scores sequences against this database (``DatabaseQuery``); ``copies`` keeps a 32-bit counter
        per entry for the copy spectrum (4 bytes per k-mer more)."""
        return DatabaseQuery(self, copies)

    def close(self) -> None:
        if self._h is not None and self._h.value:
            h, self._h = self._h, None
            lib.tbk_kmerdb_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HomopolymerCompressor:
    """Every run of equal bases of a read written once, on the device (``tbk_hpc``, include/tbk.h): byte i of a read is kept
    iff it is the read's first or differs from the byte before it - with ``fold_case`` compared as if letters were upper
    case, but written as it came.  Runs end at read boundaries; empty reads stay; bytes outside ACGT are compared like any
    others.  The counter compresses with ``fold_case`` on, the classifier with it off (lower case stays not-ACGT there).
    The session owns its buffers; a result stays valid until the session's next call."""

    def __init__(self, device: Optional[int] = None):
        self._h = C.c_void_p()
        self.device = default_device() if device is None else device
        check(lib.tbk_hpc_create(self.device, C.byref(self._h)))
        self._n_reads = 0
        self._total_given = self._total = 0  # bases of the batch the last result was made of, and of the result (``expand``: out, in)

    def _call(self, fn, n_reads, total_given, *args):
        d_bases, d_offsets, total = C.c_void_p(), C.c_void_p(), C.c_uint64()
        check(fn(self._h, *args, C.byref(d_bases), C.byref(d_offsets), C.byref(total)))
        self._n_reads, self._total_given, self._total = n_reads, int(total_given), total.value
        return d_bases.value or 0, d_offsets.value or 0, total.value

    def compress_host(self, bases: np.ndarray, offsets: np.ndarray, fold_case: bool = False) -> Tuple[int, int, int]:
        """A host batch in, the result left on the device: (d_bases, d_offsets, total) for ``Classifier.submit_device``,
        ``KmerCounter.add_device`` and the like."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.size - 1, 0)
        return self._call(lib.tbk_hpc_compress, n, offsets[-1] if n else 0, bases.ctypes.data, offsets.ctypes.data, n, int(bool(fold_case)))

    def compress_batch(self, batch, fold_case: bool = False) -> Tuple[int, int, int]:
        """``compress_host`` for a ``seq.Batch``, straight from its (pinned) buffers."""
        bases_ptr, off_ptr = batch.pointers()
        n = batch.n_reads
        total_given = C.cast(off_ptr, C.POINTER(C.c_uint64))[n] if n else 0
        return self._call(lib.tbk_hpc_compress, n, total_given, C.c_void_p(bases_ptr), C.c_void_p(off_ptr), n, int(bool(fold_case)))

    def compress_device(self, d_bases: int, d_offsets: int, n_reads: int, total_bases: int, fold_case: bool = False) -> Tuple[int, int, int]:
        """The same for a batch already in HBM (``d_bases`` 16-byte aligned)."""
        return self._call(lib.tbk_hpc_compress_device, n_reads, total_bases if n_reads else 0, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_reads, total_bases, int(bool(fold_case)))

    def fetch(self, total: int) -> Tuple[np.ndarray, np.ndarray]:
        """The last result as numpy arrays (``total``: what the compress call returned)."""
        bases, offsets = np.zeros(total, dtype=np.uint8), np.zeros(self._n_reads + 1, dtype=np.uint64)
        check(lib.tbk_hpc_fetch(self._h, bases.ctypes.data, total, offsets.ctypes.data))
        return bases, offsets

    def lift(self, positions: np.ndarray) -> np.ndarray:
        """Positions of the last result's compressed bases -> positions of the batch it was made of: kept byte j came from
        input position lift(j), and the compressed total lifts to the input's total.  Any order, duplicates allowed; a
        position above the compressed total is refused."""
        positions = np.ascontiguousarray(positions, dtype=np.uint64)
        out = np.zeros(positions.shape, dtype=np.uint64)
        check(lib.tbk_hpc_lift(self._h, positions.ctypes.data, positions.size, out.ctypes.data))
        return out

    def expand(self, values: np.ndarray) -> np.ndarray:
        """One byte per compressed base of the last result in, one per base of the batch as given out: a kept position
        gets the byte of its compressed position, every other position 0."""
        values = np.ascontiguousarray(values, dtype=np.uint8)
        if values.size != self._total:
            raise ValueError("expand: {} values for {} compressed bases".format(values.size, self._total))
        out = np.zeros(self._total_given, dtype=np.uint8)
        check(lib.tbk_hpc_expand(self._h, values.ctypes.data, out.ctypes.data))
        return out

    def compress(self, bases: np.ndarray, offsets: np.ndarray, fold_case: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """(bases, offsets) of the compressed batch, as numpy."""
        return self.fetch(self.compress_host(bases, offsets, fold_case)[2])

    def close(self) -> None:
        if self._h is not None and self._h.value:
            h, self._h = self._h, None
            lib.tbk_hpc_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# one bin of a copy-number track (``tbk_depth_bin``, 24 bytes)
DEPTH_BIN = np.dtype([("clean", "<u4"), ("absent", "<u4"), ("saturated", "<u4"), ("collapsed", "<u4"), ("expanded", "<u4"),
                      ("depth", "u1"), ("copies", "u1"), ("pad", "u1", (2,))])
assert DEPTH_BIN.itemsize == 24

# one stretch of broken windows and its repair candidates (``tbk_repair``, 40 bytes)
REPAIR = np.dtype([("read", "<u8"), ("first", "<u8"), ("pos", "<u8"), ("windows", "<u4"), ("accepted", "<u2"), ("kind", "u1"), ("base", "u1"),
                   ("support", "u1"), ("depth", "u1"), ("pad", "u1", (6,))])
assert REPAIR.itemsize == 40
REPAIR_NONE, REPAIR_SUB, REPAIR_DEL, REPAIR_INS, REPAIR_LONG = range(5)

# one sequence's k-mer evidence (``tbk_read_evidence``, 40 bytes)
READ_EVIDENCE = np.dtype([("clean", "<u8"), ("held", "<u8"), ("covered", "<u8"), ("longest", "<u8"), ("stretches", "<u8")])
assert READ_EVIDENCE.itemsize == 40

# one sequence's k-mer depth (``tbk_read_depth``, 40 bytes)
READ_DEPTH = np.dtype([("clean", "<u8"), ("present", "<u8"), ("saturated", "<u8"), ("sum", "<u8"), ("lowest", "u1"), ("q1", "u1"), ("median", "u1"),
                       ("q3", "u1"), ("highest", "u1"), ("present_median", "u1"), ("pad", "u1", (2,))])
assert READ_DEPTH.itemsize == 40

# one piece of a sequence (``tbk_read_piece``, 24 bytes): the positions [first, end) of sequence ``read``
READ_PIECE = np.dtype([("read", "<u8"), ("first", "<u8"), ("end", "<u8")])
assert READ_PIECE.itemsize == 24
PIECES_SIDES = {"covered": 0, "uncovered": 1}
PIECES_WHICH = {"all": 0, "longest": 1}


class DatabaseQuery:
    """How often did the reads see the k-mers of these sequences?  (``tbk_kmerdb_query``, include/tbk.h.)

    Every window start of a sequence whose k bases are ACGT, either case, is *clean*; its canonical k-mer's counter in
    the database is ``c``, 2..255, or 0 when the database does not hold it.  The session borrows the database and keeps
    on its device a directory over the ranks, one *seen* bit per entry, the histogram of ``c`` over all clean windows
    added so far and, with ``copies``, a copy counter per entry.  At most 2^32 - 1 window starts between two resets."""

    def __init__(self, database: "KmerDatabase", copies: bool = False):
        h = C.c_void_p()
        check(lib.tbk_kmerdb_query_create(database._h, int(bool(copies)), C.byref(h)))
        self._h = h
        self._db = database  # keep the database alive
        self.k = database.k
        self.copies = bool(copies)

    def add(self, bases: np.ndarray, offsets: np.ndarray, min_count: int = 2, return_counts: bool = False):
        """Look a batch up and add it to the session.  (n, 2) uint64: per sequence its clean windows and, of those, the found
        ones (``c >= min_count``).  With ``return_counts`` the pair (that array, the bytes of ``counts``) from one lookup."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.size - 1, 0)
        per_read = np.zeros((n, 2), dtype=np.uint64)
        counts = np.zeros(int(offsets[-1]) if offsets.size else 0, dtype=np.uint8) if return_counts else None
        check(lib.tbk_kmerdb_query_add(self._h, bases.ctypes.data, offsets.ctypes.data, n, min_count, per_read.ctypes.data,
                                       counts.ctypes.data if return_counts else None))
        return (per_read, counts) if return_counts else per_read

    def counts(self, bases: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        """One byte per base of the batch: ``c`` of the window that starts there, 0 when it is absent or not clean (a
        sequence's last k - 1 bytes are 0).  This is ``add`` bringing other answers home: the batch is added to the session."""
        return self.add(bases, offsets, 2, True)[1]

    def histogram(self) -> np.ndarray:
        """The clean windows added so far by their counter, 256 rows; row 0: absent."""
        hist = np.zeros(256, dtype=np.uint64)
        check(lib.tbk_kmerdb_query_histogram(self._h, hist.ctypes.data))
        return hist

    def completeness(self, min_count: int = 2, max_count: int = 255) -> Tuple[int, int]:
        """(seen, solid): the database's k-mers with a counter in [min_count, max_count] (clamped to 2..255), and those of
        them that a window added so far was."""
        seen, solid = C.c_uint64(), C.c_uint64()
        check(lib.tbk_kmerdb_query_completeness(self._h, min_count, max_count, C.byref(seen), C.byref(solid)))
        return seen.value, solid.value

    def copy_spectrum(self) -> np.ndarray:
        """(6, 256) uint64: ``[min(copies, 5), counter]`` = k-mers of the database that the sequences hold that many times
        (row 5: more than four) - the assembly's k-mer spectrum.  ``ValueError`` for a session made without ``copies``."""
        spec = np.zeros((6, 256), dtype=np.uint64)
        check(lib.tbk_kmerdb_query_copy_spectrum(self._h, spec.ctypes.data))
        return spec

    def track(self, bases: np.ndarray, offsets: np.ndarray, window: int, peak: int) -> Tuple[np.ndarray, np.ndarray]:
        """The copy-number track of a batch (``tbk_kmerdb_query_track``, include/tbk.h): per bin of ``window`` window starts
        the clean, absent and saturated windows, the lower medians ``depth`` (of ``c``) and ``copies`` (of the session's
        copy counter, capped at 255) over the present ones, and the windows that read as ``collapsed`` -
        ``2c > (2a + 1) peak`` - or ``expanded`` - ``a >= 1`` and ``2c < (2a - 1) peak``; ``peak`` is the read depth of a
        k-mer the sequences should hold once.  Returns (bins as a ``DEPTH_BIN`` array, uint64 prefix of ``n + 1`` entries):
        the bins of sequence ``r`` are ``bins[prefix[r]:prefix[r + 1]]``.  The session is only read.  ``ValueError`` for a
        session made without ``copies`` and for a ``window`` or ``peak`` below 1."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.size - 1, 0)
        window, peak = int(window), int(peak)
        if not self.copies or not 1 <= window < 1 << 32 or not 1 <= peak < 1 << 32:
            # the library's own refusal and message, for the values a C uint32_t can carry
            check(lib.tbk_kmerdb_query_track(self._h, None, None, 0, min(max(window, 0), 0xFFFFFFFF), min(max(peak, 0), 0xFFFFFFFF), None, 0))
            raise ValueError("track: window {} and peak {} must lie in 1 .. 2^32 - 1".format(window, peak))
        lengths = np.diff(offsets.astype(np.int64)) if n else np.zeros(0, dtype=np.int64)
        starts = np.maximum(lengths - self.k + 1, 0)
        prefix = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum((starts + window - 1) // window, out=prefix[1:])
        bins = np.zeros(int(prefix[-1]), dtype=DEPTH_BIN)
        check(lib.tbk_kmerdb_query_track(self._h, bases.ctypes.data, offsets.ctypes.data, n, window, peak, bins.ctypes.data, bins.size))
        return bins, prefix

    def repairs(self, bases: np.ndarray, offsets: np.ndarray, min_count: int = 2, min_support: int = 1) -> np.ndarray:
        """The repair candidates of a batch (``tbk_kmerdb_query_repairs``, include/tbk.h): one ``REPAIR`` record per maximal
        stretch of broken windows - clean, with ``c`` below ``max(floor, min_count)`` - ordered by (read, first).  ``windows`` is
        the stretch's length, ``accepted`` the number of one-base edits at the positions all its windows share that leave
        every window over the edit held by the database, with at least ``min_support`` clean windows to say so; ``kind``
        (``REPAIR_NONE``, ``_SUB``, ``_DEL``, ``_INS``, or ``_LONG`` for a stretch of more than k windows, which is not attempted),
        ``pos``, ``base``, ``support`` and ``depth`` describe the smallest accepted edit by (kind, pos, base).  The session is
        only read.  ``ValueError`` for a ``min_count`` outside 1..255 or a ``min_support`` outside 1..32."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.size - 1, 0)
        min_count, min_support = int(min_count), int(min_support)
        ptr, count = C.c_void_p(), C.c_uint64()
        if not 0 <= min_count < 1 << 32 or not 0 <= min_support < 1 << 32:
            # the library's own refusal and message, for the values a C uint32_t can carry
            check(lib.tbk_kmerdb_query_repairs(self._h, None, None, 0, min(max(min_count, 0), 0xFFFFFFFF), min(max(min_support, 0), 0xFFFFFFFF),
                                               C.byref(ptr), C.byref(count)))
            raise ValueError("repairs: min_count {} must lie in 1 .. 255 and min_support {} in 1 .. 32".format(min_count, min_support))
        check(lib.tbk_kmerdb_query_repairs(self._h, bases.ctypes.data, offsets.ctypes.data, n, min_count, min_support, C.byref(ptr), C.byref(count)))
        try:
            records = np.zeros(count.value, dtype=REPAIR)
            if count.value:
                C.memmove(records.ctypes.data, ptr, count.value * REPAIR.itemsize)
        finally:
            lib.tbk_host_free(ptr)
        return records

    def evidence(self, bases: np.ndarray, offsets: np.ndarray, min_count: int = 1, max_count: int = 255) -> np.ndarray:
        """The k-mer evidence of a batch of reads (``tbk_kmerdb_query_evidence``, include/tbk.h): one ``READ_EVIDENCE`` record per
        sequence.  ``clean`` counts its clean windows and ``held`` those of them whose counter lies in
        ``[max(floor, min_count), max_count]``; ``covered`` counts the bases that lie in a held window, ``stretches`` the maximal
        runs of such bases and ``longest`` the longest of them.  A sequence shorter than k gets five zeros.  The session is only
        read.  ``ValueError`` for a ``min_count`` outside 1..255 or a ``max_count`` outside ``min_count``..255."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.size - 1, 0)
        min_count, max_count = int(min_count), int(max_count)
        if not 0 <= min_count < 1 << 32 or not 0 <= max_count < 1 << 32:
            # the library's own refusal and message, for the values a C uint32_t can carry
            check(lib.tbk_kmerdb_query_evidence(self._h, None, None, 0, min(max(min_count, 0), 0xFFFFFFFF), min(max(max_count, 0), 0xFFFFFFFF), None))
            raise ValueError("evidence: min_count {} must lie in 1 .. 255 and max_count {} in min_count .. 255".format(min_count, max_count))
        records = np.zeros(n, dtype=READ_EVIDENCE)
        check(lib.tbk_kmerdb_query_evidence(self._h, bases.ctypes.data, offsets.ctypes.data, n, min_count, max_count, records.ctypes.data))
        return records

    def pieces(self, bases: np.ndarray, offsets: np.ndarray, min_count: int = 1, max_count: int = 255, side: str = "covered", which: str = "all",
               min_length: int = 1, evidence: bool = False):
        """The pieces of a batch of reads (``tbk_kmerdb_query_pieces``, include/tbk.h): the maximal runs ``[first, end)`` of
        consecutive positions of one sequence that are covered (``side="covered"``) or are not (``"uncovered"``), as a
        ``READ_PIECE`` array ordered by (read, first).  Covered is the read evidence's: a position in a clean window whose counter
        lies in ``[max(floor, min_count), max_count]``.  Pieces shorter than ``min_length`` are left out; with ``which="longest"``
        only the longest of a sequence's remaining pieces comes home, the first among equals.  With ``evidence`` the pair (pieces,
        the ``READ_EVIDENCE`` records of ``evidence()`` for the same arguments) from one lookup.  The session is only read.
        ``ValueError`` for a ``min_count`` outside 1..255, a ``max_count`` outside ``min_count``..255, a ``min_length`` outside
        0..2^64 - 1 and a ``side`` or ``which`` that is not one of the words."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.size - 1, 0)
        min_count, max_count, min_length = int(min_count), int(max_count), int(min_length)
        if side not in PIECES_SIDES or which not in PIECES_WHICH:
            raise ValueError("pieces: side {!r} must be one of {} and which {!r} one of {}".format(side, sorted(PIECES_SIDES), which, sorted(PIECES_WHICH)))
        if not 1 <= min_count <= 255 or not min_count <= max_count <= 255:
            raise ValueError("pieces: min_count {} must lie in 1 .. 255 and max_count {} in min_count .. 255".format(min_count, max_count))
        if not 0 <= min_length < 1 << 64:
            raise ValueError("pieces: min_length {} must lie in 0 .. 2^64 - 1".format(min_length))
        records = np.zeros(n, dtype=READ_EVIDENCE) if evidence else None
        ptr, count = C.c_void_p(), C.c_uint64()
        check(lib.tbk_kmerdb_query_pieces(self._h, bases.ctypes.data, offsets.ctypes.data, n, min_count, max_count, PIECES_SIDES[side], PIECES_WHICH[which],
                                          min_length, records.ctypes.data if evidence else None, C.byref(ptr), C.byref(count)))
        try:
            pieces = np.zeros(count.value, dtype=READ_PIECE)
            if count.value:
                C.memmove(pieces.ctypes.data, ptr, count.value * READ_PIECE.itemsize)
        finally:
            lib.tbk_host_free(ptr)
        return (pieces, records) if evidence else pieces

    def read_depth(self, bases: np.ndarray, offsets: np.ndarray, min_count: int = 1) -> np.ndarray:
        """The k-mer depth of a batch of reads (``tbk_kmerdb_query_read_depth``, include/tbk.h): one ``READ_DEPTH`` record per
        sequence.  The depth of a clean window is its counter when that is ``max(floor, min_count)`` or more, else 0.  ``clean``
        counts the clean windows, ``present`` those of depth 1 or more and ``saturated`` those of depth 255; ``sum`` is the sum of
        the depths, and ``lowest``, ``q1``, ``median``, ``q3`` and ``highest`` are the sorted depths at the ranks
        ``j * (clean - 1) // 4``, ``j`` = 0..4 - the median is the lower one; ``present_median`` is the lower median of the present
        windows' depths, 0 when there are none.  A sequence without a clean window gets an all-zero record.  The session is only
        read.  ``ValueError`` for a ``min_count`` outside 1..255."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.size - 1, 0)
        min_count = int(min_count)
        if not 0 <= min_count < 1 << 32:
            # the library's own refusal and message, for the values a C uint32_t can carry
            check(lib.tbk_kmerdb_query_read_depth(self._h, None, None, 0, min(max(min_count, 0), 0xFFFFFFFF), None))
            raise ValueError("read_depth: min_count {} must lie in 1 .. 255".format(min_count))
        records = np.zeros(n, dtype=READ_DEPTH)
        check(lib.tbk_kmerdb_query_read_depth(self._h, bases.ctypes.data, offsets.ctypes.data, n, min_count, records.ctypes.data))
        return records

    def reset(self) -> None:
        """Forget every batch: the next assembly against the same database."""
        check(lib.tbk_kmerdb_query_reset(self._h))

    def close(self) -> None:
        if self._h is not None and self._h.value:
            h, self._h = self._h, None
            lib.tbk_kmerdb_query_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def qv(found: int, clean: int, k: int) -> float:
    """Merqury's consensus quality value from k-mer counts: ``-10 log10(1 - (found / clean) ** (1 / k))`` - ``inf`` when
    every clean window was found, ``nan`` when there is none."""
    import math

    if clean == 0:
        return float("nan")
    if found >= clean:
        return float("inf")
    return -10.0 * math.log10(1.0 - (found / clean) ** (1.0 / k)) + 0.0  # (+ 0.0: nothing found is 0.0, not -0.0)


def pinned_empty(shape, dtype) -> np.ndarray:
    """A numpy array backed by pinned host memory (hipHostMalloc through the C-ABI), so that
    async copies to/from the GPU need no staging copy.  Freed with the array."""
    dtype = np.dtype(dtype)
    count = int(np.prod(shape))
    nbytes = max(count * dtype.itemsize, 1)
    ptr = lib.tbk_host_alloc(nbytes)
    if not ptr:
        raise MemoryError(_lib.last_error())
    buf = (C.c_char * nbytes).from_address(ptr)
    buf._tbk_owner = _PinnedOwner(ptr)  # the array keeps `buf` alive through .base
    return np.frombuffer(buf, dtype=dtype, count=count).reshape(shape)


def score_and_bin(counts: np.ndarray, num_kmers_a: int, num_kmers_b: int):
    """Scores and bins for a batch (classify_by_kmers.py:57-77,104-115), float64, in the
    reference's operation order.  Returns (score_a, score_b, bins) with bins a bytes object
    over b"ABU"."""
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    n = counts.shape[0]
    sa = np.zeros(n, dtype=np.float64)
    sb = np.zeros(n, dtype=np.float64)
    bins = C.create_string_buffer(n + 1)
    check(lib.tbk_score_and_bin(counts.ctypes.data, n, num_kmers_a, num_kmers_b, sa.ctypes.data, sb.ctypes.data, bins))
    return sa, sb, bins.raw[:n]
