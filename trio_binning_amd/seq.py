"""FASTA/FASTQ(.gz) or BAM records in, three bins out.

Host-side mirror of the reference's ``trio_binning.seq`` (src/trio_binning/seq.py):
``Read``, ``readfq``, ``open_fastx_read`` and ``open_outfiles`` with the same record
semantics and output bytes, written as an explicit line state machine.  The record rules
below are the observable behaviour of the reference parser (seq.py:45-83), including its
corner cases, because the bins must be byte-identical:

* a record starts at a line whose first character is ``>`` or ``@``; the name is the
  header without that character, cut at the first space (not tab);
* every line loses its last character, newline or not (a file without a final newline
  loses its last base / quality value);
* sequence lines run until a line starting with ``@``, ``+`` or ``>``; only ``+`` makes the
  record FASTQ;
* quality lines are taken until their summed length reaches the sequence length;
  running out of input first turns the record into FASTA (qual ``None``) and ends parsing;
* a header or separator line that is empty after losing its last character counts as
  "no line" (end of input).
"""
import gzip
import sys
from dataclasses import dataclass
from typing import IO, Iterable, Iterator, List, Optional, TextIO, Tuple, Union


@dataclass
class Read:
    """A fastx read"""

    name: str
    """The name of the read"""
    seq: str
    """The sequence of the read"""
    qual: Optional[str] = None
    """The quality score string of the read"""

    def __str__(self) -> str:
        # reference seq.py:27-31: FASTQ when there is a non-empty quality string
        if self.qual:
            return "@" + self.name + "\n" + self.seq + "\n+\n" + self.qual
        return ">" + self.name + "\n" + self.seq

    def print(self, file: TextIO = sys.stdout) -> None:
        """Print the read in fastq format if it has qualities, else fasta (seq.py:33-42)."""
        file.write(str(self))
        file.write("\n")


_SEEK, _SEQ, _QUAL = 0, 1, 2


def readfq(fp: Iterable[str]) -> Iterator[Read]:
    """Read a fast[aq] stream, yielding a ``Read`` per record (reference seq.py:45-83)."""
    state = _SEEK
    name = ""
    parts: List[str] = []
    seq = ""
    have = 0
    for line in fp:
        head = line[0] if line else ""
        body = line[:-1]
        if state == _SEEK:
            if head == ">" or head == "@":
                if not body:  # header that vanishes with its last character: input ends here
                    return
                name = body[1:].partition(" ")[0]
                parts = []
                state = _SEQ
            continue
        if state == _SEQ:
            if head == "@" or head == "+" or head == ">":
                seq = "".join(parts)
                if not body:  # separator/header reduced to nothing: FASTA record, then stop
                    yield Read(name, seq, None)
                    return
                if head == "+":
                    parts = []
                    have = 0
                    state = _QUAL
                else:
                    yield Read(name, seq, None)
                    name = body[1:].partition(" ")[0]
                    parts = []
            else:
                parts.append(body)
            continue
        # _QUAL
        parts.append(body)
        have += len(line) - 1
        if have >= len(seq):
            yield Read(name, seq, "".join(parts))
            state = _SEEK
    # input exhausted
    if state == _SEQ:
        yield Read(name, "".join(parts), None)
    elif state == _QUAL:
        yield Read(name, seq, None)  # not enough quality: emitted as FASTA (seq.py:81-83)


def open_fastx_read(filename: str) -> Iterator[Read]:
    """Open a fasta/q(.gz) file for reading (reference seq.py:86-92): gzip by file name,
    text mode with universal newlines.  A name ending in ``.bam`` is an unaligned BAM file: its reads come from the native
    reader's batches (include/tbk.h "BAM input")."""
    if filename.endswith(".bam"):
        return _native_reads(filename)
    if filename.endswith(".gz"):
        return readfq(gzip.open(filename, "rt"))
    return readfq(open(filename, "r"))


def _native_reads(filename: str) -> Iterator[Read]:
    with BatchReader(filename) as reader:
        batch = Batch()
        try:
            while reader.next_batch(batch, 1 << 24, 0):
                yield from batch.reads()
        finally:
            batch.close()


TextOrGzip = Union[TextIO, IO[str]]


def output_names(
    haplotype_a_prefix: str,
    haplotype_b_prefix: str,
    unclassified_prefix: str,
    outfile_extension: str,
    gzip_output: bool,
) -> Tuple[str, str, str]:
    """File names of the three bins: prefix + extension (+ ``.gz``), seq.py:117-134."""
    tail = outfile_extension + (".gz" if gzip_output else "")
    return haplotype_a_prefix + tail, haplotype_b_prefix + tail, unclassified_prefix + tail


def open_outfiles(
    haplotype_a_prefix: str,
    haplotype_b_prefix: str,
    unclassified_prefix: str,
    outfile_extension: str,
    gzip_output: bool,
) -> Tuple[TextOrGzip, TextOrGzip, TextOrGzip]:
    """Open the three output bins (reference seq.py:98-136).

    Deviation, on purpose: with ``gzip_output=False`` the reference opens its haplotype-B
    handle on the haplotype-A file name (seq.py:129), so B reads overwrite the front of
    the A file and no B file is created.  Here B goes to the B file.  Gzip mode (the
    default) is identical to the reference: ``gzip.open(name + ".gz", "wt")``.
    """
    names = output_names(haplotype_a_prefix, haplotype_b_prefix, unclassified_prefix, outfile_extension, gzip_output)
    if gzip_output:
        return tuple(gzip.open(n, "wt") for n in names)  # type: ignore[return-value]
    return tuple(open(n, "w") for n in names)  # type: ignore[return-value]


# ---- native batch I/O (C-ABI tbk_fastx_* / tbk_bin_writer_*) --------------------------------
# The same records and the same output bytes as readfq / Read.print above, produced by the
# library in the batch layout the classifier consumes; used by the CLI driver.  Imported
# lazily so that this module stays importable without the built library.
class Batch:
    """One batch of records read by ``BatchReader`` (owned by the native library)."""

    def __init__(self):
        import ctypes as C

        from ._lib import check, lib

        h = C.c_void_p()
        check(lib.tbk_fastx_batch_create(C.byref(h)))
        self._h = h
        self.n_reads = 0

    def _view(self):
        import ctypes as C

        from ._lib import check, lib

        n = C.c_uint64()
        ptrs = [C.c_void_p() for _ in range(7)]
        check(lib.tbk_fastx_batch_view(self._h, C.byref(n), *[C.byref(p) for p in ptrs]))
        return n.value, [p.value for p in ptrs]

    def arrays(self):
        """(bases, base_off, names, name_off, quals, qual_off, has_qual) as numpy views that
        stay valid until the batch is refilled or destroyed.  A borrowed batch has no sequence / quality
        arrays of its own: `bases` and `quals` are then copies gathered from the reader's mapping."""
        import ctypes as C

        import numpy as np

        from ._lib import check, lib

        n, (bases, boff, names, noff, quals, qoff, hq) = self._view()

        def arr(ptr, count, dtype):
            if count == 0:
                return np.zeros(0, dtype=dtype)
            ct = {np.uint8: C.c_uint8, np.uint64: C.c_uint64}[dtype]
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(count,))

        base_off = arr(boff, n + 1, np.uint64)
        name_off = arr(noff, n + 1, np.uint64)
        qual_off = arr(qoff, n + 1, np.uint64)
        if self.borrowed:
            bases_a = np.zeros(int(base_off[-1]), dtype=np.uint8)
            quals_a = np.zeros(int(qual_off[-1]), dtype=np.uint8)
            check(lib.tbk_fastx_batch_gather(self._h, bases_a.ctypes.data, bases_a.size, quals_a.ctypes.data, quals_a.size))
        else:
            bases_a, quals_a = arr(bases, int(base_off[-1]), np.uint8), arr(quals, int(qual_off[-1]), np.uint8)
        return (bases_a, base_off, arr(names, int(name_off[-1]), np.uint8), name_off, quals_a, qual_off, arr(hq, n, np.uint8))

    @property
    def borrowed(self) -> bool:
        """The batch's records lie in its reader's mapping of the input (``BatchReader(..., borrowing=True)``)."""
        from ._lib import lib

        return bool(lib.tbk_fastx_batch_borrowed(self._h))

    def pointers(self):
        """(bases_ptr, base_off_ptr) for tbk_stream_submit."""
        if self.borrowed:
            raise ValueError("a borrowed batch has no ASCII bases array: submit its packed form (packed_pointers)")
        _, p = self._view()
        return p[0], p[1]

    def packed_pointers(self):
        """(codes_ptr, exc_chunk_ptr, exc_mask_ptr, n_exc) of the batch's packed transfer form, or None when the
        reader did not make one (``BatchReader(..., packing=True)``)."""
        import ctypes as C

        from ._lib import check, lib

        codes, ec, em, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        check(lib.tbk_fastx_batch_packed(self._h, C.byref(codes), C.byref(ec), C.byref(em), C.byref(n)))
        if not codes.value:
            return None
        return codes.value, ec.value, em.value, n.value

    def packed_arrays(self):
        """(codes, exc_chunk, exc_mask) as numpy copies (tests), or None."""
        import ctypes as C

        import numpy as np

        p = self.packed_pointers()
        if p is None:
            return None
        total = int(self.arrays()[1][-1])
        n_chunks = (total + 15) // 16
        codes = np.ctypeslib.as_array(C.cast(p[0], C.POINTER(C.c_uint32)), (max(n_chunks, 1),))[:n_chunks].copy()
        ec = np.ctypeslib.as_array(C.cast(p[1], C.POINTER(C.c_uint32)), (max(p[3], 1),))[:p[3]].copy()
        em = np.ctypeslib.as_array(C.cast(p[2], C.POINTER(C.c_uint16)), (max(p[3], 1),))[:p[3]].copy()
        return codes, ec, em

    def records(self) -> List[bytes]:
        """The reads' BAM records, whole (``block_size`` and all that follows), one per read in the batch's order; empty
        when the batch carries none (``BatchReader(..., keep_records=True)`` on a ``.bam`` file)."""
        import ctypes as C

        from ._lib import lib

        recs, offs = C.c_void_p(), C.c_void_p()
        if not lib.tbk_fastx_batch_records(self._h, C.byref(recs), C.byref(offs)) or not offs.value:
            return []
        off = C.cast(offs, C.POINTER(C.c_uint64))
        return [C.string_at(recs.value + off[i], off[i + 1] - off[i]) for i in range(self.n_reads)]

    def reads(self) -> List[Read]:
        """The batch as ``Read`` objects (tests; the CLI never materialises them)."""
        bases, boff, names, noff, quals, qoff, hq = self.arrays()
        out = []
        for i in range(self.n_reads):
            name = bytes(names[int(noff[i]):int(noff[i + 1])]).decode()
            sq = bytes(bases[int(boff[i]):int(boff[i + 1])]).decode()
            ql = bytes(quals[int(qoff[i]):int(qoff[i + 1])]).decode() if hq[i] else None
            out.append(Read(name, sq, ql))
        return out

    def close(self):
        if self._h is not None and self._h.value:
            from ._lib import lib

            lib.tbk_fastx_batch_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchReader:
    """Native FASTA/FASTQ(.gz) or BAM reader: ``next_batch(batch, max_bases, max_reads)`` fills a
    ``Batch`` and returns the number of records (0 at end of input).  A name ending in ``.bam`` is read as unaligned BAM."""

    def __init__(self, filename: str, packing: bool = False, borrowing: bool = False, device: Optional[int] = None, keep_records: bool = False):
        """``keep_records``: BAM input only (refused for any other file) - every batch also carries its reads' records, whole
        (``Batch.records``), for ``BinWriter(..., bam_header=...)``.
        ``device``: BGZF input is inflated on that GPU, and BAM records are turned into FASTQ text there (``tbk_fastx_set_device``: what ``classify-by-kmers`` does by itself),
        and with ``TBK_GZIP_INFLATE=gpu`` an ordinary gzip file as well (``gzip_stats``); None: on the host's threads.
        ``inflates_on_device`` says which it is."""
        import ctypes as C
        import os

        from ._lib import check, lib

        h = C.c_void_p()
        check(lib.tbk_fastx_open(os.fsencode(filename), C.byref(h)))
        self._h = h
        if device is not None:
            check(lib.tbk_fastx_set_device(h, device))
        self.inflates_on_device = bool(lib.tbk_fastx_inflates_on_device(h)) if hasattr(lib, "tbk_fastx_inflates_on_device") else False
        if packing:  # batches also carry the packed transfer form of their bases (Batch.packed_pointers)
            check(lib.tbk_fastx_set_packing(h, 1))
        if borrowing:  # batches of a plain FASTQ file leave their records in the reader's mapping (what the native loop does):
            check(lib.tbk_fastx_set_borrowing(h, 1))  # no sequence / quality arrays; valid until close()
        if keep_records:
            try:
                check(lib.tbk_fastx_set_keep_records(h, 1))
            except Exception:
                self.close()
                raise

    def bam_header(self) -> bytes:
        """The header bytes of a BAM input, ``BAM\\1`` through the last reference entry (read now if no batch has been yet)."""
        import ctypes as C

        from ._lib import check, lib

        ptr, n = C.c_void_p(), C.c_uint64()
        check(lib.tbk_fastx_bam_header(self._h, C.byref(ptr), C.byref(n)))
        return C.string_at(ptr.value, n.value)

    def next_batch(self, batch: Batch, max_bases: int = 0, max_reads: int = 0) -> int:
        import ctypes as C

        from ._lib import check, lib

        check(lib.tbk_fastx_next(self._h, batch._h, max_bases, max_reads))
        n = C.c_uint64()
        check(lib.tbk_fastx_batch_view(batch._h, C.byref(n), None, None, None, None, None, None, None))
        batch.n_reads = n.value
        return n.value

    def close(self):
        if self._h is not None and self._h.value:
            from ._lib import lib

            lib.tbk_fastx_close(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def gzip_stats(self) -> dict:
        """The GPU gzip inflater's counts for this reader so far (``gzip_inflate_stats``'s keys); zeros when it is not in use."""
        import ctypes as C

        from ._lib import lib

        out = (C.c_uint64 * 6)()
        if self._h:
            lib.tbk_fastx_gzip_stats(self._h, out)
        return dict(zip(("windows", "guessed", "accepted", "redecoded", "handed_back", "most_accepted"), (int(v) for v in out)))

    def bam_counts(self) -> Optional[Tuple[int, int]]:
        """(records seen so far, of them skipped) of a reader whose file is BAM; None for any other."""
        import ctypes as C

        from ._lib import lib

        out = (C.c_uint64 * 2)()
        if not self._h or not lib.tbk_fastx_bam_counts(self._h, out):
            return None
        return int(out[0]), int(out[1])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


NativeReader = BatchReader


class BinWriter:
    """Native writer of the three bins (same names, same decompressed bytes as
    ``open_outfiles`` + ``Read.print``); gzip members are deflated in parallel."""

    def __init__(self, haplotype_a_prefix: str, haplotype_b_prefix: str, unclassified_prefix: str,
                 outfile_extension: str, gzip_output: bool, level: int = -1, threads: int = 0, device: Optional[int] = None,
                 bam_header: Optional[bytes] = None, haplotag_path: Optional[str] = None):
        """``haplotag_path`` (with ``bam_header``): the haplotag form (include/tbk.h "Haplotag output") - ONE BAM file of that name and
        no bins; the prefixes and the extension are not used, and batches are written with ``write_counts``.
        ``bam_header``: BAM bins (include/tbk.h "BAM output") - the files are ``prefix + outfile_extension`` as given (``.bam``), begin
        with these header bytes, and ``write`` takes batches that carry their records (``BatchReader(..., keep_records=True)``).
        ``device``: code the gzip members on that GPU (``tbk_bin_writer_use_device``: what ``classify-by-kmers`` does by itself);
        None: on the host's threads.  ``gpu_encoder`` says which it is."""
        import ctypes as C
        import os

        from ._lib import check, lib

        self.names = output_names(haplotype_a_prefix, haplotype_b_prefix, unclassified_prefix, outfile_extension, gzip_output and bam_header is None)
        h = C.c_void_p()
        if haplotag_path is not None:
            if bam_header is None:
                raise ValueError("BinWriter: the haplotag form needs the input's BAM header (bam_header)")
            self.names = [haplotag_path]
            check(lib.tbk_bin_writer_open_haplotag(os.fsencode(haplotag_path), bam_header, len(bam_header), level, threads, C.byref(h)))
        elif bam_header is not None:
            check(lib.tbk_bin_writer_open_bam(*[os.fsencode(n) for n in self.names], bam_header, len(bam_header), level, threads, C.byref(h)))
        else:
            check(lib.tbk_bin_writer_open(*[os.fsencode(n) for n in self.names], int(gzip_output), level, threads, C.byref(h)))
        self._h = h
        if device is not None:
            check(lib.tbk_bin_writer_use_device(h, device))
        self.gpu_encoder = bool(lib.tbk_bin_writer_encoder(h)) if hasattr(lib, "tbk_bin_writer_encoder") else False
        self.gpu_rewriter = bool(lib.tbk_bin_writer_rewriter(h)) if hasattr(lib, "tbk_bin_writer_rewriter") else False

    def write(self, batch: Batch, bins: bytes) -> None:
        from ._lib import check, lib

        check(lib.tbk_bin_writer_write(self._h, batch._h, bins))

    def write_pieces(self, batch: Batch, pieces, bins: bytes, suffix: bool = False) -> None:
        """The batch's records cut to their pieces (``tbk_bin_writer_write_pieces``, include/tbk.h "read pieces"): ``pieces`` is a
        ``kmers.READ_PIECE`` array ordered by (read, first), ``bins`` one byte per READ - an ``A`` read's pieces go to the first file
        (none: nothing is written), a ``B`` read goes whole to the second and any other whole to the third.  With ``suffix`` a piece
        ``[f, e)`` that is not its whole record is named ``name:f+1-e``."""
        import numpy as np

        from ._lib import check, lib

        pieces = np.ascontiguousarray(pieces)
        if pieces.dtype.itemsize != 24 or pieces.ndim != 1:
            raise ValueError("write_pieces: pieces must be a one-dimensional array of 24-byte records (kmers.READ_PIECE)")
        check(lib.tbk_bin_writer_write_pieces(self._h, batch._h, pieces.ctypes.data if pieces.size else None, pieces.size, bins, int(bool(suffix))))

    def write_counts(self, batch: Batch, bins: bytes, counts) -> None:
        """The haplotag form's ``write``: ``counts`` is the batch's (n_reads, 2) int32 array, as ``Classifier.wait`` returns it."""
        import numpy as np

        from ._lib import check, lib

        counts = np.ascontiguousarray(counts, dtype=np.int32)
        if counts.shape != (batch.n_reads, 2):
            raise ValueError("write_counts: counts must have shape ({}, 2), not {}".format(batch.n_reads, counts.shape))
        check(lib.tbk_bin_writer_write_counts(self._h, batch._h, bins, counts.ctypes.data))

    def close(self) -> None:
        if self._h is not None and self._h.value:
            from ._lib import check, lib

            h, self._h = self._h, None
            check(lib.tbk_bin_writer_close(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def format_tsv(batch: Batch, bins: bytes, score_a, score_b) -> str:
    """``name\\tbin\\tscoreA\\tscoreB`` lines for a batch, floats formatted as Python's str()."""
    import ctypes as C

    from ._lib import check, lib

    need = C.c_size_t()
    check(lib.tbk_format_tsv(batch._h, bins, score_a.ctypes.data, score_b.ctypes.data, None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value + 1)
    check(lib.tbk_format_tsv(batch._h, bins, score_a.ctypes.data, score_b.ctypes.data, buf, need.value + 1, C.byref(need)))
    return buf.raw[: need.value].decode()


def gzip_members_device(pieces, device: int = 0):
    """Each of ``pieces`` (bytes) as one gzip member, coded on the GPU (``tbk_gzip_members_device``: the bin writer's encoder by
    itself).  Returns the members as a list of bytes; ``gzip.decompress`` of each gives the piece back."""
    import ctypes as C

    from ._lib import check, lib

    text = b"".join(pieces)
    n = len(pieces)
    lens = (C.c_uint64 * max(1, n))(*[len(p) for p in pieces])
    out_lens = (C.c_uint64 * max(1, n))()
    need = C.c_uint64()
    cap = len(text) + len(text) // 8 + 1100 * (len(text) // 8192 + 1) + 64 * n + 1024
    buf = C.create_string_buffer(cap)
    check(lib.tbk_gzip_members_device(device, text, lens, n, buf, cap, out_lens, C.byref(need)))
    out, at = [], 0
    for i in range(n):
        out.append(C.string_at(C.addressof(buf) + at, out_lens[i]))
        at += out_lens[i]
    return out


def _bgzf_members(call, data: bytes, hints):
    import ctypes as C

    from ._lib import TBK_ERR_NOMEM, check

    hints = list(hints or ())
    h = (C.c_uint64 * max(1, len(hints)))(*hints)
    need, n = C.c_uint64(), C.c_uint64()
    cap = len(data) + 128 * (len(data) // 65280 + 1) + 64
    buf = C.create_string_buffer(cap)
    status = call(data, len(data), h, len(hints), buf, cap, C.byref(need), C.byref(n))
    if status == TBK_ERR_NOMEM and need.value > cap:
        cap = need.value
        buf = C.create_string_buffer(cap)
        status = call(data, len(data), h, len(hints), buf, cap, C.byref(need), C.byref(n))
    check(status)
    return C.string_at(C.addressof(buf), need.value), n.value


def bgzf_members_device(data: bytes, hints=None, device: int = 0):
    """``data`` as bgzf blocks of at most 65280 bytes of payload, coded on the GPU (``tbk_bgzf_members_device``: the BAM bin writer's
    encoder by itself; no BAM header, no end-of-file marker).  ``hints``: non-decreasing offsets into ``data`` where the kind of
    the bytes changes - a deflate block may end there.  Returns (the blocks back to back, how many)."""
    from ._lib import lib

    return _bgzf_members(lambda *a: lib.tbk_bgzf_members_device(device, *a), data, hints)


def bgzf_members_host(data: bytes, hints=None):
    """The same by the host's coder (``tbk_bgzf_members``): same contract, same cut rule, no GPU."""
    from ._lib import lib

    return _bgzf_members(lib.tbk_bgzf_members, data, hints)


def bgzf_inflate_device(data: bytes, device: int = 0) -> bytes:
    """The text of a bgzf file (bytes), inflated on the GPU (``tbk_bgzf_inflate_device``: the reader's bgzf path by itself)."""
    import ctypes as C

    from ._lib import check, lib

    n = C.c_uint64()
    status = lib.tbk_bgzf_inflate_device(device, data, len(data), None, 0, C.byref(n))
    if n.value == 0:
        check(status)
        return b""
    buf = C.create_string_buffer(n.value)
    check(lib.tbk_bgzf_inflate_device(device, data, len(data), buf, n.value, C.byref(n)))
    return C.string_at(C.addressof(buf), n.value)


def _bam_fastq(call, records: bytes, offsets, skip_flags: int):
    import ctypes as C

    from ._lib import check

    n = len(offsets)
    offs = (C.c_uint64 * max(1, n))(*offsets)
    need, written, skipped = C.c_uint64(), C.c_uint64(), C.c_uint64()
    status = call(records, len(records), offs, n, skip_flags, None, 0, C.byref(need), C.byref(written), C.byref(skipped))
    if need.value == 0:
        check(status)
        return b"", written.value, skipped.value
    buf = C.create_string_buffer(need.value)
    check(call(records, len(records), offs, n, skip_flags, buf, need.value, C.byref(need), C.byref(written), C.byref(skipped)))
    return C.string_at(C.addressof(buf), need.value), written.value, skipped.value


def bam_fastq_device(records: bytes, offsets, skip_flags: int = 0x900, device: int = 0):
    """(FASTQ text, records written, records skipped) of a run of whole BAM records (bytes; ``offsets``: where each begins),
    made on the GPU (``tbk_bam_fastq_device``: the reader's BAM kernels by themselves)."""
    from ._lib import lib

    return _bam_fastq(lambda *a: lib.tbk_bam_fastq_device(device, *a), records, offsets, skip_flags)


def bam_haplotag_status(records: bytes, offsets, bins: bytes, counts, device: Optional[int] = 0, cap: Optional[int] = None):
    """``tbk_bam_haplotag_device`` on ``device`` (None: ``tbk_bam_haplotag``, the host's rewriter) without an exception raised:
    (status, the bytes written, out_off, out_len).  ``cap``: the room given (None: ``len(records) + 18 n``, which always suffices)."""
    import ctypes as C

    import numpy as np

    from ._lib import lib

    n = len(offsets)
    offs = (C.c_uint64 * max(1, n))(*offsets)
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(n, 2)
    if cap is None:
        cap = len(records) + 18 * n
    buf = C.create_string_buffer(max(cap, 1))
    out_off = (C.c_uint64 * (n + 1))()
    out_len = C.c_uint64()
    args = (records, len(records), offs, n, bins, counts.ctypes.data_as(C.POINTER(C.c_int32)), buf, cap, out_off, C.byref(out_len))
    status = lib.tbk_bam_haplotag(*args) if device is None else lib.tbk_bam_haplotag_device(device, *args)
    return status, C.string_at(C.addressof(buf), min(out_len.value, cap) if status == 0 else 0), list(out_off), out_len.value


def bam_haplotag_device(records: bytes, offsets, bins: bytes, counts, device: int = 0):
    """(the tagged records back to back, where each begins with the total last) of a run of whole BAM records (bytes; ``offsets``:
    where each begins), every record rewritten with its bin (``bins``: one of b"ABU" per record) and its counts (n x 2 int32) as the
    tags HP, ka and kb on the GPU (``tbk_bam_haplotag_device``; include/tbk.h "Haplotag output")."""
    from ._lib import check

    status, data, out_off, _ = bam_haplotag_status(records, offsets, bins, counts, device)
    check(status)
    return data, out_off


def bam_haplotag_host(records: bytes, offsets, bins: bytes, counts):
    """The same by the host's rewriter (``tbk_bam_haplotag``)."""
    from ._lib import check

    status, data, out_off, _ = bam_haplotag_status(records, offsets, bins, counts, None)
    check(status)
    return data, out_off


def bam_fastq_host(records: bytes, offsets, skip_flags: int = 0x900):
    """The same by the host's transcoder (``tbk_bam_fastq``)."""
    from ._lib import lib

    return _bam_fastq(lib.tbk_bam_fastq, records, offsets, skip_flags)


def _gzip_inflate(call, data: bytes) -> bytes:
    import ctypes as C

    from ._lib import TBK_ERR_NOMEM, check

    # ISIZE (the last four bytes) is the size modulo 2^32 of the LAST member only: a first guess; the call says what it takes
    # (and of a file that is damaged or cut, no size at all: DEFLATE makes at most 1032 bytes of one)
    hint = min(int.from_bytes(data[-4:], "little"), 1032 * len(data)) if len(data) >= 18 else 0
    n = C.c_uint64()
    cap = max(hint, 1 << 16)
    buf = C.create_string_buffer(cap)
    status = call(buf, cap, C.byref(n))
    if status == TBK_ERR_NOMEM and n.value > cap:
        cap = n.value
        buf = C.create_string_buffer(cap)
        status = call(buf, cap, C.byref(n))
    check(status)
    return C.string_at(C.addressof(buf), n.value)


def gzip_inflate_stats() -> dict:
    """Of this thread's last ``gzip_inflate_device`` / ``gzip_inflate_host``: windows, chunks guessed / accepted / decoded again,
    bytes handed back to the host path, the most chunks accepted in one window."""
    import ctypes as C

    from ._lib import lib

    out = (C.c_uint64 * 6)()
    lib.tbk_gzip_inflate_stats(out)
    return dict(zip(("windows", "guessed", "accepted", "redecoded", "handed_back", "most_accepted"), (int(v) for v in out)))


def gzip_inflate_device(data: bytes, device: int = 0, chunk: Optional[int] = None, window: Optional[int] = None) -> bytes:
    """The text of an ordinary gzip file (bytes; one member or several), inflated on the GPU (``tbk_gzip_inflate_device``): what
    ``gzip.decompress`` returns.  ``chunk`` / ``window``: compressed bytes per chunk / per window (None: the defaults)."""
    from ._lib import lib

    return _gzip_inflate(lambda buf, cap, n: lib.tbk_gzip_inflate_device_opts(device, data, len(data), buf, cap, n, chunk or 0, window or 0), data)


def gzip_inflate_host(data: bytes, chunk: Optional[int] = None, window: Optional[int] = None) -> bytes:
    """``gzip_inflate_device``'s plan, chain check and loop with the host's decoder in the device's place (no GPU)."""
    from ._lib import lib

    return _gzip_inflate(lambda buf, cap, n: lib.tbk_gzip_inflate_host(data, len(data), buf, cap, n, chunk or 0, window or 0), data)
