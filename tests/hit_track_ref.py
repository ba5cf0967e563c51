"""The reference of the hit tracker's tests: marks from numpy (per-window canonical keys, np.isin against the lists' lines,
A first), raw runs and phase blocks from a plain Python loop over those marks.  Nothing here touches a device."""
import numpy as np

RUN_DTYPE = [("read", "<u8"), ("first", "<u8"), ("last", "<u8"), ("markers", "<u4"), ("hap", "<u4")]

_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
_CODE_ANY_CASE = _CODE.copy()
for _i, _c in enumerate(b"acgt"):
    _CODE_ANY_CASE[_c] = _i
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def pack(kmer):
    """the project's packing: base i at bits 2i..2i+1, A=0 C=1 G=2 T=3"""
    return sum("ACGT".index(c) << (2 * i) for i, c in enumerate(kmer))


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


def canonical(kmer):
    return min(pack(kmer), pack(revcomp(kmer)))


def window_keys(read, k, ignore_case):
    """(canonical key, clean) per window start 0 .. len - k of one read's bytes"""
    codes = (_CODE_ANY_CASE if ignore_case else _CODE)[np.frombuffer(read, dtype=np.uint8)]
    nw = codes.size - k + 1
    if nw <= 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=bool)
    bad = np.concatenate([[0], np.cumsum(codes == 255)])
    clean = bad[k:k + nw] == bad[:nw]
    c = (codes & 3).astype(np.uint64)
    fwd = np.zeros(nw, dtype=np.uint64)
    rc = np.zeros(nw, dtype=np.uint64)
    for j in range(k):
        fwd |= c[j:j + nw] << np.uint64(2 * j)
        rc |= (np.uint64(3) - c[k - 1 - j:k - 1 - j + nw]) << np.uint64(2 * j)
    return np.minimum(fwd, rc), clean


def marks(bases, offsets, keys_a, keys_b, k, ignore_case=False):
    """one byte per base of the batch: 0 none, 1 A, 2 B for the window that starts there"""
    out = np.zeros(int(offsets[-1]), dtype=np.uint8)
    raw = np.asarray(bases, dtype=np.uint8).tobytes()
    for r in range(len(offsets) - 1):
        lo, hi = int(offsets[r]), int(offsets[r + 1])
        key, clean = window_keys(raw[lo:hi], k, ignore_case)
        in_a = clean & np.isin(key, keys_a)
        in_b = clean & ~in_a & np.isin(key, keys_b)
        out[lo:lo + key.size] = in_a.astype(np.uint8) + 2 * in_b.astype(np.uint8)
    return out


def counts_of(mk, offsets):
    n = len(offsets) - 1
    out = np.zeros((n, 2), dtype=np.int32)
    for r in range(n):
        part = mk[int(offsets[r]):int(offsets[r + 1])]
        out[r] = (int((part == 1).sum()), int((part == 2).sum()))
    return out


def runs(mk, offsets):
    """raw runs: within a read, in position order, maximal sequences of consecutive markers of one haplotype"""
    out = []
    for r in range(len(offsets) - 1):
        lo, hi = int(offsets[r]), int(offsets[r + 1])
        cur = None
        for w in np.nonzero(mk[lo:hi])[0]:
            hap = int(mk[lo + w]) - 1
            if cur is not None and cur[4] == hap:
                cur[2] = int(w)
                cur[3] += 1
            else:
                if cur is not None:
                    out.append(tuple(cur))
                cur = [r, int(w), int(w), 1, hap]
        if cur is not None:
            out.append(tuple(cur))
    return np.array(out, dtype=RUN_DTYPE)


def blocks(raw, min_run):
    """drop the raw runs below min_run once, then merge neighbours of one read and haplotype"""
    out = []
    for run in raw:
        if int(run["markers"]) < min_run:
            continue
        if out and out[-1][0] == int(run["read"]) and out[-1][4] == int(run["hap"]):
            out[-1][2] = int(run["last"])
            out[-1][3] += int(run["markers"])
        else:
            out.append([int(run["read"]), int(run["first"]), int(run["last"]), int(run["markers"]), int(run["hap"])])
    return np.array([tuple(b) for b in out], dtype=RUN_DTYPE)


def upper_acgt(bases):
    """the batch as --ignore-case reads it: a c g t upper-cased, every other byte as it is"""
    bases = np.asarray(bases, dtype=np.uint8).copy()
    for c in b"acgt":
        bases[bases == c] = c - 32
    return bases
