"""The rule by which the GPU deflate coder (csrc/tbk_gdeflate.hip) chooses a block's codes and header, stated over a histogram: plain
integers and lists, nothing of the kernel's lanes, masks or shared memory.  A test takes a block apart with ``deflate_read``, counts
its tokens and holds what the coder wrote against what this module says it must have written.  It is a helper: pytest does not
collect it (no ``test_`` prefix).

The host's coder (csrc/tbk_deflate.cpp) limits its lengths by another rule (it halves the frequencies and builds the tree again); only
``header`` and ``coded_bits`` describe it too.
"""
from dataclasses import dataclass
from typing import List, Sequence, Tuple

from deflate_craft import CL_ORDER, LEN_EXTRA


def lengths(freq: Sequence[int], limit: int) -> Tuple[List[int], int, int]:
    """(code lengths, the Huffman tree's depth before any limit, the Kraft excess the limit had to repair - 0 where none binds) for the
    symbols of nonzero frequency; at least two of them."""
    leaves = sorted((f, s) for s, f in enumerate(freq) if f > 0)
    m = len(leaves)
    assert m >= 2, "a code needs two symbols"
    weight = [f for f, _ in leaves]
    parent = [0] * (2 * m - 1)
    leaf, inner = 0, m
    while len(weight) < 2 * m - 1:
        picked = []
        for _ in range(2):
            # the lighter head of the two queues; a leaf on a tie; inner nodes leave in the order they were made
            if leaf < m and (inner >= len(weight) or weight[leaf] <= weight[inner]):
                picked.append(leaf)
                leaf += 1
            else:
                picked.append(inner)
                inner += 1
        for p in picked:
            parent[p] = len(weight)
        weight.append(weight[picked[0]] + weight[picked[1]])
    depth = [0] * (2 * m - 1)
    for i in range(2 * m - 3, -1, -1):
        depth[i] = depth[parent[i]] + 1
    lens = [0] * len(freq)
    deepest = depth[0]            # the rarest leaf: none lies deeper
    if deepest <= limit:
        for i, (_, s) in enumerate(leaves):
            lens[s] = depth[i]
        return lens, deepest, 0
    count = [0] * (limit + 1)
    for i in range(m):
        count[min(depth[i], limit)] += 1
    excess = sum(c << (limit - d) for d, c in enumerate(count) if d) - (1 << limit)
    for _ in range(excess):
        d = max(k for k in range(1, limit) if count[k])
        count[d] -= 1             # one leaf a level down, beside one that comes up from the limit
        count[d + 1] += 2
        count[limit] -= 1
    at = 0
    for d in range(limit, 0, -1):
        for _ in range(count[d]):
            lens[leaves[at][1]] = d   # longest to rarest
            at += 1
    assert at == m
    return lens, deepest, excess


@dataclass
class Header:
    hlit: int                     # as counts
    hdist: int
    hclen: int
    tokens: List[Tuple[int, int]]   # (code-length symbol, how many lengths it stands for)
    clfreq: List[int]
    cl_lens: List[int]
    cl_depth: int                 # of the code-length tree before the 7-bit limit
    cl_excess: int
    bits: int                     # of the whole header, BFINAL and BTYPE included


def header(lit_lens: Sequence[int], runs: bool) -> Header:
    """The dynamic-block header for literal/length lengths `lit_lens`; runs: the block codes runs as matches at distance 1 and so has
    the one distance code, of length 1."""
    lit = list(lit_lens) + [0] * (286 - len(lit_lens))
    hlit = max([257] + [s + 1 for s in range(257, 286) if lit[s]]) if runs else 257
    assert not any(lit[hlit:])
    seq = lit[:hlit] + [1 if runs else 0]
    tokens: List[Tuple[int, int]] = []
    i = 0
    while i < len(seq):
        if seq[i]:
            tokens.append((seq[i], 1))
            i += 1
            continue
        z = 0
        while i + z < len(seq) and seq[i + z] == 0:
            z += 1
        i += z
        while z >= 11:
            tokens.append((18, min(z, 138)))
            z -= min(z, 138)
        if z >= 3:
            tokens.append((17, z))
            z = 0
        tokens += [(0, 1)] * z
    clfreq = [0] * 19
    for s, _ in tokens:
        clfreq[s] += 1
    if sum(1 for f in clfreq if f) < 2:
        clfreq[1 if clfreq[0] else 0] += 1    # a code needs two symbols to be complete
    cl_lens, depth, excess = lengths(clfreq, 7)
    hclen = max([4] + [k + 1 for k, s in enumerate(CL_ORDER) if cl_lens[s]])
    bits = 3 + 5 + 5 + 4 + 3 * hclen + sum(cl_lens[s] + {17: 3, 18: 7}.get(s, 0) for s, _ in tokens)
    return Header(hlit, 1, hclen, tokens, clfreq, cl_lens, depth, excess, bits)


def coded_bits(hdr: Header, lit_lens: Sequence[int], freq: Sequence[int]) -> int:
    """Bits of the coded block up to and including its end-of-block code; freq: its tokens' histogram, freq[256] = 1 among them.  (A
    match costs its length symbol, that symbol's extra bits and the one-bit distance code.)"""
    assert freq[256] == 1
    bits = hdr.bits
    for s, f in enumerate(freq):
        if f:
            assert lit_lens[s], s
            bits += f * (lit_lens[s] + (LEN_EXTRA[s - 257] + 1 if s > 256 else 0))
    return bits


def stored(n: int, bits: int) -> bool:
    """Does the coder write the block of n bytes as a stored block: the coded form with the empty stored block behind it (3 bits, up
    to the byte, LEN and NLEN) would take n + 5 bytes or more."""
    return (bits + 3 + 7) // 8 + 4 >= n + 5
