"""Inputs that drive the deflate coders (csrc/tbk_gdeflate.hip, csrc/tbk_deflate.cpp) into the paths an ordinary text never takes:
Huffman trees deeper than DEFLATE's 15 and 7 bits, every form of zero run in a block header, the threshold at which a block is coded
with runs.  Every piece is at most 16384 bytes and holds no byte 10 (a line end, where the GPU coder cuts its blocks), so it is one
block.  Which path a piece takes is never assumed: the tests parse what the coder wrote (``deflate_read``) and assert the reach from
that.  It is a helper: pytest does not collect it (no ``test_`` prefix)."""
import numpy as np

MAX_BLOCK = 16384


def spread(counts: dict, seed: int = 1) -> bytes:
    """The byte values of `counts` ({value: how often}), shuffled."""
    assert 10 not in counts and all(0 <= v < 256 for v in counts)
    a = np.repeat(np.fromiter(counts.keys(), dtype=np.uint8), np.fromiter(counts.values(), dtype=np.int64))
    np.random.default_rng(seed).shuffle(a)
    assert a.size <= MAX_BLOCK
    return a.tobytes()


def fib_counts(m: int):
    """1, 2, 3, 5, 8, ...: with the end-of-block symbol's 1 a Huffman tree of depth m."""
    f = [1, 2]
    while len(f) < m:
        f.append(f[-1] + f[-2])
    return f[:m]


def fib_piece(m: int, seed: int = 1, fill_to: int = 0) -> bytes:
    """Fibonacci counts over m byte values (33 ..).  fill_to: three more values (200 ..) that share what is missing to that many
    bytes - they lie above the chain, which only gets deeper, and keep the piece clear of the run mode."""
    counts = dict(zip(range(33, 33 + m), fib_counts(m)))
    return spread(_fill(counts, fill_to), seed)


def _fill(counts: dict, fill_to: int) -> dict:
    left = fill_to - sum(counts.values()) if fill_to else 0
    assert left >= 0
    for k in range(3 if left else 0):
        counts[200 + k] = left // 3 + (1 if k < left % 3 else 0)
    return counts


# The 15-bit limiter with a Kraft excess of 8: 24 symbols of count 1 at the foot of a chain (23 byte values and the end-of-block
# symbol), every next count the least that makes the tree one level deeper.  Found with gdeflate_rule.lengths: among the chains on
# a foot of 2 .. 39 ones and of depth 16 .. 23 this is the smallest piece whose excess reaches 8 (5111 bytes, depth 16).
FOOT_COUNTS = [1] * 23 + [17, 25, 42, 67, 109, 176, 285, 461, 746, 1207, 1953]


def foot_piece(seed: int = 1, fill_to: int = 0) -> bytes:
    return spread(_fill(dict(zip(range(33, 33 + len(FOOT_COUNTS)), FOOT_COUNTS)), fill_to), seed)


def dyadic_piece(values_per_length: dict, first_value: int, seed: int = 1, extra: int = 0) -> bytes:
    """Byte v occurs 2^(top - L) times, top the longest length; one entry of the longest length is left to the end-of-block symbol.
    The byte values are first_value .. 255 and all of them are used, so the header's zeros are one run in front of them (byte 10
    in it).  Which value gets which length is shuffled.  extra: that many more of the commonest value."""
    top = max(values_per_length)
    lens = [L for L, k in sorted(values_per_length.items()) for _ in range(k)]
    lens.remove(top)
    assert len(lens) == 256 - first_value and first_value > 10
    np.random.default_rng(seed + 100).shuffle(lens)
    counts = {first_value + i: 1 << (top - L) for i, L in enumerate(lens)}
    best = min(counts, key=lambda v: (-counts[v], v))
    counts[best] += extra
    return spread(counts, seed)


# The 7-bit limiter.  The literal/length lengths of a dyadic block are the L below; how many symbols have each length, with one zero
# run (symbol 18) and the distance code's zero, are the code-length frequencies 1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89: depth 10.
CL_DEEP = {6: 13, 7: 55, 8: 89, 9: 2, 10: 8, 11: 5, 12: 3, 13: 21, 14: 34}      # 230 symbols: byte values 27 .. 255, 16383 bytes
# Depth exactly 8: 172 unused byte values are two symbols 18, so the frequencies are 1 (zero), 1, 2 (18), 3, 5, 8, 13, 21, 34.
# Found with gdeflate_rule: the only tops <= 9 at which counts 1, 3, 5, 8, 13, 21, 34 on distinct lengths fill the code space.
CL_EIGHT = {4: 1, 3: 3, 5: 5, 6: 8, 8: 13, 7: 21, 9: 34}                        # 85 symbols: byte values 172 .. 255, 511 bytes


def cl_deep_piece(seed: int = 1, extra: int = 0) -> bytes:
    return dyadic_piece(CL_DEEP, 27, seed, extra)


def cl_eight_piece(seed: int = 1) -> bytes:
    return dyadic_piece(CL_EIGHT, 172, seed)


# Both limiters in one block: 180 byte values (76 .. 255; the 76 unused ones in front are one symbol 18), 15147 bytes.  The tree of
# these counts is 16 deep (excess 9); limited to 15 bits, 128 symbols have length 15, 12 length 14, 24 length 13, ... and those
# numbers, as code-length frequencies, make a tree 8 deep.  Found by a hill climb over histograms with gdeflate_rule as the judge;
# a dyadic body with a Fibonacci tail hung into it does not do (the body's rare symbols mix into the tail and flatten it).
BOTH_COUNTS = ([1] * 77 + [2] * 41 + [3] * 19 + [4] * 2 + [5] * 19 + [6] * 3
               + [8, 8, 11, 12, 16, 21, 22, 28, 41, 42, 52, 52, 70, 479, 794, 1347, 2302, 3708, 5797])


def both_limiters_piece(seed: int = 1) -> bytes:
    return spread(dict(zip(range(256 - len(BOTH_COUNTS), 256), BOTH_COUNTS)), seed)


# The 15-bit limiter in a block coded with runs.  Every byte stands twice in a row (half the bytes repeat their predecessor: run
# mode) and no pair stands beside a pair of its own value, so a pair is two literals whichever lane codes it; the first four bytes
# are one run of four, a literal and a match of 3.  The histogram is 1 (end of block), 1 (length symbol 257), then even counts,
# each the least that deepens the tree (gdeflate_rule.lengths): depth 16 in 5166 bytes.
RUN_PAIR_COUNTS = [2, 4, 6, 10, 16, 26, 42, 68, 110, 178, 288, 466, 754, 1220, 1972]


def run_mode_deep_piece() -> bytes:
    vals = list(range(33, 33 + len(RUN_PAIR_COUNTS)))
    units = [v for v, c in sorted(zip(vals, RUN_PAIR_COUNTS), key=lambda x: -x[1]) for _ in range(c // 2)]
    n = len(units)
    arr = [0] * n
    slots = list(range(0, n, 2)) + list(range(1, n, 2))   # the commonest value on every other place: no two beside each other
    for s, v in zip(slots, units):
        arr[s] = v
    top = vals[-1]
    k = next(i for i in range(n) if arr[i] != top and arr[i - 1] != arr[i])
    arr = arr[k:] + arr[:k]
    assert all(a != b for a, b in zip(arr, arr[1:])) and arr[0] != top
    return bytes([top] * 4) + bytes(v for v in arr for _ in range(2))


def alphabet_piece(used, n: int = 2500, seed: int = 1, equal: bool = False) -> bytes:
    """n bytes over the byte values `used`, every one of them present; frequencies fall off geometrically (equal: all the same)."""
    used = list(used)
    assert 10 not in used
    rng = np.random.default_rng(seed)
    if equal:
        a = np.resize(np.array(used, dtype=np.uint8), n)
    else:
        w = 0.97 ** np.arange(len(used))
        a = np.concatenate([np.array(used, dtype=np.uint8), rng.choice(np.array(used, dtype=np.uint8), size=n - len(used), p=w / w.sum())])
    rng.shuffle(a)
    return a.tobytes()


def used_from_gaps(plan):
    """plan: ("gap", k) leaves k byte values unused, ("use", k) uses the next k; the rest up to 255 is used."""
    used, v = [], 0
    for what, k in plan:
        if what == "use":
            used += range(v, v + k)
        v += k
    assert v <= 256
    return used + list(range(v, 256))


# Header tokens: the zero runs between used symbols.  The distance code's zero behind the end-of-block symbol is a run of 1 in every
# block without matches.  Runs of 139 .. 149 need a symbol 18 of 138 and then one or two zeros, a 17 of 3 and of 10, an 18 of 11.
HEADER_PLANS = {
    "149_2_3_10_11_bytes_0_255": [("use", 1), ("gap", 149), ("use", 1), ("gap", 2), ("use", 1), ("gap", 3), ("use", 1), ("gap", 10), ("use", 1),
                                   ("gap", 11)],
    "148_1": [("gap", 148), ("use", 1), ("gap", 1)],
    "141": [("gap", 141)],
    "140": [("gap", 140)],
    "139": [("gap", 139)],
    "138": [("gap", 138)],
}


def threshold_piece(n: int, same: int, at_cuts: bool, stretch: int, shift: int, seed: int = 1) -> bytes:
    """n bytes of which exactly `same` equal their predecessor.  The places of the equal bytes: at_cuts - the first byte of every
    lane's stretch but the first lane's (the lanes' stretches begin at multiples of `stretch` less `shift`), so that the count
    must look across the cuts; else none within 3 bytes of a cut at any shift.  The rest stand in groups of four behind one another
    (a run of five bytes: a literal and a match of 4 when the block is coded with runs), then singly."""
    rng = np.random.default_rng(seed)
    eq = np.zeros(n, dtype=bool)
    if at_cuts:
        eq[np.arange(stretch - shift, n, stretch)] = True
    left = same - int(eq.sum())
    start = 8
    while left > 0:
        k = min(4, left)
        while any((p % stretch) in (0, 1, stretch - 3, stretch - 2, stretch - 1) for p in range(start - 1, start + k + 1)) or eq[start - 1:start + k + 1].any():
            start += 1
        eq[start:start + k] = True
        left -= k
        start += k + 2
    assert start < n and int(eq.sum()) == same and not eq[0]
    vals = np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)
    step = np.where(eq, 0, 1 + rng.integers(0, vals.size - 1, n))   # an equal byte stays; any other moves on to another value
    out = vals[np.cumsum(step) % vals.size]
    assert int((out[1:] == out[:-1]).sum()) == same
    return out.tobytes()
