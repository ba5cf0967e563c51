"""The instruments of tests/test_gpu_deflate_limits.py, tested without a GPU: the DEFLATE reader that reports structure
(tests/deflate_read.py) against the writer (tests/deflate_craft.py) and zlib, the GPU coder's rule stated over a histogram
(tests/gdeflate_rule.py) against the optimum, and the HOST coder (csrc/tbk_deflate.cpp, tbk_gzip_member) on the inputs that need
DEFLATE's length limits - with the proof, from the member it wrote, that each input did need them."""
import gzip
import random
import zlib

import numpy as np
import pytest

import deflate_craft as craft
import deflate_read as rd
import gdeflate_pieces as pieces
import gdeflate_rule as rule


@pytest.fixture(scope="module")
def valid():
    return craft.valid_streams()


def test_reader_inflates_every_crafted_stream(valid):
    seen = set()
    for name, text, raw in valid:
        blocks, got, end = rd.read_raw(raw)
        assert got == text and end == len(raw), name
        assert blocks[-1].final and not any(b.final for b in blocks[:-1]), name
        assert [b.text[0] for b in blocks[1:]] == [b.text[1] for b in blocks[:-1]] and blocks[-1].text[1] == len(text), name
        assert [b.bits[0] for b in blocks[1:]] == [b.bits[1] for b in blocks[:-1]] and blocks[0].bits[0] == 0, name
        seen |= {b.kind for b in blocks}
        for bgzf in (False, True):
            m = rd.read_member(craft.member(raw, text, bgzf=bgzf, fname=b"x.fq" if not bgzf else None))
            assert m.text == text and m.crc == zlib.crc32(text) and m.isize == len(text), name
            assert (m.header["bsize"] == m.end - 1) if bgzf else (m.header["fname"] == b"x.fq"), name
    assert seen == {"stored", "fixed", "dynamic"}


def test_reader_reports_the_crafted_structure_back():
    rng = np.random.default_rng(3)
    text = craft.fastq_text(rng, 20, 150)
    toks = craft.greedy_tokens(text + text[:700])
    syms = sorted({t if isinstance(t, int) else 257 + craft.len_code(t[0]) for t in toks} | {256})
    lit = craft.chain_lengths(syms, 286, 15) + [0, 0]
    dist = craft.chain_lengths(list(range(30)), 30, 12)
    cl_tokens = craft._cl_runs(lit[:286]) + craft._cl_runs(dist)
    f = [0] * 19
    for s, _ in cl_tokens:
        f[s] += 1
    cl_lens = craft.limited_lengths(f, 7)
    plan = [craft.Block("stored", data=text[:100]),
            craft.Block("fixed", tokens=[65, 67, (5, 2), (258, 1)]),
            craft.Block("dynamic", tokens=toks, lit_lens=lit, dist_lens=dist, hlit=286, hdist=30, hclen=19, cl_lens=cl_lens, cl_tokens=cl_tokens),
            craft.Block("dynamic", tokens=list(b"ACGTTTGA"), dist_lens=[0], hdist=1, final=True)]
    raw, want = craft.deflate(plan)
    blocks, got, _ = rd.read_raw(raw)
    assert got == want and [b.kind for b in blocks] == ["stored", "fixed", "dynamic", "dynamic"]
    assert [b.final for b in blocks] == [False, False, False, True]
    assert blocks[0].tokens == [] and blocks[0].text == (0, 100)
    assert blocks[1].tokens == plan[1].tokens and blocks[1].lit_lens == craft.FIXED_LIT
    b = blocks[2]
    assert (b.hlit, b.hdist, b.hclen) == (286, 30, 19) and b.lit_lens == lit[:286] and b.dist_lens == dist and b.cl_lens == cl_lens
    assert b.tokens == toks
    extra_base = {16: 3, 17: 3, 18: 11}
    assert b.cl_tokens == [(s, extra_base[s] + x if s > 15 else 1) for s, x in cl_tokens]
    assert {16, 17, 18} <= {s for s, _ in b.cl_tokens}
    assert b.bits[0] < b.symbols_at < b.bits[1] == blocks[3].bits[0]
    assert rd.histogram(b)[256] == 1 and sum(rd.histogram(b)) == len(toks) + 1
    last = blocks[3]
    assert last.tokens == list(b"ACGTTTGA") and last.dist_lens == [0] and last.hlit == 257 and last.hclen >= 4


def test_reader_agrees_with_zlib_on_zlibs_own_output():
    rng = np.random.default_rng(4)
    text = craft.fastq_text(rng, 200, 150, dup=0.3)
    for level, strategy in ((1, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (0, zlib.Z_DEFAULT_STRATEGY)):
        co = zlib.compressobj(level, zlib.DEFLATED, 31, 8, strategy)
        z = co.compress(text) + co.flush()
        m = rd.read_member(z)
        assert m.text == zlib.decompress(z, 31) == text and m.end == len(z)
        kinds = {b.kind for b in m.blocks}
        assert kinds == ({"stored"} if level == 0 else {"fixed"} if strategy == zlib.Z_FIXED else {"dynamic"}), (level, kinds)


def _zlib_error(raw):
    d = zlib.decompressobj(-15)
    try:
        d.decompress(raw)
        d.flush()
    except zlib.error as e:
        return str(e)
    return None


def test_reader_refuses_what_zlib_refuses():
    bad_code = 0
    for name, text, raw, kw in craft.invalid_streams():
        with pytest.raises(rd.BadStream):
            rd.read_member(craft.member(raw, text, bgzf=False, **kw))
        err = _zlib_error(raw)
        if err is not None and "stored" not in err:      # a code or a code header that zlib will not take
            bad_code += 1
            with pytest.raises(rd.BadCode):
                rd.read_raw(raw)
    assert bad_code >= 12
    text, raw = craft.truncated_dynamic()
    with pytest.raises(rd.BadStream):
        rd.read_raw(raw)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------

def _huffman_cost(freq):
    """Bits of an optimal prefix code without a length limit: the sum of the inner nodes' weights."""
    import heapq

    h = [f for f in freq if f]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        cost += a + b
        heapq.heappush(h, a + b)
    return cost


def _histograms():
    r = random.Random(7)
    for i in range(3000):
        kind = i % 6
        n = r.randrange(2, 40) if kind else r.randrange(2, 287)
        if kind == 0:
            f = [r.randrange(0, 1000) for _ in range(n)]
        elif kind == 1:
            f = [r.randrange(1, 4) for _ in range(n)]
        elif kind == 2:      # Fibonacci-like: every count about the sum of the two before it
            f = [1, r.randrange(1, 3)]
            while len(f) < n:
                f.append(f[-1] + f[-2] + r.randrange(-1, 2))
            f = [max(1, x) for x in f]
        elif kind == 3:      # powers of two, some of them several times
            f = [1 << r.randrange(0, 24) for _ in range(n)]
        elif kind == 4:      # a foot of ones under a chain
            f = [1] * r.randrange(2, 30)
            while len(f) < n + 2:
                f.append(sum(f[-2:]) + r.randrange(0, 3))
        else:
            f = [int(1.6 ** r.uniform(0, 30)) + 1 for _ in range(n)]
        r.shuffle(f)
        if r.random() < 0.3:
            f += [0] * r.randrange(1, 5)
            r.shuffle(f)
        if sum(1 for x in f if x) >= 2:
            yield f


def test_rule_lengths_are_a_complete_code_within_the_limit_and_never_beat_the_optimum():
    limited = {15: 0, 7: 0}
    deepest_excess = {15: 0, 7: 0}
    for f in _histograms():
        for limit in (15, 7):
            if sum(1 for x in f if x) > 1 << limit:
                continue
            lens, depth, excess = rule.lengths(f, limit)
            assert all((l > 0) == (x > 0) for l, x in zip(lens, f))
            assert max(lens) <= limit
            assert sum(1 << (limit - l) for l in lens if l) == 1 << limit          # complete, not over-subscribed
            cost = sum(l * x for l, x in zip(lens, f))
            if depth <= limit:
                assert excess == 0 and max(lens) == depth and cost == _huffman_cost(f)
            else:
                assert excess > 0 and max(lens) == limit
                limited[limit] += 1
                deepest_excess[limit] = max(deepest_excess[limit], excess)
            assert cost >= sum(l * x for l, x in zip(craft.limited_lengths(f, limit), f))
    assert limited[15] > 100 and limited[7] > 500 and deepest_excess[15] >= 8 and deepest_excess[7] >= 8, (limited, deepest_excess)


def test_rule_header_and_size_describe_a_crafted_block():
    """header() and coded_bits() against the writer: a block written with the rule's lengths and zlib's run encoding (which, with no
    two equal nonzero lengths side by side coded as 16, is the rule's) has the rule's size."""
    text = pieces.alphabet_piece(pieces.used_from_gaps(pieces.HEADER_PLANS["149_2_3_10_11_bytes_0_255"]))
    freq = [0] * 286
    for v in text:
        freq[v] += 1
    freq[256] = 1
    lens, _, _ = rule.lengths(freq, 15)
    h = rule.header(lens, False)
    assert (h.hlit, h.hdist) == (257, 1) and {(18, 138), (18, 11), (17, 10), (17, 3), (0, 1)} <= set(h.tokens)
    assert [r for s, r in h.tokens if s == 0 or s > 15] == [138, 11, 1, 1, 3, 10, 11, 1]
    base = {17: 3, 18: 11}
    blk = craft.Block("dynamic", tokens=list(text), final=True, lit_lens=lens[:257], dist_lens=[0], hdist=1, cl_lens=h.cl_lens, hclen=h.hclen,
                      cl_tokens=[(s, r - base[s] if s > 15 else 0) for s, r in h.tokens])
    raw, _ = craft.deflate([blk])
    b = rd.read_raw(raw)[0][0]
    assert b.cl_tokens == h.tokens and b.hclen == h.hclen and b.cl_lens == h.cl_lens
    assert b.symbols_at - b.bits[0] == h.bits and b.bits[1] - b.bits[0] == rule.coded_bits(h, lens, freq)
    assert rule.stored(5, 8 * 5 + 1) and not rule.stored(5, 8 * 5 - 3 - 7)


# ---- the host coder ----------------------------------------------------------------------------------------------------------------

def _gzip_member(data: bytes) -> bytes:
    import ctypes as C

    from trio_binning_amd._lib import lib

    need = C.c_size_t(0)
    assert lib.tbk_gzip_member(data, len(data), None, 0, C.byref(need)) == -6 and need.value >= 18
    out = C.create_string_buffer(need.value)
    assert lib.tbk_gzip_member(data, len(data), out, need.value, C.byref(need)) == 0
    return out.raw[:need.value]


def _host_blocks(data: bytes):
    """The member tbk_gzip_member writes for data, parsed; every dynamic block's codes are complete (the reader refuses others) and
    within DEFLATE's limits.  Returns per dynamic block (unlimited depth of its own literal/length histogram, of its code-length
    histogram)."""
    z = _gzip_member(data)
    assert gzip.decompress(z) == data
    m = rd.read_member(z)
    assert m.text == data and m.end == len(z) and m.crc == zlib.crc32(data) and m.isize == len(data)
    depths = []
    for b in m.blocks:
        assert b.kind == "dynamic"
        assert max(b.lit_lens) <= 15 and max(b.cl_lens) <= 7
        f = rd.histogram(b)
        assert all((l > 0) == (x > 0) for l, x in zip(b.lit_lens + [0] * 29, f))
        clf = [0] * 19
        for s, _ in b.cl_tokens:
            clf[s] += 1
        assert all((l > 0) == (x > 0) for l, x in zip(b.cl_lens, clf))
        depths.append((rule.lengths(f, 99)[1], rule.lengths(clf, 99)[1]))
    return depths


HOST_LIMIT_15 = [("fib16", lambda: pieces.fib_piece(16)), ("fib17", lambda: pieces.fib_piece(17)), ("fib18", lambda: pieces.fib_piece(18)),
                 ("foot", pieces.foot_piece), ("both", pieces.both_limiters_piece), ("runs", pieces.run_mode_deep_piece)]
# (the piece that takes the GPU coder through both limiters is not here: the host halves its counts where the GPU coder repairs the
# code space, gets other lengths, and the tree of their numbers is 7 deep)
HOST_LIMIT_7 = [("cl_deep", pieces.cl_deep_piece), ("cl_eight", pieces.cl_eight_piece)]


@pytest.mark.parametrize("name,make", HOST_LIMIT_15, ids=[n for n, _ in HOST_LIMIT_15])
def test_host_coder_limits_a_literal_tree_deeper_than_15(built, name, make):
    (lit_depth, _), = _host_blocks(make())
    assert lit_depth > 15, lit_depth


@pytest.mark.parametrize("name,make", HOST_LIMIT_7, ids=[n for n, _ in HOST_LIMIT_7])
def test_host_coder_limits_a_code_length_tree_deeper_than_7(built, name, make):
    (_, cl_depth), = _host_blocks(make())
    assert cl_depth > 7, cl_depth


def test_host_coder_control_of_depth_15_and_the_skew_case(built):
    """Fibonacci counts over 15 byte values: depth exactly 15, no limit needed.  And the `skew` case of
    tests/test_host_native_io.py (counts 2^k over twenty byte values, shuffled over a megabyte, cut at its bytes 10): most of its blocks
    have trees of 14 or 15 levels, and some pass 15 - that case does reach the host coder's limit, as it says."""
    (lit_depth, _), = _host_blocks(pieces.fib_piece(15))
    assert lit_depth == 15
    rng = np.random.default_rng(5)
    skew = np.concatenate([np.full(1 << k, k, dtype=np.uint8) for k in range(20)])
    rng.shuffle(skew)
    depths = _host_blocks(skew.tobytes())
    assert len(depths) > 10 and max(d for d, _ in depths) > 15, depths
