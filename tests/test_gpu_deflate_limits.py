"""The GPU deflate coder's length limiters, header and run tokens (csrc/tbk_gdeflate.hip: gd_huffman, gd_codes, gd_tokens,
gd_encode_kernel), proven reached and held against the rule.

"zlib gives the text back" (tests/test_gpu_deflate.py) cannot tell which paths the coder took.  Here every member is taken apart
(tests/deflate_read.py) and, block by block: the literal/length lengths must be gdeflate_rule.lengths of the block's own token
histogram at 15 bits, the code-length lengths the same at 7 bits of the header's own token counts, the header tokens, HLIT, HDIST and
HCLEN those of gdeflate_rule.header, and the block's size gdeflate_rule.coded_bits - exact equalities all.  That a piece needed a
limiter (the unlimited tree is deeper than the limit, and by how much the code space was overdrawn) is asserted from the parsed block
too, never assumed.  Inputs: tests/gdeflate_pieces.py."""
import gzip
import zlib

import pytest

import deflate_read as rd
import gdeflate_pieces as pieces
import gdeflate_rule as rule

pytestmark = pytest.mark.gpu

EMPTY_STORED = b"\x00\x00\xff\xff"


def check_block(raw: bytes, blk, nxt, n: int):
    """One coded block of the GPU coder (raw: the member's DEFLATE stream; nxt: the block behind it) against the rule.  Returns
    (literal/length depth, excess, code-length depth, excess, the header) as the rule finds them for the block's own histograms."""
    assert blk.kind == "dynamic" and not blk.final
    freq = rd.histogram(blk)
    matches = [t for t in blk.tokens if not isinstance(t, int)]
    assert all(d == 1 and 3 <= length <= 68 for length, d in matches), matches[:5]
    assert blk.hdist == 1 and blk.dist_lens == ([1] if matches else [0])
    runs = bool(matches)
    lens, depth, excess = rule.lengths(freq, 15)
    assert blk.lit_lens == lens[:blk.hlit] and not any(lens[blk.hlit:]), [(s, a, b) for s, (a, b) in enumerate(zip(blk.lit_lens, lens)) if a != b]
    h = rule.header(lens, runs)
    assert (blk.hlit, blk.hdist, blk.hclen) == (h.hlit, h.hdist, h.hclen)
    assert blk.cl_tokens == h.tokens
    assert blk.cl_lens == h.cl_lens, (blk.cl_lens, h.cl_lens, h.clfreq)
    assert blk.symbols_at - blk.bits[0] == h.bits
    bits = rule.coded_bits(h, lens, freq)
    assert blk.bits[1] - blk.bits[0] == bits and not rule.stored(n, bits)
    # behind the end-of-block code: an empty stored block, not final, zero bits up to its LEN
    assert nxt.kind == "stored" and not nxt.final and nxt.text[0] == nxt.text[1] and nxt.bits[0] == blk.bits[1]
    pad_from, pad_to = blk.bits[1], nxt.bits[1] - 32
    assert 3 <= pad_to - pad_from < 11 and pad_to % 8 == 0
    assert all(not (raw[p >> 3] >> (p & 7)) & 1 for p in range(pad_from, pad_to)) and raw[pad_to // 8:pad_to // 8 + 4] == EMPTY_STORED
    return depth, excess, h.cl_depth, h.cl_excess, h


def check_one_block_member(piece: bytes, member: bytes, head: int = 10):
    """A member that holds `piece` as ONE block: coded (then the rule's, see check_block) or stored, then the member's final empty
    stored block; zlib and the reader give the piece back; CRC-32 and ISIZE.  Returns (the block, check_block's findings or None)."""
    assert gzip.decompress(member) == piece
    m = rd.read_member(member)
    assert m.text == piece and m.end == len(member) and m.header["raw_at"] == head
    assert m.crc == zlib.crc32(piece) and m.isize == len(piece)
    raw = member[head:]
    last = m.blocks[-1]
    assert last.kind == "stored" and last.final and last.text[0] == last.text[1] == len(piece) and last.bits[0] % 8 == 0
    blk = m.blocks[0]
    assert blk.text == (0, len(piece))
    if blk.kind == "stored":
        assert len(m.blocks) == 2 and not blk.final
        return blk, None
    assert len(m.blocks) == 3
    return blk, check_block(raw, blk, m.blocks[1], len(piece))


def byte_histogram(piece: bytes):
    f = [0] * 286
    for v in piece:
        f[v] += 1
    f[256] = 1
    return f


# ---- (a) (b) (c): the limiters ----------------------------------------------------------------------------------------------------------
# name -> (the piece, literal/length depth, its Kraft excess at 15 bits, code-length depth or None, its excess at 7 bits or None).
# The depths and excesses are what gdeflate_rule.lengths gives for the piece's own byte counts (the issue's CPU model gave the
# same for the Fibonacci and the dyadic pieces); the test asserts them of the block the DEVICE wrote.

def limiter_pieces():
    return {
        "fib15_control": (pieces.fib_piece(15), 15, 0, None, None),
        "fib16": (pieces.fib_piece(16), 16, 1, None, None),
        "fib17": (pieces.fib_piece(17), 17, 2, None, None),
        "fib18": (pieces.fib_piece(18), 18, 3, None, None),
        "foot_excess8": (pieces.foot_piece(), 16, 8, None, None),
        "cl_deep": (pieces.cl_deep_piece(), 14, 0, 10, 3),
        "cl_eight": (pieces.cl_eight_piece(), 9, 0, 8, 1),
        "both": (pieces.both_limiters_piece(), 16, 9, 8, 1),
        "runs_fib16": (pieces.run_mode_deep_piece(), 16, 1, None, None),
    }


def _check_limiter_block(name, found, want):
    depth, excess, cl_depth, cl_excess, _ = found
    _, w_depth, w_excess, w_cl_depth, w_cl_excess = want
    assert (depth, excess) == (w_depth, w_excess), name
    if w_cl_depth is None or name == "both":
        assert (depth > 15) == (not name.endswith("control")), name
    if w_cl_depth is not None:
        assert cl_depth > 7 and (cl_depth, cl_excess) == (w_cl_depth, w_cl_excess), name
    return depth, cl_depth


def test_limiters_in_gzip_members(gpu):
    from trio_binning_amd import seq

    table = limiter_pieces()
    assert len(pieces.fib_piece(16)) == 4179 and len(pieces.fib_piece(17)) == 6763 and len(pieces.fib_piece(18)) == 10944
    assert len(pieces.fib_piece(15)) == 2582 and len(pieces.cl_deep_piece()) == 16383
    members = seq.gzip_members_device([v[0] for v in table.values()])
    assert len(members) == len(table)
    for (name, want), member in zip(table.items(), members):
        blk, found = check_one_block_member(want[0], member)
        assert found is not None, name
        _check_limiter_block(name, found, want)
        has_matches = any(not isinstance(t, int) for t in blk.tokens)
        assert has_matches == name.startswith("runs"), name
        if not has_matches:    # literal mode: the histogram is the piece's bytes
            assert rd.histogram(blk) == byte_histogram(want[0]), name
    # the project's own inflater on the 15-bit and 7-bit codes its own encoder made
    assert seq.gzip_inflate_device(b"".join(members)) == b"".join(v[0] for v in table.values())


# ---- (g): the same through one bgzf job ---------------------------------------------------------------------------------------------
# A bgzf job is binary: its blocks are cut by position - 16384 bytes each, the fourth of a member 16128 (65280 bytes make a member) -
# and only the job's last block may be shorter.  So a piece cannot be a member of its own, as in the gzip job: the Fibonacci pieces
# are filled up to the block with three more byte values above the chain (the tree only gets deeper), the dyadic piece with one more
# byte, and the small one of depth 8 stands last.  (The control of depth 15 has no place in this job: filled up it is deeper.)

def test_limiters_in_one_bgzf_job(gpu):
    from trio_binning_amd import seq

    blocks = [("fib16", pieces.fib_piece(16, fill_to=16384)), ("fib17", pieces.fib_piece(17, fill_to=16384)),
              ("fib18", pieces.fib_piece(18, fill_to=16384)), ("foot", pieces.foot_piece(fill_to=16128)),
              ("cl_deep", pieces.cl_deep_piece(extra=1)), ("cl_eight", pieces.cl_eight_piece())]
    assert [len(p) for _, p in blocks] == [16384, 16384, 16384, 16128, 16384, 511]
    data = b"".join(p for _, p in blocks)
    out, n_members = seq.bgzf_members_device(data)
    assert n_members == 2
    members = rd.read_members(out)
    assert len(members) == 2 and [len(m.text) for m in members] == [65280, len(data) - 65280]
    assert gzip.decompress(out) == data and b"".join(m.text for m in members) == data
    coded, at = [], 0
    for m in members:
        raw = out[at + 18:m.end]
        assert m.header["raw_at"] == at + 18 and m.header["bsize"] == m.end - at - 1 and m.header["extra"] == [(b"BC", out[at + 16:at + 18])]
        piece = data[sum(len(x.text) for x in members[:members.index(m)]):][:len(m.text)]
        assert m.crc == zlib.crc32(piece) and m.isize == len(piece)
        assert m.blocks[-1].kind == "stored" and m.blocks[-1].final and m.blocks[-1].text[0] == m.blocks[-1].text[1]
        body = m.blocks[:-1]
        assert len(body) % 2 == 0
        for blk, nxt in zip(body[::2], body[1::2]):
            coded.append((blk, check_block(raw, blk, nxt, blk.text[1] - blk.text[0])))
        at = m.end
    assert len(coded) == len(blocks)
    for (name, piece), (blk, found) in zip(blocks, coded):
        assert blk.text[1] - blk.text[0] == len(piece) and rd.histogram(blk) == byte_histogram(piece), name
        depth, excess, cl_depth, cl_excess, _ = found
        want = rule.lengths(byte_histogram(piece), 15)
        assert (depth, excess) == want[1:], name
        if name.startswith("cl_"):
            assert depth <= 15 and cl_depth > 7 and cl_excess >= 1, (name, depth, cl_depth, cl_excess)
        else:
            assert depth > 15 and excess >= 1, (name, depth, excess)
    # (what gdeflate_rule finds for the filled pieces' byte counts: three more leaves above a chain make it two or three levels deeper)
    assert [f[:2] for _, f in coded[:4]] == [(18, 3), (18, 3), (18, 3), (18, 20)] and [f[2:4] for _, f in coded[4:]] == [(10, 3), (8, 1)]
    assert seq.bgzf_inflate_device(out) == data


# ---- (d): header tokens ---------------------------------------------------------------------------------------------------------------

def test_header_zero_runs_and_hclen(gpu):
    from trio_binning_amd import seq

    plan = {name: pieces.alphabet_piece(pieces.used_from_gaps(p)) for name, p in pieces.HEADER_PLANS.items()}
    # 127 byte values and the end of block, all equally common but the latter: every code 7 bits long, so that the code-length code
    # has symbols 18, 0 and 7 only and HCLEN trims to 6 (16, 17, 18, 0, 8, 7) - as far as it can: a block has at least one code
    # length of 1 .. 15, none of which stands among the first four, and a block of lengths all 8 (HCLEN 5) does not shrink: it is stored
    plan["hclen_6"] = pieces.alphabet_piece(range(129, 256), n=127 * 20, equal=True)
    plan["hclen_19"] = pieces.fib_piece(15, seed=2)      # a code of 15 bits: the last entry of the HCLEN order
    members = seq.gzip_members_device(list(plan.values()))
    seen_runs, hclens = set(), {}
    for (name, piece), member in zip(plan.items(), members):
        blk, found = check_one_block_member(piece, member)
        assert found is not None, name
        used = sorted(set(piece)) + [256]
        gaps = [b - a - 1 for a, b in zip([-1] + used, used + [258]) if b - a - 1 > 0]     # (the last: the distance code's zero)
        assert gaps[-1] == 1
        got, run = [], 0
        for s, rep in blk.cl_tokens + [(1, 1)]:
            if s == 0 or s > 16:
                run += rep
            elif run:
                got.append(run)
                run = 0
        assert got == gaps, name
        seen_runs |= set(gaps)
        hclens[name] = blk.hclen
        if name.startswith("149"):
            assert piece.count(0) and piece.count(255) and blk.lit_lens[0] and blk.lit_lens[255]
            assert [(s, r) for s, r in blk.cl_tokens if s == 0 or s > 15] == [(18, 138), (18, 11), (0, 1), (0, 1), (17, 3), (17, 10), (18, 11), (0, 1)]
        if name in ("141", "148_1"):
            assert [(s, r) for s, r in blk.cl_tokens[:2]] == [(18, 138), (17, 3 if name == "141" else 10)]
        assert not any(s == 16 for s, _ in blk.cl_tokens)
    assert {1, 2, 3, 10, 11, 138, 139, 140, 141, 148, 149} <= seen_runs
    assert hclens["hclen_6"] == 6 and hclens["hclen_19"] == 19, hclens


# ---- (e): the run-mode threshold ------------------------------------------------------------------------------------------------------

def test_run_mode_threshold_at_every_shift(gpu):
    """n = 10000: a block is coded with runs when more than 40 % of its bytes repeat their predecessor (same * 5 > n * 2): 4000 do not
    suffice, 4001 do.  The count is made by 256 lanes, each over its own stretch of the block's aligned words - 10 words here, and the
    first lane's stretch shorter by text_off & 3 bytes - so the equal bytes are put once on the first byte of every stretch (the
    count must look at the byte in front, which another lane holds) and once away from every cut, and every piece stands behind
    0, 1, 2 and 3 bytes of the job's text (the one-shot call lays its pieces back to back: tbk_gzip_members_device)."""
    from trio_binning_amd import seq

    n, stretch = 10000, 40
    assert stretch == 4 * (((n + 3 + 3) // 4 + 255) // 256) == 4 * (((n + 3) // 4 + 255) // 256)
    job, meta = [], []
    for shift in range(4):
        for same in (4000, 4001):
            for at_cuts in (True, False):
                off = sum(map(len, job))
                pad = (shift - off) % 4 or 4
                job.append(bytes([66 + shift]) * pad)
                meta.append(None)
                assert sum(map(len, job)) % 4 == shift
                job.append(pieces.threshold_piece(n, same, at_cuts, stretch, shift, seed=shift * 4 + at_cuts))
                meta.append((shift, same, at_cuts))
    members = seq.gzip_members_device(job)
    for piece, member, what in zip(job, members, meta):
        blk, found = check_one_block_member(piece, member)
        if what is None:
            assert blk.kind == "stored"      # (1 .. 4 bytes)
            continue
        shift, same, at_cuts = what
        assert found is not None and sum(a == b for a, b in zip(piece, piece[1:])) == same
        matches = [t for t in blk.tokens if not isinstance(t, int)]
        assert bool(matches) == (same == 4001), what
        if same == 4000:
            assert rd.histogram(blk) == byte_histogram(piece)
        else:
            assert all(length in (3, 4) for length, _ in matches) and len(matches) > 900


# ---- (f): runs, token by token ------------------------------------------------------------------------------------------------------------

def _run_tokens(n: int):
    """The tokens of b"A" * n alone in its job (text_off 0): the block's words are dealt to 256 lanes, segw words each; the first lane
    writes a literal and continues it with a match over the rest of its stretch, every later lane continues the run with one match
    over its own stretch; what is shorter than 3 goes as literals."""
    segw = ((n + 3) // 4 + 255) // 256
    w = 4 * segw
    first = min(w, n)
    toks = [65] + ([(first - 1, 1)] if first - 1 >= 3 else [65] * (first - 1))
    for lo in range(w, n, w):
        k = min(w, n - lo)
        toks += [(k, 1)] if k >= 3 else [65] * k
    return toks


def _expect(toks, n):
    """(stored?, the rule's header) for a block of these tokens."""
    f = [0] * 286
    f[256] = 1
    for t in toks:
        f[t if isinstance(t, int) else 257 + rd.len_code(t[0])] += 1
    lens, _, _ = rule.lengths(f, 15)
    h = rule.header(lens, True)
    return rule.stored(n, rule.coded_bits(h, lens, f)), h


@pytest.mark.parametrize("n", [1, 2, 3, 4, 68, 69, 136, 137, 16384, "AB"])
def test_runs_token_by_token(gpu, n):
    from trio_binning_amd import seq

    if n == "AB":
        piece = b"AB" + b"A" * 200
        # 51 words, a word per lane: A B A A as literals (a run of two is no match), 49 matches of 4, two bytes left
        want = [65, 66, 65, 65] + [(4, 1)] * 49 + [65, 65]
    else:
        piece = b"A" * n
        want = _run_tokens(n)
    assert sum(1 if isinstance(t, int) else t[0] for t in want) == len(piece)
    member, = seq.gzip_members_device([piece])
    blk, found = check_one_block_member(piece, member)
    if len(piece) == 1:
        stored = True      # one byte repeats nothing: literal mode, and no code is shorter than the byte
    else:
        stored, _ = _expect(want, len(piece))
    assert (blk.kind == "stored") == stored, (n, blk.kind)
    assert stored == (len(piece) <= 4), n
    if not stored:
        assert blk.tokens == want, n
        if n == 16384:
            assert want == [65, (63, 1)] + [(64, 1)] * 255
        if n == 69:
            assert want == [65, (3, 1)] + [(4, 1)] * 16 + [65]
