"""The host inflaters on hand-built DEFLATE streams (tests/deflate_craft.py) against gzip.decompress: the reference reads .gz input
through gzip.open (seq.py:86-92), so a file must give gzip's text or be refused exactly where gzip refuses it.

Streams: what zlib never writes (15-bit codes in both trees, one distance code or none, untrimmed HLIT / HDIST / HCLEN, code-length
runs across the two trees, every length code's ends against every distance code's, stored blocks at every bit offset, thousands of
empty blocks) and streams that break one rule each, with a matching CRC-32 and ISIZE.  Paths: the bgzf reader's own decoder and
zlib's (TBK_INFLATE=own|zlib), and single-member gzip through the sequential decoder (TBK_PINFLATE=0) and the guessing one."""
import gzip

import pytest

import deflate_craft as dc


def _records(path):
    from trio_binning_amd import seq

    out = []
    with seq.BatchReader(str(path)) as r:
        b = seq.Batch()
        while r.next_batch(b, 1 << 16, 0):
            bases, boff, names, noff, quals, qoff, _ = b.arrays()   # (bytes: a decoy's payload is not text)
            out += [(bytes(names[noff[i]:noff[i + 1]]), bytes(bases[boff[i]:boff[i + 1]]), bytes(quals[qoff[i]:qoff[i + 1]]))
                    for i in range(b.n_reads)]
        b.close()
    return out


def _outcome(path):
    from trio_binning_amd._lib import TbkError

    try:
        return _records(path)
    except (TbkError, ValueError, OSError) as e:
        return ("refused", type(e).__name__)


def _gzip_text(data):
    try:
        return gzip.decompress(data)
    except Exception:
        return None


def _check(tmp_path, data, name):
    """The reader on `data` gives the plain text's records when gzip reads it, and refuses it when gzip refuses it."""
    gz = tmp_path / "x.fastq.gz"
    gz.write_bytes(data)
    text = _gzip_text(data)
    got = _outcome(gz)
    if text is None:
        assert got and got[0] == "refused", (name, "gzip refuses this file; the reader returned records")
        return
    plain = tmp_path / "x.fastq"
    plain.write_bytes(text)
    want = _records(plain)
    assert got == want, name


@pytest.fixture(scope="module")
def valid():
    return dc.valid_streams()


@pytest.fixture(scope="module")
def invalid():
    return dc.invalid_streams()


def test_corpus_is_what_it_claims(valid, invalid):
    """The writer's own checks: valid streams give their text under zlib (deflate() asserts it), fit a bgzf member, and cover the
    table boundaries; gzip refuses every invalid member."""
    names = {n for n, _, _ in valid}
    for want in ("lit_chain_15", "lit_chain_11", "lit_chain_10", "dist_chain_15", "dist_chain_9", "dist_chain_8", "dist_single_len1",
                 "dist_none", "lit_two_symbols", "cross_boundary_zeros", "repeat_extremes", "repeat16_extremes", "overlap_1_65",
                 "back_across_blocks", "empty_blocks_4000", "stored_max_at_bit_7", "stored_empty_at_bit_3"):
        assert want in names, want
    assert all(len(t) <= 65536 and len(dc.member(r, t)) <= 65536 for _, t, r in valid)
    for name, text, raw, kw in invalid:
        assert _gzip_text(dc.member(raw, text, **kw) + dc.EOF_BLOCK) is None, name
        assert _gzip_text(dc.member(raw, text, bgzf=False, **kw)) is None, name


@pytest.mark.parametrize("how", ["own", "zlib"])
def test_bgzf_valid_members(built, tmp_path, monkeypatch, valid, how):
    """All valid members in one bgzf file, framed plainly, with FNAME, FCOMMENT and FHCRC, and with a second extra subfield."""
    monkeypatch.setenv("TBK_INFLATE", how)
    _check(tmp_path, dc.bgzf_file([dc.member(r, t) for _, t, r in valid]), "plain")
    _check(tmp_path, dc.bgzf_file([dc.member(r, t, fname=b"reads.fq") for _, t, r in valid if len(r) < 65400]), "fname")
    _check(tmp_path, dc.bgzf_file([dc.member(r, t, fname=b"r.fq", fcomment=b"c", fhcrc=True, other="after") for _, t, r in valid
                                   if len(r) < 65400]), "fname fcomment fhcrc, subfield after BC")
    _check(tmp_path, dc.bgzf_file([dc.member(r, t, other="before") for _, t, r in valid if len(r) < 65400]), "BC after another subfield")


@pytest.mark.parametrize("how", ["own", "zlib"])
def test_bgzf_invalid_member_is_refused(built, tmp_path, monkeypatch, valid, invalid, how):
    """One invalid member between valid ones (matching CRC-32 and ISIZE unless the case is about them); a member cut inside its
    dynamic header as the last one."""
    monkeypatch.setenv("TBK_INFLATE", how)
    good = [dc.member(r, t) for _, t, r in valid[:3]]
    for name, text, raw, kw in invalid:
        _check(tmp_path, dc.bgzf_file(good[:2] + [dc.member(raw, text, **kw)] + good[2:]), name)
    text, cut = dc.truncated_dynamic()
    _check(tmp_path, dc.bgzf_file(good, eof=True)[:-28] + dc.member(cut, text), "cut in a dynamic header, last")
    _check(tmp_path, dc.bgzf_file(good + [dc.member(cut, text)], eof=False), "cut in a dynamic header, last, no EOF block")


@pytest.mark.parametrize("guessing", [False, True])
def test_single_member_gzip(built, tmp_path, monkeypatch, valid, invalid, guessing):
    """Each stream as one ordinary gzip member (FNAME, FCOMMENT, FHCRC), through the sequential decoder and the guessing one (4 KiB
    spans, so that even these files are cut)."""
    if guessing:
        monkeypatch.setenv("TBK_PINFLATE_MIN", "0")
        monkeypatch.setenv("TBK_PINFLATE_SPAN", "4096")
    else:
        monkeypatch.setenv("TBK_PINFLATE", "0")
    for name, text, raw in valid:
        _check(tmp_path, dc.member(raw, text, bgzf=False, fname=b"x.fq", fcomment=b"y", fhcrc=True), name)
    for name, text, raw, kw in invalid:
        _check(tmp_path, dc.member(raw, text, bgzf=False, **kw), name)
    text, cut = dc.truncated_dynamic()
    _check(tmp_path, dc.member(cut, text, bgzf=False), "cut in a dynamic header")


@pytest.mark.parametrize("guessing", [False, True])
def test_stored_decoy_dynamic_header(built, tmp_path, monkeypatch, guessing):
    """A stored block whose payload is a valid non-final dynamic block (header and codes): the guessing decoder's search for block
    starts (TbkInflate::open_dynamic_block_at) finds it and must throw the false start away."""
    import numpy as np

    if guessing:
        monkeypatch.setenv("TBK_PINFLATE_MIN", "0")
        monkeypatch.setenv("TBK_PINFLATE_SPAN", "4096")
    else:
        monkeypatch.setenv("TBK_PINFLATE", "0")
    rng = np.random.default_rng(21)
    fq1, fq2 = dc.fastq_text(rng, 150, 300), dc.fastq_text(rng, 150, 300)
    d = dc.BitWriter()
    dc.write_block(d, dc.Block("dynamic", tokens=dc.greedy_tokens(fq2[:3000])))
    payload = b"@decoy\n" + d.getvalue() + b"\n+\n"
    blocks = [dc.Block("dynamic", tokens=dc.greedy_tokens(fq1))]
    for k in range(4):
        blocks += [dc.Block("stored", data=payload * 3), dc.Block("dynamic", tokens=dc.greedy_tokens(fq2))]
    blocks.append(dc.Block("fixed", tokens=list(b"@end\nA\n+\nI\n"), final=True))
    raw, text = dc.deflate(blocks)
    _check(tmp_path, dc.member(raw, text, bgzf=False), "decoy")
