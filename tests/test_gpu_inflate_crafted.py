"""The GPU inflater (gi_inflate_kernel, csrc/tbk_gdeflate.hip) on hand-built DEFLATE streams (tests/deflate_craft.py) against
gzip.decompress: what zlib never writes - codes past the look-up tables' index in both trees (the slow distance path among them),
one distance code or none, untrimmed headers, code-length runs across the trees, every length code's ends against every distance
code's, stored blocks at every bit offset, thousands of empty blocks - must come out as gzip's text; a member that breaks one rule,
with a matching CRC-32 and ISIZE, must be refused as gzip refuses it.  Through the raw entry (seq.bgzf_inflate_device) and through the
reader (seq.BatchReader(..., device=0)), whose records must equal the plain file's."""
import gzip

import pytest

import deflate_craft as dc

pytestmark = pytest.mark.gpu


def _gzip_text(data):
    try:
        return gzip.decompress(data)
    except Exception:
        return None


def _device_outcome(data):
    from trio_binning_amd import seq
    from trio_binning_amd._lib import TbkError

    try:
        return seq.bgzf_inflate_device(data)
    except (TbkError, ValueError, OSError):
        return None


def _records(path, device):
    from trio_binning_amd import seq
    from trio_binning_amd._lib import TbkError

    out = []
    try:
        with seq.BatchReader(str(path), device=device) as r:
            if device is not None:
                assert r.inflates_on_device
            b = seq.Batch()
            while r.next_batch(b, 1 << 16, 0):
                bases, boff, names, noff, quals, qoff, _ = b.arrays()
                out += [(bytes(names[noff[i]:noff[i + 1]]), bytes(bases[boff[i]:boff[i + 1]]), bytes(quals[qoff[i]:qoff[i + 1]]))
                        for i in range(b.n_reads)]
            b.close()
    except (TbkError, ValueError, OSError):
        return None
    return out


@pytest.fixture(scope="module")
def valid():
    return dc.valid_streams()


@pytest.fixture(scope="module")
def invalid():
    return dc.invalid_streams()


def test_crafted_valid_members(gpu, valid):
    """Every valid stream as a bgzf member: plainly framed, with FNAME, FCOMMENT and FHCRC, with a second extra subfield."""
    files = {
        "plain": dc.bgzf_file([dc.member(r, t) for _, t, r in valid]),
        "fname": dc.bgzf_file([dc.member(r, t, fname=b"reads.fq") for _, t, r in valid if len(r) < 65400]),
        "fname fcomment fhcrc, subfield after BC": dc.bgzf_file([dc.member(r, t, fname=b"r.fq", fcomment=b"c", fhcrc=True, other="after")
                                                                  for _, t, r in valid if len(r) < 65400]),
    }
    for name, data in files.items():
        want = gzip.decompress(data)
        assert _device_outcome(data) == want, name
    for name, t, r in valid:   # one member per call too: a failure names its case
        assert _device_outcome(dc.bgzf_file([dc.member(r, t)])) == t, name
    # BC behind another subfield: gzip's text, or refused as "not a BGZF block" - never other text
    data = dc.bgzf_file([dc.member(r, t, other="before") for _, t, r in valid[:5]])
    assert _device_outcome(data) in (None, gzip.decompress(data))


def test_crafted_invalid_member_is_refused(gpu, valid, invalid):
    """One invalid member per call, between valid ones; a member cut inside its dynamic header as the last one."""
    good = [dc.member(r, t) for _, t, r in valid[:3]]
    for name, text, raw, kw in invalid:
        data = dc.bgzf_file(good[:2] + [dc.member(raw, text, **kw)] + good[2:])
        assert _gzip_text(data) is None
        assert _device_outcome(data) is None, name
    text, cut = dc.truncated_dynamic()
    for data in (dc.bgzf_file(good, eof=False) + dc.member(cut, text), dc.bgzf_file(good + [dc.member(cut, text)], eof=False)):
        assert _gzip_text(data) is None
        assert _device_outcome(data) is None, "cut in a dynamic header"


def test_crafted_reader_on_device(gpu, tmp_path, valid, invalid):
    """The reader with its bgzf input inflated on device 0: records equal the plain file's, FNAME among the framings; the reader
    raises where gzip raises."""
    cases = {
        "plain": dc.bgzf_file([dc.member(r, t) for _, t, r in valid]),
        "fname": dc.bgzf_file([dc.member(r, t, fname=b"reads.fq", fcomment=b"c", fhcrc=True) for _, t, r in valid if len(r) < 65400]),
    }
    good = [dc.member(r, t) for _, t, r in valid[:3]]
    for name, text, raw, kw in invalid:
        cases[name] = dc.bgzf_file(good[:2] + [dc.member(raw, text, **kw)] + good[2:])
    gz, plain = tmp_path / "x.fastq.gz", tmp_path / "x.fastq"
    for name, data in cases.items():
        gz.write_bytes(data)
        text = _gzip_text(data)
        got = _records(gz, 0)
        if text is None:
            assert got is None, (name, "gzip refuses this file; the reader returned records")
            continue
        plain.write_bytes(text)
        want = _records(plain, None)
        assert want and got == want, name
