"""The files of tests/gzip_shapes.py through the GPU gzip inflater's host side with the host's decoder standing in for the device
(seq.gzip_inflate_host: csrc/tbk_gzplan.cpp's plan, chain check and loop, TbkInflate::run16 as pass a): gzip's text, or a refusal where
gzip refuses - and, from that run's stats, that every file reaches the path it was built for.  Those are conditions on the INPUTS: a
file that misses its condition is changed, the bound is not.  tests/test_gpu_inflate_gzip_shapes.py holds the device against the same
files and against ``host_stats`` of them, computed afresh there: the numbers are a property of the guesser and are not stored."""
import os
import threading

import pytest

import gzip_shapes as gs

_said = {}   # the last refusal's message, by case
STAT_KEYS = ("windows", "guessed", "accepted", "redecoded", "most_accepted")


def host_run(case, ratio=None):
    """(text or gs.REFUSED, the stats of the run) of one case with the host's decoder in the device's place.  ratio: the symbols of
    room per compressed byte the loop begins with (TBK_GZIP_RATIO; None: the default)."""
    from trio_binning_amd import seq
    from trio_binning_amd._lib import TbkError

    _, blob, chunk, window, _ = case
    old = os.environ.pop("TBK_GZIP_RATIO", None)
    if ratio is not None:
        os.environ["TBK_GZIP_RATIO"] = str(ratio)
    try:
        try:
            got = seq.gzip_inflate_host(blob, chunk, window)
        except (TbkError, ValueError, OSError) as e:
            got = gs.REFUSED
            _said[case[0]] = str(e)
        return got, seq.gzip_inflate_stats()
    finally:
        os.environ.pop("TBK_GZIP_RATIO", None)
        if old is not None:
            os.environ["TBK_GZIP_RATIO"] = old


def host_stats(case):
    return host_run(case)[1]


@pytest.fixture(scope="module")
def runs(built):
    return {c[0]: host_run(c) for c in gs.cases()}


def test_text_or_refusal(runs):
    assert len(runs) == len(gs.NAMES) >= 30
    for name, _, _, _, expect in gs.cases():
        got, st = runs[name]
        if expect is gs.REFUSED:
            assert got is gs.REFUSED, name
        else:
            assert got is not gs.REFUSED, name
            assert got == expect, name
        assert st["handed_back"] == 0, (name, st)


def test_refusals_say_why_and_come_late(runs):
    """Every refused file is refused for its own fault, and behind chunks that were guessed and kept: the fault sits where only the
    marker passes can see it."""
    names = [n for n in gs.NAMES if gs.group(n) == "refused"]
    assert len(names) == 9
    for name in names:
        messages, least = gs.refusal(name)
        got, st = runs[name]
        assert got is gs.REFUSED and any(m in _said[name] for m in messages), (name, _said.get(name))
        assert least >= 1 and st["most_accepted"] >= least, (name, least, st)
    assert gs.refusal("refused:far_back_9_chunks_in")[1] == 10 and gs.refusal("refused:bit_flip_in_nlen")[1] >= 50


def test_short_chunk_chains_are_chains(runs):
    """Flushed streams at 1024-byte chunks in one window: a run of at least 8 chunks kept in a row, and under 32 768 symbols to a kept
    chunk on average, so that a window is carried through several chunks (a match 22 - 27 KB back is some ten chunks back)."""
    names = [c[0] for c in gs.cases() if gs.group(c[0]) == "short"]
    assert len(names) == 7
    for name in names:
        _, st = runs[name]
        assert st["most_accepted"] >= 8, (name, st)
        assert len(gs.case(name)[4]) / st["accepted"] < 32768, (name, st)


def test_small_windows_are_many(runs):
    """window = 1024: at least ten times the windows of the same file in the default window, each with less than 32 KiB of text (the
    loop keeps a part of the window it had)."""
    names = [c[0] for c in gs.cases() if gs.group(c[0]) == "short_w1024"]
    assert len(names) == 4
    for name in names:
        _, st = runs[name]
        assert st["windows"] >= 10 * runs["short:" + name.split(":")[1]][1]["windows"], (name, st)
        assert len(gs.case(name)[4]) / st["windows"] < 32768, (name, st)


def test_hand_built_chunks_are_all_kept(runs):
    """Where the block positions are known, every planned chunk is kept: the blocks meant for a chunk that does not know its window
    are decoded in one."""
    planned = gs.min_accepted()
    assert len(planned) >= 6
    for name, least in planned.items():
        _, st = runs[name]
        assert least >= 2 and st["accepted"] >= least, (name, least, st)
    assert planned["extremes:chain"] >= 3 and planned["extremes:chain_empty_50"] >= 6
    _, st = runs["storedfixed:fastq_and_noise"]
    assert st["accepted"] >= 8, st


def test_decoys_are_taken_and_dropped(runs):
    for name in ("decoy:whole_streams", "decoy:headers_and_noise"):
        _, st = runs[name]
        assert st["redecoded"] > 0 and st["windows"] > 1, (name, st)


def test_many_members_are_many_windows(runs):
    _, st = runs["members:300"]
    assert st["windows"] >= 300, st


def test_high_ratio_behind_chunk_0_is_retried(runs):
    """More windows than the same file takes when every chunk has room for whatever DEFLATE can make of it (1040 symbols to a byte):
    the difference is chunks that ran out of room behind chunk 0 and were decoded again."""
    case = gs.case("ratio:periodic_after_fastq")
    got, roomy = host_run(case, ratio=1040)
    assert got == case[4]
    _, st = runs[case[0]]
    print("6 symbols to a byte:", st, "1040:", roomy)
    assert st["windows"] > roomy["windows"] and st["redecoded"] > roomy["redecoded"], (st, roomy)


def test_reader_cases_at_small_windows(built):
    """The two files the GPU test gives to the reader, at the 1024-byte chunks and windows it sets: the text, over at least 50 windows
    of one chunk each."""
    for name in ("short:zblock_l6", "storedfixed:fastq_and_noise"):
        _, blob, _, _, text = gs.case(name)
        got, st = host_run((name, blob, 1024, 1024, text))
        assert got == text, name
        assert st["windows"] >= 50 and st["most_accepted"] == 1, (name, st)


def test_reader_says_its_error_again(built, tmp_path, monkeypatch):
    """A reader whose inflating thread has ended with an error raises at every later call, too: it does not wait for text that nobody
    makes.  (The host path; the GPU test does the same with the device inflating.)"""
    from trio_binning_amd import seq
    from trio_binning_amd._lib import TbkError

    monkeypatch.setenv("TBK_PINFLATE_MIN", "0")
    f = tmp_path / "r.fastq.gz"
    f.write_bytes(gs.case("refused:far_back_9_chunks_in")[1])
    said = []

    def read():
        with seq.BatchReader(str(f)) as r:
            b = seq.Batch()
            for _ in range(3):
                try:
                    while r.next_batch(b, 1 << 20, 0):
                        pass
                    said.append(None)
                except (TbkError, ValueError, OSError) as e:
                    said.append(str(e))

    t = threading.Thread(target=read, daemon=True)
    t.start()
    t.join(60)
    assert not t.is_alive(), "the reader waits after its error"
    assert len(said) == 3 and said[0] and "too far back" in said[0] and said[1] == said[0] and said[2] == said[0], said
