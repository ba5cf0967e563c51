"""choose_passes, the rule by which find-unique-kmers decides in how many passes a library is counted, and the
--passes option (no device needed)."""
import pytest

from trio_binning_amd import find_unique_kmers as fu

GB = 10 ** 9


def test_one_pass_when_everything_fits():
    assert fu.choose_passes(10 ** 6, 10 ** 8, 200 * GB) == 1
    assert fu.choose_passes(1 * GB, 10 * GB, 200 * GB) == 1   # 4 tables of 26.7 GB within 160 GB
    # the edge: 4 * (capacity * 80 // 3) against 4/5 of the free bytes
    assert fu.choose_passes(3 * 10 ** 6, 0, 400 * 10 ** 6) == 1   # 320 000 000 <= 320 000 000
    assert fu.choose_passes(3 * 10 ** 6, 0, 400 * 10 ** 6 - 2) > 1


def test_hand_computed_cases():
    # budget 160e9.  One pass: 4 * 106.67e9 > budget.  Kept: store 20e9 + databases 2 * 9 * 0.5e9 = 9e9; 131e9 remain
    # for 3 * table(P) = 3 * ceil(4e9 / P) * 80 // 3: P = 2 -> 160e9, P = 3 -> 106.67e9.
    assert fu.choose_passes(4 * GB, 40 * GB, 200 * GB) == 3
    # budget 224e9.  store 45e9 + databases 2 * 9 * 2e9 = 36e9; 143e9 remain; 3 * table(8) = 160e9, 3 * table(9) = 142.2e9.
    assert fu.choose_passes(16 * GB, 90 * GB, 280 * GB) == 9
    # budget 80e9.  One pass: 4 * 26.67e9 = 106.67e9 > budget.  store 1e9 + databases 2.25e9; 76.75e9 remain;
    # 3 * table(2) = 40e9.
    assert fu.choose_passes(1 * GB, 2 * GB, 100 * GB) == 2


def test_monotonic_in_free_bytes_and_capacity():
    last = 0
    for free in range(300, 60, -5):
        p = fu.choose_passes(8 * GB, 40 * GB, free * GB)
        assert p >= last
        last = p
    assert last > 8
    last = 0
    for cap in range(1, 40):
        p = fu.choose_passes(cap * GB // 2, 40 * GB, 200 * GB)
        assert p >= last
        last = p
    assert last > 4


def test_error_when_the_store_alone_does_not_fit():
    with pytest.raises(ValueError, match="reads alone"):
        fu.choose_passes(50 * GB, 400 * GB, 200 * GB)    # 200e9 bytes of packed reads, 160e9 planned
    with pytest.raises(ValueError, match="--capacity"):
        fu.choose_passes(90 * GB, 90 * GB, 200 * GB)     # the databases planned for 90e9 k-mers leave no room
    with pytest.raises(ValueError):
        fu.choose_passes(0, 10, 10)


def test_parse_args_accepts_passes():
    args = fu.parse_args(["-k", "21", "--passes", "4", "a.fq", "b.fq"])
    assert args.passes == 4 and args.kmer_size == 21 and args.read_files == ["a.fq", "b.fq"]
    assert fu.parse_args(["-k", "21", "a.fq", "b.fq"]).passes == 0
