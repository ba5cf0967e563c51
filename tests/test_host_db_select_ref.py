"""tests/db_select_ref.py - the numpy restatement of tbk_kmerdb_select's rule that the device tests compare with - against
the rule worked out key by key on Python dicts: every mode pair, every counter rule, keys a partner holds outside its range,
a sum that saturates, a database as its own partner, and the empty cases."""
import itertools

import numpy as np
import pytest

import db_select_ref as ref


def _brute(base, base_range, partners, rule):
    """base: {key: counter}; partners: ({key: counter}, (min, max), mode).  The rule of include/tbk.h, one key at a time."""
    keys, counts = [], []
    for key in sorted(base):
        c = base[key]
        if not base_range[0] <= c <= base_range[1]:
            continue
        kept, low, total = True, c, c
        for held, (lo, hi), mode in partners:
            answer = key in held and lo <= held[key] <= hi
            if answer != (mode == ref.REQUIRE):
                kept = False
            if mode == ref.REQUIRE and key in held:
                low, total = min(low, held[key]), total + held[key]
        if kept:
            keys.append(key)
            counts.append({ref.BASE: c, ref.MIN: low, ref.SUM: min(255, total)}[rule])
    hist = [0] * 256
    for c in counts:
        hist[c] += 1
    hist[0] = len(keys)
    return keys, counts, hist


def _arrays(d):
    keys = sorted(d)
    return np.array(keys, dtype=np.uint64), np.array([d[k] for k in keys], dtype=np.uint8)


def _check(base, base_range, partners, rule):
    got = ref.select(*_arrays(base), base_range, [(*_arrays(d), r, m) for d, r, m in partners], rule)
    want = _brute(base, base_range, partners, rule)
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint8 and got[2].dtype == np.uint64 and got[2].shape == (256,)
    assert [int(v) for v in got[0]] == want[0] and [int(v) for v in got[1]] == want[1] and [int(v) for v in got[2]] == want[2]
    return want


VALUES = (1, 2, 127, 128, 254, 255)
TOP = (1 << 64) - 1


def _world(seed):
    """three dicts over some forty keys, among them 0, 2^63 - 1, 2^63 and 2^64 - 1, with every pair of VALUES on some shared key"""
    rng = np.random.default_rng(seed)
    pool = sorted({int(v) for v in rng.integers(0, 1 << 62, 36)} | {0, (1 << 63) - 1, 1 << 63, TOP})
    dicts = [{}, {}, {}]
    pairs = itertools.cycle(itertools.product(VALUES, VALUES, VALUES))
    for key in pool:
        which = int(rng.integers(1, 8))  # a non-empty subset of the three
        for i, c in enumerate(next(pairs)):
            if which >> i & 1:
                dicts[i][key] = c
    return dicts


RANGES = ((1, 255), (2, 255), (128, 254), (1, 1), (255, 255), (3, 126))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_every_mode_pair_rule_and_range(seed):
    base, y, z = _world(seed)
    seen = {"out_of_range_partner": 0, "saturated": 0, "min_from_partner": 0, "min_from_base": 0, "empty": 0, "kept": 0}
    modes = (ref.REQUIRE, ref.EXCLUDE)
    for rule in (ref.BASE, ref.MIN, ref.SUM):
        for base_range, y_range, z_range in itertools.product(RANGES[:3] + RANGES[3:4], RANGES, RANGES[::2]):
            shapes = [[]] + [[(y, y_range, m)] for m in modes] + [[(y, y_range, m0), (z, z_range, m1)] for m0 in modes for m1 in modes]
            for partners in shapes:
                keys, counts, _ = _check(base, base_range, partners, rule)
                seen["empty" if not keys else "kept"] += 1
                for key, c in zip(keys, counts):
                    required = [d[key] for d, _, m in partners if m == ref.REQUIRE]
                    if rule == ref.SUM and required and base[key] + sum(required) > 255:
                        assert c == 255
                        seen["saturated"] += 1
                    if rule == ref.MIN and required:
                        seen["min_from_partner" if min(required) < base[key] else "min_from_base"] += 1
                for d, (lo, hi), m in partners:
                    # an EXCLUDE partner that holds a kept key holds it outside its range
                    seen["out_of_range_partner"] += sum(1 for key in keys if m == ref.EXCLUDE and key in d and not lo <= d[key] <= hi)
    assert all(seen.values()), seen


def test_the_rule_on_a_case_written_out():
    base = {10: 2, 20: 3, 30: 200, 40: 9, 50: 255, 60: 1}
    y = {10: 1, 20: 64, 30: 100, 45: 7, 50: 255}
    z = {20: 65, 40: 2, 50: 255, 60: 2}
    R, E = ref.REQUIRE, ref.EXCLUDE
    assert _check(base, (1, 255), [], ref.SUM)[:2] == ([10, 20, 30, 40, 50, 60], [2, 3, 200, 9, 255, 1])
    assert _check(base, (2, 255), [(y, (1, 255), R)], ref.BASE)[:2] == ([10, 20, 30, 50], [2, 3, 200, 255])
    assert _check(base, (2, 255), [(y, (2, 255), R)], ref.MIN)[:2] == ([20, 30, 50], [3, 100, 255])       # y's 1 on key 10 is out of range
    assert _check(base, (2, 255), [(y, (2, 255), R)], ref.SUM)[:2] == ([20, 30, 50], [67, 255, 255])      # 300 and 510 saturate
    assert _check(base, (1, 255), [(y, (2, 255), E)], ref.SUM)[:2] == ([10, 40, 60], [2, 9, 1])           # held below the range: not excluded
    assert _check(base, (1, 255), [(y, (1, 255), R), (z, (1, 255), E)], ref.SUM)[:2] == ([10, 30], [3, 255])
    assert _check(base, (1, 255), [(z, (1, 255), E), (y, (1, 255), R)], ref.SUM)[:2] == ([10, 30], [3, 255])  # the order of the partners is none
    assert _check(base, (1, 255), [(y, (1, 255), R), (z, (1, 255), R)], ref.SUM)[:2] == ([20, 50], [132, 255])
    assert _check(base, (1, 255), [(y, (1, 255), R), (z, (1, 255), R)], ref.MIN)[:2] == ([20, 50], [3, 255])
    assert _check(base, (1, 255), [(y, (1, 255), E), (z, (1, 255), E)], ref.MIN)[:2] == ([], [])
    assert _check(base, (1, 255), [(z, (66, 255), E), (y, (64, 64), R)], ref.MIN)[:2] == ([20], [3])     # z's 65 missed by one, y's 64 met
    assert _check(base, (4, 8), [], ref.BASE)[:2] == ([], [])


def test_a_database_as_its_own_partner_and_the_empty_sides():
    base = {5: 1, 6: 2, 7: 200}
    R, E = ref.REQUIRE, ref.EXCLUDE
    assert _check(base, (1, 255), [(base, (1, 255), R)], ref.SUM)[:2] == ([5, 6, 7], [2, 4, 255])
    assert _check(base, (1, 255), [(base, (2, 255), R), (base, (200, 255), E)], ref.MIN)[:2] == ([6], [2])
    assert _check(base, (1, 255), [(base, (1, 255), E)], ref.BASE)[:2] == ([], [])
    assert _check(base, (1, 255), [({}, (1, 255), E)], ref.SUM)[:2] == ([5, 6, 7], [1, 2, 200])
    assert _check(base, (1, 255), [({}, (1, 255), R)], ref.SUM)[:2] == ([], [])
    keys, counts, hist = _check({}, (1, 255), [(base, (1, 255), E), ({}, (1, 255), R)], ref.MIN)
    assert keys == [] and counts == [] and not any(hist)
