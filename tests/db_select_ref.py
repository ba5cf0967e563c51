"""The selection from count databases into a database (include/tbk.h: tbk_kmerdb_select) restated with numpy on (ascending
keys, counters): np.searchsorted (through db_compare_ref.counter_in) and np.isin.  Keys, counters and the histogram are
integers, so what tests/test_host_db_select_ref.py and tests/test_gpu_kmerdb_select.py compare with is exact."""
import numpy as np

from db_compare_ref import counter_in

REQUIRE, EXCLUDE = 1, 2
BASE, MIN, SUM = 0, 1, 2
RULES = {"base": BASE, "min": MIN, "sum": SUM}


def select(base_keys, base_counts, base_range=(1, 255), partners=(), rule=BASE):
    """partners: up to two (keys, counts, (min, max), mode), mode REQUIRE or EXCLUDE; ranges inclusive and literal.
    Returns (keys uint64, counters uint8, hist uint64[256]) of the full database the selection is: the kept entries in base's
    order, rows 1..255 tallied from the counters, row 0 = n."""
    assert len(partners) <= 2 and rule in (BASE, MIN, SUM)
    base_keys, base_counts = np.asarray(base_keys, dtype=np.uint64), np.asarray(base_counts, dtype=np.uint8)
    mine = base_counts.astype(np.int64)
    assert 1 <= base_range[0] <= base_range[1] <= 255
    keep = (mine >= base_range[0]) & (mine <= base_range[1])
    low, total = mine.copy(), mine.copy()
    for keys, counts, (lo, hi), mode in partners:
        assert 1 <= lo <= hi <= 255 and mode in (REQUIRE, EXCLUDE)
        theirs = counter_in(keys, counts, base_keys)
        assert np.array_equal(theirs > 0, np.isin(base_keys, np.asarray(keys, dtype=np.uint64)))
        held = (theirs >= lo) & (theirs <= hi)
        keep &= held if mode == REQUIRE else ~held
        if mode == REQUIRE:  # (where it matters - on kept entries - the partner holds the key: theirs >= 1)
            low, total = np.minimum(low, theirs), total + theirs
    made = {BASE: mine, MIN: low, SUM: np.minimum(total, 255)}[rule][keep]
    hist = np.bincount(made, minlength=256).astype(np.uint64)
    assert hist[0] == 0
    hist[0] = made.size
    return base_keys[keep], made.astype(np.uint8), hist
