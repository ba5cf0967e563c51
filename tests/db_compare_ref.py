"""The comparisons between count databases (include/tbk.h: tbk_kmerdb_joint_spectrum, tbk_kmerdb_origin_spectrum) restated with
numpy on (ascending keys, counters): np.union1d, np.searchsorted and np.add.at.  Every quantity is an integer count, so what
tests/test_host_compare_databases.py and tests/test_gpu_kmerdb_compare.py compare with is exact."""
import numpy as np


def counter_in(keys, counts, wanted):
    """For every key of `wanted`: its counter among (keys, counts), 0 where `keys` lacks it."""
    keys, wanted = np.asarray(keys, dtype=np.uint64), np.asarray(wanted, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.uint8)
    out = np.zeros(wanted.size, dtype=np.int64)
    if keys.size and wanted.size:
        at = np.minimum(np.searchsorted(keys, wanted), keys.size - 1)
        found = keys[at] == wanted
        out[found] = counts[at[found]]
    return out


def joint_spectrum(x_keys, x_counts, y_keys, y_counts):
    """(256, 256) uint64: cell [cx, cy] = distinct keys with counter cx in x and cy in y, 0 = not held."""
    both = np.union1d(np.asarray(x_keys, dtype=np.uint64), np.asarray(y_keys, dtype=np.uint64))
    spec = np.zeros((256, 256), dtype=np.uint64)
    np.add.at(spec, (counter_in(x_keys, x_counts, both), counter_in(y_keys, y_counts, both)), np.uint64(1))
    return spec


def origin_spectrum(base_keys, base_counts, y_keys, y_counts, y_range, z_keys, z_counts, z_range):
    """(4, 256) uint64: cell [cls, c] = entries of base with counter c; bit 0 of cls: y holds the key with a counter in
    y_range (inclusive), bit 1: the same for z."""
    cy, cz = counter_in(y_keys, y_counts, base_keys), counter_in(z_keys, z_counts, base_keys)
    cls = ((cy >= y_range[0]) & (cy <= y_range[1])).astype(np.int64) | (((cz >= z_range[0]) & (cz <= z_range[1])).astype(np.int64) << 1)
    spec = np.zeros((4, 256), dtype=np.uint64)
    np.add.at(spec, (cls, np.asarray(base_counts, dtype=np.int64)), np.uint64(1))
    return spec


def check_joint_invariants(spec, x_counts, y_counts, union_size):
    """The properties a joint spectrum has by construction."""
    assert spec.shape == (256, 256) and spec.dtype == np.uint64
    assert int(spec[0, 0]) == 0
    rows, cols = np.bincount(np.asarray(x_counts, dtype=np.uint8), minlength=256), np.bincount(np.asarray(y_counts, dtype=np.uint8), minlength=256)
    assert np.array_equal(spec.sum(axis=1)[1:], rows[1:].astype(np.uint64))
    assert np.array_equal(spec.sum(axis=0)[1:], cols[1:].astype(np.uint64))
    assert int(spec.sum()) == union_size


def check_origin_invariants(spec, base_counts):
    assert spec.shape == (4, 256) and spec.dtype == np.uint64
    assert not spec[:, 0].any()
    assert np.array_equal(spec.sum(axis=0), np.bincount(np.asarray(base_counts, dtype=np.uint8), minlength=256).astype(np.uint64))
