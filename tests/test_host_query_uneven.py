"""The crafted database and batch of tests/uneven_case.py are what they are meant to be: every claim that
tests/test_gpu_query_uneven.py rests on, asserted from numpy and from the references' answers, without a device.  The numbers
are printed (pytest -s shows them)."""
import json

import numpy as np

import db_query_ref as ref
import uneven_case


def test_the_database_and_the_batch_are_what_they_are_meant_to_be():
    c = uneven_case.case()
    numbers = uneven_case.claims(c)
    print(json.dumps({str(key): value for key, value in numbers.items()}, indent=1))
    for full in (False, True):
        assert numbers[full]["directory bits"] == 17 and numbers[full]["deep bucket"] >= 4096
        assert numbers[full]["groups with the deep search first"] >= 4 and numbers[full]["groups with the deep search last"] >= 4
        assert min(numbers[full]["repair records by kind (none, sub, del, ins, long)"]) >= 1


def test_the_rank_backed_mapping_and_the_numpy_tally_agree_on_the_batch():
    """window for window: screen_ref's counters over rank_db are the bytes db_query_ref.TallyNp returns"""
    c = uneven_case.case()
    for full in (False, True):
        c.want_evidence(1, 255, full)
        _, counts = c.tally(full).add(c.bases, c.offsets, uneven_case.K)
        flat = np.zeros(c.bases.size, dtype=np.uint8)
        clean = np.zeros(c.bases.size, dtype=bool)
        for r, per_window in enumerate(c._counters[full]):
            for w, v in enumerate(per_window):
                if v is not None:
                    flat[int(c.offsets[r]) + w], clean[int(c.offsets[r]) + w] = v, True
        assert np.array_equal(flat, counts) and np.array_equal(clean, ref.window_ranks(c.bases, c.offsets, uneven_case.K)[1])
