"""The numpy restatement of k_scan's streamed first piece (tests/scan_first_model.py): with `first` = 8 it is
tests/scan_prune_model.py item for item, with any `first` its candidates are the oracle's matches, and the banks of
tests/scan_first_cases.py are what they are meant to be.  No GPU."""
import numpy as np
import pytest

import scan_first_cases as fcases
import scan_first_model as model
import scan_lane_cases as cases
import scan_prune_model as base

STEPS = (8, 4, 2)
MIDS = (0, 0x01, 0x7F, 0xFF)


def test_pieces():
    assert model.pieces(8, 16, 4) == [(0, 8, 0)]
    assert model.pieces(16, 8, 4) == [(0, 8, 0), (8, 4, 1), (12, 4, 1)]
    assert model.pieces(16, 12, 8) == [(0, 12, 1), (12, 4, 1)]
    assert model.pieces(16, 12, 2) == [(0, 12, 1), (12, 2, 1), (14, 2, 1)]
    assert model.pieces(24, 14, 4) == [(0, 14, 1), (14, 2, 1), (16, 4, 2), (20, 4, 2)]
    assert model.pieces(24, 16, 8) == [(0, 16, 1), (16, 8, 2)]


def test_first_8_is_the_earlier_model(oracle):
    qs, bank, _, _ = cases.lane_bank()
    lms = [oracle.build_linear_memories(q, 8) for q in qs]
    for lanes in (0, 1):
        for step in STEPS:
            for mid in (0x01, 0x55, 0x7F):
                a = base.scan(lms, bank, cases.W0, cases.H0, 8, cases.THR, mid=mid, lanes=lanes, step=step)
                b = model.scan(lms, bank, cases.W0, cases.H0, 8, cases.THR, mid=mid, lanes=lanes, step=step, first=8)
                assert len(a) == len(b)
                for x, y in zip(a, b):
                    assert all(x[k] == y[k] for k in x), (lanes, step, mid, x["g"], x["chunk"])


@pytest.mark.parametrize("modalities", (2, 1))
def test_first_cases(oracle, modalities):
    qs, bank, kinds, where, counts = fcases.first_bank(modalities=modalities)
    exp, n_exp = oracle.match_quantized(qs, cases.W0, cases.H0, [8], [bank], fcases.THR)
    assert n_exp > 0
    lms = [oracle.build_linear_memories(q, 8) for q in qs]
    loads = {}
    for first in model.FIRSTS:
        for step in STEPS:
            for lanes in (0, 1):
                for mid in MIDS:
                    key = (first, step, lanes, mid)
                    items = model.scan(lms, bank, cases.W0, cases.H0, 8, fcases.THR, mid=mid, lanes=lanes, step=step, first=first)
                    seen = fcases.check_cases(items, kinds, where, counts, mid, lanes, step, first)
                    if mid in (0x7F, 0xFF):
                        assert seen[0] > 0 and seen[1] > 0 and (modalities == 1 or seen[2] > 0), (key, seen)
                    got = model.matches(items)
                    assert len(got["x"]) == n_exp, key
                    for k in ("x", "y", "template_id"):
                        assert np.array_equal(got[k], exp[k]), (key, k)
                    assert np.array_equal(got["similarity"].view(np.uint32), exp["similarity"].view(np.uint32)), key
                    loads[key] = sum(it["loads"] for it in items)
    # behind pieces of two a longer first piece only leaves checks out, so it never loads fewer features
    assert loads[8, 2, 1, 0x7F] <= loads[12, 2, 1, 0x7F] <= loads[14, 2, 1, 0x7F] <= loads[16, 2, 1, 0x7F]
