"""The numpy restatement of k_scan's pruning (tests/scan_prune_model.py) is exact: whatever the lanes switch, the step and the
mask of checked groups, its candidates are the oracle's matches.  No GPU."""
import numpy as np

import scan_lane_cases as cases
import scan_prune_model as model
from fealess_amd import synth
from fealess_amd.bank import TemplateBank

LANES = (0, 1)
STEPS = (8, 4, 2)
MIDS = (0, 0x01, 0x55, 0x7F, 0xFF)


def _assert_model_is_the_oracle(oracle, qs, w, h, bank, thr):
    exp, n_exp = oracle.match_quantized(qs, w, h, [8], [bank], thr)
    assert n_exp > 0, "test is vacuous: no matches"
    lms = [oracle.build_linear_memories(q, 8) for q in qs]
    pruned = 0
    for lanes in LANES:
        for step in STEPS:
            for mid in MIDS:
                items = model.scan(lms, bank, w, h, 8, thr, mid=mid, lanes=lanes, step=step)
                got = model.matches(items)
                key = (lanes, step, mid)
                assert len(got["x"]) == n_exp, key
                for k in ("x", "y", "template_id"):
                    assert np.array_equal(got[k], exp[k]), (key, k)
                assert np.array_equal(got["similarity"].view(np.uint32), exp["similarity"].view(np.uint32)), key
                pruned += sum(any(mask != (1 << 64) - 1 for _, mask in it["checks"]) for it in items)
    assert pruned > 0, "test is vacuous: no check ever removed a lane"
    return lms


def test_two_chunks(oracle):
    """320x240 at T = 8: 1200 positions, two chunks, the second with 176 positions."""
    qs, bank, kinds, where = cases.lane_bank()
    lms = _assert_model_is_the_oracle(oracle, qs, cases.W0, cases.H0, bank, cases.THR)
    items = model.scan(lms, bank, cases.W0, cases.H0, 8, cases.THR)
    assert {it["chunk"] for it in items} == {0, 1}
    assert any(it["chunk"] == 1 and it["candidates"] for it in items)
    # the unpruned walk loads every feature for every lane with positions, the pruned ones less and less
    loads = {(l, s): sum(it["lane_loads"] for it in model.scan(lms, bank, cases.W0, cases.H0, 8, cases.THR, lanes=l, step=s))
             for l in LANES for s in STEPS}
    full = sum(it["lane_loads"] for it in model.scan(lms, bank, cases.W0, cases.H0, 8, cases.THR, prune=0))
    assert full > loads[0, 8] > loads[1, 8] > loads[1, 4] > loads[1, 2]


def test_four_lanes(oracle):
    """64x48: 48 positions, four lanes."""
    rng = np.random.default_rng(7)
    qs = [synth.random_quantized(rng, 64, 48, 0.5) for _ in range(2)]
    bank = synth.make_bank("obj", 5, 1, 2, 64, 48, seed=5, qs=qs, planted_frac=0.4, bbox=24)
    _assert_model_is_the_oracle(oracle, qs, 64, 48, bank, 60.0)


def test_modalities_with_different_template_positions(oracle):
    """The colour template's positions end in chunk 0 (200x100 pixels: 273 positions), the depth template's reach chunk 1."""
    rng = np.random.default_rng(3)
    qs = [synth.random_quantized(rng, cases.W0, cases.H0, 0.12) for _ in range(2)]
    bank = TemplateBank("obj", 1, 2)
    for i in range(12):
        def tpl(s_w, s_h, n):
            f = np.stack([rng.integers(0, s_w + 1, n), rng.integers(0, s_h + 1, n), rng.integers(0, 8, n)], 1).astype(np.int32)
            return dict(width=s_w, height=s_h, offset_x=0, offset_y=0, pyramid_level=0, features=f)
        bank.add_pyramid([tpl(200, 100, 4 + i), tpl(40, 40, 12 + 2 * i)])
    lms = _assert_model_is_the_oracle(oracle, qs, cases.W0, cases.H0, bank, 20.0)
    items = model.scan(lms, bank, cases.W0, cases.H0, 8, 20.0)
    assert any(it["chunk"] == 1 for it in items)


def test_every_lane_case_is_what_it_is_meant_to_be(oracle):
    """The bank of tests/test_gpu_scan_lanes.py, by the model: see check_cases."""
    qs, bank, kinds, where = cases.lane_bank()
    lms = [oracle.build_linear_memories(q, 8) for q in qs]
    for lanes in LANES:
        for step in STEPS:
            for mid in MIDS:
                cases.check_cases(model.scan(lms, bank, cases.W0, cases.H0, 8, cases.THR, mid=mid, lanes=lanes, step=step), kinds, where, mid, lanes)
