"""GPU parity of k_scan's per-lane pruning and its finer steps between checks: whatever `scan_prune_lanes`, `scan_prune_step`,
`scan_prune_mid` and `scan_run` hold, the match list and the raw maps are the oracle's, bit for bit.  Shapes as in
tests/test_gpu_scan_runs.py: 320x240 at T = 8 (1200 positions: two chunks, the second with 176 positions) and 64x48 (48 positions:
four lanes).  The 320x240 bank is tests/scan_lane_cases.py's: single survivors in lane 0, a middle lane, lane 63, the last lane with
positions and chunk 1, candidates on a lane's last position with a dead upper neighbour, adjacent and distant pairs, lanes that die
at the modality boundary, items that die inside modality 1, in rotated orders -- each asserted on the numpy model
(tests/scan_prune_model.py) under the very option values, so that no case is vacuous."""
import numpy as np
import pytest

import scan_lane_cases as cases
import scan_prune_model as model
from fealess_amd import api, synth
from util import options

pytestmark = pytest.mark.gpu

LANES = (0, 1)
STEPS = (8, 4, 2)
MIDS = (0, 0x01, 0x55, 0x7F, 0xFF)
RUNS = (1, 3, 8)
T = [8]


def _assert_matches_equal(got, exp):
    assert len(got) == len(exp), (len(got), len(exp))
    for k in ("x", "y", "class_idx", "template_id"):
        assert np.array_equal(got[k], exp[k]), k
    assert np.array_equal(got["similarity"].view(np.uint32), exp["similarity"].view(np.uint32))


@pytest.fixture(scope="module")
def lane_scene(oracle):
    """The bank, the oracle's matches and raw maps: computed once, read by every case."""
    qs, bank, kinds, where = cases.lane_bank()
    exp, n_exp = oracle.match_quantized(qs, cases.W0, cases.H0, T, [bank], cases.THR)
    assert n_exp > 0
    lms = [oracle.build_linear_memories(q, T[0]) for q in qs]
    maps = np.stack([oracle.total_similarity(lms, bank, g, cases.W0, cases.H0, T[0]) for g in range(bank.n_pyramids)])
    for a in (exp, maps):
        a.setflags(write=False)
    return dict(qs=qs, bank=bank, kinds=kinds, where=where, exp=exp, n_exp=n_exp, lms=lms, maps=maps)


@pytest.fixture(scope="module")
def lane_detector(ctx, lane_scene):
    det = api.Detector(ctx, 2, T)
    det.add_class(lane_scene["bank"])
    det.finalize(cases.W0, cases.H0)
    yield det
    det.close()


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("lanes", LANES)
def test_lane_cases(ctx, lane_scene, lane_detector, lanes, step):
    s, det = lane_scene, lane_detector
    n = s["bank"].n_pyramids
    taps = ((1, 1), (n // 2, 2), (n - 3, 3))              # tapped items between pruned and surviving ones, whatever the run
    for mid in MIDS:
        cases.check_cases(model.scan(s["lms"], s["bank"], cases.W0, cases.H0, T[0], cases.THR, mid=mid, lanes=lanes, step=step),
                          s["kinds"], s["where"], mid, lanes)
        for run in RUNS:
            key = (lanes, step, mid, run)
            with options(ctx, {"scan_prune_lanes": lanes, "scan_prune_step": step, "scan_prune_mid": mid, "scan_run": run}):
                got, n_got = det.match_quantized(s["qs"], cases.THR)
                maps = [det.similarity_maps(first, count) for first, count in taps]
                if run == 3:
                    maps.append(det.similarity_maps(0, n))
            assert n_got == s["n_exp"], key
            _assert_matches_equal(got, s["exp"])
            for (first, count), m in zip(taps + ((0, n),), maps):
                assert np.array_equal(m, s["maps"][first:first + count]), (key, first)


@pytest.mark.parametrize("lanes", LANES)
def test_four_lanes(ctx, oracle, lanes):
    """64x48: 48 positions, lanes_on = 4."""
    rng = np.random.default_rng(7)
    qs = [synth.random_quantized(rng, 64, 48, 0.5) for _ in range(2)]
    bank = synth.make_bank("obj", 5, 1, 2, 64, 48, seed=5, qs=qs, planted_frac=0.4, bbox=24)
    n = bank.n_pyramids
    exp, n_exp = oracle.match_quantized(qs, 64, 48, T, [bank], 60.0)
    assert n_exp > 0, "test is vacuous: no matches"
    lms = [oracle.build_linear_memories(q, T[0]) for q in qs]
    exp_maps = np.stack([oracle.total_similarity(lms, bank, g, 64, 48, T[0]) for g in range(n)])
    det = api.Detector(ctx, 2, T)
    det.add_class(bank)
    det.finalize(64, 48)
    try:
        for step in STEPS:
            for mid in MIDS:
                for run in RUNS:
                    key = (lanes, step, mid, run)
                    with options(ctx, {"scan_prune_lanes": lanes, "scan_prune_step": step, "scan_prune_mid": mid, "scan_run": run}):
                        got, n_got = det.match_quantized(qs, 60.0)
                        maps = det.similarity_maps(0, n)
                        one = det.similarity_maps(n // 2, 1)
                    assert n_got == n_exp, key
                    _assert_matches_equal(got, exp)
                    assert np.array_equal(maps, exp_maps) and np.array_equal(one, exp_maps[n // 2:n // 2 + 1]), key
    finally:
        det.close()


def test_option_ranges(ctx):
    for name, good, bad in (("scan_prune_lanes", (0, 1), (-1, 2)), ("scan_prune_step", (0, 2, 4, 8), (-1, 1, 3, 6, 16))):
        before = ctx.get_option(name)
        for v in bad:
            with pytest.raises(api.FealessError):
                ctx.set_option(name, v)
            assert ctx.get_option(name) == before
        for v in good:
            ctx.set_option(name, v)
            assert ctx.get_option(name) == v
        ctx.set_option(name, before)
