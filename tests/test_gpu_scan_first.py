"""GPU parity of k_scan's streamed first piece: whatever `scan_first`, `scan_prune_step`, `scan_prune_lanes`, `scan_prune_mid` and
`scan_run` hold, the match list and the tapped raw maps are the oracle's, bit for bit.  Banks: (a) tests/scan_lane_cases.py's at
320x240 (two chunks, lane 63, dead upper neighbours, deaths at the modality boundary and inside modality 1), (b) the 64x48
four-lane shape, (c) tests/scan_first_cases.py's, whose modalities have 1 .. 31 features so that a first piece ends at the
modality's end, at a pad and inside a group of eight, and one detector with a single modality.  Every case of (c) is asserted on
the numpy model (tests/scan_first_model.py) under the very option values first, so that none is vacuous: for every `first` an
item ends at the first piece's check, one survives it to a candidate and one dies at a later check."""
import numpy as np
import pytest

import scan_first_cases as fcases
import scan_first_model as model
import scan_lane_cases as cases
from fealess_amd import api, synth
from util import options

pytestmark = pytest.mark.gpu

FIRSTS = (8, 12, 14, 16)
STEPS = (8, 4, 2)
LANES = (0, 1)
MIDS = (0, 0x01, 0x7F, 0xFF)
RUNS = (1, 3, 8)
T = [8]


def _assert_matches_equal(got, exp):
    assert len(got) == len(exp), (len(got), len(exp))
    for k in ("x", "y", "class_idx", "template_id"):
        assert np.array_equal(got[k], exp[k]), k
    assert np.array_equal(got["similarity"].view(np.uint32), exp["similarity"].view(np.uint32))


def _scene(oracle, qs, bank, w, h, thr):
    """The oracle's matches and raw maps of a bank: computed once, read by every case."""
    exp, n_exp = oracle.match_quantized(qs, w, h, T, [bank], thr)
    assert n_exp > 0, "test is vacuous: no matches"
    lms = [oracle.build_linear_memories(q, T[0]) for q in qs]
    maps = np.stack([oracle.total_similarity(lms, bank, g, w, h, T[0]) for g in range(bank.n_pyramids)])
    for a in (exp, maps):
        a.setflags(write=False)
    return dict(qs=qs, bank=bank, exp=exp, n_exp=n_exp, lms=lms, maps=maps, w=w, h=h, thr=thr)


def _detector(ctx, s):
    det = api.Detector(ctx, len(s["qs"]), T)
    det.add_class(s["bank"])
    det.finalize(s["w"], s["h"])
    return det


@pytest.fixture(scope="module")
def scenes(ctx, oracle):
    """name -> (scene, detector) of the four banks."""
    out = {}
    qs, bank, _, _ = cases.lane_bank()
    out["lanes"] = _scene(oracle, qs, bank, cases.W0, cases.H0, cases.THR)
    rng = np.random.default_rng(7)
    qs = [synth.random_quantized(rng, 64, 48, 0.5) for _ in range(2)]
    out["four"] = _scene(oracle, qs, synth.make_bank("obj", 5, 1, 2, 64, 48, seed=5, qs=qs, planted_frac=0.4, bbox=24), 64, 48, 60.0)
    for name, modalities in (("first", 2), ("single", 1)):
        qs, bank, kinds, where, counts = fcases.first_bank(modalities=modalities)
        out[name] = dict(_scene(oracle, qs, bank, cases.W0, cases.H0, fcases.THR), kinds=kinds, where=where, counts=counts)
    dets = {name: _detector(ctx, s) for name, s in out.items()}
    yield {name: (s, dets[name]) for name, s in out.items()}
    for det in dets.values():
        det.close()


def _assert_gpu_is_the_oracle(ctx, s, det, first, step, lanes, mid):
    n = s["bank"].n_pyramids
    taps = ((1, 1), (n // 2, 2), (n - 3, 3))              # tapped items between pruned and surviving ones, whatever the run
    for run in RUNS:
        key = (first, step, lanes, mid, run)
        with options(ctx, {"scan_first": first, "scan_prune_step": step, "scan_prune_lanes": lanes, "scan_prune_mid": mid,
                           "scan_run": run}):
            got, n_got = det.match_quantized(s["qs"], s["thr"])
            maps = [det.similarity_maps(f, c) for f, c in taps]
            if run == 3:
                maps.append(det.similarity_maps(0, n))
        assert n_got == s["n_exp"], key
        _assert_matches_equal(got, s["exp"])
        for (f, c), m in zip(taps + ((0, n),), maps):
            assert np.array_equal(m, s["maps"][f:f + c]), (key, f)


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("first", FIRSTS)
def test_first_piece(ctx, scenes, first, step):
    for lanes in LANES:
        for mid in MIDS:
            seen = [0, 0, 0]
            for name in ("first", "single"):
                s, det = scenes[name]
                items = model.scan(s["lms"], s["bank"], cases.W0, cases.H0, T[0], fcases.THR, mid=mid, lanes=lanes, step=step,
                                   first=first)
                for i, v in enumerate(fcases.check_cases(items, s["kinds"], s["where"], s["counts"], mid, lanes, step, first)):
                    seen[i] += v
            if mid in (0x7F, 0xFF):
                assert min(seen) > 0, (first, step, lanes, mid, seen)
            for name in ("first", "single", "lanes", "four"):
                s, det = scenes[name]
                _assert_gpu_is_the_oracle(ctx, s, det, first, step, lanes, mid)


def test_option_range(ctx):
    before = ctx.get_option("scan_first")
    for v in (-1, 1, 4, 9, 10, 13, 15, 17, 24, 32):
        with pytest.raises(api.FealessError):
            ctx.set_option("scan_first", v)
        assert ctx.get_option("scan_first") == before
    for v in (0, 8, 12, 14, 16):
        ctx.set_option("scan_first", v)
        assert ctx.get_option("scan_first") == v
    ctx.set_option("scan_first", before)
