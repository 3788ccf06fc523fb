"""GPU parity on cluttered frames (tests/clutter.py): three instances of the object in front of a textured, non-planar
background, a bank of near views of every instance (trained by the oracle) padded with random pyramids.  Every coarse
candidate of an instance has neighbours that tie or nearly tie with it, which is where the scan's pruning, the refinement's
argmax, the sort / unique and the lazy fine levels have to get every tie right; the ICP crops hold background and parts of
neighbouring instances.  Everything is compared with the oracle bit for bit, under every value of the runtime options
(fl_context_set_option: "speed only: results are identical whatever they hold")."""
import numpy as np
import pytest

import clutter
from fealess_amd import api
from fealess_amd import _lib as L
from util import options as _options

pytestmark = pytest.mark.gpu

PARAMS = ((75.0, 10, 0.5, 0.01), (75.0, 20, 0.0, -3.0e38))       # the second one runs all 20 iterations
TOPK, NMS_DIST = 12, 60.0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def scene(oracle):
    sc = clutter.build(oracle)
    sc["bgrs"] = [sc["frames"][f][0] for f in clutter.FRAMES]
    sc["depths"] = [sc["frames"][f][1] for f in clutter.FRAMES]
    return sc


@pytest.fixture(scope="module")
def expected(oracle, scene):
    """The oracle's Recognition() per parameter set and frame, and its match list per frame."""
    reco = {p: [oracle.recognition(b, d, scene["K"], clutter.T, scene["bank"], *p) for b, d in zip(scene["bgrs"], scene["depths"])]
            for p in PARAMS}
    matches = [oracle.match_images(b, d, clutter.T, [scene["bank"]], 75.0) for b, d in zip(scene["bgrs"], scene["depths"])]
    return dict(reco=reco, matches=matches)


def _detector(ctx, scene, max_batch=len(clutter.FRAMES), max_candidates=0):
    det = api.Detector(ctx, 2, clutter.T)
    det.add_class(scene["bank"])
    det.finalize(clutter.W, clutter.H, max_batch=max_batch, max_candidates=max_candidates)
    return det


def _assert_reco_equal(g, e, tag):
    """A Recognition() result against another (the oracle's or the library's own), bit for bit."""
    assert g["status"] == 0 and g["found"] == e["found"] and g["n_matches"] == e["n_matches"], tag
    if not e["found"]:
        return
    assert (g["best"]["x"], g["best"]["y"], g["best"]["template_id"]) == (e["best"]["x"], e["best"]["y"], e["best"]["template_id"]), tag
    assert _bits(g["best"]["similarity"]) == _bits(e["best"]["similarity"]), tag
    assert g["det"]["n_points"] == e["det"]["n_points"] and g["det"]["icp"]["iters"] == e["det"]["icp"]["iters"], tag
    assert _bits(g["det"]["icp"]["dist_mean"]) == _bits(e["det"]["icp"]["dist_mean"]), tag
    assert np.array_equal(_bits(g["pose"]), _bits(e["pose"])), tag


def _assert_matches_equal(got, exp, tag):
    assert len(got) == len(exp), (tag, len(got), len(exp))
    for k in ("x", "y", "class_idx", "template_id"):
        assert np.array_equal(got[k], exp[k]), (tag, k)
    assert np.array_equal(got["similarity"].view(np.uint32), exp["similarity"].view(np.uint32)), tag


def test_clutter_recognition_matches_oracle(ctx, scene, expected):
    """Recognition() of frames a - d in one batch, lazy and eager fine levels, equals the oracle's; so does the whole refined
    match list.  Frame a must really be cluttered on the GPU side too: at least 100 coarse candidates."""
    for mode in ("lazy", "eager"):
        ctx.set_option("eager_frontend", 1 if mode == "eager" else 0)       # sampled by fl_detector_finalize
        try:
            det = _detector(ctx, scene)
        finally:
            ctx.set_option("eager_frontend", 0)
        for p in PARAMS:
            got = det.recognize_batch(scene["bgrs"], scene["depths"], scene["K"], *p)
            for i, f in enumerate(clutter.FRAMES):
                _assert_reco_equal(got[i], expected["reco"][p][i], (mode, p, f))
            assert [g["found"] for g in got] == [1, 1, 1, 0]
            cnt = det.frame_counters(0)
            assert cnt[0] >= 100 and cnt[2] == 0, (mode, cnt)
        lists = det.match_batch(scene["bgrs"], scene["depths"], 75.0)
        for i, f in enumerate(clutter.FRAMES):
            exp, n_exp = expected["matches"][i]
            assert lists[i][1] == n_exp, (mode, f)
            _assert_matches_equal(lists[i][0], exp, (mode, f))
        det.close()


def test_clutter_topk_and_nms_match_oracle(ctx, oracle, scene):
    """The first 12 matches of every frame refined in one launch, and the NMS winners among them, equal the oracle's: this
    refines every instance, the occluded one of frame b and the one across frame c's border included."""
    det = _detector(ctx, scene)
    p = PARAMS[0]
    got = det.recognize_batch_topk(scene["bgrs"], scene["depths"], scene["K"], TOPK, *p)
    n_win = []
    for i, f in enumerate(clutter.FRAMES):
        exp, win = oracle.recognition_topk(scene["bgrs"][i], scene["depths"][i], scene["K"], clutter.T, scene["bank"], TOPK, *p,
                                           nms_dist=NMS_DIST)
        assert len(got[i]) == len(exp), f
        for r, (g, e) in enumerate(zip(got[i], exp)):
            tag = (f, r)
            assert g["status"] == 0 and g["found"] == e["found"], tag
            assert (g["best"]["x"], g["best"]["y"], g["best"]["template_id"]) == (e["best"]["x"], e["best"]["y"], e["best"]["template_id"]), tag
            if e["found"]:
                assert g["det"]["n_points"] == e["det"]["n_points"], tag
                assert _bits(g["det"]["icp"]["dist_mean"]) == _bits(e["det"]["icp"]["dist_mean"]), tag
                assert np.array_equal(_bits(g["pose"]), _bits(e["pose"])), tag
        one = det.recognize_topk(scene["bgrs"][i], scene["depths"][i], scene["K"], TOPK, *p)     # det.nms works on this call
        assert len(one) == len(got[i]) and all(np.array_equal(_bits(a["pose"]), _bits(b["pose"])) for a, b in zip(one, got[i])), f
        assert det.nms(len(one), NMS_DIST) == win, f
        n_win.append(len(win))
    assert n_win[0] == 3 and n_win[1] >= 2 and n_win[2] >= 2 and n_win[3] == 0, n_win
    det.close()


# Every option value the runs below force, one at a time (with icp_wide 0 where the option only acts on the 256-thread ICP
# kernel, which a batch of four frames would not otherwise get).
OPTION_RUNS = [
    {"scan_prune": 0},
    {"scan_prune_mid": 0}, {"scan_prune_mid": 0x01}, {"scan_prune_mid": 0x55}, {"scan_prune_mid": 0xFF},
    {"icp_wide": 0}, {"icp_wide": 1},
    {"icp_wide": 0, "icp_occ": 4}, {"icp_wide": 0, "icp_occ": 5},
    {"icp_wide": 0, "icp_wg_per_cu": 1}, {"icp_wide": 0, "icp_wg_per_cu": 2}, {"icp_wide": 0, "icp_wg_per_cu": 3},
]


def test_clutter_results_do_not_depend_on_runtime_options(oracle, scene, expected):
    """One default run, then every option value of OPTION_RUNS set AFTER that first launch (so that a kernel attribute set
    once per process has to serve every later launch), the options sampled at finalize on detectors of their own, and a batch
    of 1100 frames (more than four per CU: the ICP jobs are dealt longest first, or in frame order with icp_order 0): every
    frame equals the default run, which equals the oracle."""
    import torch
    c = api.Context(0)                      # a context of its own: an option left set cannot leak into other tests
    p = PARAMS[1]
    try:
        det = _detector(c, scene, max_batch=1100, max_candidates=4096)
        base = det.recognize_batch(scene["bgrs"], scene["depths"], scene["K"], *p)
        for i, f in enumerate(clutter.FRAMES):
            _assert_reco_equal(base[i], expected["reco"][p][i], ("default", f))
        for opts in OPTION_RUNS:
            with _options(c, opts):
                got = det.recognize_batch(scene["bgrs"], scene["depths"], scene["K"], *p)
                lists = det.match_batch(scene["bgrs"], scene["depths"], 75.0)
            for i, f in enumerate(clutter.FRAMES):
                _assert_reco_equal(got[i], base[i], (opts, f))
                _assert_matches_equal(lists[i][0], expected["matches"][i][0], (opts, f))
        # options read by fl_detector_finalize: a new detector each
        for opts, keep in (({"eager_frontend": 1, "scan_prune": 0}, True), ({"ws_pad": 4096}, False)):
            with _options(c, opts):
                d2 = _detector(c, scene)
                if keep:
                    got = d2.recognize_batch(scene["bgrs"], scene["depths"], scene["K"], *p)
            if not keep:
                got = d2.recognize_batch(scene["bgrs"], scene["depths"], scene["K"], *p)
            d2.close()
            for i, f in enumerate(clutter.FRAMES):
                _assert_reco_equal(got[i], base[i], (opts, f))
        # 1100 frames by device pointer, each one of a - d
        n = 1100
        d_b = torch.from_numpy(np.stack(scene["bgrs"])).cuda()
        d_d = torch.from_numpy(np.stack(scene["depths"]).view(np.int16)).cuda()
        torch.cuda.synchronize()
        order = [(3 * i + i // 7) % len(clutter.FRAMES) for i in range(n)]
        bp = [d_b.data_ptr() + o * clutter.W * clutter.H * 3 for o in order]
        dp = [d_d.data_ptr() + o * clutter.W * clutter.H * 2 for o in order]
        params = L.RecognitionParams(*p, L.FL_ICP_PARITY)
        for icp_order in (1, 0):
            with _options(c, {"icp_order": icp_order}):
                det.recognize_submit_device(bp, dp, scene["K"], params)
                res = [api.recognition_result_to_dict(r) for r in det.recognize_collect(n)]
            for i in range(n):
                _assert_reco_equal(res[i], base[order[i]], ("batch", icp_order, i))
        det.close()
    finally:
        c.close()
