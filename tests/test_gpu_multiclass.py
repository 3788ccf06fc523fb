"""Recognition with several classes on one detector (tests/multiclass.py: three classes added in an order that is not the
sorted one, class_first = {0, 8, 116}): every entry point that goes from a match to a pose, against the oracle's match list
over the three classes and its refinement of the match the entry point has to have chosen (oracle_py.refine_match), bit for
bit.  A wrong class offset anywhere behind the match list -- pyr[g], poses + 13 g, depth_ptrs[g], a class's end, a class index
that moved when a later class sorted in front of it -- refines another instance's view and fails here.

Class indices refined, per entry point (asserted below): fl_recognize_batch and _submit/_collect 2, 0, 2 on frames a - c and 1
(then 0) under the class filter; fl_recognize_batch_topk / _topk 0, 1, 2 on frame a; fl_refine_matches 0, 1, 2;
fl_recognize_batch_instances 0, 1, 2 on frame a; the facade 1 of {alpha, zeta}."""
import ctypes as C

import numpy as np
import pytest
import torch

import cadreco_py
import clutter
import instances_model as M
import multiclass
from fealess_amd import api
from fealess_amd import _lib as L
from fealess_amd.bank import MATCH_DTYPE
from test_abi_cpu import write_bank_dir
from test_gpu_icp import width  # noqa: F401    the fixture that forces each build of the ICP kernels in turn

pytestmark = pytest.mark.gpu

P = (75.0, 10, 0.5, 0.01)                      # Recognition()'s defaults
TOPK, NMS_DIST, MIN_DIST = 16, 60.0, 48
NF = len(clutter.FRAMES)
W, H = clutter.W, clutter.H


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def mc(oracle):
    sc = multiclass.build(oracle)
    sc["refined"] = [dict() for _ in range(NF)]
    return sc


def _refined(oracle, mc, fi, j):
    """The oracle's refinement of entry j of frame fi's match list over the three classes; computed once."""
    cache = mc["refined"][fi]
    if j not in cache:
        m = mc["lists"][fi][j]
        cache[j] = oracle.refine_match(mc["depths"][fi], mc["K"], mc["banks"][int(m["class_idx"])], m, *P[1:], n_matches=len(mc["lists"][fi]))
        assert cache[j]["found"] == 1 and not cache[j]["no_render"], (fi, j)       # every listed match has a render and a crop inside the frame
    return cache[j]


class _Refined:
    """refined[j] as instances_model.pick reads it."""

    def __init__(self, oracle, mc, fi):
        self.args = (oracle, mc, fi)

    def __getitem__(self, j):
        return _refined(*self.args, j)


def _detector(ctx, banks, max_batch=8):
    det = api.Detector(ctx, 2, clutter.T)
    for b in banks:
        det.add_class(b)
    det.finalize(W, H, max_batch=max_batch)
    return det


@pytest.fixture(scope="module")
def det(ctx, mc):
    d = _detector(ctx, mc["added"])
    assert [b.class_id for b in d.banks] == list(multiclass.SORTED_IDS) and d.num_templates() == 124
    yield d
    d.close()


def _assert_refined(g, e, tag, n_matches=None):
    """A result of the library against the oracle's refinement e of the same match, bit for bit."""
    assert g["status"] == 0 and g["found"] == e["found"] == 1, tag
    assert g["n_matches"] == (e["n_matches"] if n_matches is None else n_matches), tag
    gb, eb = g["best"], e["best"]
    assert (gb["x"], gb["y"], gb["class_idx"], gb["template_id"]) == (eb["x"], eb["y"], eb["class_idx"], eb["template_id"]), tag
    assert _bits(gb["similarity"]) == _bits(eb["similarity"]), tag
    assert g["det"]["n_points"] == e["det"]["n_points"] and g["det"]["icp"]["iters"] == e["det"]["icp"]["iters"], tag
    assert g["det"]["icp"]["n_corr_last"] == e["det"]["icp"]["n_corr_last"], tag
    for k in ("R", "T", "dist_mean", "px_ratio"):
        assert np.array_equal(_bits(g["det"]["icp"][k]), _bits(e["det"]["icp"][k])), (tag, k)
    for k in ("R_final", "T_final"):
        assert np.array_equal(_bits(g["det"][k]), _bits(e["det"][k])), (tag, k)
    assert np.array_equal(_bits(g["pose"]), _bits(e["pose"])), tag


def _assert_same(g, e, tag):
    """Two results of the library: every field, bit for bit."""
    for k, v in e.items():
        if isinstance(v, dict):
            _assert_same(g[k], v, (tag, k))
        elif isinstance(v, (np.ndarray, np.floating)):
            assert np.asarray(g[k]).tobytes() == np.asarray(v).tobytes(), (tag, k)
        else:
            assert g[k] == v, (tag, k)


def _assert_best_of_list(oracle, mc, got, tag):
    """fl_recognize_batch's results of frames a - d against matches[0] of the oracle's list, refined."""
    for fi, f in enumerate(clutter.FRAMES):
        n = len(mc["lists"][fi])
        if n == 0:
            assert (got[fi]["status"], got[fi]["found"], got[fi]["n_matches"]) == (0, 0, 0), (tag, f)
        else:
            _assert_refined(got[fi], _refined(oracle, mc, fi, 0), (tag, f))
    assert [g["best"]["class_idx"] for g in got[:3]] == [2, 0, 2] and [g["found"] for g in got] == [1, 1, 1, 0], tag


def _submit_collect(det, mc):
    bs = [np.ascontiguousarray(b, np.uint8) for b in mc["bgrs"]]
    ds = [np.ascontiguousarray(d, np.uint16) for d in mc["depths"]]
    det.recognize_submit_host([b.ctypes.data for b in bs], [d.ctypes.data for d in ds], mc["K"], L.RecognitionParams(*P, L.FL_ICP_PARITY))
    return [api.recognition_result_to_dict(r) for r in det.recognize_collect(NF)]


def test_recognize_batch_and_submit_collect(oracle, mc, det, width):
    """Frames a - d in one batch: the best match lies in class index 2, 0, 2, none."""
    got = det.recognize_batch(mc["bgrs"], mc["depths"], mc["K"], *P)
    _assert_best_of_list(oracle, mc, got, ("batch", width))
    _assert_best_of_list(oracle, mc, _submit_collect(det, mc), ("submit", width))


def test_batch_topk_and_nms(oracle, mc, det, width):
    """The first 16 matches of every frame (all three classes on frame a: class index 1 at rank 1, class index 0 from rank 11
    on), and fl_nms's winners against orc_nms on the oracle's records."""
    got = det.recognize_batch_topk(mc["bgrs"], mc["depths"], mc["K"], TOPK, *P)
    seen = []
    for fi, f in enumerate(clutter.FRAMES):
        n = min(TOPK, len(mc["lists"][fi]))
        assert len(got[fi]) == n, f
        exp = [_refined(oracle, mc, fi, r) for r in range(n)]
        for r in range(n):
            _assert_refined(got[fi][r], exp[r], (width, f, r))
        seen.append({g["best"]["class_idx"] for g in got[fi]})
        one = det.recognize_topk(mc["bgrs"][fi], mc["depths"][fi], mc["K"], TOPK, *P)          # det.nms works on this call
        assert len(one) == n, f
        for r in range(n):
            _assert_same(one[r], got[fi][r], (width, f, r, "single"))
        win = oracle.nms([e["det"]["T_final"] for e in exp], [e["det"]["n_points"] for e in exp], [e["det"]["icp"]["dist_mean"] for e in exp],
                         NMS_DIST)
        assert det.nms(n, NMS_DIST) == win, (f, win)
        if f == "a":
            assert len({exp[w]["best"]["class_idx"] for w in win}) == 3, win            # one winner per instance = per class
    assert seen == [{0, 1, 2}, {0, 1}, {0, 1, 2}, set()]


def test_class_filter_between_calls_on_one_detector(oracle, mc, det, width):
    """("mid",), then ("alpha", "nope"), then (): each run equals the oracle's Recognition() over the classes the filter
    leaves, with class_idx still counting in the full list; afterwards the detector gives the unfiltered results again."""
    base = det.recognize_batch(mc["bgrs"], mc["depths"], mc["K"], *P)
    try:
        for ids, idx in ((("mid",), 1), (("alpha", "nope"), 0), ((), None)):
            det.set_class_filter(ids)
            got = det.recognize_batch(mc["bgrs"], mc["depths"], mc["K"], *P)
            queued = _submit_collect(det, mc)
            for fi, f in enumerate(clutter.FRAMES):
                tag = (width, ids, f)
                _assert_same(queued[fi], got[fi], (tag, "submit"))
                if not ids:
                    _assert_same(got[fi], base[fi], tag)
                    continue
                exp = oracle.recognition_banks(mc["bgrs"][fi], mc["depths"][fi], mc["K"], clutter.T, mc["added"], 1, *P, class_ids=ids)
                if not exp:
                    assert f == "d" and (got[fi]["status"], got[fi]["found"], got[fi]["n_matches"]) == (0, 0, 0), tag
                else:
                    assert exp[0]["best"]["class_idx"] == idx and exp[0]["found"] == 1, tag
                    _assert_refined(got[fi], exp[0], tag)
        _assert_best_of_list(oracle, mc, got, "after the filter")
    finally:
        det.set_class_filter(())


def _results(res, n):
    return [api.recognition_result_to_dict(res[i]) for i in range(n)]


def test_refine_matches_names_every_class(oracle, mc, det, width):
    """Jobs from frame a's list (and frame b's head) that name all three classes, in an order that is not the list's, around a
    pyramid of class mid that has no render: that job reports FL_ERR_STATE and leaves its neighbours' bits alone.  A class
    index outside the detector is refused before any launch."""
    la, lb = mc["lists"][0], mc["lists"][1]
    first = {c: int(np.nonzero(la["class_idx"] == c)[0][0]) for c in (0, 1, 2)}
    zeta2 = int(np.nonzero(la["class_idx"] == 2)[0][1])
    picks = [(0, first[0]), (0, first[2]), None, (0, first[1]), (1, 0), (0, zeta2)]           # (frame, list index); None: the ghost
    assert [p[1] for p in picks if p and p[0] == 0] != sorted(p[1] for p in picks if p and p[0] == 0)
    jobs = np.zeros(len(picks), MATCH_DTYPE)
    for j, p in enumerate(picks):
        if p:
            jobs[j] = mc["lists"][p[0]][p[1]]
    ghost = picks.index(None)
    jobs[ghost] = la[first[1]]
    jobs["template_id"][ghost] = 8 + 5                                   # mid's pyramids from 8 on are random ones without renders
    assert jobs["class_idx"][ghost] == 1 and jobs["template_id"][ghost] >= len(mc["by_id"]["mid"].model_depths)
    frames = [p[0] if p else 0 for p in picks]
    params = L.RecognitionParams(*P, L.FL_ICP_PARITY)
    det.match_batch(mc["bgrs"], mc["depths"], P[0])
    got = _results(det.refine_matches(frames, jobs, mc["K"], params), len(picks))
    for j, p in enumerate(picks):
        if p:
            _assert_refined(got[j], _refined(oracle, mc, *p), (width, j), n_matches=1)
    assert {got[j]["best"]["class_idx"] for j, p in enumerate(picks) if p} == {0, 1, 2}
    g = got[ghost]
    assert g["status"] == L.FL_ERR_STATE and g["found"] == 0 and (g["best"]["class_idx"], g["best"]["template_id"]) == (1, 13)
    keep = [j for j, p in enumerate(picks) if p]
    alone = _results(det.refine_matches([frames[j] for j in keep], jobs[keep], mc["K"], params), len(keep))
    for a, j in zip(alone, keep):
        _assert_same(a, got[j], (width, j, "without the ghost"))
    for bad_class in (3, -1):
        bad = jobs.copy()
        bad["class_idx"][1] = bad_class
        with pytest.raises(api.FealessError) as ex:
            det.refine_matches(frames, bad, mc["K"], params)
        assert ex.value.code == L.FL_ERR_INVALID, bad_class
    again = _results(det.refine_matches(frames, jobs, mc["K"], params), len(picks))             # a refused call changes nothing
    for j in range(len(picks)):
        _assert_same(again[j], got[j], (width, j, "again"))


@pytest.mark.parametrize("hyp", [4, 1])
def test_instances_never_mix_classes(oracle, mc, det, width, hyp):
    """{8, 48, hyp}: the groups are those of tests/instances_model.py on the oracle's list over the three classes, no group
    holds two classes, and every pick is the oracle's refinement of that list entry."""
    got, dropped = det.recognize_batch_instances(mc["bgrs"], mc["depths"], mc["K"], 8, MIN_DIST, hyp, *P, with_dropped=True)
    wh = M.widths_heights(mc["banks"])
    for fi, f in enumerate(clutter.FRAMES):
        m = mc["lists"][fi]
        gof, size, n_groups = M.group(m, wh, 8, MIN_DIST)
        for g in range(n_groups):
            assert len(set(m["class_idx"][gof == g].tolist())) == 1, (f, g)
        exp, exp_dropped = M.instances(m, wh, _Refined(oracle, mc, fi), 8, MIN_DIST, hyp)
        tag = (width, hyp, f)
        assert [(g["rank"], g["n_members"], g["n_refined"]) for g in got[fi]] == [(e["rank"], e["n_members"], e["n_refined"]) for e in exp], tag
        assert dropped[fi] == exp_dropped, tag
        for g in got[fi]:
            _assert_refined(g, _refined(oracle, mc, fi, g["rank"]), (tag, g["rank"]))
    # frame a: the first three groups are the three instances, one class each
    assert len(got[0]) >= 3 and {g["best"]["class_idx"] for g in got[0][:3]} == {0, 1, 2}
    assert got[3] == []


def _assert_batches_same(a, b, tag):
    assert len(a) == len(b), tag
    for i, (x, y) in enumerate(zip(a, b)):
        _assert_same(x, y, (tag, i))


def test_depth_renders_travel_with_their_class(ctx, mc, det):
    """fl_detector_set_model_depths takes the class's index at the time of the call: zeta's renders go in with index 0 while
    zeta is alone, alpha's with index 0 once alpha has sorted in front of it, mid's with index 1.  Every class must keep its
    own renders: the results equal those of api.Detector, which uploads them after the last class was added."""
    raw = api.Detector(ctx, 2, clutter.T)
    lib = ctx.lib
    index_when_added = {"zeta": 0, "alpha": 0, "mid": 1}
    try:
        for b in mc["added"]:
            t, f, p = b.arrays()
            ctx.check(lib.fl_detector_add_class(raw.h, b.class_id.encode(), b.n_pyramids, t.ctypes.data_as(C.c_void_p),
                                                f.ctypes.data_as(C.c_void_p), len(f), p.ctypes.data_as(C.c_void_p)))
            d = np.ascontiguousarray(np.stack(b.model_depths), np.uint16)
            assert d.shape == (8, H, W)
            ctx.check(lib.fl_detector_set_model_depths(raw.h, index_when_added[b.class_id], 0, len(d), d.ctypes.data_as(C.c_void_p), W, H,
                                                       L.FL_MEM_HOST))
        assert lib.fl_detector_num_classes(raw.h) == 3
        ctx.check(lib.fl_detector_finalize(raw.h, W, H, NF, 0))
        raw.w0, raw.h0, raw.max_batch = W, H, NF
        _assert_batches_same(raw.recognize_batch(mc["bgrs"], mc["depths"], mc["K"], *P), det.recognize_batch(mc["bgrs"], mc["depths"], mc["K"], *P),
                             "best")
        a = raw.recognize_batch_topk(mc["bgrs"][:1], mc["depths"][:1], mc["K"], TOPK, *P)[0]
        b = det.recognize_batch_topk(mc["bgrs"][:1], mc["depths"][:1], mc["K"], TOPK, *P)[0]
        assert {r["best"]["class_idx"] for r in b} == {0, 1, 2} and all(r["found"] for r in b)
        _assert_batches_same(a, b, "topk")
    finally:
        raw.close()


def test_a_class_without_any_render(ctx, mc, det):
    """alpha without renders: frame b, whose best match is alpha's, reports FL_ERR_STATE and no pose; frames a and c, whose
    best is zeta's, keep every bit (so the ICP workspaces still cover zeta's crops: no FL_ERR_ASSERT); frame d stays empty."""
    bare = mc["by_id"]["alpha"].subset(0, 8)
    bare.class_id, bare.model_depths = "alpha", []
    d2 = _detector(ctx, [mc["by_id"]["zeta"], bare, mc["by_id"]["mid"]], max_batch=NF)
    try:
        got = d2.recognize_batch(mc["bgrs"], mc["depths"], mc["K"], *P)
        base = det.recognize_batch(mc["bgrs"], mc["depths"], mc["K"], *P)
        for fi in (0, 2, 3):
            _assert_same(got[fi], base[fi], clutter.FRAMES[fi])
        assert base[1]["found"] == 1 and base[1]["best"]["class_idx"] == 0
        assert (got[1]["status"], got[1]["found"], got[1]["n_matches"]) == (L.FL_ERR_STATE, 0, base[1]["n_matches"])
        assert got[1]["best"] == base[1]["best"] and not got[1]["pose"].any()
        # the renders arrive after fl_detector_finalize: of another size they are refused, frame-sized they serve from the next
        # call on, for the pyramids they were given for (alpha's first four: frame b's best, alpha 4, still has none)
        renders = np.ascontiguousarray(np.stack(mc["by_id"]["alpha"].model_depths), np.uint16)
        set_depths = ctx.lib.fl_detector_set_model_depths
        assert set_depths(d2.h, 0, 0, 8, renders.ctypes.data_as(C.c_void_p), W // 2, H * 2, L.FL_MEM_HOST) == L.FL_ERR_INVALID
        ctx.check(set_depths(d2.h, 0, 0, 4, renders.ctypes.data_as(C.c_void_p), W, H, L.FL_MEM_HOST))
        assert base[1]["best"]["template_id"] == 4
        assert d2.recognize_batch(mc["bgrs"], mc["depths"], mc["K"], *P)[1]["status"] == L.FL_ERR_STATE
        ctx.check(set_depths(d2.h, 0, 4, 4, renders[4:].ctypes.data_as(C.c_void_p), W, H, L.FL_MEM_HOST))
        _assert_batches_same(d2.recognize_batch(mc["bgrs"], mc["depths"], mc["K"], *P), base, "renders after finalize")
    finally:
        d2.close()


def test_template_sharding_refuses_several_classes(mc, det):
    """fl_select_best_batch refines on ONE class per detector: a detector with three refuses the call, whichever count of
    pyramids the caller names."""
    k = 4
    gathered = torch.zeros(NF * k * MATCH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    best = torch.zeros(NF * MATCH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for tid_count in (124, 8, 108):
        with pytest.raises(api.FealessError) as ex:
            det.select_best_batch(gathered.data_ptr(), 1, NF, k, 0, tid_count, best.data_ptr())
        assert ex.value.code == L.FL_ERR_INVALID, tid_count


def _facade_recognition(lib, directory, bgr, depth, K):
    """Create -> AddObj(directory) -> Recognition of one 640 x 480 frame: (number of results, tag, pose)."""
    with cadreco_py.handle() as h:
        assert lib.cadreco_add_obj(h, str(directory).encode()) == 0
        rc, n, tag, pose = cadreco_py.recognition(h, bgr, depth, K)
    assert rc == 0
    return n, tag, pose.reshape(4, 4)


def test_facade_translates_the_class_index(tmp_path, oracle, mc):
    """A directory whose YAML holds "zeta" (the eight views of instance 0) first and "alpha" (eight random pyramids) second:
    the facade sorts the ids, so zeta is class index 1 there.  Recognition of frame a must name "zeta", with the pose of the
    directory that holds zeta alone, bit for bit."""
    zeta = mc["by_id"]["zeta"]
    rand = mc["by_id"]["mid"].subset(8, 8)
    rand.class_id = "alpha"
    assert rand.model_depths == []
    dirs = {}
    for name, banks in (("two", [zeta, rand]), ("one", zeta)):
        d = tmp_path / name
        write_bank_dir(d, banks, clutter.T, zeta.model_depths)          # all classes of a directory share depth/<p>.png
        dirs[name] = d
    lib = cadreco_py.lib()
    bgr, depth = np.ascontiguousarray(mc["bgrs"][0]), np.ascontiguousarray(mc["depths"][0])
    n2, tag2, pose2 = _facade_recognition(lib, dirs["two"], bgr, depth, mc["K"])
    n1, tag1, pose1 = _facade_recognition(lib, dirs["one"], bgr, depth, mc["K"])
    assert (n1, tag1) == (1, b"zeta") and (n2, tag2) == (1, b"zeta")
    assert np.array_equal(_bits(pose2), _bits(pose1))
    exp = _refined(oracle, mc, 0, 0)                                     # frame a's best match: zeta 4
    assert exp["best"]["class_idx"] == 2 and np.array_equal(_bits(pose1), _bits(exp["pose"]))
