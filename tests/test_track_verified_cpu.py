"""CPU: verified tracking (fl_track_batch_verified, include/fealess_hip.h) without a GPU -- the decision and the pick of
tests/track_verified_model.py on hand-made records; what the numpy models say about a followed object, a frame without it and an
object that stands still, which is where the thresholds of tests/test_gpu_track_verified.py come from; and the argument checks of
the library itself, which come before its first HIP call and so run on a tracker without a device.
"""
import ctypes as C

import numpy as np
import pytest

import test_verify_cpu as TV
import track_model as TM
import track_verified_model as TVM
import verify_model as VM
from fealess_amd import _lib as L
from fealess_amd import synth

W, H = 640, 480
K0 = TM.MODEL_K
MAX_CROP = 40000
MOTION_T, MOTION_A = (4.0, -2.0, 3.0), (0.02, -0.01, 0.015)     # tests/test_gpu_track.py's motion per frame
# the gates of tests/test_gpu_track_verified.py, and the sides they must separate
MIN_INLIER, MAX_BEHIND = 0.7, 0.1


def _rec(accepted, n_inlier, n_model):
    r = np.zeros((), VM.DTYPE)
    r["accepted"], r["n_inlier"], r["n_model"] = accepted, n_inlier, n_model
    return r


ZERO = _rec(0, 0, 0)


# ---- (a) the decision and the pick on hand-made records -----------------------------------------------------------------------
def test_decision_rule():
    good, better, bad = _rec(1, 90, 100), _rec(1, 91, 100), _rec(0, 99, 100)
    assert TVM.decide(1, good, ZERO, 0) == (1, 0)                                  # only A
    assert TVM.decide(1, good, bad, 1) == (1, 0)                                   # only A, the input verified and refused
    assert TVM.decide(1, bad, good, 1) == (1, 1)                                   # only B
    assert TVM.decide(1, good, better, 1) == (1, 1)                                # both, B strictly better
    assert TVM.decide(1, better, good, 1) == (1, 0)
    assert TVM.decide(1, _rec(1, 2, 4), _rec(1, 3, 6), 1) == (1, 0)                # an exact tie keeps the ICP pose
    assert TVM.decide(1, _rec(1, 3, 6), _rec(1, 2, 4), 1) == (1, 0)
    # equal as float32, the input larger exactly -- and the other way round
    lo, hi = _rec(1, 33554431, 33554432), _rec(1, 33554432, 33554432)
    assert np.float32(33554431) / np.float32(33554432) == np.float32(1)
    assert TVM.decide(1, lo, hi, 1) == (1, 1) and TVM.decide(1, hi, lo, 1) == (1, 0)
    assert TVM.decide(1, bad, bad, 1) == (0, 0) and TVM.decide(1, bad, ZERO, 0) == (0, 0)    # neither
    assert TVM.decide(1, bad, good, 0) == (0, 0)                                   # keep_input off: the input does not count
    assert TVM.decide(0, ZERO, good, 1) == (0, 0)                                  # lost in the passes stays lost
    assert TVM.decide(0, good, good, 1) == (0, 0)


def test_pick_rule():
    # (tracked, kept_input, verify, verify_in)
    rows = [(1, 0, _rec(1, 2, 4), ZERO), (1, 1, _rec(1, 1, 9), _rec(1, 3, 6)), (1, 0, _rec(1, 1, 3), ZERO),     # group 0: 2/4 == 3/6, the lower index
            (0, 0, _rec(0, 9, 10), ZERO), (0, 0, ZERO, ZERO),                                                   # group 1: nobody tracked
            (1, 0, _rec(1, 0, 7), ZERO),                                                                        # group 2: one member
            (0, 0, _rec(0, 99, 100), ZERO), (1, 0, _rec(1, 1, 100), ZERO), (1, 1, _rec(0, 50, 100), _rec(1, 2, 100)),   # group 3: the later, by verify_in
            (1, 0, _rec(1, 33554431, 33554432), ZERO), (1, 0, _rec(1, 33554432, 33554432), ZERO)]               # group 5 (4 is empty)
    cols = [[r[k] for r in rows] for k in range(4)]
    assert TVM.pick(*cols, group_first=[0, 3, 5, 6, 9, 9, 11]) == [1, 0, 0, 0, 0, 1, 0, 0, 1, 0, 1]
    assert TVM.pick(*cols, group_first=None) == cols[0]
    assert TVM.pick(*cols, group_first=list(range(len(rows) + 1))) == cols[0]
    assert TVM.pick(*cols, group_first=[0, len(rows)]) == [0] * 10 + [1]
    # the kept input counts with ITS record: as verify alone (1/9) the second member would lose to the third (1/3)
    cols[1][1] = 0
    assert TVM.pick(*cols, group_first=[0, 3, 5, 6, 9, 9, 11])[:3] == [1, 0, 0]
    cols[0][0] = 0
    assert TVM.pick(*cols, group_first=[0, 3, 5, 6, 9, 9, 11])[:3] == [0, 0, 1]


# ---- (b) the figures the GPU test's thresholds rest on ------------------------------------------------------------------------
def _gt(k):
    return synth.object_pose(10 + MOTION_T[0] * k, -5 + MOTION_T[1] * k, 720.0 + MOTION_T[2] * k, 0.3 + MOTION_A[0] * k, 0.35 + MOTION_A[1] * k,
                             0.1 + MOTION_A[2] * k)


@pytest.fixture(scope="module")
def figures():
    """track_verified_model on the sequence of tests/test_gpu_track.py (point-to-plane, one pass, default thresholds, tau_mm = 10,
    no gates, keep_input = 1): frames 1 - 3 chained from frame 0's true pose, frame 0 itself from its true pose, and frames that hold
    only a plane 700 / 740 / 780 / 820 mm away.  Computed once, read only."""
    mesh = synth.object_mesh(2)
    pose0 = synth.pose13(*_gt(0))
    moving, pose = [], pose0
    for k in (1, 2, 3):
        r = TVM.track_verified(mesh, [synth.render(W, H, *_gt(k), seed=100 + k)[0]], [0], pose[None], K0, keep_input=1, max_crop_px=MAX_CROP)[0]
        assert r["icp_tracked"] == 1
        moving.append(r)
        pose = TM.pose13_of(TM.pose4x4(pose) if r["kept_input"] else r["track"]["pose"])
    static = TVM.track_verified(mesh, [synth.render(W, H, *_gt(0), seed=100)[0]], [0], pose0[None], K0, keep_input=1, max_crop_px=MAX_CROP)[0]
    empty = []
    for z in (700.0, 740.0, 780.0, 820.0):
        scene = synth.render(W, H, _gt(0)[0], np.array([0.0, 0.0, -500.0]), seed=7, plane_z=z)[0]
        empty.append(TVM.track_verified(mesh, [scene], [0], pose0[None], K0, keep_input=1, max_crop_px=MAX_CROP)[0])
    return dict(moving=moving, static=static, empty=empty)


def _beats(a, b):
    return int(a["n_inlier"]) * int(b["n_model"]) > int(b["n_inlier"]) * int(a["n_model"])


def test_model_separates_a_followed_object_from_a_frame_without_it(figures):
    for name in ("moving", "empty"):
        for r in figures[name]:
            print(name, "in", r["verify_in"]["inlier_ratio"], r["verify_in"]["behind_ratio"], "out", r["verify"]["inlier_ratio"], r["verify"]["behind_ratio"],
                  "dist_mean", r["track"]["det"]["icp"]["dist_mean"])
    for r in figures["moving"]:
        assert r["icp_tracked"] == 1 and VM.invariant(r["verify"]) and VM.invariant(r["verify_in"])
        assert r["verify"]["inlier_ratio"] >= 0.95 > MIN_INLIER and r["verify"]["behind_ratio"] <= 0.02 < MAX_BEHIND
        assert _beats(r["verify"], r["verify_in"]) and r["kept_input"] == 0 and r["track"]["tracked"] == 1     # the step improved the pose
    for r in figures["empty"]:
        assert r["icp_tracked"] == 1 and r["track"]["tracked"] == 1                   # the ICP returns some pose and no gate is on
        assert MIN_INLIER > 0.55 >= r["verify"]["inlier_ratio"] and MAX_BEHIND < 0.4 <= r["verify"]["behind_ratio"]
        assert r["track"]["det"]["icp"]["dist_mean"] > 10.0


def test_model_keeps_the_input_pose_of_an_object_that_stands_still(figures):
    r = figures["static"]
    print("static in", r["verify_in"], "out", r["verify"])
    assert r["icp_tracked"] == 1 and r["verify"]["accepted"] == 1 and r["verify_in"]["accepted"] == 1
    assert _beats(r["verify_in"], r["verify"])
    assert r["kept_input"] == 1 and r["track"]["tracked"] == 1
    assert np.array_equal(r["track"]["pose"], TM.pose4x4(synth.pose13(*_gt(0))))
    assert r["verify_in"]["n_behind"] == 0 and r["verify_in"]["inlier_ratio"] > 0.999


def test_model_gates_lose_the_frame_without_the_object():
    mesh = synth.object_mesh(2)
    pose0 = synth.pose13(*_gt(0))
    scene = synth.render(W, H, _gt(0)[0], np.array([0.0, 0.0, -500.0]), seed=7, plane_z=740.0)[0]
    for gate in (dict(min_inlier_ratio=MIN_INLIER), dict(max_behind_ratio=MAX_BEHIND)):
        r = TVM.track_verified(mesh, [scene], [0], pose0[None], K0, max_crop_px=MAX_CROP, **gate)[0]
        assert r["icp_tracked"] == 1 and r["track"]["tracked"] == 0 and r["kept_input"] == 0 and r["best"] == 0
        assert r["verify"]["n_model"] > 5000 and r["verify"]["accepted"] == 0 and not r["verify_in"]["n_model"]
        assert np.array_equal(r["track"]["pose"], TM.pose4x4(pose0))


# ---- (c) the library's argument checks, on a tracker without a device ---------------------------------------------------------
TW, TH, MAX_TRACKS = TV.TW, TV.TH, TV.MAX_TRACKS
host_tracker = TV.host_tracker
NAN, INF = float("nan"), float("inf")
TRACK_OK = (12, 1, 10, 0.5, 0.01, L.FL_ICP_POINT_TO_PLANE, 0.0, 0.0)


def _track_params(**over):
    names = [f[0] for f in L.TrackParams._fields_]
    p = dict(zip(names, TRACK_OK))
    p.update(over)
    return dict(track_params=tuple(p[k] for k in names))


def _call(lib, tracker, **over):
    """fl_track_batch_verified with the valid argument list of tests/test_verify_cpu.py (two frames, three tracks, two groups; its
    `params` are the fl_verify_params) plus track_params and keep_input, except for what `over` replaces.  Returns (rc, results
    untouched?)."""
    a = dict(n_frames=2, depth=[np.full((TH, TW), 700, np.uint16)] * 2, mem=L.FL_MEM_HOST, n_poses=3, frame_of=[0, 1, 1],
             poses=np.stack([TV._p13((0, 0, 700, 0.3, 0.35, 0.1))] * 3), n_groups=2, group_first=[0, 1, 3], K=(TW, TH, 60.0, 61.0, 32.0, 24.0),
             params=(10, 1, 0.0, 0.0), results=True, trk=tracker, track_params=TRACK_OK, keep_input=0, vparams=True)
    a.update(over)
    dp = None
    if a["depth"] is not None:
        dp = (C.c_void_p * max(1, len(a["depth"])))(*[None if d is None else d.ctypes.data for d in a["depth"]])
    fof = None if a["frame_of"] is None else np.ascontiguousarray(a["frame_of"], np.int32)
    poses = None if a["poses"] is None else np.ascontiguousarray(a["poses"], np.float32)
    gf = None if a["group_first"] is None else np.ascontiguousarray(a["group_first"], np.int32)
    k = None if a["K"] is None else L.Intrinsics(*a["K"])
    tp = None if a["track_params"] is None else L.TrackParams(*a["track_params"])
    vp = None if a["params"] is None or not a["vparams"] else L.TrackVerifyParams(L.VerifyParams(*a["params"]), a["keep_input"], 0)
    out = np.full(MAX_TRACKS * C.sizeof(L.VerifiedTrackResult), 0xA5, np.uint8)
    rc = lib.fl_track_batch_verified(a["trk"], a["n_frames"], dp, a["mem"], a["n_poses"], None if fof is None else fof.ctypes.data,
                                     None if poses is None else poses.ctypes.data, a["n_groups"], None if gf is None else gf.ctypes.data,
                                     None if k is None else C.byref(k), None if tp is None else C.byref(tp), None if vp is None else C.byref(vp),
                                     out.ctypes.data if a["results"] else None)
    return rc, bool((out == 0xA5).all())


# everything fl_verify_batch refuses (the common checks, K as floats -- fx = 1e-60 among them --, every broken group_first,
# fl_verify_params' ranges), then fl_track_params' ranges and keep_input
INVALID = dict(TV.INVALID, **{
    "passes 0": _track_params(passes=0), "passes 5": _track_params(passes=L.FL_TRACK_MAX_PASSES + 1), "margin_px -1": _track_params(margin_px=-1),
    "margin_px 8193": _track_params(margin_px=8193), "icp_it_thr -1": _track_params(icp_it_thr=-1),
    "dist_mean_thr nan": _track_params(dist_mean_thr=NAN), "dist_diff_thr inf": _track_params(dist_diff_thr=INF),
    "max_dist_mean nan": _track_params(max_dist_mean=NAN), "min_px_ratio -inf": _track_params(min_px_ratio=-INF),
    "icp_mode 3": _track_params(icp_mode=3), "icp_mode -1": _track_params(icp_mode=-1),
    "keep_input 2": dict(keep_input=2), "keep_input -1": dict(keep_input=-1),
})


def test_the_shared_refusals_are_all_there():
    assert "fx 0 as a float" in INVALID and INVALID["fx 0 as a float"]["K"][2] == 1e-60
    assert {"tau 65536", "min_model_px 0", "group_first decreasing", "n_groups above max_tracks", "pose nan", "mem 2"} <= set(INVALID)


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_are_refused_before_any_device_work(host_tracker, case):
    lib, trk = host_tracker
    rc, untouched = _call(lib, trk, **INVALID[case])
    assert rc == L.FL_ERR_INVALID and untouched, case


def test_valid_arguments_reach_the_device_check(host_tracker):
    lib, trk = host_tracker
    valid = TV.COMMON_VALID + [dict(params=(0, 1, 0.0, 0.0)), dict(params=(65535, 1 << 30, 0.5, 0.25)), dict(params=(10, 1, -1.0, -2.0)),
                               dict(group_first=None, n_groups=-5), dict(group_first=[0, 0, 3, 3, 3], n_groups=MAX_TRACKS), dict(group_first=[0, 3], n_groups=1),
                               dict(vparams=False), dict(track_params=None), dict(vparams=False, track_params=None), dict(keep_input=1),
                               _track_params(passes=L.FL_TRACK_MAX_PASSES, margin_px=8192, icp_it_thr=0, icp_mode=L.FL_ICP_PARITY, max_dist_mean=10.0,
                                             min_px_ratio=-1.0)]
    for over in valid:
        rc, untouched = _call(lib, trk, **over)
        assert rc == L.FL_ERR_NO_DEVICE and untouched, over
    assert lib.fl_track_batch_verified(None, 1, None, 0, 1, None, None, 0, None, None, None, None, None) == L.FL_ERR_INVALID


def test_result_record_layout():
    from fealess_amd import api
    assert C.sizeof(L.VerifiedTrackResult) == TVM.DTYPE.itemsize == 368 and C.sizeof(L.TrackVerifyParams) == 24
    assert TVM.TRACK_DTYPE.itemsize == C.sizeof(L.TrackResult)
    assert api.VERIFIED_TRACK_DTYPE == TVM.DTYPE
    for name, _ in L.VerifiedTrackResult._fields_:
        assert getattr(L.VerifiedTrackResult, name).offset == TVM.DTYPE.fields[name][1], name
    for name, _ in L.TrackResult._fields_:
        assert getattr(L.TrackResult, name).offset == TVM.TRACK_DTYPE.fields[name][1], name
