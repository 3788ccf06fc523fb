"""CPU: hypothesis verification (fl_verify_batch, include/fealess_hip.h) without a GPU -- what tests/verify_model.py, the numpy
statement of the contract, says about right and wrong poses; the pick rule; and the argument checks of the library itself,
which come before its first HIP call and so run on a tracker without a device (fl_dev_tracker_create_host).
"""
import ctypes as C

import numpy as np
import pytest

import verify_model as VM
from fealess_amd import _lib as L
from fealess_amd import synth
from util import p13 as _p13

W, H = 640, 480
K0 = (608.0, 608.0, 320.0, 240.0)
POSE = (10, -5, 720, 0.30, 0.35, 0.10)                           # POSES[0] of tests/test_gpu_track.py
MOTION = ((4.0, -2.0, 3.0), (0.02, -0.01, 0.015))                # that file's one-frame motion: mm, and rad of yaw / tilt / roll


@pytest.fixture(scope="module")
def mesh():
    return synth.object_mesh(2)


@pytest.fixture(scope="module")
def single(mesh):
    """One object, noise and background on, and the model's record (tau_mm = 10, no gates) of the true pose and of five wrong
    ones; computed once, read only."""
    scene = synth.render(W, H, *synth.object_pose(*POSE), seed=40)[0]
    poses = dict(true=_p13(POSE), motion=_p13(POSE, MOTION), yaw=_p13(POSE, ((0, 0, 0), (1.0, 0, 0))), shift=_p13(POSE, ((150, 0, 0), (0, 0, 0))),
                 nearer=_p13(POSE, ((0, 0, -20), (0, 0, 0))), farther=_p13(POSE, ((0, 0, 20), (0, 0, 0))))
    names = list(poses)
    rec = VM.verify(mesh, [scene], np.zeros(len(names), np.int32), np.stack([poses[k] for k in names]), K0)
    return dict(scene=scene, poses=poses, rec=dict(zip(names, rec)))


# ---- (a) the model on right and wrong poses -----------------------------------------------------------------------------------
def test_model_orders_the_true_pose_before_the_wrong_ones(single):
    """The numpy model, tau_mm = 10: n_inlier / n_model and n_behind / n_model are 12720 / 12726 and 0 at the true pose, 0.896 and
    0.038 one frame of motion away, 0.245 and 0.579 with the yaw off by 1 rad, 0.057 and 0.925 with the object 150 mm to the
    side; a render 20 mm nearer than the object is seen through everywhere, one 20 mm farther stands behind the scene
    everywhere.  The orderings and the invariant are asserted, not the digits."""
    r = single["rec"]
    for k, v in r.items():
        print(k, v)
        assert v["status"] == 0 and v["accepted"] == 1 and v["best"] == 1 and v["n_model"] > 5000 and VM.invariant(v), k
        assert v["inlier_ratio"] == np.float32(v["n_inlier"]) / np.float32(v["n_model"])
        assert v["rect"][2] > 0 and v["rect"][3] > 0 and v["rect"][2] * v["rect"][3] >= v["n_model"]
    assert r["true"]["inlier_ratio"] > r["motion"]["inlier_ratio"] > r["yaw"]["inlier_ratio"] > r["shift"]["inlier_ratio"] > 0
    assert r["true"]["behind_ratio"] <= r["motion"]["behind_ratio"] < r["yaw"]["behind_ratio"] < r["shift"]["behind_ratio"] < r["nearer"]["behind_ratio"]
    assert r["true"]["n_behind"] == 0 and 0 < r["true"]["sum_abs_inlier"] <= 10 * r["true"]["n_inlier"]
    assert r["nearer"]["n_inlier"] == 0 and r["nearer"]["n_front"] == 0 and r["nearer"]["n_behind"] == r["nearer"]["n_model"]
    assert r["farther"]["n_inlier"] == 0 and r["farther"]["n_behind"] == 0 and r["farther"]["n_front"] == r["farther"]["n_model"]
    assert all(v["n_missing"] == 0 for v in r.values())          # the background fills every pixel of this scene


def test_model_gates_separate_the_true_pose_from_a_wrong_one(mesh, single):
    """Each gate halfway between the two sides it must separate, both taken from the model's own ungated output."""
    r, scene = single["rec"], single["scene"]
    lo = (float(r["true"]["inlier_ratio"]) + float(r["yaw"]["inlier_ratio"])) / 2
    hi = (float(r["true"]["behind_ratio"]) + float(r["yaw"]["behind_ratio"])) / 2
    assert r["true"]["inlier_ratio"] > lo > r["yaw"]["inlier_ratio"] and r["true"]["behind_ratio"] < hi < r["yaw"]["behind_ratio"]
    poses = np.stack([single["poses"]["true"], single["poses"]["yaw"]])
    assert VM.verify(mesh, [scene], [0, 0], poses, K0, min_inlier_ratio=lo)["accepted"].tolist() == [1, 0]
    assert VM.verify(mesh, [scene], [0, 0], poses, K0, max_behind_ratio=hi)["accepted"].tolist() == [1, 0]
    n = int(r["true"]["n_model"])
    assert VM.verify(mesh, [scene], [0], poses[:1], K0, min_model_px=n)["accepted"][0] == 1
    assert VM.verify(mesh, [scene], [0], poses[:1], K0, min_model_px=n + 1)["accepted"][0] == 0


def test_model_missing_depth_and_the_band_edge(mesh, single):
    """Holes in the frame count as missing, not as anything else; tau_mm = 0 keeps only exact hits."""
    scene = single["scene"].copy()
    scene[:, ::2] = 0
    r = VM.verify(mesh, [scene], [0], single["poses"]["true"][None], K0)[0]
    full = single["rec"]["true"]
    assert VM.invariant(r) and r["n_model"] == full["n_model"] and 0 < r["n_missing"] < r["n_model"]
    assert r["n_missing"] + r["n_inlier"] + r["n_front"] == r["n_model"] and r["n_inlier"] < full["n_inlier"]
    exact = VM.verify(mesh, [single["scene"]], [0], single["poses"]["true"][None], K0, tau_mm=0)[0]
    assert VM.invariant(exact) and 0 < exact["n_inlier"] < full["n_inlier"] and exact["sum_abs_inlier"] == 0


def test_model_tells_an_occluder_from_seeing_through(mesh):
    """Three objects (render_clutter, seed 3), the first one partly behind the second: its hidden pixels count as n_front, none
    as n_behind, and the two unoccluded objects show next to no n_front."""
    objs = [(0, 0, 760, 0.3, 0.35, 0.1), (70, 10, 640, -0.5, 0.2, 0.3), (-200, -100, 720, 0.9, 0.5, -0.2)]
    scene, _, masks = synth.render_clutter(W, H, [synth.object_pose(*p) for p in objs], seed=3)
    r = VM.verify(mesh, [scene], [0, 0, 0], np.stack([_p13(p) for p in objs]), K0)
    print(r)
    assert VM.invariant(r) and (r["n_behind"] == 0).all() and (r["n_missing"] == 0).all()
    assert r["n_front"][0] > 0.2 * r["n_model"][0] and r["n_inlier"][0] > 0.2 * r["n_model"][0]
    assert (r["n_front"][1:] < 0.01 * r["n_model"][1:]).all()
    # the same first pose without the occluder in the scene is seen whole
    alone = synth.render_clutter(W, H, [synth.object_pose(*objs[0])], seed=3)[0]
    assert VM.verify(mesh, [alone], [0], _p13(objs[0])[None], K0)[0]["n_front"] < 0.01 * r["n_model"][0]


def test_model_empty_render():
    scene = np.full((48, 64), 700, np.uint16)
    r = VM.score(np.zeros((48, 64), np.uint16), scene)
    assert r.tobytes() == bytes(64)


# ---- (b) the pick -------------------------------------------------------------------------------------------------------------
def _records(rows):
    """(accepted, n_inlier, n_model) per pose."""
    r = np.zeros(len(rows), VM.DTYPE)
    for i, (a, ni, nm) in enumerate(rows):
        r[i]["accepted"], r[i]["n_inlier"], r[i]["n_model"] = a, ni, nm
    return r


def test_pick_rule():
    rows = [(1, 2, 4), (1, 3, 6), (1, 1, 3),            # group 0: 2/4 == 3/6 exactly, the lower index wins
            (0, 9, 10), (0, 5, 10),                     # group 1: nobody accepted
            (1, 0, 7),                                  # group 2: one member, accepted with no inlier at all
            (0, 99, 100), (1, 1, 100), (1, 2, 100),     # group 3: the best ratio is not accepted; of the others the later one is better
            (1, 33554431, 33554432), (1, 33554432, 33554432)]   # group 5 (4 is empty): equal as float32, the second larger exactly
    gf = [0, 3, 5, 6, 9, 9, 11]
    got = VM.pick(_records(rows), gf)
    assert got["best"].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 1, 0, 1]
    assert np.float32(33554431) / np.float32(33554432) == np.float32(33554432) / np.float32(33554432)
    assert 33554432 * 33554432 > 33554431 * 33554432
    # no groups: best = accepted
    assert VM.pick(_records(rows), None)["best"].tolist() == [r[0] for r in rows]
    # every pose its own group says the same
    assert VM.pick(_records(rows), list(range(len(rows) + 1)))["best"].tolist() == [r[0] for r in rows]
    # one group over everything: the exact maximum among the accepted
    assert VM.pick(_records(rows), [0, len(rows)])["best"].tolist() == [0] * 10 + [1]


# ---- (c) the library's argument checks, on a tracker without a device ---------------------------------------------------------
TW, TH, MAX_FRAMES, MAX_TRACKS = 64, 48, 2, 4


@pytest.fixture(scope="module")
def host_tracker():
    lib = L.load()
    h = C.c_void_p()
    assert L.dev(lib, "fl_dev_tracker_create_host")(TW, TH, MAX_FRAMES, MAX_TRACKS, 100, C.byref(h)) == 0 and h.value
    yield lib, h
    lib.fl_tracker_destroy(h)


def _call(lib, tracker, entry="verify", **over):
    """fl_verify_batch with valid arguments (two frames, three poses, two groups) except for what `over` replaces; entry =
    "track": fl_track_batch with the arguments the two have in common (its params: NULL).  Returns (rc, results untouched?)."""
    a = dict(n_frames=2, depth=[np.full((TH, TW), 700, np.uint16)] * 2, mem=L.FL_MEM_HOST, n_poses=3, frame_of=[0, 1, 1],
             poses=np.stack([_p13((0, 0, 700, 0.3, 0.35, 0.1))] * 3), n_groups=2, group_first=[0, 1, 3], K=(TW, TH, 60.0, 61.0, 32.0, 24.0),
             params=(10, 1, 0.0, 0.0), results=True, trk=tracker)
    a.update(over)
    dp = None
    if a["depth"] is not None:
        dp = (C.c_void_p * max(1, len(a["depth"])))(*[None if d is None else d.ctypes.data for d in a["depth"]])
    fof = None if a["frame_of"] is None else np.ascontiguousarray(a["frame_of"], np.int32)
    poses = None if a["poses"] is None else np.ascontiguousarray(a["poses"], np.float32)
    gf = None if a["group_first"] is None else np.ascontiguousarray(a["group_first"], np.int32)
    k = None if a["K"] is None else L.Intrinsics(*a["K"])
    prm = None if a["params"] is None else L.VerifyParams(*a["params"])
    out = np.full(MAX_TRACKS * C.sizeof(L.TrackResult if entry == "track" else L.VerifyResult), 0xA5, np.uint8)
    common = (a["trk"], a["n_frames"], dp, a["mem"], a["n_poses"], None if fof is None else fof.ctypes.data, None if poses is None else poses.ctypes.data)
    if entry == "track":
        rc = lib.fl_track_batch(*common, None if k is None else C.byref(k), None, out.ctypes.data if a["results"] else None)
    else:
        rc = lib.fl_verify_batch(*common, a["n_groups"], None if gf is None else gf.ctypes.data, None if k is None else C.byref(k),
                                 None if prm is None else C.byref(prm), out.ctypes.data if a["results"] else None)
    return rc, bool((out == 0xA5).all())


def _bad_pose(value, at):
    p = np.stack([_p13((0, 0, 700, 0.3, 0.35, 0.1))] * 3)
    p[2, at] = value
    return p


NAN, INF = float("nan"), float("inf")
# what fl_track_batch and fl_verify_batch check alike (fl_tracker_check_call): run against both below
COMMON_INVALID = {
    "tracker null": dict(trk=None), "fx negative": dict(K=(TW, TH, -60.0, 61.0, 32.0, 24.0)),
    "depth null": dict(depth=None), "frame_of null": dict(frame_of=None), "poses null": dict(poses=None), "K null": dict(K=None),
    "results null": dict(results=False), "a null frame": dict(depth=[np.zeros((TH, TW), np.uint16), None]),
    "n_frames 0": dict(n_frames=0), "n_frames above max_frames": dict(n_frames=MAX_FRAMES + 1, depth=[np.zeros((TH, TW), np.uint16)] * 3),
    "n_poses 0": dict(n_poses=0), "n_poses above max_tracks": dict(n_poses=MAX_TRACKS + 1, frame_of=[0] * 5, poses=np.zeros((5, 13)), group_first=[0, 1, 5]),
    "frame_of -1": dict(frame_of=[0, -1, 1]), "frame_of n_frames": dict(frame_of=[0, 1, 2]),
    "frame_of beyond a smaller n_frames": dict(n_frames=1),
    "pose nan": dict(poses=_bad_pose(NAN, 0)), "pose inf": dict(poses=_bad_pose(INF, 11)), "pose -inf": dict(poses=_bad_pose(-INF, 7)),
    "fx nan": dict(K=(TW, TH, NAN, 61.0, 32.0, 24.0)), "fy inf": dict(K=(TW, TH, 60.0, INF, 32.0, 24.0)),
    "cx nan": dict(K=(TW, TH, 60.0, 61.0, NAN, 24.0)), "cy -inf": dict(K=(TW, TH, 60.0, 61.0, 32.0, -INF)),
    "fx 0": dict(K=(TW, TH, 0.0, 61.0, 32.0, 24.0)), "fy negative": dict(K=(TW, TH, 60.0, -61.0, 32.0, 24.0)),
    "K width": dict(K=(TW + 1, TH, 60.0, 61.0, 32.0, 24.0)), "K height": dict(K=(TW, TH - 1, 60.0, 61.0, 32.0, 24.0)),
    "mem 2": dict(mem=2), "mem -1": dict(mem=-1),
}
# fl_verify_batch alone: K as floats (what its rasteriser gets), the groups, its parameters
INVALID = dict(COMMON_INVALID, **{
    "fx 0 as a float": dict(K=(TW, TH, 1e-60, 61.0, 32.0, 24.0)), "cx inf as a float": dict(K=(TW, TH, 60.0, 61.0, 1e300, 24.0)),
    "group_first[0] != 0": dict(group_first=[1, 1, 3]), "group_first decreasing": dict(group_first=[0, 2, 1, 3], n_groups=3),
    "group_first beyond n_poses in the middle": dict(group_first=[0, 4, 3]),
    "group_first ends before n_poses": dict(group_first=[0, 1, 2]), "group_first ends after n_poses": dict(group_first=[0, 1, 4]),
    "n_groups 0": dict(n_groups=0), "n_groups negative": dict(n_groups=-1),
    "n_groups above max_tracks": dict(n_groups=MAX_TRACKS + 1, group_first=[0, 0, 0, 1, 2, 3]),
    "tau -1": dict(params=(-1, 1, 0.0, 0.0)), "tau 65536": dict(params=(65536, 1, 0.0, 0.0)), "min_model_px 0": dict(params=(10, 0, 0.0, 0.0)),
    "min_inlier_ratio nan": dict(params=(10, 1, NAN, 0.0)), "max_behind_ratio inf": dict(params=(10, 1, 0.0, INF)),
    "min_inlier_ratio -inf": dict(params=(10, 1, -INF, 0.0)),
})
# in range for both entry points: the 13th pose float is ignored, frames may be device memory, every slot may be used
COMMON_VALID = [dict(), dict(poses=_bad_pose(NAN, 12)), dict(mem=L.FL_MEM_DEVICE), dict(n_frames=1, frame_of=[0, 0, 0]),
                dict(n_poses=MAX_TRACKS, frame_of=[0, 1, 0, 1], poses=np.stack([_p13((0, 0, 700, 0.3, 0.35, 0.1))] * 4), group_first=[0, 2, 4])]


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_are_refused_before_any_device_work(host_tracker, case):
    lib, trk = host_tracker
    rc, untouched = _call(lib, trk, **INVALID[case])
    assert rc == L.FL_ERR_INVALID and untouched, case


def test_valid_arguments_reach_the_device_check(host_tracker):
    """Everything the contract allows passes the checks and then fails for want of a device, with nothing written: the
    baseline, the band's two ends, gates on, no groups (n_groups is ignored then), empty groups, as many groups as max_tracks,
    params == NULL, device memory, and a 13th pose float that is not a number (it is ignored)."""
    lib, trk = host_tracker
    valid = [dict(), dict(params=(0, 1, 0.0, 0.0)), dict(params=(65535, 1 << 30, 0.5, 0.25)), dict(params=(10, 1, -1.0, -2.0)),
             dict(group_first=None, n_groups=-5), dict(group_first=[0, 0, 3, 3, 3], n_groups=MAX_TRACKS), dict(group_first=[0, 3], n_groups=1),
             dict(params=None), dict(mem=L.FL_MEM_DEVICE), dict(poses=_bad_pose(NAN, 12)),
             dict(n_poses=MAX_TRACKS, frame_of=[0, 1, 0, 1], poses=np.stack([_p13((0, 0, 700, 0.3, 0.35, 0.1))] * 4), group_first=[0, 2, 4])]
    for over in valid:
        rc, untouched = _call(lib, trk, **over)
        assert rc == L.FL_ERR_NO_DEVICE and untouched, over
    assert lib.fl_verify_batch(None, 1, None, 0, 1, None, None, 0, None, None, None, None) == L.FL_ERR_INVALID


@pytest.mark.parametrize("entry", ["track", "verify"])
def test_the_common_checks_are_shared_by_both_entry_points(host_tracker, entry):
    """One list of bad and one of good argument lists against fl_track_batch and fl_verify_batch on one tracker: each refuses
    the bad ones (FL_ERR_INVALID) and passes the good ones on to the device check (FL_ERR_NO_DEVICE), nothing written."""
    lib, trk = host_tracker
    for case, over in COMMON_INVALID.items():
        rc, untouched = _call(lib, trk, entry, **over)
        assert rc == L.FL_ERR_INVALID and untouched, (entry, case)
    for over in COMMON_VALID:
        rc, untouched = _call(lib, trk, entry, **over)
        assert rc == L.FL_ERR_NO_DEVICE and untouched, (entry, over)


def test_the_one_difference_between_the_entry_points_checks_of_K(host_tracker):
    """fx = 1e-60 is a positive double and a zero float.  fl_verify_batch hands K to the rasteriser as floats and refuses it;
    fl_track_batch renders at the model camera and reads the scene's K in fp64, so it passes its argument checks."""
    lib, trk = host_tracker
    tiny = dict(K=(TW, TH, 1e-60, 61.0, 32.0, 24.0))
    assert _call(lib, trk, "verify", **tiny) == (L.FL_ERR_INVALID, True)
    assert _call(lib, trk, "track", **tiny) == (L.FL_ERR_NO_DEVICE, True)


def test_result_record_layout():
    from fealess_amd import api
    assert C.sizeof(L.VerifyResult) == 64 and C.sizeof(L.VerifyParams) == 16
    assert api.VERIFY_DTYPE == VM.DTYPE
    for name, _ in L.VerifyResult._fields_:
        assert getattr(L.VerifyResult, name).offset == VM.DTYPE.fields[name][1], name
