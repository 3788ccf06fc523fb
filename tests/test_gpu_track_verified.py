"""GPU: fl_track_batch_verified (api.Tracker.track_verified) and the facade's CadRecoSetVerifiedTracking against
tests/track_verified_model.py, against Tracker.track and Tracker.verify, and beside its neighbours.

The poses, scenes, sequence and special poses are those of tests/test_gpu_track.py; the gates 0.7 / 0.1 are the ones
tests/test_track_verified_cpu.py derives from the models.
"""
import ctypes as C

import numpy as np
import pytest

import cadreco_py
import track_model as TM
import track_verified_model as TVM
import util
import verify_model as VM
from fealess_amd import _lib as L
from fealess_amd import api, synth
from test_gpu_track import BIG_POSE, GONE_POSE, K0, LOST_POSE, MAX_CROP, OFFSETS, POSES, H, W, _bits, _gt, _same_as_parity_model
from test_track_verified_cpu import MAX_BEHIND, MIN_INLIER
from util import p13 as _p13, pose as _pose

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mesh():
    return synth.object_mesh(2)


@pytest.fixture(scope="module")
def tracker(ctx, mesh):
    t = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], W, H, 8, 8, MAX_CROP)
    yield t
    t.close()


@pytest.fixture(scope="module")
def moving(mesh, oracle):
    """The six input poses, their scenes one frame of motion on (noise and background on), and the model's parity step with
    keep_input = 1 (so both records); computed once, read only."""
    poses = np.stack([_p13(p) for p in POSES])
    scenes = [synth.render(W, H, *_pose(p, OFFSETS[0]), seed=40 + i)[0] for i, p in enumerate(POSES)]
    return dict(poses=poses, scenes=scenes, exp=_model(mesh, oracle, scenes, poses, K0))


@pytest.fixture(scope="module")
def sequence():
    return [dict(R=_gt(k)[0], t=_gt(k)[1], pose=synth.pose13(*_gt(k)), scene=synth.render(W, H, *_gt(k), seed=100 + k)[0]) for k in range(4)]


@pytest.fixture(scope="module")
def empty(sequence):
    return synth.render(W, H, sequence[0]["R"], np.array([0.0, 0.0, -500.0]), seed=7, plane_z=740.0)[0]


ZERO_V = bytes(64)


def _same_as_model(got, exp, keep_input):
    """One record of a track the passes kept against track_verified_model's dict (parity mode), bit for bit.  exp was computed
    with keep_input = 1; without it verify_in is zero and the decision is the model's rule on that."""
    assert exp["icp_tracked"] == 1
    vin = exp["verify_in"] if keep_input else np.zeros((), VM.DTYPE)
    tracked, kept = TVM.decide(1, exp["verify"], vin, keep_input)
    assert got["icp_tracked"] == 1 and got["kept_input"] == kept and got["reserved"] == 0
    assert got["verify"].tobytes() == exp["verify"].tobytes(), (got["verify"], exp["verify"])
    assert got["verify_in"].tobytes() == vin.tobytes(), (got["verify_in"], vin)
    icp = np.eye(4, dtype=np.float32)
    icp[:3, :3], icp[:3, 3] = exp["track"]["det"]["R_final"], exp["track"]["det"]["T_final"]
    _same_as_parity_model(got["track"], dict(exp["track"], tracked=tracked, pose=icp if tracked and not kept else TM.pose4x4(exp["pose_in"])))


def _model(mesh, oracle, scenes, poses, K):
    exp = TVM.track_verified(mesh, scenes, np.arange(len(poses)), poses, K, keep_input=1, max_crop_px=MAX_CROP, oracle=oracle, icp_mode=TM.PARITY)
    for r, p in zip(exp, poses):
        r["pose_in"] = p
    return exp


def _track_part_equals_track(got, plain):
    """The `track` part against Tracker.track's records: byte for byte, apart from tracked and pose where the decision says so."""
    for g, p in zip(got, plain):
        assert g["icp_tracked"] == p["tracked"]
        a, b = g["track"].copy(), p.copy()
        if g["kept_input"] or (g["icp_tracked"] and not g["track"]["tracked"]):
            a["tracked"], a["pose"] = b["tracked"], b["pose"]
        assert a.tobytes() == b.tobytes()


# ---- 1. parity mode against the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["1024", "256", "256x5"])
def test_parity_mode_equals_the_model(ctx, tracker, moving, build):
    exp = moving["exp"]
    assert all(e["icp_tracked"] == 1 and e["verify"]["n_model"] > 5000 for e in exp)
    with util.options(ctx, {"icp_wide": 1 if build == "1024" else 0, "icp_occ": 5 if build == "256x5" else 0}):
        plain = tracker.track(moving["scenes"], np.arange(6), moving["poses"], K0, icp_mode=L.FL_ICP_PARITY)
        for keep in (0, 1):
            got = tracker.track_verified(moving["scenes"], np.arange(6), moving["poses"], K0, keep_input=keep, icp_mode=L.FL_ICP_PARITY)
            _track_part_equals_track(got, plain)
            for i in range(6):
                _same_as_model(got[i], exp[i], keep)
            assert got["best"].tolist() == got["track"]["tracked"].tolist()


# ---- 2. the verification is of the pose the GPU returned ----------------------------------------------------------------------
def _pose_out(rec):
    p = np.zeros(13, np.float32)
    p[:12] = np.concatenate([rec["track"]["det"]["R_final"].reshape(3, 3), rec["track"]["det"]["T_final"].reshape(3, 1)], 1).ravel()
    return p


def test_the_verification_is_of_the_pose_the_gpu_returned(ctx, tracker, mesh, sequence):
    scenes = [sequence[k]["scene"] for k in (1, 2, 3)]
    poses = np.stack([sequence[k - 1]["pose"] for k in (1, 2, 3)])
    got = tracker.track_verified(scenes, [0, 1, 2], poses, K0, keep_input=1)
    assert got["icp_tracked"].tolist() == [1, 1, 1]
    out = np.stack([_pose_out(r) for r in got])
    for name, p in (("verify", out), ("verify_in", poses)):
        model = VM.verify(mesh, scenes, [0, 1, 2], p, K0)
        assert got[name].tobytes() == model.tobytes(), (name, got[name], model)
        with util.options(ctx, {"verify_fused": 0}):
            rendered = tracker.verify(scenes, [0, 1, 2], p, K0)
        assert got[name].tobytes() == rendered.tobytes(), name
    assert (got["verify"]["n_model"] > 5000).all() and (got["kept_input"] == 0).all() and (got["track"]["tracked"] == 1).all()
    with util.options(ctx, {"verify_fused_px": 1024}):                  # several bands per pose
        banded = tracker.track_verified(scenes[:1], [0], poses[:1], K0, keep_input=1)
    assert banded.tobytes() == got[:1].tobytes()


# ---- 3. a scene camera other than the model camera ----------------------------------------------------------------------------
def test_scene_camera_other_than_the_model_camera(tracker, mesh, oracle):
    """The passes render at 608 / 608 / 320 / 240, the verification at the scene's 600 / 608 / 327.4 / 234.4."""
    K = (600.0, 608.0, 327.4, 234.4)
    poses = np.stack([_p13(POSES[0]), _p13(POSES[2])])
    scenes = [synth.render(W, H, *_pose(POSES[0], OFFSETS[0]), seed=61, fx=K[0], fy=K[1], cx=K[2], cy=K[3])[0],
              synth.render(W, H, *_pose(POSES[2], OFFSETS[1]), seed=62, fx=K[0], fy=K[1], cx=K[2], cy=K[3])[0]]
    exp = _model(mesh, oracle, scenes, poses, K)
    got = tracker.track_verified(scenes, [0, 1], poses, K, keep_input=1, icp_mode=L.FL_ICP_PARITY)
    for i in range(2):
        assert exp[i]["icp_tracked"] == 1 and exp[i]["verify"]["n_model"] > 5000
        _same_as_model(got[i], exp[i], 1)
    at_model_camera = VM.verify(mesh, scenes, [0, 1], np.stack([_pose_out(r) for r in got]), K0)
    assert got["verify"].tobytes() != at_model_camera.tobytes()


# ---- 4. an image whose pixel count is no multiple of eight --------------------------------------------------------------------
def test_image_whose_pixel_count_is_no_multiple_of_eight(ctx, mesh, oracle):
    w, h = 322, 250
    p = (-150, -100, 700, 0.3, 0.35, 0.1)
    poses = _p13(p)[None]
    scene = synth.render(w, h, *_pose(p, OFFSETS[0]), seed=71)[0]
    exp = _model(mesh, oracle, [scene], poses, K0)
    t = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], w, h, 1, 1, MAX_CROP)
    try:
        got = t.track_verified([scene], [0], poses, K0, keep_input=1, icp_mode=L.FL_ICP_PARITY)
    finally:
        t.close()
    assert exp[0]["icp_tracked"] == 1 and exp[0]["verify"]["n_model"] > 1000
    _same_as_model(got[0], exp[0], 1)


# ---- 5. a frame without the object --------------------------------------------------------------------------------------------
def test_a_frame_without_the_object_is_lost_by_the_verification(tracker, sequence, empty):
    pose = sequence[0]["pose"]
    args = ([empty, sequence[1]["scene"]], [0, 1], np.stack([pose, pose]), K0)
    free = tracker.track_verified(*args)
    print("inlier_ratio", free["verify"]["inlier_ratio"], "behind_ratio", free["verify"]["behind_ratio"])
    assert free["track"]["tracked"].tolist() == [1, 1] and free["icp_tracked"].tolist() == [1, 1] and free["best"].tolist() == [1, 1]
    assert free["verify"]["inlier_ratio"][0] <= 0.55 and free["verify"]["inlier_ratio"][1] >= 0.95
    assert free["verify"]["behind_ratio"][0] >= 0.4 and free["verify"]["behind_ratio"][1] <= 0.02
    for gate in (dict(min_inlier_ratio=MIN_INLIER), dict(max_behind_ratio=MAX_BEHIND)):
        got = tracker.track_verified(*args, **gate)
        assert got["track"]["tracked"].tolist() == [0, 1] and got["icp_tracked"].tolist() == [1, 1] and got["best"].tolist() == [0, 1], gate
        assert got["verify"]["accepted"].tolist() == [0, 1] and got["track"]["status"].tolist() == [0, 0]
        assert np.array_equal(_bits(got[0]["track"]["pose"]).reshape(4, 4), _bits(TM.pose4x4(pose)))
        # the lost track's figures are still there, and nothing but accepted / best / tracked / pose differs from the ungated call
        a, b = got.copy(), free.copy()
        for r in (a, b):
            r["verify"]["accepted"], r["verify"]["best"], r["best"], r["track"]["tracked"], r["track"]["pose"] = 0, 0, 0, 0, 0
        assert a.tobytes() == b.tobytes() and got[0]["verify"]["n_model"] > 5000
        assert got[1].tobytes() == free[1].tobytes()


# ---- 6. the drift guard -------------------------------------------------------------------------------------------------------
def test_an_object_that_stands_still_keeps_its_input_pose(tracker, sequence):
    p0 = sequence[0]["pose"]
    args = ([sequence[0]["scene"], sequence[1]["scene"]], [0, 1], np.stack([p0, p0]), K0)
    got = tracker.track_verified(*args, keep_input=1)
    print("static: in", got[0]["verify_in"], "out", got[0]["verify"])
    assert got["icp_tracked"].tolist() == [1, 1] and got["track"]["tracked"].tolist() == [1, 1]
    assert got["kept_input"].tolist() == [1, 0]
    assert np.array_equal(_bits(got[0]["track"]["pose"]).reshape(4, 4), _bits(TM.pose4x4(p0)))
    assert TVM.decide(1, got[0]["verify"], got[0]["verify_in"], 1) == (1, 1) and TVM.decide(1, got[1]["verify"], got[1]["verify_in"], 1) == (1, 0)
    assert np.array_equal(_bits(api.poses13_of(got["track"])[1]), _bits(_pose_out(got[1])))
    off = tracker.track_verified(*args, keep_input=0)
    assert off["verify_in"].tobytes() == 2 * ZERO_V and off["kept_input"].tolist() == [0, 0] and off["track"]["tracked"].tolist() == [1, 1]
    assert off["verify"].tobytes() == got["verify"].tobytes()
    for i in range(2):
        assert np.array_equal(_bits(api.poses13_of(off["track"])[i]), _bits(_pose_out(off[i])))


# ---- 7. hypothesis groups -----------------------------------------------------------------------------------------------------
def test_hypothesis_groups(tracker, sequence):
    poses = np.stack([sequence[0]["pose"], sequence[1]["pose"], _p13(LOST_POSE), _p13(GONE_POSE), sequence[2]["pose"]])
    gf = [0, 3, 4, 5]
    for keep in (0, 1):
        got = tracker.track_verified([sequence[2]["scene"]], np.zeros(5, np.int32), poses, K0, group_first=gf, keep_input=keep)
        print("inlier_ratio", got["verify"]["inlier_ratio"], got["verify_in"]["inlier_ratio"], "kept", got["kept_input"], "best", got["best"])
        exp = TVM.pick(got["track"]["tracked"].tolist(), got["kept_input"].tolist(), got["verify"], got["verify_in"], gf)
        assert got["best"].tolist() == exp
        assert got["icp_tracked"].tolist() == [1, 1, 0, 0, 1] and got["track"]["tracked"].tolist() == [1, 1, 0, 0, 1]
        assert got["best"][:3].sum() == 1 and got["best"][2] == 0 and got["best"][3] == 0 and got["best"][4] == 1
        for i in (2, 3):
            assert got[i]["verify"].tobytes() == ZERO_V and got[i]["verify_in"].tobytes() == ZERO_V and got[i]["kept_input"] == 0
            assert np.array_equal(_bits(got[i]["track"]["pose"]).reshape(4, 4), _bits(TM.pose4x4(poses[i])))
        for i in range(5):
            assert TVM.decide(got[i]["icp_tracked"], got[i]["verify"], got[i]["verify_in"], keep) == (got[i]["track"]["tracked"], got[i]["kept_input"])
        ungrouped = tracker.track_verified([sequence[2]["scene"]], np.zeros(5, np.int32), poses, K0, keep_input=keep)
        assert ungrouped["best"].tolist() == ungrouped["track"]["tracked"].tolist()
        a = got.copy()
        a["best"] = ungrouped["best"]
        assert a.tobytes() == ungrouped.tobytes()


# ---- 8. batch structure -------------------------------------------------------------------------------------------------------
def test_batch_equals_single_calls_in_either_order(ctx, tracker, moving, sequence):
    import torch
    scenes = moving["scenes"] + [sequence[0]["scene"], sequence[1]["scene"]]
    poses = np.concatenate([moving["poses"], np.stack([sequence[0]["pose"]] * 2)])
    kw = dict(keep_input=1, min_inlier_ratio=0.5)
    single = np.concatenate([tracker.track_verified([scenes[i]], [0], poses[i:i + 1], K0, **kw) for i in range(8)])
    assert single["track"]["tracked"].all() and single["kept_input"][6] == 1
    batch = tracker.track_verified(scenes, np.arange(8), poses, K0, **kw)
    assert batch.tobytes() == single.tobytes()
    order = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    assert tracker.track_verified([scenes[i] for i in order], np.arange(8), poses[order], K0, **kw).tobytes() == single[order].tobytes()
    assert tracker.track_verified(scenes, order, poses[order], K0, **kw).tobytes() == single[order].tobytes()
    mixed_poses = poses.copy()
    mixed_poses[2], mixed_poses[3], mixed_poses[4] = _p13(LOST_POSE), _p13(BIG_POSE), _p13(GONE_POSE)
    mixed = tracker.track_verified(scenes, np.arange(8), mixed_poses, K0, **kw)
    for i in (0, 1, 5, 6, 7):
        assert mixed[i].tobytes() == single[i].tobytes(), i
    assert mixed["track"]["tracked"].tolist() == mixed["icp_tracked"].tolist() == mixed["best"].tolist() == [1, 1, 0, 0, 0, 1, 1, 1]
    assert mixed["track"]["status"].tolist() == [0, 0, 0, L.FL_ERR_OVERFLOW, 0, 0, 0, 0]
    plain = tracker.track(scenes, np.arange(8), mixed_poses, K0)
    _track_part_equals_track(mixed, plain)
    for i in (2, 3, 4):
        assert mixed[i]["track"].tobytes() == plain[i].tobytes() and mixed[i].tobytes()[plain.itemsize:] == bytes(single.itemsize - plain.itemsize), i
    # host and device frames
    dev = [torch.from_numpy(s.view(np.int16)).to(f"cuda:{ctx.device}") for s in scenes]
    torch.cuda.synchronize()
    assert tracker.track_verified(dev, np.arange(8), poses, K0, **kw).tobytes() == single.tobytes()
    # two passes
    twice = tracker.track_verified(scenes, np.arange(8), mixed_poses, K0, passes=2, **kw)
    _track_part_equals_track(twice, tracker.track(scenes, np.arange(8), mixed_poses, K0, passes=2))
    assert not np.array_equal(twice["track"]["det"]["T_final"][0], mixed["track"]["det"]["T_final"][0])
    assert twice["track"]["tracked"].tolist() == [1, 1, 0, 0, 0, 1, 1, 1]


# ---- 9. the neighbours --------------------------------------------------------------------------------------------------------
def test_neighbours_are_unaffected(ctx, tracker, mesh, moving, sequence, oracle):
    import clutter
    scenes, poses = moving["scenes"], moving["poses"]
    tv = dict(keep_input=1, group_first=[0, 2, 6], min_inlier_ratio=MIN_INLIER)
    first = tracker.track(scenes, np.arange(6), poses, K0)
    mid = tracker.track_verified(scenes, np.arange(6), poses, K0, **tv)
    assert tracker.track(scenes, np.arange(6), poses, K0).tobytes() == first.tobytes()
    for fused in (1, 0):
        with util.options(ctx, {"verify_fused": fused}):
            v0 = tracker.verify(scenes, np.arange(6), poses, K0, group_first=[0, 3, 6])
            assert tracker.track_verified(scenes, np.arange(6), poses, K0, **tv).tobytes() == mid.tobytes()
            assert tracker.verify(scenes, np.arange(6), poses, K0, group_first=[0, 3, 6]).tobytes() == v0.tobytes()
    # the recognition that shares the fused kernel, on the cluttered frame a, around a verified tracking call on its mesh tracker
    sc = clutter.build(oracle)
    bgr, depth = sc["frames"]["a"]
    det = api.Detector(ctx, 2, clutter.T)
    det.add_class(sc["bank"])
    det.finalize(clutter.W, clutter.H, max_batch=1)
    try:
        def reco():
            got, members = det.recognize_batch_instances_verified(tracker, [bgr], [depth], sc["K"], 8, 48, 4, -1, True)
            return [(g["rank"], g["verify"].tobytes(), np.asarray(g["pose"], np.float32).tobytes()) for g in got[0]], members.tobytes()
        before = reco()
        assert len(before[0]) >= 3 and any(v != ZERO_V for _, v, _ in before[0])
        assert tracker.track_verified(scenes, np.arange(6), poses, K0, **tv).tobytes() == mid.tobytes()
        assert reco() == before
    finally:
        det.close()


# ---- 10. the facade -----------------------------------------------------------------------------------------------------------
INVALID = cadreco_py.INVALID


def test_facade_verified_tracking(ctx, mesh, sequence, empty, tmp_path):
    cad = cadreco_py.lib()
    obj = str(tmp_path / "object.obj")
    synth.write_obj(obj, mesh)

    def track(h, depth, poses16):
        p = np.ascontiguousarray(poses16, np.float32).copy()
        trk = np.full(len(p), -7, np.int32)
        rc = cad.cadreco_track(h, *cadreco_py.frame_args(depth, 0.0, K0), len(p), p.ctypes.data, trk.ctypes.data)
        return rc, p, trk

    with cadreco_py.handle() as h:
        assert cad.cadreco_set_verified_tracking(h, 1, 10.0, 0.0, 0.0, 0) == INVALID          # no mesh yet
        assert cad.cadreco_set_verified_tracking(h, 0, 10.0, 0.0, 0.0, 0) == 0                # off is always fine
        assert cad.cadreco_set_tracking_mesh(h, obj.encode(), 1.0) == 0
        for bad in ((1, -1.0, 0.0, 0.0, 0), (1, 65536.0, 0.0, 0.0, 0), (1, float("nan"), 0.0, 0.0, 0), (1, 10.0, float("nan"), 0.0, 0),
                    (1, 10.0, 0.0, float("inf"), 0), (1, 10.0, 0.0, 0.0, 2), (1, 10.0, 0.0, 0.0, -1)):
            assert cad.cadreco_set_verified_tracking(h, *bad) == INVALID, bad
        V, _, T = cadreco_py.read_obj(obj)
        ref = api.Tracker(ctx, V, T, W, H, 1, 16, 320 * 240)
        try:
            poses = np.stack([TM.pose4x4(sequence[0]["pose"]), TM.pose4x4(_p13(LOST_POSE))])
            frames = (sequence[1]["scene"], sequence[0]["scene"], empty)
            off = [track(h, f, poses) for f in frames]
            for (rc, out, trk), f in zip(off, frames):                                        # off: fl_track_batch, as ever
                exp = ref.track([f], [0, 0], poses, K0)
                assert rc == 0 and trk.tolist() == exp["tracked"].tolist() and np.array_equal(_bits(out).reshape(2, 16), _bits(exp["pose"]))
            assert off[2][2].tolist() == [1, 0]                                               # the empty frame counts as tracked
            assert cad.cadreco_set_verified_tracking(h, 1, 10.0, MIN_INLIER, MAX_BEHIND, 1) == 0
            tracked = []
            for f in frames:
                rc, out, trk = track(h, f, poses)
                exp = ref.track_verified([f], [0, 0], poses, K0, keep_input=1, tau_mm=10, min_inlier_ratio=MIN_INLIER, max_behind_ratio=MAX_BEHIND)
                assert rc == 0 and trk.tolist() == exp["track"]["tracked"].tolist()
                assert np.array_equal(_bits(out).reshape(2, 16), _bits(exp["track"]["pose"]))
                assert np.array_equal(out[1], poses[1])
                tracked.append((trk.tolist(), exp["kept_input"].tolist()))
            assert tracked == [([1, 0], [0, 0]), ([1, 0], [1, 0]), ([0, 0], [0, 0])]        # followed; stands still; nothing there
            assert np.array_equal(track(h, frames[1], poses)[1][0], poses[0])
            assert cad.cadreco_set_verified_tracking(h, 0, 0.0, 0.0, 0.0, 0) == 0
            for (rc, out, trk), f in zip(off, frames):
                again = track(h, f, poses)
                assert again[0] == rc and again[1].tobytes() == out.tobytes() and again[2].tolist() == trk.tolist()
        finally:
            ref.close()
