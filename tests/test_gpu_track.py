"""GPU: fl_tracker_create / fl_track_batch (api.Tracker) and the facade's CadRecoTrack against tests/track_model.py.

Everything is at 640 x 480 (the model camera 608 / 608 / 320 / 240 belongs to that image) except one 322 x 250 case, whose pixel
count is no multiple of eight (k_track_rects then reads the render pixel by pixel).  The object is synth.object_mesh(2) at
tz = 680 .. 760 mm: detection() drops every point beyond 900 mm (vvalid, ICP/common.cpp:261-266), so an object at 900 - 1000 mm
would leave the ICP little or nothing to work on; at 720 mm a crop is about 190 x 145 pixels.
"""
import ctypes as C

import numpy as np
import pytest

import cadreco_py
from cadreco_py import INVALID, OPEN_FAILED
import track_model as TM
import util
from fealess_amd import _lib as L
from fealess_amd import api, synth
from util import p13 as _p13, pose as _pose

pytestmark = pytest.mark.gpu

W, H = 640, 480
K0 = TM.MODEL_K
MAX_CROP = 40000
MOTION_T, MOTION_A = (4.0, -2.0, 3.0), (0.02, -0.01, 0.015)     # per frame: mm, and rad of yaw / tilt / roll

# (tx, ty, tz, yaw, tilt, roll) of the poses the tracks come in with
POSES = [(10, -5, 720, 0.30, 0.35, 0.10), (-60, 30, 690, -0.50, 0.20, 0.30), (80, -40, 750, 0.90, 0.50, -0.20),
         (0, 0, 700, 0.00, 0.30, 0.00), (-100, -60, 760, 1.40, 0.10, 0.25), (120, 70, 680, -1.10, 0.45, -0.15)]
# how far the scene's object is from the pose a track comes in with: translation (mm), yaw / tilt / roll (rad)
OFFSETS = [(MOTION_T, MOTION_A), ((-3.0, 3.0, -2.0), (-0.015, 0.01, 0.01)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))]


@pytest.fixture(scope="module")
def mesh():
    return synth.object_mesh(2)


@pytest.fixture(scope="module")
def tracker(ctx, mesh):
    t = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], W, H, 8, 8, MAX_CROP)
    yield t
    t.close()


@pytest.fixture(scope="module")
def cases(mesh, oracle):
    """Per scene offset: the six input poses, their scenes (noise and background on) and the model's parity step, computed
    once and shared (read only)."""
    out = []
    for j, off in enumerate(OFFSETS):
        poses = np.stack([_p13(p) for p in POSES])
        scenes = [synth.render(W, H, *_pose(p, off), seed=40 + 7 * j + i)[0] for i, p in enumerate(POSES)]
        exp = [TM.step(mesh, poses[i], scenes[i], K0, max_crop_px=MAX_CROP, oracle=oracle, icp_mode=TM.PARITY) for i in range(len(POSES))]
        out.append(dict(poses=poses, scenes=scenes, exp=exp))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_rects(got, exp):
    assert tuple(got["rect_model"]) == tuple(exp["rect_model"]) and tuple(got["rect_ref"]) == tuple(exp["rect_ref"]), (got, exp)
    assert got["status"] == exp["status"] and got["tracked"] == exp["tracked"], (got, exp)


def _same_as_parity_model(got, exp):
    """Every compared field of one record against track_model's step on the oracle's detection(), bit for bit."""
    _same_rects(got, exp)
    d, e = got["det"], exp["det"]
    assert d["n_points"] == e["n_points"]
    assert np.array_equal(_bits(d["R_final"]).ravel(), _bits(e["R_final"]).ravel())
    assert np.array_equal(_bits(d["T_final"]), _bits(e["T_final"]))
    assert np.array_equal(_bits(got["pose"]).reshape(4, 4), _bits(exp["pose"]))
    gi, ei = d["icp"], e["icp"]
    assert np.array_equal(_bits(gi["R"]).ravel(), _bits(ei["R"]).ravel()) and np.array_equal(_bits(gi["T"]), _bits(ei["T"]))
    assert _bits(gi["dist_mean"]) == _bits(ei["dist_mean"]) and _bits(gi["px_ratio"]) == _bits(ei["px_ratio"])
    assert gi["iters"] == ei["iters"] and gi["n_corr_last"] == ei["n_corr_last"]


def _angle_deg(Ra, Rb):
    """Rotation angle of Ra Rb^T from its skew part and its trace (atan2), as tests/test_gpu_icp.py measures it: the arccos of
    a trace made of float32-rounded entries resolves nothing below 0.03 degrees."""
    M = np.asarray(Ra, np.float64).reshape(3, 3) @ np.asarray(Rb, np.float64).reshape(3, 3).T
    s = 0.5 * np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return float(np.degrees(np.arctan2(s, (np.trace(M) - 1) / 2)))


# ---- 1. parity mode, bit for bit, on every ICP build --------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["1024", "256", "256x5"])
def test_parity_mode_equals_the_model_on_the_oracle(ctx, tracker, cases, build):
    """6 poses x 3 scene offsets, one pass: rects, n_points and every bit of R_final, T_final, pose and icp.* equal
    track_model.step built on oracle_py.detection -- the render equals raster_model and the ICP the oracle, so this pins the
    plumbing between them."""
    with util.options(ctx, {"icp_wide": 1 if build == "1024" else 0, "icp_occ": 5 if build == "256x5" else 0}):
        for c in cases:
            got = tracker.track(c["scenes"], np.arange(6), c["poses"], K0, icp_mode=L.FL_ICP_PARITY)
            for i in range(6):
                assert c["exp"][i]["tracked"] == 1 and c["exp"][i]["det"]["n_points"] > 5000
                _same_as_parity_model(got[i], c["exp"][i])


# ---- 2. rectangles ------------------------------------------------------------------------------------------------------------
def test_rects_at_the_borders_out_of_view_and_behind_the_camera(tracker, mesh, cases):
    scene = cases[0]["scenes"][0]
    partly = [(-360, 0, 720, 0.3, 0.35, 0.1), (360, 0, 720, 0.3, 0.35, 0.1), (0, -270, 720, 0.3, 0.35, 0.1), (0, 270, 720, 0.3, 0.35, 0.1),
              (-350, -260, 720, 0.3, 0.35, 0.1), (350, 265, 700, 0.3, 0.35, 0.1)]
    gone = [(900, 0, 720, 0.3, 0.35, 0.1), (0, 0, -720, 0.3, 0.35, 0.1)]           # out of view; behind the camera
    poses = np.stack([_p13(p) for p in partly + gone])
    got = tracker.track([scene], np.zeros(8, np.int32), poses, K0, icp_mode=L.FL_ICP_PARITY)
    for i in range(8):
        r = TM.rects(TM.render(mesh, poses[i], W, H), poses[i], K0, 12)
        if i < 6:
            assert r is not None and (r[0][0] == 0 or r[0][1] == 0 or r[0][0] + r[0][2] == W or r[0][1] + r[0][3] == H), i
            assert tuple(got[i]["rect_model"]) == r[0] and tuple(got[i]["rect_ref"]) == r[1] and got[i]["status"] == 0, i
        else:
            assert r is None
            assert got[i]["status"] == 0 and got[i]["tracked"] == 0 and not got[i]["rect_model"].any() and not got[i]["rect_ref"].any()
            assert np.array_equal(got[i]["pose"].reshape(4, 4), TM.pose4x4(poses[i]))
            assert got[i]["det"]["n_points"] == 0


def test_crop_one_pixel_over_and_under_max_crop_px(ctx, mesh, cases):
    c = cases[0]
    rm = c["exp"][0]["rect_model"]
    area = rm[2] * rm[3]
    for cap, status in ((area - 1, L.FL_ERR_OVERFLOW), (area, 0)):
        t = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], W, H, 1, 1, cap)
        try:
            got = t.track(c["scenes"][:1], [0], c["poses"][:1], K0, icp_mode=L.FL_ICP_PARITY)[0]
        finally:
            t.close()
        assert got["status"] == status and tuple(got["rect_model"]) == rm and tuple(got["rect_ref"]) == c["exp"][0]["rect_ref"]
        if status:
            assert got["tracked"] == 0 and np.array_equal(got["pose"].reshape(4, 4), TM.pose4x4(c["poses"][0])) and got["det"]["n_points"] == 0
        else:
            _same_as_parity_model(got, c["exp"][0])


def test_scene_camera_other_than_the_model_camera(tracker, mesh, oracle):
    """cx, cy moved by (+7.4, -5.6) and fx = 600: rect_ref is shifted against rect_model, and the step still equals the model on
    oracle_py.detection with that K, bit for bit."""
    K = (600.0, 608.0, 327.4, 234.4)
    poses = np.stack([_p13(POSES[0]), _p13(POSES[2]), _p13((-250, 40, 700, 0.2, 0.3, 0.1))])
    scenes = [synth.render(W, H, *_pose(POSES[0], OFFSETS[0]), seed=61, fx=K[0], fy=K[1], cx=K[2], cy=K[3])[0],
              synth.render(W, H, *_pose(POSES[2], OFFSETS[1]), seed=62, fx=K[0], fy=K[1], cx=K[2], cy=K[3])[0],
              synth.render(W, H, *_pose((-250, 40, 700, 0.2, 0.3, 0.1), OFFSETS[0]), seed=63, fx=K[0], fy=K[1], cx=K[2], cy=K[3])[0]]
    got = tracker.track(scenes, [0, 1, 2], poses, K, icp_mode=L.FL_ICP_PARITY)
    shifts = set()
    for i in range(3):
        exp = TM.step(mesh, poses[i], scenes[i], K, max_crop_px=MAX_CROP, oracle=oracle, icp_mode=TM.PARITY)
        shifts.add((exp["rect_ref"][0] - exp["rect_model"][0], exp["rect_ref"][1] - exp["rect_model"][1]))
        assert exp["tracked"] == 1
        _same_as_parity_model(got[i], exp)
    assert (7, -6) in shifts and len(shifts) > 1            # the fx term moves the shift with tx / tz


def test_image_whose_pixel_count_is_no_multiple_of_eight(ctx, mesh, oracle):
    w, h = 322, 250
    p = (-150, -100, 700, 0.3, 0.35, 0.1)
    poses = np.stack([_p13(p), _p13((20, 10, 700, 0.3, 0.35, 0.1))])                # the second one leaves the image bottom right
    scene = synth.render(w, h, *_pose(p, OFFSETS[0]), seed=71)[0]
    t = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], w, h, 1, 2, MAX_CROP)
    try:
        got = t.track([scene], [0, 0], poses, K0, icp_mode=L.FL_ICP_PARITY)
    finally:
        t.close()
    for i in range(2):
        exp = TM.step(mesh, poses[i], scene, K0, max_crop_px=MAX_CROP, oracle=oracle, icp_mode=TM.PARITY)
        assert exp["rect_model"][2] > 0
        if exp["tracked"]:
            _same_as_parity_model(got[i], exp)
        else:
            _same_rects(got[i], exp)
    assert TM.step(mesh, poses[0], scene, K0, oracle=oracle, icp_mode=TM.PARITY)["tracked"] == 1


# ---- 3. batch structure -------------------------------------------------------------------------------------------------------
LOST_POSE = (0, 0, 1100, 0.3, 0.35, 0.1)        # the render lies beyond 900 mm: no valid model point, icp.dist_mean = -1
BIG_POSE = (0, 0, 400, 0.3, 0.35, 0.1)          # a crop of more than MAX_CROP pixels
GONE_POSE = (2000, 0, 720, 0.3, 0.35, 0.1)      # out of view


@pytest.mark.parametrize("mode", [L.FL_ICP_PARITY, L.FL_ICP_POINT_TO_PLANE])
def test_batch_equals_single_calls_in_either_order(tracker, cases, mode):
    c0, c1 = cases[0], cases[1]
    scenes = c0["scenes"] + c1["scenes"][:2]
    poses = np.concatenate([c0["poses"], c1["poses"][:2]])
    single = np.concatenate([tracker.track([scenes[i]], [0], poses[i:i + 1], K0, icp_mode=mode) for i in range(8)])
    assert single["tracked"].all()
    batch = tracker.track(scenes, np.arange(8), poses, K0, icp_mode=mode)
    assert batch.tobytes() == single.tobytes()
    order = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    shuffled = tracker.track([scenes[i] for i in order], np.arange(8), poses[order], K0, icp_mode=mode)
    assert shuffled.tobytes() == single[order].tobytes()
    # frames in one order, tracks in another
    crossed = tracker.track(scenes, order, poses[order], K0, icp_mode=mode)
    assert crossed.tobytes() == single[order].tobytes()
    # a lost, an overflowing and an out-of-view track in the middle leave the others' bits unchanged
    mixed_poses = poses.copy()
    mixed_poses[2], mixed_poses[3], mixed_poses[4] = _p13(LOST_POSE), _p13(BIG_POSE), _p13(GONE_POSE)
    mixed = tracker.track(scenes, np.arange(8), mixed_poses, K0, icp_mode=mode)
    for i in (0, 1, 5, 6, 7):
        assert mixed[i].tobytes() == single[i].tobytes(), i
    assert mixed["tracked"].tolist() == [1, 1, 0, 0, 0, 1, 1, 1]
    assert mixed["status"].tolist() == [0, 0, 0, L.FL_ERR_OVERFLOW, 0, 0, 0, 0]
    assert mixed[2]["rect_model"][2] > 0 and mixed[2]["det"]["icp"]["dist_mean"] < 0 and mixed[2]["det"]["n_points"] == 0
    assert mixed[3]["rect_model"][2] * mixed[3]["rect_model"][3] > MAX_CROP and not mixed[4]["rect_model"].any()
    for i in (2, 3, 4):
        assert np.array_equal(mixed[i]["pose"].reshape(4, 4), TM.pose4x4(mixed_poses[i])), i


def test_two_tracks_on_one_frame_and_device_frames(ctx, tracker, cases):
    import torch
    c = cases[0]
    near = np.stack([c["poses"][0], _p13(POSES[0], ((2.0, 1.0, -1.0), (0.01, 0.0, -0.01)))])
    both = tracker.track([c["scenes"][0]], [0, 0], near, K0, icp_mode=L.FL_ICP_PARITY)
    for i in range(2):
        one = tracker.track([c["scenes"][0]], [0], near[i:i + 1], K0, icp_mode=L.FL_ICP_PARITY)
        assert both[i].tobytes() == one[0].tobytes() and one[0]["tracked"] == 1
    assert both[0].tobytes() != both[1].tobytes()
    # host and device frames
    host = tracker.track(c["scenes"], np.arange(6), c["poses"], K0)
    dev = [torch.from_numpy(s.view(np.int16)).to(f"cuda:{ctx.device}") for s in c["scenes"]]
    torch.cuda.synchronize()
    got = tracker.track(dev, np.arange(6), c["poses"], K0)
    assert got.tobytes() == host.tobytes() and host["tracked"].all()


def test_more_tracks_than_max_tracks_is_refused_and_70_tracks_cross_the_render_chunk(ctx, tracker, mesh, cases):
    c = cases[0]
    with pytest.raises(api.FealessError) as e:
        tracker.track(c["scenes"], np.zeros(9, np.int32), np.tile(c["poses"][0], (9, 1)), K0)
    assert e.value.code == L.FL_ERR_INVALID
    with pytest.raises(api.FealessError) as e:
        tracker.track(c["scenes"] * 2, np.zeros(2, np.int32), c["poses"][:2], K0)              # 12 frames, max_frames = 8
    assert e.value.code == L.FL_ERR_INVALID
    # the rasteriser takes 64 views per launch: 70 tracks go through in two chunks
    big = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], W, H, 6, 70, MAX_CROP)
    try:
        idx = np.arange(70) % 6
        got = big.track(c["scenes"], idx, c["poses"][idx], K0, icp_mode=L.FL_ICP_PARITY)
    finally:
        big.close()
    for t in range(70):
        _same_as_parity_model(got[t], c["exp"][idx[t]])


# ---- 4. point-to-plane mode against its model ---------------------------------------------------------------------------------
def _gt(k, tz0=720.0):
    return synth.object_pose(10 + MOTION_T[0] * k, -5 + MOTION_T[1] * k, tz0 + MOTION_T[2] * k, 0.3 + MOTION_A[0] * k, 0.35 + MOTION_A[1] * k,
                             0.1 + MOTION_A[2] * k)


@pytest.fixture(scope="module")
def sequence():
    """Six frames of the object moving by MOTION_T / MOTION_A per frame from frame 0's pose, noise and background on."""
    return [dict(R=_gt(k)[0], t=_gt(k)[1], scene=synth.render(W, H, *_gt(k), seed=100 + k)[0]) for k in range(7)]


def test_point_to_plane_steps_against_the_model(ctx, tracker, mesh, sequence):
    """Four steps of one sequence; per step the GPU and p2plane_model start from the SAME input pose (the previous GPU result),
    and agree within the tolerances tests/test_gpu_icp.py holds that mode to against that model: 0.02 degrees, 0.05 mm."""
    pose = synth.pose13(sequence[0]["R"], sequence[0]["t"])
    for k in range(1, 5):
        exp = TM.step(mesh, pose, sequence[k]["scene"], K0, max_crop_px=MAX_CROP)
        assert exp["tracked"] == 1
        for w in (1024, 256):
            with util.options(ctx, {"icp_wide": 1 if w == 1024 else 0, "icp_occ": 0}):
                got = tracker.track([sequence[k]["scene"]], [0], pose[None], K0)[0]
            _same_rects(got, exp)
            assert got["det"]["n_points"] == exp["det"]["n_points"], (k, w)
            print(f"step {k} width {w}: iters {got['det']['icp']['iters']} / {exp['det']['icp']['iters']}, rotation "
                  f"{_angle_deg(got['det']['R_final'], exp['det']['R_final']):.4f} deg, T {np.abs(got['det']['T_final'] - exp['det']['T_final']).max():.4f} mm")
            assert _angle_deg(got["det"]["R_final"], exp["det"]["R_final"]) <= 0.02, (k, w)
            assert np.abs(got["det"]["T_final"] - exp["det"]["T_final"]).max() <= 0.05, (k, w)
            assert np.array_equal(got["pose"].reshape(4, 4)[:3, :3].ravel(), got["det"]["R_final"])
            assert np.array_equal(got["pose"].reshape(4, 4)[:3, 3], got["det"]["T_final"])
        pose = api.poses13_of(got)[0]


# ---- 5. passes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [L.FL_ICP_PARITY, L.FL_ICP_POINT_TO_PLANE])
def test_two_passes_equal_two_chained_calls(tracker, cases, mode):
    c = cases[0]
    poses = np.concatenate([c["poses"][:4], _p13(LOST_POSE)[None]])
    scenes = c["scenes"][:4] + [c["scenes"][0]]
    first = tracker.track(scenes, np.arange(5), poses, K0, icp_mode=mode)
    assert first["tracked"].tolist() == [1, 1, 1, 1, 0]
    second = tracker.track(scenes[:4], np.arange(4), api.poses13_of(first[:4]), K0, icp_mode=mode)
    twice = tracker.track(scenes, np.arange(5), poses, K0, icp_mode=mode, passes=2)
    assert second["tracked"].all() and twice[:4].tobytes() == second.tobytes()
    assert not np.array_equal(first["pose"][:4], second["pose"])                     # the second pass did move the poses
    # lost in pass 1: the input pose, and the record of the pass that lost it
    assert twice[4].tobytes() == first[4].tobytes() and twice[4]["tracked"] == 0
    assert np.array_equal(twice[4]["pose"].reshape(4, 4), TM.pose4x4(poses[4]))


# ---- 6. it tracks -------------------------------------------------------------------------------------------------------------
def test_point_to_plane_tracks_a_moving_object(tracker, sequence):
    """The object moves by (4, -2, 3) mm and (0.02, -0.01, 0.015) rad of yaw / tilt / roll per frame (1.5 degrees, 5.4 mm), six
    frames from frame 0's true pose, noise and background on, point-to-plane, passes = 2.  On every frame the pose error
    against ground truth is smaller after the step than before it, in rotation and in translation, and after the last frame
    it is no larger than one frame's motion.

    tests/track_model.py on the CPU, this sequence (rotation error in degrees / translation error in mm, before -> after):
      frame 1  1.75 / 5.39 -> 0.49 / 0.86      frame 4  2.25 / 6.25 -> 0.99 / 0.95
      frame 2  2.15 / 6.23 -> 0.67 / 0.86      frame 5  2.28 / 6.32 -> 1.11 / 1.01
      frame 3  2.27 / 6.23 -> 0.77 / 0.88      frame 6  2.34 / 6.37 -> 1.16 / 0.90
    so the model meets both conditions with room (the last frame's 1.16 degrees / 0.90 mm against a motion of 1.54 / 5.39).

    The same loop in FL_ICP_PARITY is NOT asserted to track, because the reference's point-to-point ICP does not: each step
    removes about a tenth of the gap, so the error grows with the motion.  The model with oracle_py.detection, passes = 2:
    1.75 / 5.39 -> 1.60 / 3.41 on frame 1, then 3.33 / 8.63 -> 3.07 / 6.10, 4.79 / 11.10 -> 4.51 / 8.82, ... and
    8.90 / 19.01 -> 8.05 / 17.01 on frame 6 (DESIGN.md section 0, rows f "next" rank 4 and f5)."""
    pose = synth.pose13(sequence[0]["R"], sequence[0]["t"])
    motion = TM.pose_error(TM.pose4x4(pose), sequence[1]["R"], sequence[1]["t"])
    for k in range(1, 7):
        before = TM.pose_error(TM.pose4x4(pose), sequence[k]["R"], sequence[k]["t"])
        got = tracker.track([sequence[k]["scene"]], [0], pose[None], K0, passes=2)[0]
        after = TM.pose_error(got["pose"].reshape(4, 4), sequence[k]["R"], sequence[k]["t"])
        print(f"frame {k}: {before[0]:.2f} deg / {before[1]:.2f} mm -> {after[0]:.2f} deg / {after[1]:.2f} mm, dist_mean {got['det']['icp']['dist_mean']:.3f}")
        assert got["tracked"] == 1 and got["status"] == 0
        assert after[0] < before[0] and after[1] < before[1], (k, before, after)
        pose = api.poses13_of(got)[0]
    assert after[0] <= motion[0] and after[1] <= motion[1], (after, motion)


# ---- 7. lost ------------------------------------------------------------------------------------------------------------------
def test_a_frame_without_the_object_is_lost_only_with_the_gate(tracker, sequence):
    """A frame that holds only the background, a plane 740 mm away (inside the 900 mm detection() keeps, so the ICP has points
    to converge on).  tests/track_model.py on the CPU, point-to-plane, one pass, the default thresholds: icp.dist_mean is
    4.24 - 5.46 on the six frames of the tracked sequence and 21.5 on the empty frame (18.4 - 24.4 for planes 700 - 820 mm
    away), so max_dist_mean = 10 -- about the geometric middle -- separates them.  With the gates off the empty frame
    counts as tracked: the ICP always returns some pose, which is what the gates are for."""
    pose = synth.pose13(sequence[0]["R"], sequence[0]["t"])
    empty = synth.render(W, H, sequence[0]["R"], np.array([0.0, 0.0, -500.0]), seed=7, plane_z=740.0)[0]
    assert (np.abs(empty.astype(np.int32) - 740) <= 1).all()
    gated = tracker.track([empty, sequence[1]["scene"]], [0, 1], np.stack([pose, pose]), K0, max_dist_mean=10.0)
    print("dist_mean: empty frame", gated[0]["det"]["icp"]["dist_mean"], "tracked frame", gated[1]["det"]["icp"]["dist_mean"])
    assert gated["tracked"].tolist() == [0, 1] and gated["status"].tolist() == [0, 0]
    assert gated[0]["det"]["icp"]["dist_mean"] > 10.0 > gated[1]["det"]["icp"]["dist_mean"] > 0
    assert np.array_equal(gated[0]["pose"].reshape(4, 4), TM.pose4x4(pose))
    free = tracker.track([empty], [0], pose[None], K0)
    assert free[0]["tracked"] == 1 and free[0]["det"]["icp"]["dist_mean"] == gated[0]["det"]["icp"]["dist_mean"]
    # the other gate: a px_ratio no result reaches
    assert tracker.track([sequence[1]["scene"]], [0], pose[None], K0, min_px_ratio=1.5)[0]["tracked"] == 0


# ---- 8. the facade ------------------------------------------------------------------------------------------------------------


def test_facade_track_equals_fl_track_batch(ctx, mesh, sequence, tmp_path):
    cad = cadreco_py.lib()
    obj = str(tmp_path / "object.obj")
    synth.write_obj(obj, mesh)

    def track(h, depth, poses16, n=None, ts=0.0):
        p = np.ascontiguousarray(poses16, np.float32).copy()
        n = len(p) if n is None else n
        trk = np.full(max(1, n), -7, np.int32)
        rc = cad.cadreco_track(h, *cadreco_py.frame_args(depth, ts, K0), n, p.ctypes.data, trk.ctypes.data)
        return rc, p, trk[:n]

    with cadreco_py.handle() as h:
        p0 = TM.pose4x4(synth.pose13(sequence[0]["R"], sequence[0]["t"]))[None]
        scene1 = sequence[1]["scene"]
        assert track(h, scene1, p0)[0] == INVALID                                   # no mesh yet
        assert cad.cadreco_set_tracking_mesh(h, str(tmp_path / "missing.obj").encode(), 1.0) == OPEN_FAILED
        assert cad.cadreco_set_tracking_mesh(h, obj.encode(), 0.0) == INVALID
        assert cad.cadreco_set_tracking_mesh(h, obj.encode(), 1.0) == 0
        assert track(h, np.zeros((240, 320), np.uint16), p0)[0] == INVALID          # frames must be 640 x 480
        assert track(h, scene1, p0, ts=-1.0)[0] == INVALID                          # CheckTImage: a negative timestamp
        assert track(h, scene1, np.tile(p0, (17, 1, 1)))[0] == INVALID              # more than FEALESS_TRACK_MAX_OBJECTS
        assert track(h, scene1, p0, n=0)[0] == 0
        # the mesh as the facade reads it
        V, _, T = cadreco_py.read_obj(obj)
        ref = api.Tracker(ctx, V, T, W, H, 1, 16, 320 * 240)
        try:
            lost = TM.pose4x4(_p13(LOST_POSE))[None]
            poses = np.concatenate([p0, lost])
            for k in (1, 2):
                rc, out, trk = track(h, sequence[k]["scene"], poses)
                exp = ref.track([sequence[k]["scene"]], [0, 0], poses, K0)
                assert rc == 0 and trk.tolist() == exp["tracked"].tolist() == [1, 0]
                assert np.array_equal(_bits(out).reshape(2, 16), _bits(exp["pose"]))
                assert np.array_equal(out[1], lost[0])                              # a lost entry keeps its pose
                poses = out
        finally:
            ref.close()
