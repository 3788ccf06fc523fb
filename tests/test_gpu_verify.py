"""GPU: fl_verify_batch (api.Tracker.verify) and the facade's CadRecoVerify against tests/verify_model.py.

Every field of every record equals the model bit for bit: the counts are integers, the ratios single float32 divisions, and the
render under them equals tests/raster_model.py.  The image sizes: 640 x 480 = 37.5 strips of k_verify_score (eight pixels per
load, a half-full last strip), 160 x 120 = 2.3 strips, 64 x 48 = less than one strip, and 322 x 250, whose pixel count is no
multiple of eight (the pixel-by-pixel path) and leaves 0.83 of a last strip.
"""
import ctypes as C

import numpy as np
import pytest

import cadreco_py
import track_model as TM
import verify_model as VM
from fealess_amd import _lib as L
from fealess_amd import api, synth
from util import p13 as _p13, pose as _pose

pytestmark = pytest.mark.gpu

W, H = 640, 480
K0 = (608.0, 608.0, 320.0, 240.0)
KS = (152.0, 152.0, 80.0, 60.0)                 # the same field of view at 160 x 120
WS, HS = 160, 120
# (tx, ty, tz, yaw, tilt, roll): the poses of tests/test_gpu_track.py, and that file's one-frame motion
POSES = [(10, -5, 720, 0.30, 0.35, 0.10), (-60, 30, 690, -0.50, 0.20, 0.30), (80, -40, 750, 0.90, 0.50, -0.20),
         (0, 0, 700, 0.00, 0.30, 0.00), (-100, -60, 760, 1.40, 0.10, 0.25), (120, 70, 680, -1.10, 0.45, -0.15)]
MOTION = ((4.0, -2.0, 3.0), (0.02, -0.01, 0.015))
YAW, SHIFT = ((0, 0, 0), (1.0, 0, 0)), ((150, 0, 0), (0, 0, 0))


@pytest.fixture(scope="module")
def mesh():
    return synth.object_mesh(2)


@pytest.fixture(scope="module")
def tracker(ctx, mesh):
    t = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], W, H, 8, 16, 40000)
    yield t
    t.close()


@pytest.fixture(scope="module")
def small(ctx, mesh):
    t = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], WS, HS, 3, 70, WS * HS)
    yield t
    t.close()


@pytest.fixture(scope="module")
def scenes():
    """One scene per entry of POSES (noise and background on), shared and read only."""
    return [synth.render(W, H, *_pose(p), seed=40 + i)[0] for i, p in enumerate(POSES)]


def _same(got, exp):
    """Every field of every record, bit for bit."""
    assert len(got) == len(exp)
    for i in range(len(exp)):
        for name in VM.DTYPE.names:
            assert np.array_equal(got[name][i], exp[name][i]), (i, name, got[i], exp[i])
    assert got.tobytes() == exp.tobytes()
    assert VM.invariant(got)


# ---- 1. right and wrong poses -------------------------------------------------------------------------------------------------
def test_six_poses_and_a_wrong_pose_each(tracker, mesh, scenes):
    poses = np.stack([_p13(p, off) for p in POSES for off in (((0, 0, 0), (0, 0, 0)), YAW)])
    fof = np.repeat(np.arange(6), 2)
    exp = VM.verify(mesh, scenes, fof, poses, K0)
    got = tracker.verify(scenes, fof, poses, K0)
    print(got)
    _same(got, exp)
    for i in range(6):
        assert exp["n_model"][2 * i] > 5000 and exp["inlier_ratio"][2 * i] > 0.99 > 0.5 > exp["inlier_ratio"][2 * i + 1]
        assert exp["behind_ratio"][2 * i] < 0.01 < exp["behind_ratio"][2 * i + 1]
    assert (got["status"] == 0).all() and (got["accepted"] == 1).all() and (got["best"] == 1).all()


# ---- 2. the band's edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0, 10, 65535])
def test_band_edges(tracker, mesh, tau):
    """scene = render + a pattern that cycles through -tau-1, -tau, 0, +tau, +tau+1 and "missing" (clipped to 1..65535, so at
    tau = 65535 every pixel that has depth is an inlier), then a frame of all 65535 against the near render: seen through
    everywhere at tau 0 and 10 -- |d| does not wrap in 16 bits -- and all inliers at 65535, where sum_abs_inlier passes 2^32."""
    near = _p13((0, 0, 300, 0.3, 0.35, 0.1))
    poses = np.stack([_p13(POSES[0]), near])
    rend = [VM.render(mesh, p, K0, W, H) for p in poses]
    idx = np.arange(W * H).reshape(H, W)
    pat = np.array([-tau - 1, -tau, 0, tau, tau + 1, 0], np.int64)[idx % 6]
    frames = []
    for r in rend:
        s = np.where(r > 0, np.clip(r.astype(np.int64) + pat, 1, 65535), 1200)
        s[(idx % 6 == 5) & (r > 0)] = 0
        frames.append(s.astype(np.uint16))
    frames.append(np.full((H, W), 65535, np.uint16))
    fof = [0, 1, 2, 2]
    p4 = np.stack([poses[0], poses[1], poses[0], poses[1]])
    exp = VM.verify(mesh, frames, fof, p4, K0, renders=[rend[0], rend[1], rend[0], rend[1]], tau_mm=tau)
    got = tracker.verify(frames, fof, p4, K0, tau_mm=tau)
    print(got)
    _same(got, exp)
    for i in (0, 1):
        assert exp["n_missing"][i] > 0 and exp["n_inlier"][i] > 0
        assert (exp["n_front"][i] > 0 and exp["n_behind"][i] > 0) == (tau < 65535)
    for i in (2, 3):
        n = int(exp["n_model"][i])
        if tau < 65535:
            assert exp["n_behind"][i] == n and exp["sum_abs_inlier"][i] == 0
        else:
            assert exp["n_inlier"][i] == n
    assert exp["n_model"][3] > 50000 and (tau < 65535 or exp["sum_abs_inlier"][3] > 2 ** 32)


# ---- 3. other image sizes -----------------------------------------------------------------------------------------------------
def test_image_whose_pixel_count_is_no_multiple_of_eight(ctx, mesh):
    w, h = 322, 250
    assert (w * h) % 8 != 0 and (w * h) % 8192 != 0
    p = (-150, -100, 700, 0.3, 0.35, 0.1)
    poses = np.stack([_p13(p), _p13(p, MOTION), _p13((20, 10, 700, 0.3, 0.35, 0.1)), _p13((5000, 0, 700, 0.3, 0.35, 0.1))])
    scene = synth.render(w, h, *_pose(p), seed=71)[0]
    scene[200:, :] = 0                                                              # a band without depth, the last rows included
    t = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], w, h, 1, 4, 1000)
    try:
        got = t.verify([scene], [0, 0, 0, 0], poses, K0)
    finally:
        t.close()
    exp = VM.verify(mesh, [scene], [0, 0, 0, 0], poses, K0)
    print(got)
    _same(got, exp)
    assert exp["n_inlier"][0] + exp["n_missing"][0] > 0.99 * exp["n_model"][0] and 0 < exp["n_missing"][0] < 0.1 * exp["n_model"][0]
    assert exp["n_model"][2] > 0 and exp["n_missing"][2] > 0 and exp["n_model"][3] == 0
    assert exp["rect"][2][1] + exp["rect"][2][3] == h                               # the third pose reaches the last row


def test_image_smaller_than_one_strip(ctx, mesh):
    w, h, K = 64, 48, (60.8, 60.8, 32.0, 24.0)
    poses = np.stack([_p13(POSES[3]), _p13(POSES[3], SHIFT)])
    scene = synth.render(w, h, *_pose(POSES[3]), seed=5, fx=K[0], fy=K[1], cx=K[2], cy=K[3])[0]
    t = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], w, h, 1, 2, 100)
    try:
        got = t.verify([scene], [0, 0], poses, K)
    finally:
        t.close()
    exp = VM.verify(mesh, [scene], [0, 0], poses, K)
    _same(got, exp)
    assert exp["n_model"][0] > 50 and exp["inlier_ratio"][0] > 0.8 > exp["inlier_ratio"][1]


# ---- 4. borders, out of view, behind the camera; another camera ----------------------------------------------------------------
def test_poses_at_the_borders_out_of_view_and_behind_the_camera(tracker, mesh, scenes):
    partly = [(-360, 0, 720, 0.3, 0.35, 0.1), (360, 0, 720, 0.3, 0.35, 0.1), (0, -270, 720, 0.3, 0.35, 0.1), (0, 270, 720, 0.3, 0.35, 0.1),
              (-350, -260, 720, 0.3, 0.35, 0.1), (350, 265, 700, 0.3, 0.35, 0.1)]
    gone = [(900, 0, 720, 0.3, 0.35, 0.1), (0, 0, -720, 0.3, 0.35, 0.1)]           # out of view; behind the camera
    poses = np.stack([_p13(p) for p in partly + gone])
    fof = np.zeros(8, np.int32)
    exp = VM.verify(mesh, scenes[:1], fof, poses, K0)
    got = tracker.verify(scenes[:1], fof, poses, K0)
    _same(got, exp)
    for i in range(6):
        x, y, w, h = exp["rect"][i]
        assert exp["n_model"][i] > 0 and (x == 0 or y == 0 or x + w == W or y + h == H), i
    assert exp["rect"][4][0] == 0 and exp["rect"][4][1] == 0 and exp["rect"][5][0] + exp["rect"][5][2] == W and exp["rect"][5][1] + exp["rect"][5][3] == H
    for i in (6, 7):                                                               # status FL_OK, not accepted, everything zero
        assert got[i].tobytes() == bytes(64)


def test_scene_camera_other_than_the_model_camera(tracker, mesh):
    """fx = 600 and cx, cy moved by (+7.4, -5.6): the render uses that camera, so the true pose still lies on its frame."""
    K = (600.0, 608.0, 327.4, 234.4)
    ps = [POSES[0], POSES[2], (-250, 40, 700, 0.2, 0.3, 0.1)]
    frames = [synth.render(W, H, *_pose(p), seed=61 + i, fx=K[0], fy=K[1], cx=K[2], cy=K[3])[0] for i, p in enumerate(ps)]
    poses = np.stack([_p13(p) for p in ps])
    exp = VM.verify(mesh, frames, [0, 1, 2], poses, K)
    got = tracker.verify(frames, [0, 1, 2], poses, K)
    _same(got, exp)
    assert (exp["inlier_ratio"] > 0.99).all()
    at_model_k = VM.verify(mesh, frames, [0, 1, 2], poses, K0)
    assert (at_model_k["inlier_ratio"] < 0.95).all() and not np.array_equal(at_model_k["rect"], exp["rect"])   # K matters here


# ---- 5. batch structure -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_case(mesh):
    """Three 160 x 120 frames and 70 poses spread over them: every frame's true pose and perturbations of it."""
    ps = [(10, -5, 720, 0.30, 0.35, 0.10), (-60, 30, 690, -0.50, 0.20, 0.30), (80, -40, 750, 0.90, 0.50, -0.20)]
    frames = [synth.render(WS, HS, *_pose(p), seed=80 + i, fx=KS[0], fy=KS[1], cx=KS[2], cy=KS[3])[0] for i, p in enumerate(ps)]
    rng = np.random.default_rng(11)
    fof = (np.arange(70) * 7 % 3).astype(np.int32)
    poses = []
    for t in range(70):
        off = ((0, 0, 0), (0, 0, 0)) if t < 3 else (tuple(rng.uniform(-40, 40, 3)), tuple(rng.uniform(-0.5, 0.5, 3)))
        poses.append(_p13(ps[fof[t]], off))
    poses = np.stack(poses)
    return dict(frames=frames, fof=fof, poses=poses, exp=VM.verify(mesh, frames, fof, poses, KS))


def test_70_poses_cross_the_render_chunk_over_three_frames(small, small_case):
    c = small_case
    got = small.verify(c["frames"], c["fof"], c["poses"], KS)
    _same(got, c["exp"])
    assert (c["exp"]["n_model"] > 300).all() and len(set(c["exp"]["n_inlier"].tolist())) > 35
    assert (c["exp"]["inlier_ratio"][:3] > 0.9).all()


def test_batch_equals_single_calls_and_device_frames_equal_host_frames(ctx, small, small_case):
    import torch
    c = small_case
    batch = small.verify(c["frames"], c["fof"][:12], c["poses"][:12], KS)
    _same(batch, c["exp"][:12])
    single = np.concatenate([small.verify([c["frames"][c["fof"][i]]], [0], c["poses"][i:i + 1], KS) for i in range(12)])
    assert single.tobytes() == batch.tobytes()
    dev = [torch.from_numpy(s.view(np.int16)).to(f"cuda:{ctx.device}") for s in c["frames"]]
    torch.cuda.synchronize()
    assert small.verify(dev, c["fof"][:12], c["poses"][:12], KS).tobytes() == batch.tobytes()
    # (n, 4, 4) poses are the same poses
    p4 = np.zeros((12, 4, 4), np.float32)
    p4[:, :3, :] = c["poses"][:12, :12].reshape(12, 3, 4)
    p4[:, 3, 3] = 1
    assert small.verify(c["frames"], c["fof"][:12], p4, KS).tobytes() == batch.tobytes()


# ---- 6. groups ----------------------------------------------------------------------------------------------------------------
def test_groups(tracker, mesh, scenes):
    true, yaw, shift, motion = _p13(POSES[0]), _p13(POSES[0], YAW), _p13(POSES[0], SHIFT), _p13(POSES[0], MOTION)
    poses = np.stack([true, yaw, shift,             # group 0: the first wins
                      shift, yaw, true,             # group 1: the last wins
                      yaw, shift,                   # group 2: nobody passes the gate
                      motion, motion,               # group 3: an exact tie, the lower index wins
                      true])                        # group 5 (4 is empty): a single member
    gf = [0, 3, 6, 8, 10, 10, 11]
    fof = np.zeros(len(poses), np.int32)
    by_pose = {p.tobytes(): VM.render(mesh, p, K0, W, H) for p in (true, yaw, shift, motion)}
    rend = [by_pose[p.tobytes()] for p in poses]

    def model(**kw):
        return VM.verify(mesh, scenes[:1], fof, poses, K0, renders=rend, **kw)
    free = model()
    lo = (float(free["inlier_ratio"][8]) + float(free["inlier_ratio"][1])) / 2       # between one frame of motion and the wrong yaw
    assert free["inlier_ratio"][0] > free["inlier_ratio"][8] > lo > free["inlier_ratio"][1] > free["inlier_ratio"][2]
    exp = model(group_first=gf, min_inlier_ratio=lo)
    assert exp["accepted"].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 1, 1, 1] and exp["best"].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 1, 0, 1]
    got = tracker.verify(scenes[:1], fof, poses, K0, group_first=gf, min_inlier_ratio=lo)
    _same(got, exp)
    # without the gate everyone is accepted and the same members win, except in group 2, where the yaw beats the shift
    exp = model(group_first=gf)
    assert exp["best"].tolist() == [1, 0, 0, 0, 0, 1, 1, 0, 1, 0, 1]
    _same(tracker.verify(scenes[:1], fof, poses, K0, group_first=gf), exp)
    # no groups: best = accepted; one group over everything: the first of the equal true poses
    _same(tracker.verify(scenes[:1], fof, poses, K0, min_inlier_ratio=lo), model(min_inlier_ratio=lo))
    one = tracker.verify(scenes[:1], fof, poses, K0, group_first=[0, len(poses)])
    assert one["best"].tolist() == [1] + [0] * 10
    # the other gates
    hi = (float(free["behind_ratio"][0]) + float(free["behind_ratio"][1])) / 2
    assert free["behind_ratio"][8] < hi < free["behind_ratio"][1] < free["behind_ratio"][2]
    n = int(free["n_model"][0])
    for prm in (dict(max_behind_ratio=hi), dict(min_model_px=n), dict(min_model_px=n + 1)):
        exp = model(group_first=gf, **prm)
        _same(tracker.verify(scenes[:1], fof, poses, K0, group_first=gf, **prm), exp)
    assert exp["accepted"][0] == 0 and exp["accepted"].any()                       # other poses render more pixels than the true one


# ---- 7. beside tracking -------------------------------------------------------------------------------------------------------
def test_tracking_is_unchanged_by_a_verify_call_between(tracker, mesh, scenes):
    """fl_verify_batch uses the tracker's frame slots and render images; fl_track_batch stages both again on every call."""
    poses = np.stack([_p13(p, MOTION) for p in POSES])
    before = tracker.track(scenes, np.arange(6), poses, K0)
    assert before["tracked"].all()
    got = tracker.verify(scenes[::-1], np.arange(6), poses[::-1], K0)
    _same(got, VM.verify(mesh, scenes[::-1], np.arange(6), poses[::-1], K0))
    after = tracker.track(scenes, np.arange(6), poses, K0)
    assert after.tobytes() == before.tobytes()
    # the tracked poses feed straight in, and fit their frames better than the poses the tracks came in with
    moved = tracker.verify(scenes, np.arange(6), after["pose"].reshape(-1, 4, 4), K0)
    _same(moved, VM.verify(mesh, scenes, np.arange(6), api.poses13_of(after), K0))
    assert (moved["inlier_ratio"] > got["inlier_ratio"][::-1]).all()


def test_verification_is_unchanged_by_a_tracking_call_between(small, mesh, small_case):
    """The other direction: fl_track_batch leaves its renders x 10 in the images verification renders into, its own poses and
    frame indices in the arrays both stage through, and the frames in the slots.  Three tracks, two passes, at poses the MODEL
    camera (608 / 608 / 320 / 240, which is what fl_track_batch renders with) sees inside the 160 x 120 image: t = (-276, -207,
    700) mm projects to (80, 60).  Then the same verification again, and a shorter one without groups: stale groups, stale
    poses beyond n and stale accumulators would all show."""
    c = small_case
    gf = [0, 5, 5, 12]
    exp = VM.pick(c["exp"][:12].copy(), gf)
    v1 = small.verify(c["frames"], c["fof"][:12], c["poses"][:12], KS, group_first=gf)
    _same(v1, exp)
    assert exp["best"].sum() == 2 and exp["accepted"].sum() > 2                     # the pick did choose
    # the tracks' frames show the object where their poses put it, through the model camera: both passes then have something
    # to hold on to (track_model.step on these frames, two chained steps: tracked, dist_mean 0.99 - 1.06, rects of 157 - 160 x 120)
    ps = [(-276, -207, 700, 0.3, 0.35, 0.1), (-270, -200, 720, -0.5, 0.2, 0.3), (-282, -212, 690, 0.9, 0.5, -0.2)]
    tracks = np.stack([_p13(p) for p in ps])
    fx, fy, cx, cy = TM.MODEL_K
    seen = [synth.render(WS, HS, *_pose(p), seed=90 + i, fx=fx, fy=fy, cx=cx, cy=cy)[0] for i, p in enumerate(ps)]
    for p in tracks:                                                                # on the CPU: the model camera sees them
        r = TM.rects(TM.render(mesh, p, WS, HS), p, TM.MODEL_K, 12)
        assert r is not None and r[0][2] > 0 and r[0][3] > 0
    got = small.track(seen, [1, 2, 0], tracks[[1, 2, 0]], TM.MODEL_K, passes=2)
    print(got[["status", "tracked", "rect_model"]])
    assert (got["rect_model"][:, 2] > 0).all() and (got["rect_model"][:, 3] > 0).all()
    v2 = small.verify(c["frames"], c["fof"][:12], c["poses"][:12], KS, group_first=gf)
    assert v1.tobytes() == v2.tobytes()
    _same(v2, exp)
    _same(small.verify(c["frames"], c["fof"][:5], c["poses"][:5], KS), c["exp"][:5])


def test_more_poses_than_max_tracks_is_refused(tracker, scenes):
    with pytest.raises(api.FealessError) as e:
        tracker.verify(scenes[:1], np.zeros(17, np.int32), np.tile(_p13(POSES[0]), (17, 1)), K0)
    assert e.value.code == L.FL_ERR_INVALID
    with pytest.raises(TypeError):
        tracker.verify(scenes[:1], [0], _p13(POSES[0])[None], K0, tau=3)


# ---- 8. the facade ------------------------------------------------------------------------------------------------------------
INVALID = cadreco_py.INVALID
FACADE_RESULT = np.dtype([("accepted", "<i4"), ("n_model", "<i4"), ("n_missing", "<i4"), ("n_inlier", "<i4"), ("n_front", "<i4"), ("n_behind", "<i4"),
                          ("inlier_ratio", "<f4"), ("behind_ratio", "<f4")])


def test_facade_verify_on_a_recognised_frame(ctx, tmp_path):
    """Train a small bank from the OBJ, recognise a frame through the facade, then CadRecoVerify the recognised pose and the
    same pose moved 150 mm: the records equal the model on the mesh the facade read, and a gate halfway between the model's two
    inlier ratios accepts the first and rejects the second."""
    cad = cadreco_py.lib()
    mesh = synth.object_mesh(2)
    obj = str(tmp_path / "object.obj")
    synth.write_obj(obj, mesh)

    def verify(h, depth, poses16, tau=10.0, n=None, ts=0.0):
        p = np.ascontiguousarray(poses16, np.float32)
        n = len(p) if n is None else n
        out = np.zeros(max(1, n), FACADE_RESULT)
        rc = cad.cadreco_verify(h, *cadreco_py.frame_args(depth, ts, K0), n, p.ctypes.data, tau, out.ctypes.data)
        return rc, out[:n]

    with cadreco_py.handle() as h:
        # train and load, the mesh as the facade reads it, and a frame that shows it at a trained view
        V, N, T, depth, pose = cadreco_py.recognised_mesh_frame(h, ctx, obj, str(tmp_path / "bank"))
        moved = pose.copy()
        moved[3] += 150.0
        poses = np.stack([pose, moved])
        # the facade's limits
        assert verify(h, depth, poses)[0] == INVALID                                # no mesh yet
        assert cad.cadreco_set_tracking_mesh(h, obj.encode(), 1.0) == 0
        assert verify(h, np.zeros((240, 320), np.uint16), poses)[0] == INVALID      # frames must be 640 x 480
        assert verify(h, depth, poses, ts=-1.0)[0] == INVALID                       # CheckTImage: a negative timestamp
        assert verify(h, depth, np.tile(pose, (17, 1)))[0] == INVALID               # more than FEALESS_TRACK_MAX_OBJECTS
        assert verify(h, depth, poses, tau=-1.0)[0] == INVALID and verify(h, depth, poses, tau=65536.0)[0] == INVALID
        assert verify(h, depth, poses, n=0)[0] == 0
        # the records
        rc, got = verify(h, depth, poses)
        p13 = np.zeros((2, 13), np.float32)
        p13[:, :12] = poses[:, :12]
        exp = VM.verify(dict(vertices=V, triangles=T), [depth], [0, 0], p13, K0)
        print(got, exp)
        assert rc == 0
        for name in FACADE_RESULT.names:
            assert np.array_equal(got[name], exp[name]), name
        gate = (float(exp["inlier_ratio"][0]) + float(exp["inlier_ratio"][1])) / 2
        assert exp["inlier_ratio"][0] > gate > exp["inlier_ratio"][1] and exp["inlier_ratio"][0] > 0.9
        assert got["inlier_ratio"][0] >= gate > got["inlier_ratio"][1] and got["accepted"].tolist() == [1, 1]
