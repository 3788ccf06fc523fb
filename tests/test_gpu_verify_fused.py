"""GPU: fl_verify_batch with the context option verify_fused = 1 (k_verify_fused: the mesh rendered into a workgroup's LDS and
scored there, band by band) against tests/verify_model.py and against the same call with verify_fused = 0.

Every field of every record equals both, bit for bit, whatever the band budget (verify_fused_px): a pixel's depth is the
minimum over the triangles that cover it, and that does not depend on which band the pixel falls in.  The compiled budget is
36864 pixels, so a 640 x 480 window takes nine bands and an object's own window one; the smaller budgets below move the band
boundaries through the object, down to one 64-pixel piece of a row per band.
"""
import numpy as np
import pytest

import verify_model as VM
from fealess_amd import api, synth
from util import options, p13 as _p13, pose as _pose

pytestmark = pytest.mark.gpu

BUDGET = 36864                                  # FL_VERIFY_FUSED_PX
W, H = 640, 480
K0 = (608.0, 608.0, 320.0, 240.0)
KS = (152.0, 152.0, 80.0, 60.0)                 # the same field of view at 160 x 120
WS, HS = 160, 120
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
    return [synth.render(W, H, *_pose(p), seed=40 + i)[0] for i, p in enumerate(POSES)]


def _same(got, exp):
    assert len(got) == len(exp)
    for i in range(len(exp)):
        for name in VM.DTYPE.names:
            assert np.array_equal(got[name][i], exp[name][i]), (i, name, got[i], exp[i])
    assert got.tobytes() == exp.tobytes()
    assert VM.invariant(got)


def _fused(ctx, trk, exp, *args, px=(0,), **kw):
    """The call with verify_fused = 1 at every budget of px, each against the model's records and against the call with
    verify_fused = 0."""
    with options(ctx, {"verify_fused": 0}):
        plain = trk.verify(*args, **kw)
    _same(plain, exp)
    for b in px:
        with options(ctx, {"verify_fused": 1, "verify_fused_px": b}):
            got = trk.verify(*args, **kw)
        _same(got, exp)
        assert got.tobytes() == plain.tobytes(), b


# ---- 1. right and wrong poses -------------------------------------------------------------------------------------------------
def test_six_poses_and_a_wrong_pose_each(ctx, tracker, mesh, scenes):
    poses = np.stack([_p13(p, off) for p in POSES for off in (((0, 0, 0), (0, 0, 0)), YAW)])
    fof = np.repeat(np.arange(6), 2)
    exp = VM.verify(mesh, scenes, fof, poses, K0)
    assert (exp["n_model"] > 5000).all() and (exp["accepted"] == 1).all()
    _fused(ctx, tracker, exp, scenes, fof, poses, K0)


# ---- 2. the band's edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0, 10, 65535])
def test_inlier_band_edges(ctx, tracker, mesh, tau):
    """scene = render + a pattern that cycles through -tau-1, -tau, 0, +tau, +tau+1 and "missing", then a frame of all 65535
    against a near render: all inliers at tau = 65535, where sum_abs_inlier passes 2^32 (a 64-bit sum in the kernel)."""
    poses = np.stack([_p13(POSES[0]), _p13((0, 0, 300, 0.3, 0.35, 0.1))])
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
    for i in (0, 1):
        assert exp["n_missing"][i] > 0 and exp["n_inlier"][i] > 0
        assert (exp["n_front"][i] > 0 and exp["n_behind"][i] > 0) == (tau < 65535)
    assert exp["n_model"][3] > 50000 and (tau < 65535 or exp["sum_abs_inlier"][3] > 2 ** 32)
    _fused(ctx, tracker, exp, frames, fof, p4, K0, tau_mm=tau)


# ---- 3. other image sizes -----------------------------------------------------------------------------------------------------
def test_322_by_250_and_a_mesh_across_the_camera_plane(ctx, mesh):
    """An odd image size; and a pose that puts the camera inside the object: triangles with a vertex at z <= 0 have the whole
    image for their box, so the window is the image, 80500 pixels = three bands of the compiled budget."""
    w, h = 322, 250
    p = (-150, -100, 700, 0.3, 0.35, 0.1)
    across = _p13((0, 0, 30, 0.3, 0.35, 0.1))
    poses = np.stack([_p13(p), _p13(p, MOTION), _p13((20, 10, 700, 0.3, 0.35, 0.1)), _p13((5000, 0, 700, 0.3, 0.35, 0.1)), across])
    scene = synth.render(w, h, *_pose(p), seed=71)[0]
    scene[200:, :] = 0
    fof = np.zeros(5, np.int32)
    exp = VM.verify(mesh, [scene], fof, poses, K0)
    v = mesh["vertices"].astype(np.float32)
    z = ((across[8] * v[:, 0] + across[9] * v[:, 1]) + across[10] * v[:, 2]) + across[11]
    assert (z <= 0).any() and (z > 0).any() and exp["n_model"][4] > 0 and w * h > 2 * BUDGET
    assert exp["n_model"][2] > 0 and exp["n_missing"][2] > 0 and exp["n_model"][3] == 0
    assert exp["rect"][2][1] + exp["rect"][2][3] == h
    t = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], w, h, 1, 5, 1000)
    try:
        _fused(ctx, t, exp, [scene], fof, poses, K0, px=(0, 4096))
    finally:
        t.close()


def test_64_by_48(ctx, mesh):
    w, h, K = 64, 48, (60.8, 60.8, 32.0, 24.0)
    poses = np.stack([_p13(POSES[3]), _p13(POSES[3], SHIFT)])
    scene = synth.render(w, h, *_pose(POSES[3]), seed=5, fx=K[0], fy=K[1], cx=K[2], cy=K[3])[0]
    exp = VM.verify(mesh, [scene], [0, 0], poses, K)
    assert exp["n_model"][0] > 50 and exp["inlier_ratio"][0] > 0.8 > exp["inlier_ratio"][1]
    t = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], w, h, 1, 2, 100)
    try:
        _fused(ctx, t, exp, [scene], [0, 0], poses, K, px=(0, 64))
    finally:
        t.close()


# ---- 4. borders, out of view, behind the camera; another camera ----------------------------------------------------------------
def test_poses_at_the_borders_out_of_view_and_behind_the_camera(ctx, tracker, mesh, scenes):
    partly = [(-360, 0, 720, 0.3, 0.35, 0.1), (360, 0, 720, 0.3, 0.35, 0.1), (0, -270, 720, 0.3, 0.35, 0.1), (0, 270, 720, 0.3, 0.35, 0.1),
              (-350, -260, 720, 0.3, 0.35, 0.1), (350, 265, 700, 0.3, 0.35, 0.1)]
    gone = [(900, 0, 720, 0.3, 0.35, 0.1), (0, 0, -720, 0.3, 0.35, 0.1)]
    poses = np.stack([_p13(p) for p in partly + gone])
    fof = np.zeros(8, np.int32)
    exp = VM.verify(mesh, scenes[:1], fof, poses, K0)
    for i in range(6):
        x, y, w, h = exp["rect"][i]
        assert exp["n_model"][i] > 0 and (x == 0 or y == 0 or x + w == W or y + h == H), i
    for i in (6, 7):
        assert exp[i].tobytes() == bytes(64)
    _fused(ctx, tracker, exp, scenes[:1], fof, poses, K0)


def test_scene_camera_other_than_the_model_camera(ctx, tracker, mesh):
    K = (600.0, 608.0, 327.4, 234.4)
    ps = [POSES[0], POSES[2], (-250, 40, 700, 0.2, 0.3, 0.1)]
    frames = [synth.render(W, H, *_pose(p), seed=61 + i, fx=K[0], fy=K[1], cx=K[2], cy=K[3])[0] for i, p in enumerate(ps)]
    poses = np.stack([_p13(p) for p in ps])
    exp = VM.verify(mesh, frames, [0, 1, 2], poses, K)
    assert (exp["inlier_ratio"] > 0.99).all()
    _fused(ctx, tracker, exp, frames, [0, 1, 2], poses, K)


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


def test_70_poses_over_three_frames(ctx, small, small_case):
    c = small_case
    assert (c["exp"]["n_model"] > 300).all() and len(set(c["exp"]["n_inlier"].tolist())) > 35
    _fused(ctx, small, c["exp"], c["frames"], c["fof"], c["poses"], KS, px=(0, 640))


def test_device_frames_equal_host_frames(ctx, small, small_case):
    import torch
    c = small_case
    dev = [torch.from_numpy(s.view(np.int16)).to(f"cuda:{ctx.device}") for s in c["frames"]]
    torch.cuda.synchronize()
    with options(ctx, {"verify_fused": 1}):
        host = small.verify(c["frames"], c["fof"][:12], c["poses"][:12], KS)
        got = small.verify(dev, c["fof"][:12], c["poses"][:12], KS)
        single = np.concatenate([small.verify([c["frames"][c["fof"][i]]], [0], c["poses"][i:i + 1], KS) for i in range(12)])
    _same(host, c["exp"][:12])
    assert got.tobytes() == host.tobytes() == single.tobytes()


# ---- 6. groups, with every gate -----------------------------------------------------------------------------------------------
def test_groups_with_every_gate(ctx, tracker, mesh, scenes):
    true, yaw, shift, motion = _p13(POSES[0]), _p13(POSES[0], YAW), _p13(POSES[0], SHIFT), _p13(POSES[0], MOTION)
    poses = np.stack([true, yaw, shift, shift, yaw, true, yaw, shift, motion, motion, true])
    gf = [0, 3, 6, 8, 10, 10, 11]                   # the first wins; the last wins; nobody passes; a tie; empty; a single member
    fof = np.zeros(len(poses), np.int32)
    by_pose = {p.tobytes(): VM.render(mesh, p, K0, W, H) for p in (true, yaw, shift, motion)}
    rend = [by_pose[p.tobytes()] for p in poses]

    def model(**kw):
        return VM.verify(mesh, scenes[:1], fof, poses, K0, renders=rend, **kw)
    free = model()
    lo = (float(free["inlier_ratio"][8]) + float(free["inlier_ratio"][1])) / 2
    hi = (float(free["behind_ratio"][0]) + float(free["behind_ratio"][1])) / 2
    n = int(free["n_model"][0])
    assert free["inlier_ratio"][0] > free["inlier_ratio"][8] > lo > free["inlier_ratio"][1] > free["inlier_ratio"][2]
    assert free["behind_ratio"][8] < hi < free["behind_ratio"][1] < free["behind_ratio"][2]
    exp = model(group_first=gf, min_inlier_ratio=lo)
    assert exp["accepted"].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 1, 1, 1] and exp["best"].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 1, 0, 1]
    _fused(ctx, tracker, exp, scenes[:1], fof, poses, K0, group_first=gf, min_inlier_ratio=lo)
    _fused(ctx, tracker, model(group_first=gf), scenes[:1], fof, poses, K0, group_first=gf)
    _fused(ctx, tracker, model(min_inlier_ratio=lo), scenes[:1], fof, poses, K0, min_inlier_ratio=lo)
    for prm in (dict(max_behind_ratio=hi), dict(min_model_px=n), dict(min_model_px=n + 1)):
        exp = model(group_first=gf, **prm)
        _fused(ctx, tracker, exp, scenes[:1], fof, poses, K0, group_first=gf, **prm)
    assert exp["accepted"][0] == 0 and exp["accepted"].any()


# ---- 7. the band boundaries ---------------------------------------------------------------------------------------------------
def test_band_boundaries_through_the_object(ctx, small, mesh, small_case):
    """160 x 120: the true pose, a near pose whose window is wider than the smallest budget, and a far one, at the compiled
    budget (one band), at a budget whose rows-per-band is below the object's height, and at 64 pixels, one piece of a row per
    band.  The window contains the model's rect, so its width is at least rect's: a band has at most budget // rect_w rows,
    boundaries repeat at that distance from a first row that is not below rect's, and with fewer rows per band than rect has,
    one of them lies between two rows of the object."""
    ps = [(10, -5, 720, 0.30, 0.35, 0.10), (5, 5, 300, 0.30, 0.35, 0.10), (-30, 20, 1400, 0.5, 0.2, 0.3)]
    poses = np.stack([_p13(p) for p in ps])
    frames = small_case["frames"][:1]
    fof = np.zeros(3, np.int32)
    exp = VM.verify(mesh, frames, fof, poses, KS)
    px = 1024
    for i in (0, 1):
        _, _, rw, rh = (int(v) for v in exp["rect"][i])
        assert rw > 0 and 1 <= px // rw < rh, (i, rw, rh)
    assert exp["rect"][1][2] > 64                   # the near pose: a row of its window is cut into pieces at 64
    assert exp["n_model"][2] > 0
    _fused(ctx, small, exp, frames, fof, poses, KS, px=(0, px, 64, 100, BUDGET))


def test_shared_edge_on_a_band_boundary(ctx):
    """Two triangles that share the edge y = 0, seen head-on at z = 512 with K = 128 / 128 / 80 / 60: every number is exact in
    float32.  The corners (0, -/+128) project to rows 28 and 92, (-/+128, 0) to columns 48 and 112 of row 60, so the window is
    columns 47 .. 113 (67 of them) and rows 27 .. 93, and the shared edge lies on the centres of row 60 = window row 33: the
    top-left rule gives each of its pixels to one of the two triangles.  A budget of 33 * 67 ends a band after row 59, 34 * 67 after row 60,
    67 is one window row per band, 64 cuts every row."""
    K = (128.0, 128.0, 80.0, 60.0)
    V = np.array([[-128, 0, 0], [128, 0, 0], [0, -128, 0], [0, 128, 0]], np.float32)
    T = np.array([[0, 1, 2], [1, 0, 3]], np.int32)
    m = dict(vertices=V, triangles=T)
    flat = np.zeros(13, np.float32)
    flat[[0, 5, 10]] = 1
    flat[11] = 512
    tilted = synth.pose13(*synth.object_pose(0, 0, 512, 0.0, 0.2, 0.0))
    poses = np.stack([flat, tilted])
    rend = VM.render(m, flat, K, WS, HS)
    rows, cols = np.flatnonzero(rend.any(axis=1)), np.flatnonzero(rend[60])
    assert rows[0] >= 28 and rows[-1] <= 92 and rend[59].any() and rend[60].any() and rend[61].any()
    assert cols[0] >= 48 and cols[-1] <= 112 and len(cols) > 60 and (rend[rend > 0] == 512).all()
    scene = np.full((HS, WS), 515, np.uint16)
    scene[::3, :] = 530
    scene[:, ::7] = 0
    exp = VM.verify(m, [scene], [0, 0], poses, K, renders=[rend, VM.render(m, tilted, K, WS, HS)])
    assert 0 < exp["n_inlier"][0] < exp["n_model"][0] and exp["n_behind"][0] > 0 and exp["n_missing"][0] > 0
    t = api.Tracker(ctx, V, T, WS, HS, 1, 2, WS * HS)
    try:
        _fused(ctx, t, exp, [scene], [0, 0], poses, K, px=(0, 33 * 67, 34 * 67, 67, 64, 32 * 67 + 5))
    finally:
        t.close()


# ---- 8. the options -----------------------------------------------------------------------------------------------------------
def test_option_ranges(ctx):
    for name, bad, good in (("verify_fused", (-1, 2), (0, 1)), ("verify_fused_px", (-1, 1, 63, BUDGET + 1), (0, 64, 4096, BUDGET))):
        before = ctx.get_option(name)
        for v in bad:
            with pytest.raises(api.FealessError):
                ctx.set_option(name, v)
            assert ctx.get_option(name) == before
        for v in good:
            ctx.set_option(name, v)
            assert ctx.get_option(name) == v
        ctx.set_option(name, before)
