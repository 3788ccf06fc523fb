"""GPU: scene arbitration (fl_verify_scene_batch, api.Tracker.verify_scene) and the facade's CadRecoArbitrate against
tests/scene_model.py, the numpy statement of the contract: the records byte for byte, the compact shared array
(dev_scene_shared) entry for entry, and the `verify` part against Tracker.verify on the same tracker.  The shapes are the smallest
at which each piece can go wrong; tests/test_scene_cpu.py has the rule itself and the argument checks.
"""
import ctypes as C

import numpy as np
import pytest

import cadreco_py
import clutter
import meshes as MS
import multiclass
import scene_model as SM
import util
import verify_model as VM
from fealess_amd import _lib as L
from fealess_amd import api, synth
from test_gpu_meshes import SIZES
from test_instances_cpu import MIN_DIST
from test_scene_cpu import HYP, K as KQ, ON, TRUE, real_case
from util import p13 as _p13, pose as _pose

pytestmark = pytest.mark.gpu

IDX = MS.INDEX
KT = (60.8, 60.8, 32.0, 24.0)                    # the camera of the 64 x 48 cases


@pytest.fixture(scope="module")
def meshes():
    ms = MS.all_meshes()
    return [ms[n] for n in MS.ORDER]


def _tracker(ctx, w, h, max_frames=2, max_tracks=70):
    return api.Tracker(ctx, meshes=MS.in_order(MS.all_meshes()), w=w, h=h, max_frames=max_frames, max_tracks=max_tracks, max_crop_px=min(w * h, 1000))


@pytest.fixture(scope="module")
def quarter(ctx):
    t = _tracker(ctx, 160, 120)
    yield t
    t.close()


@pytest.fixture(scope="module")
def tiny(ctx):
    t = _tracker(ctx, 64, 48, max_tracks=140)
    yield t
    t.close()


def _mesh_of(names):
    return np.array([IDX[n] for n in names], np.int32)


def _check(trk, meshes, scenes, fof, poses, K, sf, mesh_of, **params):
    """verify_scene against the model: records, shared array, and the verify part against Tracker.verify.  Returns
    (records, the model's full matrix)."""
    want, sh, M = SM.verify_scene(meshes, scenes, fof, poses, K, sf, mesh_of=mesh_of, **params)
    got = trk.verify_scene(scenes, fof, poses, K, sf, mesh_of=mesh_of, **params)
    dev = trk.dev_scene_shared()
    assert dev.dtype == np.int32 and dev.tolist() == sh.tolist(), (dev, sh)
    assert got.tobytes() == want.tobytes(), (got, want)
    vp = {k: v for k, v in params.items() if k in VM.DEFAULTS}
    assert got["verify"].tobytes() == trk.verify(scenes, fof, poses, K, mesh_of=mesh_of, **vp).tobytes()
    return got, M


# ---- 1. the real case of tests/test_scene_cpu.py ---------------------------------------------------------------------------------
def test_real_case_at_160x120(quarter, meshes):
    _, scene, poses, mesh_of = real_case()
    got, M = _check(quarter, meshes, [scene], [0] * 6, poses, KQ, [0, 6], mesh_of)
    assert got["kept"].tolist() == [1, 0, 0, 0, 1, 0] and [int(got["rival"][t]) for t in (1, 2, 3, 5)] == [0, 0, 0, 4]
    assert M[0, 1] > 700 and M[4, 5] == 1
    assert _check(quarter, meshes, [scene], [0] * 6, poses, KQ, [0, 6], mesh_of, min_shared_px=2)[0]["kept"].tolist() == [1, 0, 0, 0, 1, 1]
    full = _check(quarter, meshes, [scene], [0] * 6, poses, KQ, [0, 6], mesh_of, max_shared_ratio=1.0)[0]
    assert full["kept"].tolist() != got["kept"].tolist()
    # a pose with an empty render, and poses refused by a gate: C (a third of it supported) and D (one pixel of 110)
    gone = np.concatenate([poses, _p13((2000, 0, 720, 0.3, 0.35, 0.1))[None]])
    mo = np.concatenate([mesh_of, [IDX["A"]]]).astype(np.int32)
    g, M = _check(quarter, meshes, [scene], [0] * 7, gone, KQ, [0, 7], mo, min_inlier_ratio=0.5)
    assert g["verify"]["accepted"].tolist() == [1, 1, 1, 0, 1, 0, 0] and g["verify"]["n_model"][6] == 0 and g["verify"]["n_model"][3] > 400
    assert g["order"].tolist() == [1, 2, 3, -1, 0, -1, -1] and g["kept"].tolist() == [1, 0, 0, 0, 1, 0, 0]
    assert (M[3] == 0).all() and (M[5] == 0).all() and (M[6] == 0).all()                  # shared is taken as 0 for them
    # the same poses in another order: the order of the input is not the order of the scene
    perm = np.array([3, 5, 2, 4, 1, 0])
    p = _check(quarter, meshes, [scene], [0] * 6, poses[perm], KQ, [0, 6], mesh_of[perm])[0]
    assert p["kept"].tolist() == got["kept"][perm].tolist() and p["order"].tolist() == got["order"][perm].tolist()


# ---- 2. 322 x 250 (the pixel count is no multiple of eight) and 64 x 48 (a render across the border, a render of a few pixels) ----
@pytest.mark.parametrize("size", ["322x250", "64x48"])
def test_every_mesh_on_two_frames(ctx, meshes, size):
    w, h, K, ps = SIZES[size]
    scenes = [synth.render(w, h, *_pose(p), seed=11 + i, fx=K[0], fy=K[1], cx=K[2], cy=K[3])[0] for i, p in enumerate(ps)]
    names = list("ABCDA") * 2                                                            # per frame: every mesh, and A moved
    fof = np.repeat([0, 1], 5).astype(np.int32)
    poses = np.stack([_p13(ps[f], ((2, 0, 1), (0, 0, 0)) if k % 5 == 4 else ((0, 0, 0), (0, 0, 0))) for k, f in enumerate(fof)])
    trk = _tracker(ctx, w, h)
    try:
        got, M = _check(trk, meshes, scenes, fof, poses, K, [0, 5, 10], _mesh_of(names))
        assert (got["verify"]["n_model"] > 0).all() and got["kept"].sum() < 10 and (M > 0).sum() >= 8
        if size == "64x48":
            a1 = got["verify"]["rect"][5]
            assert got["verify"]["n_model"][3] < 40 and a1[0] + a1[2] == w                # D: a few pixels; A across the right border
        rev = _check(trk, meshes, scenes[::-1], 1 - fof, poses, K, [0, 5, 10], _mesh_of(names))[0]   # the frame index is read, not assumed
        assert rev.tobytes() == got.tobytes()
    finally:
        trk.close()


# ---- 3. rect pairs at 64 x 48: mesh D, one triangle, on a flat frame -------------------------------------------------------------
def _flat(tx, ty, rot=0.0, tz=700.0):
    return synth.pose13(synth.rot_z(rot), np.array([tx, ty, tz], np.float64))


def _rect_pairs(mesh_d, scene):
    """Second poses for a first pose _flat(0, 0), found with the model: rects disjoint; rects intersecting with no shared pixel;
    rects intersecting in a single column; in a single row."""
    def look(p):
        r = VM.render(mesh_d, p, KT, 64, 48)
        rec = VM.score(r, scene)
        return rec, SM.support(r, scene, 10)

    r0, m0 = look(_flat(0, 0))
    x0, y0, w0, h0 = [int(v) for v in r0["rect"]]
    found = {}
    cands = [(tx, 0.0, 0.0) for tx in range(20, 140, 3)] + [(0.0, ty, 0.0) for ty in range(20, 140, 3)] + \
            [(tx, ty, np.pi) for ty in range(-60, 61, 12) for tx in range(10, 110, 6)]
    for tx, ty, rot in cands:
        rec, m = look(_flat(tx, ty, rot))
        if rec["n_inlier"] == 0:
            continue
        x, y, w, h = [int(v) for v in rec["rect"]]
        iw, ih = min(x0 + w0, x + w) - max(x0, x), min(y0 + h0, y + h) - max(y0, y)
        shared = int((m0 & m).sum())
        kind = "disjoint" if iw <= 0 or ih <= 0 else "column" if iw == 1 and ih > 1 else "row" if ih == 1 and iw > 1 else \
               "zero" if shared == 0 and iw > 1 and ih > 1 else None
        if kind and kind not in found:
            found[kind] = (_flat(tx, ty, rot), shared)
    assert set(found) == {"disjoint", "zero", "column", "row"}, sorted(found)
    assert r0["n_inlier"] == r0["n_model"] > 10
    return found


def test_rect_pairs(tiny, meshes):
    scene = np.full((48, 64), 700, np.uint16)
    pairs = _rect_pairs(meshes[IDX["D"]], scene)
    kinds = ["disjoint", "zero", "column", "row"]
    print({k: pairs[k][1] for k in kinds})
    assert pairs["disjoint"][1] == 0 and pairs["zero"][1] == 0
    first = _flat(0, 0)
    # four scenes of two, then all five poses as one scene
    poses = np.stack([p for k in kinds for p in (first, pairs[k][0])] + [first] + [pairs[k][0] for k in kinds])
    sf = [0, 2, 4, 6, 8, 13]
    got, M = _check(tiny, meshes, [scene], [0] * 13, poses, KT, sf, _mesh_of("D" * 13), max_shared_ratio=0.05)
    assert [int(M[2 * i, 2 * i + 1]) for i in range(4)] == [pairs[k][1] for k in kinds]
    assert got["kept"][:4].tolist() == [1, 1, 1, 1]


# ---- 4. scene sizes --------------------------------------------------------------------------------------------------------------
def test_scene_sizes(tiny, meshes):
    w, h, K, ps = SIZES["64x48"]
    scene = synth.render(w, h, *_pose(ps[0]), seed=11, fx=K[0], fy=K[1], cx=K[2], cy=K[3])[0]
    a, b = _p13(ps[0]), _p13(ps[0], ((3, 0, 2), (0, 0, 0)))
    # a scene of one; an empty scene between two full ones; empty scenes at both ends
    poses = np.stack([a, b, a, a, b, b])
    got, _ = _check(tiny, meshes, [scene], [0] * 6, poses, K, [0, 0, 1, 3, 3, 6, 6], _mesh_of("AAABAB"))
    assert got["kept"][0] == 1 and got["order"][0] == 0 and got["rival"][0] == -1
    assert got["kept"][1:3].sum() == 1 and got["kept"][3:].sum() == 1 and set(got["rival"][3:].tolist()) <= {-1, 3, 4, 5}
    # 64 identical poses: 2016 pairs, all but the first suppressed by the first
    same = np.stack([a] * 64)
    got, M = _check(tiny, meshes, [scene], [0] * 64, same, K, [0, 64], _mesh_of("A" * 64))
    n = int(got["verify"]["n_inlier"][0])
    assert n > 20 and len(tiny.dev_scene_shared()) == 2016 and (M + n * np.eye(64, dtype=np.int64) == n).all()
    assert got["kept"].tolist() == [1] + [0] * 63 and got["rival"].tolist() == [-1] + [0] * 63 and got["order"].tolist() == list(range(64))
    assert (got["n_shared"][1:] == n).all()
    # two scenes of 64 and one of 12 in one call: pair_first past one scene's 2016
    got, _ = _check(tiny, meshes, [scene], [0] * 140, np.stack([a, b] * 70), K, [0, 64, 128, 140], _mesh_of("AB" * 70))
    assert got["kept"].sum() == 3 and got["rival"][130] == 128


# ---- 5. one call over several scenes = the single calls; device frames; verify_fused; the other calls are left alone -------------
def test_three_scenes_over_two_frames_equal_the_single_calls(ctx, quarter, meshes):
    import torch
    _, scene0, poses6, mesh6 = real_case()
    obj = (-60, 30, 690, -0.50, 0.20, 0.30)
    scene1 = synth.render(160, 120, *_pose(obj), seed=5, fx=KQ[0], fy=KQ[1], cx=KQ[2], cy=KQ[3])[0]
    on1 = [("A", obj), ("C", obj), ("B", obj), ("A", (-58, 30, 692) + obj[3:]), ("D", obj), ("A", HYP[0][1]), ("B", (-61, 31, 690) + obj[3:])]
    poses = np.concatenate([poses6[[3, 1, 0, 2, 5]], poses6[4:5], np.stack([_p13(p) for _, p in on1])])
    mesh_of = np.concatenate([mesh6[[3, 1, 0, 2, 5]], mesh6[4:5], _mesh_of([n for n, _ in on1])]).astype(np.int32)
    fof = np.array([0] * 5 + [0] + [1] * 7, np.int32)                                     # scenes 0 and 1 share frame 0
    sf = [0, 5, 6, 13]
    scenes = [scene0, scene1]
    got, _ = _check(quarter, meshes, scenes, fof, poses, KQ, sf, mesh_of)
    assert got["kept"].sum() >= 3 and 0 < got["kept"][6:].sum() < 7
    for s in range(3):
        a, b = sf[s], sf[s + 1]
        one = quarter.verify_scene([scenes[fof[a]]], [0] * (b - a), poses[a:b], KQ, [0, b - a], mesh_of=mesh_of[a:b])
        one["rival"][one["rival"] >= 0] += a                                              # a rival is an index in its call
        assert one.tobytes() == got[a:b].tobytes(), s
    # device frames
    dev = [torch.from_numpy(s.view(np.int16)).to(f"cuda:{ctx.device}") for s in scenes]
    torch.cuda.synchronize()
    assert quarter.verify_scene(dev, fof, poses, KQ, sf, mesh_of=mesh_of).tobytes() == got.tobytes()
    # the context option verify_fused is ignored
    for fused in (0, 1):
        with util.options(ctx, {"verify_fused": fused}):
            assert quarter.verify_scene(scenes, fof, poses, KQ, sf, mesh_of=mesh_of).tobytes() == got.tobytes(), fused
    ms = quarter.scene_ms()
    assert set(ms) == {"copy", "render", "score", "finish", "overlap", "pick"} and all(v >= 0 for v in ms.values())


def test_verify_and_track_are_unchanged_by_a_scene_call(ctx, meshes):
    w, h, K, ps = SIZES["640x480"]
    trk = api.Tracker(ctx, meshes=MS.in_order(MS.all_meshes()), w=w, h=h, max_frames=2, max_tracks=8, max_crop_px=40000)
    try:
        scenes = [synth.render(w, h, *_pose(p), seed=11 + i)[0] for i, p in enumerate(ps)]
        fof = np.array([0, 0, 1, 1], np.int32)
        poses = np.stack([_p13(ps[f], ((3, -2, 2), (0.01, 0, 0))) for f in fof])
        mo = _mesh_of("ABAC")
        v0 = {f: None for f in (0, 1)}
        for fused in (0, 1):
            with util.options(ctx, {"verify_fused": fused}):
                v0[fused] = trk.verify(scenes, fof, poses, K, group_first=[0, 2, 4], mesh_of=mo)
        t0 = trk.track(scenes, fof, poses, K, mesh_of=mo)
        got = trk.verify_scene(scenes, fof, poses, K, [0, 2, 4], mesh_of=mo)
        assert got["verify"]["n_model"].min() > 1000 and got["kept"][[0, 2]].tolist() == [1, 1] and got["order"][[0, 2]].tolist() == [0, 0]
        assert trk.track(scenes, fof, poses, K, mesh_of=mo).tobytes() == t0.tobytes()
        trk.verify_scene(scenes, fof, poses, K, [0, 2, 4], mesh_of=mo)
        for fused in (0, 1):
            with util.options(ctx, {"verify_fused": fused}):
                assert trk.verify(scenes, fof, poses, K, group_first=[0, 2, 4], mesh_of=mo).tobytes() == v0[fused].tobytes()
        nogroups = trk.verify(scenes, fof, poses, K, mesh_of=mo)
        assert got["verify"].tobytes() == nogroups.tobytes() and v0[0].tobytes() == v0[1].tobytes() != nogroups.tobytes()
        with pytest.raises(api.FealessError) as e:
            trk.verify_scene(scenes, fof, poses, K, [0, 3, 4], mesh_of=mo)                # two frames in one scene
        assert e.value.code == L.FL_ERR_INVALID
        with pytest.raises(TypeError):
            trk.verify_scene(scenes, fof, poses, K, [0, 2, 4], mesh_of=mo, ratio=0.5)
    finally:
        trk.close()


# ---- 6. composition: recognise verified, then arbitrate ---------------------------------------------------------------------------
def test_recognised_instances_of_three_classes_are_arbitrated(ctx, oracle, meshes):
    """tests/multiclass.py's detector: three classes cut from one object's bank, so two classes found groups on one physical
    object.  Frames a and b."""
    sc = clutter.build(oracle)
    frames = ("a", "b")
    bgrs, depths = [sc["frames"][f][0] for f in frames], [sc["frames"][f][1] for f in frames]
    K = sc["K"]
    det = api.Detector(ctx, 2, clutter.T)
    trk = api.Tracker(ctx, meshes=MS.in_order(MS.all_meshes()), w=clutter.W, h=clutter.H, max_frames=2, max_tracks=16, max_crop_px=40000)
    try:
        for b in multiclass.split(sc["bank"]):
            det.add_class(b)
        det.finalize(clutter.W, clutter.H, max_batch=2)
        mesh_of_class = [IDX["A"]] * 3
        res = det.recognize_batch_instances_verified(trk, bgrs, depths, K, 8, MIN_DIST, 2, mesh_of_class=mesh_of_class)
        fof, poses, sf, mesh_of = api.scene_of_instances(res, None, mesh_of_class)
        found = [[r for r in row if r["found"] == 1] for row in res]
        assert sf.tolist() == [0, len(found[0]), len(found[0]) + len(found[1])] and fof.tolist() == [0] * len(found[0]) + [1] * len(found[1])
        assert (mesh_of == IDX["A"]).all() and all(np.array_equal(poses[i, :12], r["pose"].reshape(-1)[:12]) for i, r in enumerate(found[0]))
        classes = [int(r["best"]["class_idx"]) for row in found for r in row]
        assert len(set(classes[:sf[1]])) >= 2 and len(poses) > 4
        got = trk.verify_scene(depths, fof, poses, K, sf, mesh_of=mesh_of)
        want, sh, M = SM.verify_scene(meshes, depths, fof, poses, K, sf, mesh_of=mesh_of)
        assert trk.dev_scene_shared().tolist() == sh.tolist() and got.tobytes() == want.tobytes()
        print(got[["kept", "order", "rival", "n_shared"]], got["verify"][["n_inlier", "n_model"]], classes)
        kept = np.flatnonzero(got["kept"])
        assert 0 < len(kept) < got["verify"]["accepted"].sum()                            # something was suppressed
        for a in kept:                                                                    # no two kept poses share more than the threshold
            for b in kept:
                if got["order"][a] < got["order"][b] and fof[a] == fof[b]:
                    assert M[a, b] < 1 or np.float32(M[a, b]) / np.float32(got["verify"]["n_inlier"][b]) < np.float32(0.5), (a, b)
        # every physical object a hypothesis stands on keeps one: the model's support masks against the instances' visible masks
        rec, masks = SM.masks_and_records(meshes, depths, fof, poses, K, mesh_of)
        for f, name in enumerate(frames):
            for j, vis in enumerate(sc["masks"][name]):
                on = [t for t in range(sf[f], sf[f + 1]) if rec["accepted"][t] and 2 * int((masks[t] & vis).sum()) > int(rec["n_inlier"][t])]
                if on:
                    assert any(got["kept"][t] for t in on), (name, j, on)
        assert sum(1 for t in range(len(poses)) if rec["accepted"][t] and rec["n_inlier"][t] > 1000) >= 3
    finally:
        trk.close()
        det.close()


# ---- 7. the facade ---------------------------------------------------------------------------------------------------------------
INVALID = cadreco_py.INVALID
FACADE_SCENE = np.dtype([("accepted", "<i4"), ("n_model", "<i4"), ("n_missing", "<i4"), ("n_inlier", "<i4"), ("n_front", "<i4"), ("n_behind", "<i4"),
                         ("inlier_ratio", "<f4"), ("behind_ratio", "<f4"), ("kept", "<i4"), ("rival", "<i4"), ("n_shared", "<i4")])
K0, W, H = (608.0, 608.0, 320.0, 240.0), 640, 480


def test_facade_arbitrate_on_a_recognised_frame(ctx, tmp_path):
    """Train a small bank from the OBJ, recognise a frame through the facade, then CadRecoArbitrate the recognised pose and a copy
    of it: the copy is suppressed by entry 0, the records equal the model on the mesh the facade read, and the limits hold."""
    cad = cadreco_py.lib()
    mesh = synth.object_mesh(2)
    obj = str(tmp_path / "object.obj")
    synth.write_obj(obj, mesh)

    def arbitrate(h, depth, poses16, tau=10.0, ratio=0.5, n=None, ts=0.0):
        p = np.ascontiguousarray(poses16, np.float32)
        n = len(p) if n is None else n
        out = np.zeros(max(1, n), FACADE_SCENE)
        rc = cad.cadreco_arbitrate(h, *cadreco_py.frame_args(depth, ts, K0), n, p.ctypes.data, None, tau, ratio, out.ctypes.data)
        return rc, out[:n]

    with cadreco_py.handle() as h:
        V, N, T, depth, pose = cadreco_py.recognised_mesh_frame(h, ctx, obj, str(tmp_path / "bank"))
        moved = pose.copy()
        moved[3] += 150.0
        poses = np.stack([pose, pose.copy(), moved])
        # the facade's limits
        assert arbitrate(h, depth, poses)[0] == INVALID                              # no mesh yet
        assert cad.cadreco_set_tracking_mesh(h, obj.encode(), 1.0) == 0
        assert arbitrate(h, np.zeros((240, 320), np.uint16), poses)[0] == INVALID    # frames must be 640 x 480
        assert arbitrate(h, depth, poses, ts=-1.0)[0] == INVALID                     # CheckTImage: a negative timestamp
        assert arbitrate(h, depth, np.tile(pose, (17, 1)))[0] == INVALID             # more than FEALESS_TRACK_MAX_OBJECTS
        assert arbitrate(h, depth, poses, tau=-1.0)[0] == INVALID and arbitrate(h, depth, poses, tau=65536.0)[0] == INVALID
        for bad in (0.0, -0.5, 1.5, float("nan"), float("inf")):
            assert arbitrate(h, depth, poses, ratio=bad)[0] == INVALID, bad
        assert arbitrate(h, depth, poses, n=0)[0] == 0
        # the records
        rc, got = arbitrate(h, depth, poses)
        p13 = np.zeros((3, 13), np.float32)
        p13[:, :12] = poses[:, :12]
        exp = SM.verify_scene([dict(vertices=V, triangles=T)], [depth], [0, 0, 0], p13, K0, [0, 3])[0]
        print(got, exp)
        assert rc == 0
        for name in FACADE_SCENE.names:
            want = exp[name] if name in ("kept", "rival", "n_shared") else exp["verify"][name]
            assert np.array_equal(got[name], want), name
        assert got["kept"][:2].tolist() == [1, 0] and got["rival"][1] == 0 and got["n_shared"][1] == got["n_inlier"][0] > 1000
        assert got["rival"][0] == -1 and got["inlier_ratio"][0] > 0.9
