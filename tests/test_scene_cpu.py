"""CPU: scene arbitration (fl_verify_scene_batch, fl_scene_pick; include/fealess_hip.h) without a GPU -- what
tests/scene_model.py, the numpy statement of the contract, decides on a frame where several meshes explain one object; the
library's host-only fl_scene_pick against that model on constructed records; and the argument checks of both entry points, which
come before the first HIP call and so run on a tracker without a device (fl_dev_tracker_create_host_meshes).
"""
import ctypes as C

import numpy as np
import pytest

import meshes as MS
import scene_model as SM
import verify_model as VM
from fealess_amd import _lib as L
from fealess_amd import api, synth
from util import p13 as _p13

W, H, K = 160, 120, (152.0, 152.0, 80.0, 60.0)
OBJ0, OBJ1 = (10, -5, 720, .30, .35, .10), (-200, -100, 720, .9, .5, -.2)
# (mesh, pose): four hypotheses on object 0, two on object 1
HYP = [("A", OBJ0), ("A", (12, -5, 721) + OBJ0[3:]), ("B", OBJ0), ("C", OBJ0), ("A", OBJ1), ("D", OBJ1)]
ON = [0, 0, 0, 0, 1, 1]                        # the object each hypothesis stands on
TRUE = {0: 0, 1: 4}                            # the true-pose A of each object


def real_case():
    """(meshes in tracker order, scene, poses13, mesh_of) of the case above; shared with tests/test_gpu_scene.py."""
    scene = synth.render_clutter(W, H, [synth.object_pose(*OBJ0), synth.object_pose(*OBJ1)], seed=3, fx=K[0], fy=K[1], cx=K[2], cy=K[3])[0]
    ms = MS.all_meshes()
    return [ms[n] for n in MS.ORDER], scene, np.stack([_p13(p) for _, p in HYP]), np.array([MS.INDEX[n] for n, _ in HYP], np.int32)


@pytest.fixture(scope="module")
def case():
    meshes, scene, poses, mesh_of = real_case()
    rec, masks = SM.masks_and_records(meshes, [scene], [0] * 6, poses, K, mesh_of)
    M = SM.shared_matrix(rec, masks, [0, 6])
    return dict(rec=rec, M=M, sh=SM.compact(M, [0, 6]))


# ---- (a) the model on a real case ----------------------------------------------------------------------------------------------
def test_model_keeps_one_pose_per_object(case):
    """The model's n_inlier / n_model per hypothesis: 793 / 793, 773 / 791, 326 / 413, 161 / 503 on object 0 (sharing 771, 326,
    160 pixels with the first) and 855 / 855, 1 / 110 on object 1 (sharing 1).  The consequences are asserted, from the model's
    own counts, not the digits."""
    rec, M = case["rec"], case["M"]
    print(rec[["n_inlier", "n_model"]], M)
    assert (rec["accepted"] == 1).all() and VM.invariant(rec) and (M == M.T).all()
    for a in range(6):
        for b in range(6):
            assert M[a, b] <= min(rec["n_inlier"][a], rec["n_inlier"][b])
            assert ON[a] == ON[b] or M[a, b] == 0                       # the two objects stand apart
    out = SM.pick(rec, [0, 6], case["sh"])
    assert out["verify"].tobytes() == rec.tobytes()
    for obj, true in TRUE.items():
        on = [t for t in range(6) if ON[t] == obj]
        assert [t for t in on if out["kept"][t]] == [true]
        for t in on:
            if t != true:
                assert out["rival"][t] == true and out["n_shared"][t] == M[true, t] > 0
                assert np.float32(M[true, t]) / np.float32(rec["n_inlier"][t]) >= np.float32(0.5)
        assert out["rival"][true] == -1 and out["n_shared"][true] == 0      # nothing kept before it on its object
    assert sorted(out["order"].tolist()) == list(range(6))
    by_place = np.argsort(out["order"])
    assert (np.diff(rec["n_inlier"][by_place]) <= 0).all()                   # more explained surface first


def test_model_thresholds(case):
    rec, M, sh = case["rec"], case["M"], case["sh"]
    d = 5                                                                   # mesh D on object 1: a single shared pixel
    assert rec["n_inlier"][d] == M[TRUE[1], d] == 1
    two = SM.pick(rec, [0, 6], sh, min_shared_px=2)
    assert two["kept"][d] == 1 and two["rival"][d] == TRUE[1] and two["n_shared"][d] == 1
    assert two["kept"].tolist() == [1, 0, 0, 0, 1, 1]
    full = SM.pick(rec, [0, 6], sh, max_shared_ratio=1.0)
    for t in range(6):
        suppressed = not full["kept"][t]
        if suppressed:
            assert full["n_shared"][t] == rec["n_inlier"][t] == M[full["rival"][t], t]
        else:                                                               # no kept pose before it holds all of its inliers
            assert all(M[a, t] < rec["n_inlier"][t] for a in range(6) if full["kept"][a] and full["order"][a] < full["order"][t])
    assert 0 < full["kept"].sum() < 6 and not full["kept"][2] and full["kept"][1]   # B lies inside A; the moved A does not


# ---- (b) fl_scene_pick against the model ---------------------------------------------------------------------------------------
def _records(rows):
    """(accepted, n_inlier, n_model) per pose."""
    r = np.zeros(len(rows), VM.DTYPE)
    for i, (a, ni, nm) in enumerate(rows):
        r[i]["accepted"], r[i]["n_inlier"], r[i]["n_model"] = a, ni, nm
    r["best"] = r["accepted"]
    return r


def _full(n, pairs):
    M = np.zeros((n, n), np.int64)
    for (a, b), v in pairs.items():
        M[a, b] = M[b, a] = v
    return M


def _both(rec, scene_first, M, **params):
    sh = SM.compact(M, scene_first)
    want = SM.pick(rec, scene_first, sh, **params)
    got = api.scene_pick(rec, scene_first, sh if len(sh) else None, **params)
    assert got.dtype == SM.DTYPE and got.tobytes() == want.tobytes(), (got, want)
    return got


def test_pick_order_is_not_the_input_order():
    rec = _records([(1, 10, 20), (1, 30, 40), (1, 20, 20), (1, 30, 60)])
    got = _both(rec, [0, 4], _full(4, {}))
    assert got["order"].tolist() == [3, 0, 2, 1]                            # 30/40 before 30/60 before 20 before 10
    assert got["kept"].tolist() == [1, 1, 1, 1] and (got["rival"] == -1).all()
    got = _both(rec, [0, 4], _full(4, {(1, 3): 15, (1, 0): 4, (3, 0): 9, (2, 0): 5}))
    assert got["kept"].tolist() == [0, 1, 1, 0] and got["rival"].tolist() == [2, -1, -1, 1] and got["n_shared"].tolist() == [5, 0, 0, 15]


def test_pick_ties():
    same = _records([(1, 50, 60)] * 3)
    got = _both(same, [0, 3], _full(3, {(0, 1): 50, (0, 2): 50, (1, 2): 50}))
    assert got["order"].tolist() == [0, 1, 2] and got["kept"].tolist() == [1, 0, 0] and got["rival"].tolist() == [-1, 0, 0]
    ratio = _records([(1, 50, 70), (1, 50, 60), (1, 50, 60)])              # equal n_inlier: the smaller n_model first, then the index
    got = _both(ratio, [0, 3], _full(3, {}))
    assert got["order"].tolist() == [2, 0, 1]
    big = _records([(1, 1 << 30, (1 << 30) + 1), (1, 1 << 30, 1 << 30)])  # the products pass 2^32 and differ in int64 only
    assert _both(big, [0, 2], _full(2, {}))["order"].tolist() == [1, 0]


def test_pick_chain_and_most_shared_rival():
    rec = _records([(1, 100, 100), (1, 90, 100), (1, 80, 100)])
    got = _both(rec, [0, 3], _full(3, {(0, 1): 60, (1, 2): 70}))           # b suppressed by a; c overlaps b only
    assert got["kept"].tolist() == [1, 0, 1] and got["rival"].tolist() == [-1, 0, -1] and got["n_shared"].tolist() == [0, 60, 0]
    got = _both(rec, [0, 3], _full(3, {(0, 1): 60, (1, 2): 70, (0, 2): 7}))
    assert got["kept"].tolist() == [1, 0, 1] and got["rival"][2] == 0 and got["n_shared"][2] == 7
    # a kept pose's rival is the kept pose it shares most with, the earlier of equals; the suppressor is the FIRST kept pose that suppresses
    rec = _records([(1, 100, 100), (1, 90, 100), (1, 80, 100), (1, 40, 100)])
    got = _both(rec, [0, 4], _full(4, {(0, 2): 9, (1, 2): 9, (0, 3): 20, (1, 3): 30, (2, 3): 35}))
    assert got["kept"].tolist() == [1, 1, 1, 0] and got["rival"].tolist() == [-1, -1, 0, 0] and got["n_shared"].tolist() == [0, 0, 9, 20]


def test_pick_ratio_exactly_at_the_threshold_in_float32():
    third = np.float32(1) / np.float32(3)
    assert np.float32(third) == np.float32(0.33333334) and float(third) > 1 / 3          # 1/3 rounds up in float32
    rec = _records([(1, 10, 10), (1, 3, 10)])
    M = _full(2, {(0, 1): 1})
    assert _both(rec, [0, 2], M, max_shared_ratio=float(third))["kept"].tolist() == [1, 0]    # 1.f / 3.f >= the threshold as a float
    above = float(np.nextafter(third, np.float32(1)))
    assert _both(rec, [0, 2], M, max_shared_ratio=above)["kept"].tolist() == [1, 1]
    rec = _records([(1, 10, 10), (1, 4, 10)])
    assert _both(rec, [0, 2], _full(2, {(0, 1): 2}))["kept"].tolist() == [1, 0]               # exactly 0.5, the default
    assert _both(rec, [0, 2], _full(2, {(0, 1): 2}), min_shared_px=3)["kept"].tolist() == [1, 1]


def test_pick_degenerate_poses_and_scenes():
    # n_inlier = 0 is accepted with the default gates, shares nothing and is never suppressed; poses that are not accepted
    rec = _records([(1, 0, 9), (0, 50, 60), (1, 5, 9), (1, 0, 3), (0, 0, 0)])
    M = _full(5, {(1, 2): 5})                                               # with a pose that is not accepted: ignored
    sh = SM.compact(M, [0, 5])
    got = api.scene_pick(rec, [0, 5], sh)
    want = SM.pick(rec, [0, 5], SM.compact(_full(5, {}), [0, 5]))
    assert got.tobytes() == want.tobytes()
    assert got["kept"].tolist() == [1, 0, 1, 1, 0] and got["order"].tolist() == [1, -1, 0, 2, -1]   # 0 / 9 and 0 / 3 tie: the index
    assert got["rival"].tolist() == [-1] * 5 and got["n_shared"].tolist() == [0] * 5
    # empty scenes, scenes of one, no pair at all: shared may be NULL
    one = _records([(1, 5, 9), (0, 5, 9)])
    got = _both(one, [0, 0, 1, 1, 2, 2], _full(2, {}))
    assert got["kept"].tolist() == [1, 0] and got["order"].tolist() == [0, -1]
    assert len(api.scene_pick(np.zeros(0, VM.DTYPE), [0, 0], None)) == 0


def test_pick_a_scene_of_64_and_the_pair_index():
    rng = np.random.default_rng(7)
    sizes = [5, 0, 64, 1, 7, 2]
    sf = np.concatenate([[0], np.cumsum(sizes)])
    n = int(sf[-1])
    rec = _records([(int(rng.random() < 0.85), int(rng.integers(0, 40)), 40 + int(rng.integers(0, 3))) for _ in range(n)])
    M = np.zeros((n, n), np.int64)
    for s in range(len(sizes)):
        for a in range(sf[s], sf[s + 1]):
            for b in range(a + 1, sf[s + 1]):
                M[a, b] = M[b, a] = rng.integers(0, min(rec["n_inlier"][a], rec["n_inlier"][b]) + 1) if rng.random() < 0.3 else 0
    assert len(SM.compact(M, sf)) == 10 + 2016 + 21 + 1
    got = _both(rec, sf, M)
    assert 0 < got["kept"].sum() < rec["accepted"].sum()
    for s in range(len(sizes)):                                             # a rival is a pose of the same scene, by its index in the call
        part = got[sf[s]:sf[s + 1]]
        assert ((part["rival"] == -1) | ((part["rival"] >= sf[s]) & (part["rival"] < sf[s + 1]))).all()
        acc = part["verify"]["accepted"] == 1
        assert sorted(part["order"][acc].tolist()) == list(range(acc.sum())) and (part["order"][~acc] == -1).all()
    same = _records([(1, 30, 40)] * 64)
    got = _both(same, [0, 64], np.full((64, 64), 30) - 30 * np.eye(64, dtype=np.int64))
    assert got["kept"].tolist() == [1] + [0] * 63 and got["rival"].tolist() == [-1] + [0] * 63 and got["order"].tolist() == list(range(64))


NAN, INF = float("nan"), float("inf")


def _pick_raw(lib, rec, sf, sh, params, results=True, n_scenes=None, n_poses=None):
    rec = None if rec is None else np.ascontiguousarray(rec, VM.DTYPE)
    sf = None if sf is None else np.ascontiguousarray(sf, np.int32)
    sh = None if sh is None else np.ascontiguousarray(sh, np.int32)
    prm = None if params is None else L.SceneParams(L.VerifyParams(*params[:4]), params[4], params[5])
    out = np.full(80 * 70, 0xA5, np.uint8)
    rc = lib.fl_scene_pick(None if rec is None else rec.ctypes.data, len(rec) if n_poses is None else n_poses,
                           (len(sf) - 1) if n_scenes is None else n_scenes, None if sf is None else sf.ctypes.data,
                           None if sh is None else sh.ctypes.data, None if prm is None else C.byref(prm), out.ctypes.data if results else None)
    return rc, bool((out == 0xA5).all())


def test_pick_refusals():
    lib = L.load()
    rec = _records([(1, 10, 10), (1, 4, 10), (1, 6, 10)])
    sf, sh, ok = [0, 3], [2, 1, 3], (10, 1, 0.0, 0.0, 0.5, 1)
    assert _pick_raw(lib, rec, sf, sh, ok) == (L.FL_OK, False) and _pick_raw(lib, rec, sf, sh, None) == (L.FL_OK, False)
    bad = {
        "records null": dict(rec=None, n_poses=3), "scene_first null": dict(sf=None, n_scenes=1), "results null": dict(results=False),
        "shared null with pairs": dict(sh=None), "n_scenes 0": dict(n_scenes=0), "n_scenes negative": dict(n_scenes=-1),
        "scene_first[0] != 0": dict(sf=[1, 3]), "decreasing": dict(sf=[0, 2, 1, 3], sh=[0, 0]), "ends early": dict(sf=[0, 2], sh=[0]),
        "ends late": dict(sf=[0, 4], sh=[0] * 6), "beyond n_poses in the middle": dict(sf=[0, 4, 3], sh=[0] * 6),
        "ratio 0": dict(params=(10, 1, 0.0, 0.0, 0.0, 1)), "ratio above 1": dict(params=(10, 1, 0.0, 0.0, 1.0000001, 1)),
        "ratio negative": dict(params=(10, 1, 0.0, 0.0, -0.5, 1)), "ratio nan": dict(params=(10, 1, 0.0, 0.0, NAN, 1)),
        "ratio inf": dict(params=(10, 1, 0.0, 0.0, INF, 1)), "min_shared_px 0": dict(params=(10, 1, 0.0, 0.0, 0.5, 0)),
        "tau -1": dict(params=(-1, 1, 0.0, 0.0, 0.5, 1)), "min_model_px 0": dict(params=(10, 0, 0.0, 0.0, 0.5, 1)),
        "gate nan": dict(params=(10, 1, NAN, 0.0, 0.5, 1)),
        "shared negative": dict(sh=[-1, 1, 3]), "shared above n_inlier_b": dict(sh=[5, 1, 3]), "shared above the smaller": dict(sh=[2, 1, 5]),
    }
    for name, over in bad.items():
        a = dict(rec=rec, sf=sf, sh=sh, params=ok)
        a.update(over)
        assert _pick_raw(lib, a.pop("rec"), a.pop("sf"), a.pop("sh"), a.pop("params"), **a) == (L.FL_ERR_INVALID, True), name
    assert _pick_raw(lib, _records([(1, 9, 9)] * 65), [0, 65], [0] * 2080, ok) == (L.FL_ERR_INVALID, True)       # a scene of 65
    assert _pick_raw(lib, rec, sf, sh, (10, 1, 0.0, 0.0, 1.0, 1))[0] == L.FL_OK                                  # the ends of the ranges
    assert _pick_raw(lib, rec, sf, sh, (10, 1, 0.0, 0.0, 1e-30, 1 << 30))[0] == L.FL_OK


# ---- (c) fl_verify_scene_batch's argument checks, on a tracker without a device -------------------------------------------------
TW, TH, MAX_FRAMES, MAX_TRACKS = 64, 48, 2, 70


@pytest.fixture(scope="module")
def host_tracker():
    lib = L.load()
    ms = MS.in_order(MS.all_meshes())
    arr = (L.Mesh * 4)(*[L.Mesh(v.ctypes.data, t.ctypes.data, len(v), len(t)) for v, t in ms])
    h = C.c_void_p()
    assert L.dev(lib, "fl_dev_tracker_create_host_meshes")(arr, 4, TW, TH, MAX_FRAMES, MAX_TRACKS, 100, C.byref(h)) == 0 and h.value
    yield lib, h
    lib.fl_tracker_destroy(h)


POSE = _p13((0, 0, 700, 0.3, 0.35, 0.1))


def _call(lib, tracker, **over):
    """fl_verify_scene_batch with valid arguments (two frames, five poses, three scenes) except for what `over` replaces.
    Returns (rc, results untouched?)."""
    a = dict(n_frames=2, depth=[np.full((TH, TW), 700, np.uint16)] * 2, mem=L.FL_MEM_HOST, n_poses=5, frame_of=[0, 0, 1, 1, 1], mesh_of=[0, 3, 1, 2, 3],
             poses=np.stack([POSE] * 5), n_scenes=3, scene_first=[0, 2, 2, 5], K=(TW, TH, 60.0, 61.0, 32.0, 24.0),
             params=(10, 1, 0.0, 0.0, 0.5, 1), results=True, trk=tracker)
    a.update(over)
    dp = None
    if a["depth"] is not None:
        dp = (C.c_void_p * max(1, len(a["depth"])))(*[None if d is None else d.ctypes.data for d in a["depth"]])
    arr = {k: None if a[k] is None else np.ascontiguousarray(a[k], t) for k, t in
           (("frame_of", np.int32), ("mesh_of", np.int32), ("poses", np.float32), ("scene_first", np.int32))}
    ptr = {k: None if v is None else v.ctypes.data for k, v in arr.items()}
    k = None if a["K"] is None else L.Intrinsics(*a["K"])
    prm = None if a["params"] is None else L.SceneParams(L.VerifyParams(*a["params"][:4]), a["params"][4], a["params"][5])
    out = np.full(MAX_TRACKS * C.sizeof(L.SceneResult), 0xA5, np.uint8)
    rc = lib.fl_verify_scene_batch(a["trk"], a["n_frames"], dp, a["mem"], a["n_poses"], ptr["frame_of"], ptr["mesh_of"], ptr["poses"], a["n_scenes"],
                                   ptr["scene_first"], None if k is None else C.byref(k), None if prm is None else C.byref(prm),
                                   out.ctypes.data if a["results"] else None)
    return rc, bool((out == 0xA5).all())


def _bad_pose(value, at):
    p = np.stack([POSE] * 5)
    p[4, at] = value
    return p


def _many(n, **over):
    return dict(dict(n_poses=n, frame_of=[0] * n, mesh_of=[0] * n, poses=np.stack([POSE] * n)), **over)


INVALID = {
    # what fl_verify_batch_meshes refuses
    "tracker null": dict(trk=None), "depth null": dict(depth=None), "frame_of null": dict(frame_of=None), "poses null": dict(poses=None),
    "K null": dict(K=None), "results null": dict(results=False), "a null frame": dict(depth=[np.zeros((TH, TW), np.uint16), None]),
    "n_frames 0": dict(n_frames=0), "n_frames above max_frames": dict(n_frames=MAX_FRAMES + 1, depth=[np.zeros((TH, TW), np.uint16)] * 3),
    "n_poses 0": dict(n_poses=0, scene_first=[0, 0, 0, 0]),
    "n_poses above max_tracks": _many(MAX_TRACKS + 1, n_scenes=2, scene_first=[0, 40, MAX_TRACKS + 1]),
    "frame_of -1": dict(frame_of=[0, 0, 1, 1, -1]), "frame_of n_frames": dict(frame_of=[0, 0, 2, 2, 2]), "frame_of beyond a smaller n_frames": dict(n_frames=1),
    "mesh_of -1": dict(mesh_of=[0, -1, 1, 2, 3]), "mesh_of n_meshes": dict(mesh_of=[0, 3, 1, 2, 4]),
    "pose nan": dict(poses=_bad_pose(NAN, 0)), "pose inf": dict(poses=_bad_pose(INF, 11)),
    "fx nan": dict(K=(TW, TH, NAN, 61.0, 32.0, 24.0)), "fy inf": dict(K=(TW, TH, 60.0, INF, 32.0, 24.0)), "cx nan": dict(K=(TW, TH, 60.0, 61.0, NAN, 24.0)),
    "fx 0": dict(K=(TW, TH, 0.0, 61.0, 32.0, 24.0)), "fy negative": dict(K=(TW, TH, 60.0, -61.0, 32.0, 24.0)),
    "fx 0 as a float": dict(K=(TW, TH, 1e-60, 61.0, 32.0, 24.0)), "cx inf as a float": dict(K=(TW, TH, 60.0, 61.0, 1e300, 24.0)),
    "K width": dict(K=(TW + 1, TH, 60.0, 61.0, 32.0, 24.0)), "K height": dict(K=(TW, TH - 1, 60.0, 61.0, 32.0, 24.0)), "mem 2": dict(mem=2),
    "tau -1": dict(params=(-1, 1, 0.0, 0.0, 0.5, 1)), "tau 65536": dict(params=(65536, 1, 0.0, 0.0, 0.5, 1)),
    "min_model_px 0": dict(params=(10, 0, 0.0, 0.0, 0.5, 1)), "min_inlier_ratio nan": dict(params=(10, 1, NAN, 0.0, 0.5, 1)),
    "max_behind_ratio inf": dict(params=(10, 1, 0.0, INF, 0.5, 1)),
    # the scene rules
    "scene_first null": dict(scene_first=None), "scene_first[0] != 0": dict(scene_first=[1, 2, 2, 5]),
    "scene_first decreasing": dict(scene_first=[0, 2, 1, 5]), "scene_first beyond n_poses in the middle": dict(scene_first=[0, 2, 6, 5]),
    "scene_first ends before n_poses": dict(scene_first=[0, 2, 2, 4]), "scene_first ends after n_poses": dict(scene_first=[0, 2, 2, 6]),
    "n_scenes 0": dict(n_scenes=0), "n_scenes negative": dict(n_scenes=-1),
    "n_scenes above max_tracks": dict(n_scenes=MAX_TRACKS + 1, scene_first=[0] * MAX_TRACKS + [2, 5]),
    "a scene of 65": _many(65, n_scenes=1, scene_first=[0, 65]), "a scene of 65 after a scene of 5": _many(70, n_scenes=2, scene_first=[0, 5, 70]),
    "two frames in one scene": dict(frame_of=[0, 0, 1, 1, 0]), "two frames in the first scene": dict(frame_of=[0, 1, 1, 1, 1]),
    # the two fields fl_scene_params adds
    "ratio 0": dict(params=(10, 1, 0.0, 0.0, 0.0, 1)), "ratio negative": dict(params=(10, 1, 0.0, 0.0, -1.0, 1)),
    "ratio above 1": dict(params=(10, 1, 0.0, 0.0, 1.0000001, 1)), "ratio nan": dict(params=(10, 1, 0.0, 0.0, NAN, 1)),
    "ratio inf": dict(params=(10, 1, 0.0, 0.0, INF, 1)), "ratio -inf": dict(params=(10, 1, 0.0, 0.0, -INF, 1)),
    "min_shared_px 0": dict(params=(10, 1, 0.0, 0.0, 0.5, 0)), "min_shared_px negative": dict(params=(10, 1, 0.0, 0.0, 0.5, -3)),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_are_refused_before_any_device_work(host_tracker, case):
    lib, trk = host_tracker
    rc, untouched = _call(lib, trk, **INVALID[case])
    assert rc == L.FL_ERR_INVALID and untouched, case


def test_valid_arguments_reach_the_device_check(host_tracker):
    """Everything the contract allows passes the checks and then fails for want of a device, with nothing written."""
    lib, trk = host_tracker
    valid = [dict(), dict(params=None), dict(mesh_of=None), dict(mem=L.FL_MEM_DEVICE), dict(poses=_bad_pose(NAN, 12)),
             dict(params=(0, 1, 0.0, 0.0, 1.0, 1)), dict(params=(65535, 1 << 30, 0.5, 0.25, 1e-30, 1 << 30)),
             dict(n_scenes=1, scene_first=[0, 5], frame_of=[1] * 5), dict(n_scenes=5, scene_first=[0, 0, 2, 2, 5, 5]),
             dict(n_scenes=MAX_TRACKS, scene_first=[0] * (MAX_TRACKS - 1) + [2, 5]),
             _many(64, n_scenes=1, scene_first=[0, 64]), _many(MAX_TRACKS, n_scenes=3, scene_first=[0, 64, 64, MAX_TRACKS])]
    for over in valid:
        rc, untouched = _call(lib, trk, **over)
        assert rc == L.FL_ERR_NO_DEVICE and untouched, over
    assert lib.fl_verify_scene_batch(None, 1, None, 0, 1, None, None, None, 1, None, None, None, None) == L.FL_ERR_INVALID


def test_record_layout():
    assert C.sizeof(L.SceneResult) == 80 and C.sizeof(L.SceneParams) == 24
    assert api.SCENE_DTYPE == SM.DTYPE
    for name, _ in L.SceneResult._fields_:
        assert getattr(L.SceneResult, name).offset == SM.DTYPE.fields[name][1], name
    assert SM.MAX_POSES == 64
