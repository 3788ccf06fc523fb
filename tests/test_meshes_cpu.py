"""CPU: several meshes on one tracker (fl_tracker_create_meshes and the *_meshes entry points, include/fealess_hip.h) -- the
refusals, all of which come before the first device call, the header and the bindings, and the reason the GPU comparisons of
tests/test_gpu_meshes.py have teeth: at one pose the right mesh verifies and another one does not."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import meshes as MS
import instances_model as M
import track_model as TM
import verify_model as VM
from fealess_amd import _lib as L
from fealess_amd import api, synth
from util import p13 as _p13, pose as _pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 640, 480
P0 = synth.pose13(np.eye(3), np.array([0.0, 0.0, 700.0]))
NEW_SYMBOLS = ("fl_tracker_create_meshes", "fl_tracker_num_meshes", "fl_track_batch_meshes", "fl_verify_batch_meshes",
               "fl_track_batch_verified_meshes", "fl_recognize_batch_instances_verified_meshes")


@pytest.fixture(scope="module")
def meshes():
    return MS.all_meshes()


def _mesh_array(ms):
    """(the fl_mesh array, what keeps its arrays alive) of a list of mesh dicts; None stays a null entry pointer pair."""
    keep = [(np.ascontiguousarray(m["vertices"], np.float32), np.ascontiguousarray(m["triangles"], np.int32)) for m in ms]
    arr = (L.Mesh * max(1, len(keep)))(*[L.Mesh(v.ctypes.data, t.ctypes.data, len(v), len(t)) for v, t in keep])
    return arr, keep


def test_the_four_meshes_are_what_the_tests_say(meshes):
    assert {k: len(m["triangles"]) for k, m in meshes.items()} == MS.N_TRIANGLES
    for m in meshes.values():
        assert m["triangles"].min() == 0 and m["triangles"].max() == len(m["vertices"]) - 1
    assert MS.ORDER[0] != "C" and MS.INDEX["D"] == 1 and MS.INDEX["C"] == 2     # the largest is not mesh 0, a small one between large ones


# ---- header and bindings ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "fealess_hip.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert "fl_dev_tracker_create_host_meshes" in L.DEV_SIGNATURES and "fl_dev_tracker_create_host_meshes" not in header
    assert re.search(r"#define\s+FL_TRACK_MAX_MESHES\s+256", header) and L.FL_TRACK_MAX_MESHES == 256
    assert C.sizeof(L.Mesh) == 24 and L.Mesh.n_vertices.offset == 16 and L.Mesh.n_triangles.offset == 20
    assert lib.fl_tracker_num_meshes(None) == L.FL_ERR_INVALID


# ---- creation refusals --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_ctx():
    """A context without a device: the one a host-only detector carries; it keeps a refusal's text."""
    det = api._host_only_detector(2, [5, 8])
    yield det.ctx.h
    det.close()


def _create(lib, ctx, ms, n=None, null=False, w=W, h=H, max_frames=2, max_tracks=4, max_crop_px=40000):
    arr, keep = _mesh_array(ms)
    hd = C.c_void_p(0x1234)
    rc = lib.fl_tracker_create_meshes(ctx, None if null else arr, len(ms) if n is None else n, w, h, max_frames, max_tracks, max_crop_px, C.byref(hd))
    return rc, hd.value, lib.fl_last_error(ctx).decode()


def test_tracker_create_meshes_refusals(host_ctx, meshes):
    lib = L.load()
    four = [meshes[k] for k in MS.ORDER]
    for kw, text in ((dict(n=0), "n_meshes 0"), (dict(n=257), "n_meshes 257"), (dict(null=True), "null meshes")):
        rc, hd, err = _create(lib, host_ctx, four, **kw)
        assert rc == L.FL_ERR_INVALID and hd == 0x1234 and text in err, (kw, rc, err)
    # a mesh whose pointers are null
    arr, keep = _mesh_array(four)
    arr[1].vertices = None
    hd = C.c_void_p(0x1234)
    assert lib.fl_tracker_create_meshes(host_ctx, arr, 4, W, H, 2, 4, 40000, C.byref(hd)) == L.FL_ERR_INVALID and hd.value == 0x1234
    assert "mesh 1" in lib.fl_last_error(host_ctx).decode()
    # an index that is valid in the concatenation of the meshes but not in its own mesh: D has 3 vertices, B before it 24
    bad = dict(meshes["D"], triangles=np.array([[0, 1, 3]], np.int32))
    rc, hd, err = _create(lib, host_ctx, [meshes["B"], bad, meshes["C"], meshes["A"]])
    assert rc == L.FL_ERR_INVALID and hd == 0x1234 and "mesh 1" in err and "vertex index 3" in err, err
    # a non-finite vertex in mesh 2: the text names it
    nan_c = dict(meshes["C"], vertices=meshes["C"]["vertices"].copy())
    nan_c["vertices"][7, 1] = np.nan
    rc, hd, err = _create(lib, host_ctx, [meshes["B"], meshes["D"], nan_c, meshes["A"]])
    assert rc == L.FL_ERR_INVALID and hd == 0x1234 and "mesh 2" in err and "non-finite" in err, err
    # the sizes are still checked, and everything in range stops at the missing device only
    assert _create(lib, host_ctx, four, max_crop_px=0)[0] == L.FL_ERR_INVALID
    for ms in (four, four[:1], four * 64):                                       # 256 meshes
        rc, hd, err = _create(lib, host_ctx, ms)
        assert rc == L.FL_ERR_NO_DEVICE and hd == 0x1234, (len(ms), err)
    # the test aid runs the same mesh checks
    hd = C.c_void_p(0x1234)
    create_host = L.dev(lib, "fl_dev_tracker_create_host_meshes")
    arr, keep = _mesh_array([meshes["B"], bad])
    assert create_host(arr, 2, W, H, 2, 4, 40000, C.byref(hd)) == L.FL_ERR_INVALID and hd.value == 0x1234
    assert create_host(None, 2, W, H, 2, 4, 40000, C.byref(hd)) == L.FL_ERR_INVALID and create_host(arr, 0, W, H, 2, 4, 40000, C.byref(hd)) == L.FL_ERR_INVALID


# ---- call refusals on a host tracker with three meshes ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_tracker3(meshes):
    lib = L.load()
    arr, keep = _mesh_array([meshes["B"], meshes["D"], meshes["C"]])
    h = C.c_void_p()
    assert L.dev(lib, "fl_dev_tracker_create_host_meshes")(arr, 3, W, H, 2, 4, 40000, C.byref(h)) == L.FL_OK and h.value
    assert lib.fl_tracker_num_meshes(h) == 3
    yield h
    lib.fl_tracker_destroy(h)


def _tracker_call(lib, trk, which, mesh_of):
    """One of the three *_meshes calls over two poses on two frames, everything but mesh_of in range: (rc, results untouched)."""
    frames = [np.zeros((H, W), np.uint16) for _ in range(2)]
    dp = (C.c_void_p * 2)(*[f.ctypes.data for f in frames])
    fof, poses = np.array([0, 1], np.int32), np.ascontiguousarray(np.tile(P0, (2, 1)), np.float32)
    mo = None if mesh_of is None else np.array(mesh_of, np.int32)
    mop = None if mo is None else mo.ctypes.data
    k = L.Intrinsics(W, H, 608.0, 608.0, 320.0, 240.0)
    size = {"track": C.sizeof(L.TrackResult), "verify": C.sizeof(L.VerifyResult), "track_verified": C.sizeof(L.VerifiedTrackResult)}[which]
    out = np.full(2 * size, 0x5A, np.uint8)
    if which == "track":
        rc = lib.fl_track_batch_meshes(trk, 2, dp, L.FL_MEM_HOST, 2, fof.ctypes.data, mop, poses.ctypes.data, C.byref(k), None, out.ctypes.data)
    elif which == "verify":
        rc = lib.fl_verify_batch_meshes(trk, 2, dp, L.FL_MEM_HOST, 2, fof.ctypes.data, mop, poses.ctypes.data, 0, None, C.byref(k), None, out.ctypes.data)
    else:
        rc = lib.fl_track_batch_verified_meshes(trk, 2, dp, L.FL_MEM_HOST, 2, fof.ctypes.data, mop, poses.ctypes.data, 0, None, C.byref(k), None, None,
                                                out.ctypes.data)
    return rc, bool((out == 0x5A).all())


@pytest.mark.parametrize("which", ["track", "verify", "track_verified"])
def test_mesh_of_out_of_range_is_refused_with_nothing_written(host_tracker3, which):
    lib = L.load()
    for mesh_of in ((-1, 0), (0, 3), (3, -1)):
        assert _tracker_call(lib, host_tracker3, which, mesh_of) == (L.FL_ERR_INVALID, True), mesh_of
    # in range, and NULL: what stops the call is the missing device
    for mesh_of in (None, (0, 0), (2, 1), (1, 2)):
        assert _tracker_call(lib, host_tracker3, which, mesh_of) == (L.FL_ERR_NO_DEVICE, True), mesh_of


def test_python_surface(host_tracker3):
    class Ctx:
        lib = L.load()
    trk = api.Tracker.__new__(api.Tracker)
    trk.ctx, trk.lib, trk.handle, trk.w, trk.h = Ctx(), Ctx.lib, host_tracker3, W, H
    assert trk.num_meshes == 3
    for call in (trk.track, trk.verify, trk.track_verified):
        with pytest.raises(ValueError):
            call([np.zeros((H, W), np.uint16)], [0, 0], [P0, P0], TM.MODEL_K, mesh_of=[0])
    with pytest.raises(TypeError):
        api.Tracker(Ctx(), w=W, h=H, max_frames=1, max_tracks=1, max_crop_px=100)
    with pytest.raises(TypeError):
        api.Tracker(Ctx(), np.zeros((3, 3)), np.zeros((1, 3)), W, H, 1, 1, 100, meshes=[])


# ---- fl_recognize_batch_instances_verified_meshes: the refusals that need no device -------------------------------------------
@pytest.fixture(scope="module")
def host_det():
    det = api._host_only_detector(2, [5, 8])
    for b in M.small_banks():
        det.add_class(b)
    yield det
    det.close()


def _instances_call(lib, det, trk, mesh_of_class, class_idx=-1):
    bgr, depth = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint16)
    bp, dp = (C.c_void_p * 1)(bgr.ctypes.data), (C.c_void_p * 1)(depth.ctypes.data)
    k = L.Intrinsics(W, H, 608.0, 608.0, 320.0, 240.0)
    p = L.RecognitionParams(75.0, 10, 0.5, 0.01, L.FL_ICP_PARITY)
    ip = L.InstanceParams(8, 48, 4)
    vp = L.InstanceVerifyParams(L.VerifyParams(10, 1, 0.0, 0.0), class_idx, 0)
    moc = None if mesh_of_class is None else np.array(mesh_of_class, np.int32)
    out = np.full(8 * C.sizeof(L.VerifiedInstanceResult), 0xA5, np.uint8)
    cnt, drop = (C.c_int32 * 1)(-7), (C.c_int32 * 1)(-7)
    rc = lib.fl_recognize_batch_instances_verified_meshes(det.h, trk, 1, bp, dp, L.FL_MEM_HOST, C.byref(k), C.byref(p), C.byref(ip), C.byref(vp),
                                                          None if moc is None else moc.ctypes.data, out.ctypes.data, cnt, drop, None)
    return rc, bool((out == 0xA5).all()) and cnt[0] == -7 and drop[0] == -7, lib.fl_last_error(det.ctx.h).decode()


def test_instances_verified_meshes_refusals(host_det, host_tracker3):
    """As tests/test_instances_verified_cpu.py: the host tracker owns a context of its own, so a call that passes every check of
    the map is refused as a tracker on another context, and the error text tells the refusals apart."""
    lib = L.load()
    n_cls = lib.fl_detector_num_classes(host_det.h)
    assert n_cls >= 2
    ok = [0] + [-1] * (n_cls - 2) + [2]
    for kw, text in ((dict(mesh_of_class=None), "null mesh_of_class"), (dict(mesh_of_class=ok[:-1] + [3]), "= 3 outside [-1, 3)"),
                     (dict(mesh_of_class=[-2] + ok[1:]), "= -2 outside [-1, 3)"), (dict(mesh_of_class=ok, class_idx=0), "must be -1"),
                     (dict(mesh_of_class=ok, class_idx=-2), "must be -1"), (dict(mesh_of_class=ok), "another context")):
        rc, untouched, err = _instances_call(lib, host_det, host_tracker3, **kw)
        assert rc == L.FL_ERR_INVALID and untouched and text in err, (kw, rc, err)


# ---- the choice of the mesh matters -------------------------------------------------------------------------------------------
def test_the_right_mesh_verifies_and_another_one_does_not(meshes):
    """The object at POSES[0] of tests/test_gpu_track.py in a synth.render frame, verified at that pose: mesh A gives the
    12720 inliers of 12726 model pixels that DESIGN.md row f6 records.  The same pose with mesh C (a sphere of radius 60 at the
    object's origin) gives n_model 8082, n_inlier 2509, n_front 1169, n_behind 4404: inlier_ratio 0.31044295, behind_ratio
    0.5449146 -- more than half of its pixels look through where the object is not.  Mesh B (the box alone) gives 5209 of 6599,
    0.789362, and mesh D 0 of 1896."""
    p = (10, -5, 720, 0.30, 0.35, 0.10)
    scene = synth.render(W, H, *_pose(p), seed=40)[0]
    rec = {k: VM.verify(meshes[k], [scene], [0], _p13(p)[None], TM.MODEL_K)[0] for k in "ACBD"}
    for k, r in rec.items():
        print(k, "n_model", r["n_model"], "n_inlier", r["n_inlier"], "n_front", r["n_front"], "n_behind", r["n_behind"], "inlier_ratio",
              r["inlier_ratio"], "behind_ratio", r["behind_ratio"])
    assert (rec["A"]["n_inlier"], rec["A"]["n_model"]) == (12720, 12726)
    assert rec["A"]["inlier_ratio"] > rec["C"]["inlier_ratio"] and rec["C"]["n_behind"] > 0
    assert len({r.tobytes() for r in rec.values()}) == 4                  # every mesh gives a record of its own
