"""CPU: the numpy statement of a tracking step (tests/track_model.py) on hand-made cases -- the rectangle rule at every image
border, the x10 / rint(d * 0.1f) round trip of the model image against the oracle's detection(), the lost rule -- and the
argument refusals of fl_tracker_create / fl_track_batch, which come before the first device call."""
import ctypes as C

import numpy as np
import pytest

import track_model as TM
from fealess_amd import _lib as L
from fealess_amd import api, synth

W, H = 640, 480
RESULT_BYTES = C.sizeof(L.TrackResult)          # fl_track_result: 2 + 4 + 4 ints, 16 floats, fl_detection_result


def _box_image(x0, x1, y0, y1, w=W, h=H, z=700):
    d = np.zeros((h, w), np.uint16)
    d[y0:y1 + 1, x0:x1 + 1] = z
    return d


P0 = synth.pose13(np.eye(3), np.array([0.0, 0.0, 700.0]))


def test_rule_in_the_middle_and_at_each_border():
    K = TM.MODEL_K
    assert TM.rects(_box_image(100, 199, 50, 89), P0, K, 12) == ((88, 38, 124, 64), (88, 38, 124, 64))
    assert TM.rects(_box_image(0, 30, 200, 220), P0, K, 12) == ((0, 188, 43, 45), (0, 188, 43, 45))               # left
    assert TM.rects(_box_image(600, 639, 200, 220), P0, K, 12) == ((588, 188, 52, 45), (588, 188, 52, 45))        # right
    assert TM.rects(_box_image(300, 310, 0, 5), P0, K, 12) == ((288, 0, 35, 18), (288, 0, 35, 18))                # top
    assert TM.rects(_box_image(300, 310, 470, 479), P0, K, 12) == ((288, 458, 35, 22), (288, 458, 35, 22))        # bottom
    assert TM.rects(_box_image(5, 5, 7, 7), P0, K, 0) == ((5, 7, 1, 1), (5, 7, 1, 1))                             # one pixel, no margin
    assert TM.rects(_box_image(5, 5, 7, 7), P0, K, 3) == ((2, 4, 7, 7), (2, 4, 7, 7))
    assert TM.rects(_box_image(0, 0, 0, 0), P0, K, 1) == ((0, 0, 2, 2), (0, 0, 2, 2))                             # the corner pixel
    assert TM.rects(_box_image(639, 639, 479, 479), P0, K, 1) == ((638, 478, 2, 2), (638, 478, 2, 2))
    # a margin larger than the image: the whole image
    assert TM.rects(_box_image(300, 310, 200, 210), P0, K, 8192) == ((0, 0, W, H), (0, 0, W, H))
    # an empty render
    assert TM.rects(np.zeros((H, W), np.uint16), P0, K, 12) is None
    # two blobs: one box around both
    d = _box_image(10, 20, 30, 40)
    d[400:411, 500:521] = 5
    assert TM.rects(d, P0, K, 0) == ((10, 30, 511, 381), (10, 30, 511, 381))


def test_rule_shift_pushes_rect_ref_out_on_each_side():
    box = (100, 199, 50, 89)             # with margin 12: x 88..211, y 38..101
    r = TM.rects_from_box(box, W, H, 12, (7, -6))
    assert r == ((88, 38, 124, 64), (95, 32, 124, 64))
    # left: the reference rectangle loses its first 12 columns, and so does the model rectangle
    assert TM.rects_from_box(box, W, H, 12, (-100, 0)) == ((100, 38, 112, 64), (0, 38, 112, 64))
    # top
    assert TM.rects_from_box(box, W, H, 12, (0, -50)) == ((88, 50, 124, 52), (88, 0, 124, 52))
    # right: x 88 + 500 .. 639
    assert TM.rects_from_box(box, W, H, 12, (500, 0)) == ((88, 38, 52, 64), (588, 38, 52, 64))
    # bottom: y 38 + 400 .. 479
    assert TM.rects_from_box(box, W, H, 12, (0, 400)) == ((88, 38, 124, 42), (88, 438, 124, 42))
    # both at once, and sizes stay equal
    rm, rr = TM.rects_from_box(box, W, H, 12, (-95, 410))
    assert rm[2:] == rr[2:] and rr[0] == 0 and rr[1] + rr[3] == H and rm[0] - rr[0] == 95 and rm[1] - rr[1] == -410
    # pushed out entirely on each side: out of view
    for d in ((-212, 0), (552, 0), (0, -102), (0, 442), (10 ** 6, 0)):
        assert TM.rects_from_box(box, W, H, 12, d) is None, d
    # the last column / row still in view
    assert TM.rects_from_box(box, W, H, 12, (-211, 0)) == ((211, 38, 1, 64), (0, 38, 1, 64))
    assert TM.rects_from_box(box, W, H, 12, (0, 441)) == ((88, 38, 124, 1), (88, 479, 124, 1))


def test_shift_is_zero_for_the_model_camera_and_rounds_half_to_even():
    assert TM.shift(TM.MODEL_K, (123.0, -45.0, 700.0)) == (0, 0)
    assert TM.shift((608.0, 608.0, 327.4, 234.4), (0.0, 0.0, 700.0)) == (7, -6)
    assert TM.shift((608.0, 608.0, 320.5, 241.5), (0.0, 0.0, 700.0)) == (0, 2)          # rint: ties to even
    # fx = 600: (600 - 608) * (70 / 700) = -0.8, plus 7.4
    assert TM.shift((600.0, 608.0, 327.4, 234.4), (70.0, 0.0, 700.0)) == (7, -6)
    assert TM.shift((600.0, 600.0, 320.0, 240.0), (350.0, -175.0, 700.0)) == (-4, 2)
    # tz = 0, a pose behind the camera with a huge ratio, NaN: out of view (never an integer conversion of them)
    assert TM.shift((600.0, 608.0, 320.0, 240.0), (1.0, 0.0, 0.0)) is None
    assert TM.shift((600.0, 608.0, 320.0, 240.0), (0.0, 0.0, 0.0)) is None
    assert TM.shift((600.0, 608.0, 320.0, 240.0), (1e9, 0.0, 1e-3)) is None
    assert TM.shift(TM.MODEL_K, (1.0, 0.0, 0.0)) is None                                 # 0 * inf


def test_times10_round_trip_is_exact_up_to_6553_mm():
    d = np.arange(0, 65536, dtype=np.uint32).astype(np.uint16)
    back = TM.back_to_mm(TM.times10(d))
    assert np.array_equal(back[:6554], d[:6554])
    assert (TM.times10(d)[6554:] == 65535).all() and (back[6554:] == back[6554]).all()
    assert TM.times10(np.array([0, 1, 6553, 6554, 65535], np.uint16)).tolist() == [0, 10, 65530, 65535, 65535]


def test_oracle_detection_on_the_round_tripped_model_image_equals_the_mm_image(oracle):
    R, t = synth.object_pose(tx=10, ty=-5, tz=700)
    scene, _, _ = synth.render(W, H, R, t, seed=3)
    R2 = synth.rot_z(0.02) @ R
    p13 = synth.pose13(R2, t + np.array([4.0, -2.0, 3.0]))
    model = TM.render(synth.object_mesh(2), p13, W, H)
    assert 0 < model.max() <= 6553
    rm, rr = TM.rects(model, p13, TM.MODEL_K, 12)
    args = (scene, TM.MODEL_K, rm, rr, 10, 0.5, 0.01, R2.astype(np.float32), p13[[3, 7, 11]])
    a = oracle.detection(model, *args)
    b = oracle.detection(TM.back_to_mm(TM.times10(model)), *args)
    assert a["n_points"] == b["n_points"] > 5000
    for k in ("R_final", "T_final"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))
    assert a["icp"]["iters"] == b["icp"]["iters"] and a["icp"]["dist_mean"] == b["icp"]["dist_mean"]


def test_result_record_layout():
    assert RESULT_BYTES == 4 * (2 + 4 + 4 + 16) + C.sizeof(L.DetectionResult) == api.TRACK_DTYPE.itemsize
    assert api.TRACK_DTYPE.fields["pose"][1] == L.TrackResult.pose.offset and api.TRACK_DTYPE.fields["det"][1] == L.TrackResult.det.offset
    assert C.sizeof(L.TrackParams) == 32


def test_lost_rule():
    assert not TM.is_lost(1, 2.0, 0.9)
    assert TM.is_lost(0, 2.0, 0.9) and TM.is_lost(1, -1.0, 0.9)
    assert TM.is_lost(1, 2.0, 0.9, max_dist_mean=1.9) and not TM.is_lost(1, 2.0, 0.9, max_dist_mean=2.0)
    assert TM.is_lost(1, 2.0, 0.9, min_px_ratio=0.91) and not TM.is_lost(1, 2.0, 0.9, min_px_ratio=0.9)
    assert not TM.is_lost(1, 2.0, 0.9, max_dist_mean=-1.0, min_px_ratio=-1.0)           # <= 0: no test


def test_one_model_step_moves_towards_the_truth(oracle):
    mesh = synth.object_mesh(2)
    R0, t0 = synth.object_pose(10, -5, 720, 0.3, 0.35, 0.1)
    R1, t1 = synth.object_pose(14, -7, 723, 0.32, 0.34, 0.115)
    scene, _, _ = synth.render(W, H, R1, t1, seed=101)
    r = TM.step(mesh, synth.pose13(R0, t0), scene, TM.MODEL_K, oracle=oracle)
    before, after = TM.pose_error(TM.pose4x4(synth.pose13(R0, t0)), R1, t1), TM.pose_error(r["pose"], R1, t1)
    assert r["tracked"] == 1 and r["status"] == 0 and r["rect_model"] == r["rect_ref"]
    assert after[0] < before[0] and after[1] < 0.5 * before[1]
    # a crop over the limit, and a pose behind the camera
    over = TM.step(mesh, synth.pose13(R0, t0), scene, TM.MODEL_K, oracle=oracle, max_crop_px=r["rect_model"][2] * r["rect_model"][3] - 1)
    assert over["status"] == TM.OVERFLOW and over["tracked"] == 0 and over["rect_model"] == r["rect_model"] and over["det"] is None
    assert np.array_equal(over["pose"], TM.pose4x4(synth.pose13(R0, t0)))
    behind = TM.step(mesh, synth.pose13(R0, np.array([0.0, 0.0, -700.0])), scene, TM.MODEL_K, oracle=oracle)
    assert behind["status"] == 0 and behind["tracked"] == 0 and behind["rect_model"] == (0, 0, 0, 0)


# ---- argument refusals: none of them reaches a device call -------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_ctx():
    """A context without a device: the one a host-only detector carries (fl_dev_detector_create_host)."""
    det = api._host_only_detector(2, [5, 8])
    yield det.ctx.h
    det.close()


def _create(lib, ctx, V, T, w=W, h=H, max_frames=2, max_tracks=4, max_crop_px=40000, nv=None, nt=None, out=True):
    hd = C.c_void_p(0x1234)
    rc = lib.fl_tracker_create(ctx, None if V is None else V.ctypes.data, (100 if V is None else len(V)) if nv is None else nv, None if T is None else T.ctypes.data,
                               (100 if T is None else len(T)) if nt is None else nt, w, h, max_frames, max_tracks, max_crop_px, C.byref(hd) if out else None)
    return rc, hd.value


def test_tracker_create_refusals(host_ctx):
    lib = L.load()
    m = synth.object_mesh(0)
    V, T = np.ascontiguousarray(m["vertices"], np.float32), np.ascontiguousarray(m["triangles"], np.int32)
    bad_index, nan_vertex = T.copy(), V.copy()
    bad_index[3, 1] = len(V)
    nan_vertex[2, 0] = np.nan
    cases = [dict(V=None), dict(T=None), dict(out=False), dict(nv=2), dict(nt=0), dict(nv=(1 << 26) + 1), dict(T=bad_index), dict(V=nan_vertex),
             dict(w=0), dict(h=0), dict(w=8193), dict(h=8193), dict(max_frames=0), dict(max_tracks=0), dict(max_frames=(1 << 16) + 1),
             dict(max_tracks=(1 << 16) + 1), dict(max_crop_px=0), dict(max_crop_px=-5), dict(max_crop_px=W * H + 1),
             dict(w=8192, h=8192, max_crop_px=1 << 24),                # beyond the crop size the ICP's organised search is exact for
             dict(w=8192, h=8192, max_crop_px=(1 << 24) - 4, max_tracks=1 << 10)]     # more than 96 GB of workspaces
    for kw in cases:
        a = dict(V=V, T=T)
        a.update(kw)
        rc, hd = _create(lib, host_ctx, a.pop("V"), a.pop("T"), **a)
        assert rc == L.FL_ERR_INVALID and hd == 0x1234, kw
    assert _create(lib, None, V, T)[0] == L.FL_ERR_INVALID
    # everything in range: the refusal is the missing device, not an argument
    for kw in (dict(), dict(max_crop_px=W * H), dict(max_crop_px=1), dict(w=8192, h=8192, max_crop_px=(1 << 24) - 4, max_tracks=1)):
        rc, hd = _create(lib, host_ctx, V, T, **kw)
        assert rc == L.FL_ERR_NO_DEVICE and hd == 0x1234, kw


@pytest.fixture()
def host_tracker():
    lib = L.load()
    h = C.c_void_p()
    assert L.dev(lib, "fl_dev_tracker_create_host")(W, H, 2, 4, 40000, C.byref(h)) == L.FL_OK
    yield h
    lib.fl_tracker_destroy(h)


def test_track_batch_refusals(host_tracker):
    lib = L.load()
    frames = [np.zeros((H, W), np.uint16) for _ in range(3)]
    pose = np.tile(P0, (5, 1))
    sentinel = np.full(5, 0x5A, np.uint8).tobytes()

    def call(n_frames=2, depth="ok", mem=L.FL_MEM_HOST, n_tracks=2, fof=(0, 1), poses=pose, K=(W, H, 608.0, 608.0, 320.0, 240.0), prm=None,
             results=True, trk=host_tracker):
        dp = None if depth is None else (C.c_void_p * 3)(*[None if (depth == "null1" and i == 1) else f.ctypes.data for i, f in enumerate(frames)])
        fo = None if fof is None else np.array(list(fof) + [0] * 5, np.int32)
        ps = None if poses is None else np.ascontiguousarray(poses, np.float32)
        out = np.frombuffer(sentinel * RESULT_BYTES, np.uint8).copy()
        k = None if K is None else L.Intrinsics(*K)
        p = None if prm is None else L.TrackParams(**dict(dict(margin_px=12, passes=1, icp_it_thr=10, dist_mean_thr=0.5, dist_diff_thr=0.01,
                                                               icp_mode=2, max_dist_mean=0.0, min_px_ratio=0.0), **prm))
        rc = lib.fl_track_batch(trk, n_frames, dp, mem, n_tracks, None if fo is None else fo.ctypes.data, None if ps is None else ps.ctypes.data,
                                None if k is None else C.byref(k), None if p is None else C.byref(p), out.ctypes.data if results else None)
        assert (out == 0x5A).all(), "a refused call wrote results"
        return rc

    nan_pose, inf_pose = pose.copy(), pose.copy()
    nan_pose[1, 5] = np.nan
    inf_pose[0, 11] = np.inf
    nan13 = pose.copy()
    nan13[:, 12] = np.nan                                              # the 13th float is ignored
    bad = [dict(trk=None), dict(depth=None), dict(depth="null1"), dict(fof=None), dict(poses=None), dict(K=None), dict(results=False),
           dict(mem=2), dict(n_frames=0), dict(n_frames=3), dict(n_tracks=0), dict(n_tracks=5), dict(fof=(0, 2)), dict(fof=(-1, 0)),
           dict(poses=nan_pose), dict(poses=inf_pose), dict(K=(W, H, np.nan, 608.0, 320.0, 240.0)), dict(K=(W, H, 608.0, np.inf, 320.0, 240.0)),
           dict(K=(W, H, 608.0, 608.0, np.nan, 240.0)), dict(K=(W, H, 608.0, 608.0, 320.0, -np.inf)), dict(K=(W, H, 0.0, 608.0, 320.0, 240.0)),
           dict(K=(W, H, 608.0, -1.0, 320.0, 240.0)), dict(K=(W + 1, H, 608.0, 608.0, 320.0, 240.0)), dict(K=(W, H - 1, 608.0, 608.0, 320.0, 240.0)),
           dict(prm=dict(passes=0)), dict(prm=dict(passes=5)), dict(prm=dict(margin_px=-1)), dict(prm=dict(margin_px=8193)),
           dict(prm=dict(icp_it_thr=-1)), dict(prm=dict(icp_mode=3)), dict(prm=dict(icp_mode=-1)), dict(prm=dict(dist_mean_thr=np.nan)),
           dict(prm=dict(dist_diff_thr=np.inf)), dict(prm=dict(max_dist_mean=np.nan)), dict(prm=dict(min_px_ratio=np.nan))]
    for kw in bad:
        assert call(**kw) == L.FL_ERR_INVALID, kw
    # in range: what stops the call is the missing device
    for kw in (dict(), dict(poses=nan13), dict(n_tracks=4, fof=(0, 1, 1, 0)), dict(prm=dict(passes=4, margin_px=0)), dict(prm=dict(margin_px=8192)),
               dict(prm=dict(icp_mode=0, icp_it_thr=0, dist_diff_thr=-3.0e38)), dict(mem=L.FL_MEM_DEVICE), dict(n_frames=1, fof=(0, 0))):
        assert call(**kw) == L.FL_ERR_NO_DEVICE, kw


def test_python_surface_checks(host_tracker):
    class Ctx:
        lib = L.load()
    trk = api.Tracker.__new__(api.Tracker)
    trk.ctx, trk.lib, trk.handle, trk.w, trk.h = Ctx(), Ctx.lib, host_tracker, W, H
    with pytest.raises(ValueError):
        trk.track([np.zeros((H, W + 1), np.uint16)], [0], [P0], TM.MODEL_K)
    with pytest.raises(ValueError):
        trk.track([np.zeros((H, W), np.uint16)], [0, 0], [P0], TM.MODEL_K)
    with pytest.raises(TypeError):
        trk.track([np.zeros((H, W), np.uint16)], [0], [P0], TM.MODEL_K, margin=3)
    assert api.poses13_of(np.zeros(3, api.TRACK_DTYPE)).shape == (3, 13)
