"""CPU: depth registration (fl_register_depth_batch, include/fealess_hip.h) without a GPU -- what tests/register_model.py, the
numpy statement of the contract, does on hand-made cases and on a two-camera scene; the argument checks of the library itself,
which come before its first HIP call and so run on a context without a device (the one of fl_dev_detector_create_host); and the
refusals of the facade's shim with a null handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cadreco_depth_py as CD
import cadreco_py as CR
import register_cases as RC
import register_model as GM
import verify_model as VM
from fealess_amd import _lib as L

EYE, ZERO = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)


# ---- (a) the model on hand-made cases -------------------------------------------------------------------------------------------
def test_model_identity_gives_the_input_back():
    """Equal cameras and identity extrinsics: the footprint of a pixel is the pixel itself, at every depth a u16 holds."""
    rng = np.random.default_rng(0)
    for (w, h, K4) in [(64, 48, (60.0, 61.0, 31.5, 24.25)), (37, 23, (580.0, 580.0, 18.0, 12.0)), (640, 480, (608.0, 608.0, 320.0, 240.0))]:
        d = rng.integers(1, 65536, (h, w)).astype(np.uint16)
        d[rng.random((h, w)) < 0.2] = 0
        d[0, 0], d[h - 1, w - 1] = 65535, 1
        K = (w, h) + K4
        assert np.array_equal(GM.register(d, K, K, EYE, ZERO, fill_cracks=0), d)
        assert np.array_equal(GM.register(d, K, K, EYE, ZERO, fill_cracks=1), GM.fill(d))


def test_model_crack_rule():
    E = np.zeros((5, 7), np.uint16)
    E[1, 0], E[1, 2] = 700, 650                 # (1, 1): left and right present -> their minimum
    E[2, 4], E[4, 4] = 900, 800                 # (3, 4): only up and down present -> their minimum
    E[0, 5], E[0, 6] = 500, 0                   # (0, 6): a border pixel without a right neighbour, nothing above: stays 0
    F = GM.fill(E)
    assert F[1, 1] == 650 and F[3, 4] == 800 and F[0, 6] == 0
    changed = np.argwhere(F != E)
    assert sorted(map(tuple, changed)) == [(1, 1), (3, 4)]
    # left / right goes first where both pairs are present
    E = np.zeros((3, 3), np.uint16)
    E[1, 0], E[1, 2], E[0, 1], E[2, 1] = 40, 50, 10, 20
    assert GM.fill(E)[1, 1] == 40
    # border pixels with one pair only
    E = np.array([[5, 0, 7]], np.uint16)        # one row: left and right exist, up and down do not
    assert GM.fill(E).tolist() == [[5, 5, 7]]
    E = np.array([[5], [0], [7]], np.uint16)    # one column
    assert GM.fill(E).ravel().tolist() == [5, 5, 7]
    E = np.array([[0, 4], [3, 0]], np.uint16)   # corners: no pair exists
    assert np.array_equal(GM.fill(E), E)
    # two adjacent holes are not filled from filled values
    E = np.array([[9, 0, 0, 8]], np.uint16)
    assert GM.fill(E).tolist() == [[9, 0, 0, 8]]
    E = np.array([[0, 6, 0, 0], [9, 0, 0, 8], [0, 4, 0, 0]], np.uint16)    # (1, 1) fills from up / down; (1, 2) sees only the unfilled image
    assert GM.fill(E).tolist() == [[0, 6, 0, 0], [9, 4, 0, 8], [0, 4, 0, 0]]


def test_model_footprint_cap_and_minimum():
    """A footprint wider than FL_REGISTER_MAX_SPLAT is cut at x0 + 7 (y0 + 7); where footprints overlap the minimum decides."""
    d = np.zeros((6, 8), np.uint16)
    d[2, 3] = 1000
    Kd, Kc = (8, 6, 8.0, 8.0, 4.0, 3.0), (128, 96, 128.0, 128.0, 64.0, 48.0)        # 16 colour pixels per depth pixel, all exact in binary
    E = GM.splat(d, Kd, Kc, EYE, ZERO)
    ys, xs = np.nonzero(E)
    # the pixel spans [3 - 0.5 - 4, 3 + 0.5 - 4] / 8 * 128 + 64 = [40, 56] and rows [24, 40]: cut to 8 x 8 from the lower end
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (40, 47, 24, 31) and len(xs) == 64 and (E[ys, xs] == 1000).all()
    live, val, x0, x1, y0, y1 = GM.footprints(d, Kd, Kc, EYE, ZERO)
    assert live.sum() == 1 and (x1 - x0)[live][0] == GM.MAX_SPLAT - 1
    # a footprint smaller than a pixel lands only where it holds a pixel centre, its closed ends included: four depth pixels per
    # colour pixel here, u = 0 alone on column 0 ([0, 0.25]), u = 3 and u = 4 on column 1 ([0.75, 1] and [1, 1.25]), rows likewise;
    # where several land the nearest wins
    d = np.full((8, 8), 900, np.uint16)
    d[3, 3] = 650
    d[0, 0] = 0
    E = GM.splat(d, (8, 8, 32.0, 32.0, 4.0, 4.0), (2, 2, 8.0, 8.0, 1.125, 1.125), EYE, ZERO)
    assert E.tolist() == [[0, 900], [900, 650]]
    live = GM.footprints(d, (8, 8, 32.0, 32.0, 4.0, 4.0), (2, 2, 8.0, 8.0, 1.125, 1.125), EYE, ZERO)[0].reshape(8, 8)
    assert sorted(map(tuple, np.argwhere(live))) == [(0, 3), (0, 4), (3, 0), (3, 3), (3, 4), (4, 0), (4, 3), (4, 4)]
    # the transformed depth is stored, not the source depth; saturation at 65535
    d = np.full((4, 4), 65535, np.uint16)
    K = (4, 4, 50.0, 50.0, 2.0, 2.0)
    assert (GM.splat(d, K, K, EYE, np.array([0, 0, 10], np.float32)) == 65535).all()
    d[:] = 700
    assert (GM.splat(d, K, K, EYE, np.array([0, 0, -100], np.float32))[1:3, 1:3] == 600).all()
    assert not GM.splat(d, K, K, EYE, np.array([0, 0, -700], np.float32)).any()        # Z = 0 everywhere
    assert not GM.splat(d, K, K, np.diag([-1.0, 1.0, -1.0]), ZERO).any()                # 180 degrees about y: behind the camera


# ---- (b) the model does what registration is for ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_cameras():
    s = RC.scene()
    R, t = RC.extrinsics()
    E = GM.splat(s["depth_cam"], RC.K_DEPTH, RC.K_COLOR, R, t)
    Eh = GM.splat(s["depth_cam_half"], RC.K_DEPTH_HALF, RC.K_COLOR, R, t)
    return dict(s, E=E, F=GM.fill(E), Eh=Eh)


def _pp(measured, stated):
    """Within one percentage point of the figure the issue states (both as fractions)."""
    return abs(measured - stated) <= 0.01


def _near(measured, model):
    """Within 3 % of the count this model gave when it was measured."""
    return abs(int(measured) - model) <= 0.03 * model


def test_model_registers_the_depth_camera_onto_the_colour_camera(two_cameras):
    """The depth camera's render of the scene, registered, against the colour camera's own render of it (307200 pixels, all with
    depth).  Measured with this model:
      without the fill   both have depth and lie within 2 mm: 304564 of 304797 = 99.92 %; empty where the direct render has depth:
                         2403 = 0.78 %, 733 of them isolated (all four neighbours have depth)
      with the fill      915 pixels filled, 1488 still empty; 879 of the filled ones within 2 mm = 96.1 %; overall 305443 of
                         305712 = 99.91 %
      320 x 240 depth camera (K = 290 / 290 / 159 / 121) onto 640 x 480: within 2 mm 304151 of 305030 = 99.71 %; empty 2170 =
                         0.71 %; isolated cracks 0
    A prototype of the contract on this scene gave 99.92 %, 0.74 % (2273, 634 isolated), 793 filled, 1480 still empty, 95.6 %,
    99.91 %, 99.7 %, 0.63 %, 0: the assertions hold this model within one percentage point of those shares, and the counts within
    3 % of this model's own figures above."""
    c, direct = two_cameras, two_cameras["color_cam"]
    n = direct.size
    assert (direct != 0).all()
    a, b, h = RC.compare(c["E"], direct), RC.compare(c["F"], direct), RC.compare(c["Eh"], direct)
    filled = (c["E"] == 0) & (c["F"] != 0)
    close = np.abs(c["F"].astype(np.int64) - direct.astype(np.int64)) <= 2
    print("no fill", a, "fill", b, "filled", int(filled.sum()), "of them within 2 mm", int((filled & close).sum()), "half", h)
    assert _pp(a["within2"] / a["both"], 0.9992)
    assert _pp(a["empty"] / n, 0.0074)
    # the counts are held to what this model measures (the docstring), within 3 %: a percentage point of the image is 3072 pixels,
    # which would let any of them pass; the prototype's 634, 793 and 1480 lie 14 %, 13 % and 0.5 % away, its scene's quad and this one's differ
    assert _near(a["empty"], 2403) and _near(a["isolated"], 733) and _near(filled.sum(), 915) and _near(b["empty"], 1488)
    assert _near((filled & close).sum(), 879) and _near(h["empty"], 2170) and h["isolated"] <= 2
    assert filled.sum() + b["empty"] == a["empty"]                         # the fill only ever fills
    assert _pp((filled & close).sum() / filled.sum(), 0.956)
    assert _pp(b["within2"] / b["both"], 0.9991)
    assert _pp(h["within2"] / h["both"], 0.997) and _pp(h["empty"] / n, 0.0063) and _pp(h["isolated"] / n, 0.0)
    assert (c["F"][c["E"] != 0] == c["E"][c["E"] != 0]).all()


def test_model_registered_frame_verifies_like_the_direct_render(two_cameras):
    """verify_model.verify (tau 10 mm) at the true pose, expressed in the colour camera: n_inlier / n_model is 15671 / 15671 on the
    colour camera's own render and 15562 / 15671 = 0.9930 on the registered frame with the fill (63 pixels without depth, 3 in
    front, 43 behind: the object's silhouette, where the depth camera saw the backdrop); 15334 / 15671 = 0.9785 without the fill."""
    c = two_cameras
    rec = VM.verify(c["mesh"], [c["color_cam"], c["F"], c["E"]], [0, 1, 2], np.stack([c["pose13_color"]] * 3), RC.K_COLOR[2:])
    ratio = rec["n_inlier"] / rec["n_model"]
    print(rec, ratio)
    assert VM.invariant(rec) and rec["n_model"][0] > 10000 and (rec["n_model"] == rec["n_model"][0]).all()
    assert abs(ratio[1] - ratio[0]) <= 0.01
    assert ratio[2] <= ratio[1]


# ---- (c) the library's argument checks, on a context without a device --------------------------------------------------------------
WD, HD, WC, HC = 16, 12, 20, 14


@pytest.fixture(scope="module")
def host_ctx():
    lib = L.load()
    det = C.c_void_p()
    assert L.dev(lib, "fl_dev_detector_create_host")(2, 2, (C.c_int * 2)(5, 8), C.byref(det)) == 0 and det.value
    ctx = C.c_void_p(lib.fl_detector_get_context(det))
    assert ctx.value and lib.fl_context_get_device(ctx) == -1
    yield lib, ctx
    lib.fl_detector_destroy(det)


def _call(lib, host, **over):
    """fl_register_depth_batch with valid arguments (two frames) except for what `over` replaces.  Returns (rc, outputs untouched?)."""
    a = dict(ctx=host, n_frames=2, depth=[np.full((HD, WD), 700, np.uint16)] * 2, mem=L.FL_MEM_HOST, Kd=(WD, HD, 15.0, 15.5, 8.0, 6.0),
             Kc=(WC, HC, 19.0, 19.5, 10.0, 7.0), R=np.eye(3), t=(25.0, -1.0, 2.0), ext=True, params=1, out=True, out_hole=False)
    a.update(over)
    outs = [np.full((HC, WC), 0xA5A5, np.uint16) for _ in range(2)]
    dp = None if a["depth"] is None else (C.c_void_p * max(1, len(a["depth"])))(*[None if d is None else d.ctypes.data for d in a["depth"]])
    op = None if not a["out"] else (C.c_void_p * 2)(outs[0].ctypes.data, None if a["out_hole"] else outs[1].ctypes.data)
    kd = None if a["Kd"] is None else L.Intrinsics(*a["Kd"])
    kc = None if a["Kc"] is None else L.Intrinsics(*a["Kc"])
    ext = None
    if a["ext"]:
        ext = L.Extrinsics((C.c_float * 9)(*np.asarray(a["R"], np.float32).ravel()), (C.c_float * 3)(*np.asarray(a["t"], np.float32)))
    prm = None if a["params"] is None else L.RegisterParams(a["params"])
    rc = lib.fl_register_depth_batch(a["ctx"], a["n_frames"], dp, a["mem"], None if kd is None else C.byref(kd), None if kc is None else C.byref(kc),
                                     None if ext is None else C.byref(ext), None if prm is None else C.byref(prm), op)
    return rc, all((o == 0xA5A5).all() for o in outs)


NAN, INF = float("nan"), float("inf")


def _rot(i, j, v):
    R = np.eye(3)
    R[i, j] = v
    return R


INVALID = {
    "ctx null": dict(ctx=None), "n_frames 0": dict(n_frames=0), "n_frames negative": dict(n_frames=-3),
    "depth null": dict(depth=None), "out null": dict(out=False), "K_depth null": dict(Kd=None), "K_color null": dict(Kc=None),
    "extrinsics null": dict(ext=False), "a null input frame": dict(depth=[np.zeros((HD, WD), np.uint16), None]), "a null output frame": dict(out_hole=True),
    "mem 2": dict(mem=2), "mem -1": dict(mem=-1),
    "depth width 0": dict(Kd=(0, HD, 15.0, 15.5, 8.0, 6.0)), "depth height negative": dict(Kd=(WD, -1, 15.0, 15.5, 8.0, 6.0)),
    "colour width above the maximum": dict(Kc=(8193, HC, 19.0, 19.5, 10.0, 7.0)), "colour height 0": dict(Kc=(WC, 0, 19.0, 19.5, 10.0, 7.0)),
    "depth height above the maximum": dict(Kd=(WD, 8193, 15.0, 15.5, 8.0, 6.0)),
    "depth fx nan": dict(Kd=(WD, HD, NAN, 15.5, 8.0, 6.0)), "depth fy inf": dict(Kd=(WD, HD, 15.0, INF, 8.0, 6.0)),
    "depth fx 0": dict(Kd=(WD, HD, 0.0, 15.5, 8.0, 6.0)), "depth fy negative": dict(Kd=(WD, HD, 15.0, -15.5, 8.0, 6.0)),
    "depth cx nan": dict(Kd=(WD, HD, 15.0, 15.5, NAN, 6.0)), "depth cy -inf": dict(Kd=(WD, HD, 15.0, 15.5, 8.0, -INF)),
    "colour fx 0": dict(Kc=(WC, HC, 0.0, 19.5, 10.0, 7.0)), "colour fy nan": dict(Kc=(WC, HC, 19.0, NAN, 10.0, 7.0)),
    "colour fx negative": dict(Kc=(WC, HC, -19.0, 19.5, 10.0, 7.0)), "colour cx inf": dict(Kc=(WC, HC, 19.0, 19.5, INF, 7.0)),
    "colour cy nan": dict(Kc=(WC, HC, 19.0, 19.5, 10.0, NAN)), "depth fx 0 as a float": dict(Kd=(WD, HD, 1e-60, 15.5, 8.0, 6.0)),
    "colour cx inf as a float": dict(Kc=(WC, HC, 19.0, 19.5, 1e300, 7.0)),
    "R nan": dict(R=_rot(1, 1, NAN)), "R inf": dict(R=_rot(0, 2, INF)), "t nan": dict(t=(0.0, NAN, 0.0)), "t -inf": dict(t=(0.0, 0.0, -INF)),
    "R scaled": dict(R=np.eye(3) * 1.01), "R sheared": dict(R=_rot(0, 1, 0.01)), "R zero": dict(R=np.zeros((3, 3))),
    "R a reflection": dict(R=np.diag([1.0, 1.0, -1.0])), "R off by 2e-3": dict(R=_rot(2, 2, 1.001)),
    "fill_cracks 2": dict(params=2), "fill_cracks -1": dict(params=-1),
}
VALID = [dict(), dict(params=None), dict(params=0), dict(mem=L.FL_MEM_DEVICE), dict(n_frames=1), dict(R=GM.rodrigues(RC.RVEC)),
         dict(R=GM.rodrigues((0.0, np.pi, 0.0))), dict(R=_rot(0, 1, 5e-4)), dict(Kd=(8192, 8192, 15.0, 15.5, 8.0, 6.0), depth=[np.zeros(1, np.uint16)] * 2),
         dict(Kd=(WD, HD, 15.0, 15.5, -8.0, 600.0)), dict(t=(1e30, 0.0, 0.0))]


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_are_refused_before_any_device_work(host_ctx, case):
    lib, ctx = host_ctx
    rc, untouched = _call(lib, ctx, **INVALID[case])
    assert rc == L.FL_ERR_INVALID and untouched, case


def test_valid_arguments_reach_the_device_check(host_ctx):
    """Everything the contract allows passes the checks and then fails for want of a device, with nothing written."""
    lib, ctx = host_ctx
    for over in VALID:
        rc, untouched = _call(lib, ctx, **over)
        assert rc == L.FL_ERR_NO_DEVICE and untouched, over


def test_header_states_the_contract():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "fealess_hip.h")).read()
    assert int(re.search(r"#define FL_REGISTER_MAX_SPLAT (\d+)", hdr).group(1)) == GM.MAX_SPLAT == L.FL_REGISTER_MAX_SPLAT
    assert int(re.search(r"#define FL_REGISTER_CHUNK_FRAMES (\d+)", hdr).group(1)) == L.FL_REGISTER_CHUNK_FRAMES
    assert C.sizeof(L.Extrinsics) == 48 and C.sizeof(L.RegisterParams) == 4
    assert "Lens distortion is out of scope" in hdr


# ---- (d) the facade's shim, with a null handle --------------------------------------------------------------------------------------
def test_facade_refusals_with_a_null_handle():
    """cadreco_set_depth_camera refuses `on` outside {0, 1} and a null R or t before anything touches the handle, and a null handle
    is not a handle of this library whatever the other arguments are: ERROR_INVALID_PARAM each time."""
    K = (640, 480, 580.0, 580.0, 318.0, 242.0)
    R, t = RC.extrinsics()
    for on in (2, -1):
        assert CD.set_depth_camera(None, on, K, R, t) == CR.INVALID
    assert CD.set_depth_camera(None, 1, K, None, t) == CR.INVALID and CD.set_depth_camera(None, 1, K, R, None) == CR.INVALID
    assert CD.set_depth_camera(None, 1, K, R, t) == CR.INVALID and CD.set_depth_camera(None, 0, K, None, None) == CR.INVALID
    pose, tag, n = np.full(16, 7, np.float32), C.create_string_buffer(8), C.c_int(-1)
    img = np.zeros((480, 640, 3), np.uint8)
    assert CD.lib().cadreco_recognition_depth(None, img.ctypes.data, 640, 480, img.ctypes.data, 640, 480, 1.0, 608.0, 608.0, 320.0, 240.0,
                                              C.byref(n), pose.ctypes.data, tag, 8) == CR.INVALID
    assert n.value == -1 and (pose == 7).all()


def test_facade_refusals_on_a_handle():
    """On a real handle (it needs no GPU to exist): every camera fl_register_depth_batch would refuse is refused when it is set;
    on = 0 always succeeds; a good camera is ERROR_UNKNOW without a GPU and SUCCESS with one."""
    import torch
    K = (640, 480, 580.0, 580.0, 318.0, 242.0)
    R, t = RC.extrinsics()
    with CR.handle() as h:
        assert CD.set_depth_camera(h, 0, K, None, None) == 0
        bad = [dict(K=(0, 480) + K[2:]), dict(K=(640, 8193) + K[2:]), dict(K=(640, 480, 0.0, 580.0, 318.0, 242.0)), dict(K=(640, 480, 580.0, NAN, 318.0, 242.0)),
               dict(K=(640, 480, 580.0, 580.0, INF, 242.0)), dict(R=np.eye(3) * 1.01), dict(R=np.diag([1.0, 1.0, -1.0])), dict(R=_rot(0, 0, NAN)),
               dict(t=(0.0, INF, 0.0)), dict(fill=2), dict(fill=-1), dict(on=2)]
        for o in bad:
            assert CD.set_depth_camera(h, o.get("on", 1), o.get("K", K), o.get("R", R), o.get("t", t), o.get("fill", 1)) == CR.INVALID, o
        want = 0 if torch.cuda.is_available() else C.c_int(0x80000005).value            # ERROR_UNKNOW
        assert CD.set_depth_camera(h, 1, K, R, t, 1) == want
        assert CD.set_depth_camera(h, 0, K, R, t, 1) == 0


def test_the_depth_shim_table_is_its_header():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(CR.ROOT, "fealess_amd", "cadreco", "cadreco_depth_c.h")).read(), flags=re.S)
    decl = dict(re.findall(r"\b(cadreco_\w+)\s*\(([^()]*)\)\s*;", text))
    assert sorted(decl) == sorted(CD.SIGNATURES)
    lib = CD.lib()
    for name, params in decl.items():
        params = [p.strip() for p in params.split(",")]
        res, args = CD.SIGNATURES[name]
        assert getattr(lib, name) is not None and len(args) == len(params), name
        for p, a in zip(params, args):
            assert ("*" in p) == (a is C.c_void_p), (name, p)
