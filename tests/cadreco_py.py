"""ctypes binding of libcadreco_hip.so's flat C shim (fealess_amd/cadreco/cadreco_c.h), for the tests that drive the C++
facade.  One table, as fealess_amd/_lib.py has for libfealess_hip.so: every pointer is declared, so a handle is never
truncated to 32 bits.  tests/test_cadreco_table_cpu.py holds the table against the header."""
import contextlib
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "fealess_amd", "cadreco", "libcadreco_hip.so")

INVALID, OPEN_FAILED = C.c_int(0x80000001).value, C.c_int(0x80000002).value   # ERROR_INVALID_PARAM, ERROR_OPEN_FILE_FAILED as ints

# _P, any pointer but a string: takes an address, a ctypes array, byref(...) or None
_P, _S, _I, _F, _D = C.c_void_p, C.c_char_p, C.c_int, C.c_float, C.c_double
_FRAME = [_P, _I, _I, _D, _D, _D, _D, _D]      # depth, w, h_, ts, fx, fy, cx, cy
_COLOUR_FRAME = [_P, _P, _I, _I, _D, _I, _I, _D, _D, _D, _D]   # bgr, depth, w, h_, ts, kw, kh, fx, fy, cx, cy

# name -> (restype, argtypes); every function cadreco_c.h declares
SIGNATURES = {
    "cadreco_create": (_P, [_I]),
    "cadreco_destroy": (None, [_P]),
    "cadreco_add_obj": (_I, [_P, _S]),
    "cadreco_version": (_S, []),
    "cadreco_set_params": (_I, [_P, _F, _I, _F, _F, _I]),
    "cadreco_set_multi_hypothesis": (_I, [_P, _I, _F]),
    "cadreco_set_multi_instance": (_I, [_P, _I, _I, _I]),
    "cadreco_set_verified_pick": (_I, [_P, _I, _F, _F, _F]),
    "cadreco_set_verified_tracking": (_I, [_P, _I, _F, _F, _F, _I]),
    "cadreco_recognition": (_I, [_P] + _COLOUR_FRAME + [_P, _P, _P, _I]),
    "cadreco_recognition_all": (_I, [_P] + _COLOUR_FRAME + [_P, _P, _I]),
    "cadreco_set_tracking_mesh": (_I, [_P, _S, _F]),
    "cadreco_set_tracking_meshes": (_I, [_P, _I, _P, _P, _F]),
    "cadreco_track": (_I, [_P] + _FRAME + [_I, _P, _P]),
    "cadreco_verify": (_I, [_P] + _FRAME + [_I, _P, _F, _P]),
    "cadreco_verify_tagged": (_I, [_P] + _FRAME + [_I, _P, _P, _F, _P]),
    "cadreco_arbitrate": (_I, [_P] + _FRAME + [_I, _P, _P, _F, _F, _P]),
    "cadreco_train_views": (_I, [_P, _S, _S, _I, _P, _P, _P, _I, _I, _P, _I, _P, _P]),
    "cadreco_train_mesh": (_I, [_P, _S, _S, _S, _F, _I, _I, _P, _I, _I, _F, _I, _P, _P, _I]),
    "cadreco_read_obj": (_I, [_S, _F, _P, _P, _P, _P, _P, _P, _I, _I]),
    "cadreco_read_linemod": (_I, [_S, _P, _P, _P, _P]),
    "cadreco_read_linemod_cached": (_I, [_S, _P, _P, _P]),
    "cadreco_read_png16": (_I, [_S, _P, _I, _P, _P]),
    "cadreco_write_png16": (_I, [_S, _P, _I, _I]),
}

_lib = None


def lib():
    """libcadreco_hip.so with every signature set; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


@contextlib.contextmanager
def handle(kind=1):
    """A CObjRecoCAD handle (kind 1: EObjReco_LmICP) as a c_void_p, destroyed on the way out."""
    h = C.c_void_p(lib().cadreco_create(kind))
    assert h.value
    try:
        yield h
    finally:
        lib().cadreco_destroy(h)


def frame_args(depth, ts, K):
    """(depth, w, h_, ts, fx, fy, cx, cy) of the track / verify / arbitrate entries; depth: a 2-D uint16 array."""
    return (depth.ctypes.data, depth.shape[1], depth.shape[0], ts, *K)


def recognition(h, bgr, depth, K, ts=1.0, camera_size=None):
    """cadreco_recognition on one frame; the camera K is of the frame's size unless camera_size = (kw, kh) says otherwise.
    Returns (code, number of results, tag of result 0, pose of result 0 as 16 floats)."""
    (hh, w), pose, tag, n = depth.shape, np.zeros(16, np.float32), C.create_string_buffer(64), C.c_int(-1)
    kw, kh = camera_size or (w, hh)
    rc = lib().cadreco_recognition(h, bgr.ctypes.data, depth.ctypes.data, w, hh, ts, kw, kh, *K, C.byref(n), pose.ctypes.data, tag, 64)
    return rc, n.value, tag.value, pose


def recognition_all(h, bgr, depth, K, cap=8):
    """cadreco_recognition_all on one frame: (code, number of results, their poses in a (cap, 16) array, zero beyond them)."""
    (hh, w), poses, n = depth.shape, np.zeros((cap, 16), np.float32), C.c_int(-1)
    rc = lib().cadreco_recognition_all(h, bgr.ctypes.data, depth.ctypes.data, w, hh, 1.0, w, hh, *K, C.byref(n), poses.ctypes.data, cap)
    return rc, n.value, poses


def train_mesh(h, d, obj, n_views, sphere, levels=2, T=(5, 8)):
    """cadreco_train_mesh of class "mesh" into directory d; sphere: dict(subdivisions, upper, distances, n_inplane, inplane_deg).
    Returns (code, template_of_view, -9 where the call wrote nothing)."""
    dist, Ta, tov = np.array(sphere["distances"], np.float32), (C.c_int * len(T))(*T), np.full(n_views, -9, np.int32)
    rc = lib().cadreco_train_mesh(h, str(d).encode(), b"mesh", str(obj).encode(), 1.0, sphere["subdivisions"], sphere["upper"],
                                  dist.ctypes.data, len(dist), sphere["n_inplane"], sphere["inplane_deg"], levels, Ta, tov.ctypes.data, n_views)
    return rc, tov


def read_obj(path, scale=1.0):
    """cadreco_read_obj in its two passes: (vertices, normals, triangles) as the facade reads the OBJ, normals None where the
    file has none; or, where the first pass fails, its code."""
    l, nv, nt, hn = lib(), C.c_int(), C.c_int(), C.c_int()
    path = str(path).encode()
    rc = l.cadreco_read_obj(path, scale, C.byref(nv), C.byref(nt), C.byref(hn), None, None, None, 0, 0)
    if rc:
        return rc
    V, N, T = np.zeros((nv.value, 3), np.float32), np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.int32)
    assert l.cadreco_read_obj(path, scale, C.byref(nv), C.byref(nt), C.byref(hn), V.ctypes.data, N.ctypes.data, T.ctypes.data,
                              nv.value, nt.value) == 0
    return V, (N if hn.value else None), T


def recognised_mesh_frame(h, ctx, obj, bank_dir):
    """Train class "mesh" on handle h from the OBJ (the views of an icosahedron's upper half at 700 mm), load it, and recognise a
    640 x 480 frame that shows the first view that gave a template in front of a sloping, chequered wall.  Returns the mesh as
    the facade reads it (V, N, T), the depth frame and the recognised pose as 16 floats."""
    from fealess_amd import api
    K0, W, H = (608.0, 608.0, 320.0, 240.0), 640, 480
    P = api.view_sphere(0, [700.0], n_inplane=1, inplane_deg=0.0, upper_hemisphere=True)
    rc, tov = train_mesh(h, bank_dir, obj, len(P), dict(subdivisions=0, upper=1, distances=[700.0], n_inplane=1, inplane_deg=0.0))
    assert rc == 0 and (tov >= 0).any() and lib().cadreco_add_obj(h, bank_dir.encode()) == 0
    V, N, T = read_obj(obj)
    view = P[int(np.flatnonzero(tov >= 0)[0])]
    bgr, dep, msk, _ = ctx.render_views(V, T, view[None], K0, W, H, normals=N)
    u, v = np.meshgrid(np.arange(float(W)), np.arange(float(H)))
    m = msk[0] > 0
    depth = np.ascontiguousarray(np.where(m, dep[0], np.rint(950.0 + 0.06 * u + 0.04 * v)).astype(np.uint16))
    cell = (np.floor(u / 23.0) + 2 * np.floor(v / 17.0)) % 5
    col = np.where(m[..., None], bgr[0].astype(np.float64), (70 + 30 * cell)[..., None] * np.array([1.0, 0.9, 0.75]))
    col = np.ascontiguousarray(np.clip(np.rint(col), 0, 255).astype(np.uint8))
    rc, n, tag, pose = recognition(h, col, depth, K0)
    assert rc == 0 and n == 1 and tag == b"mesh"
    return V, N, T, depth, pose
