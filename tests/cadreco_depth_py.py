"""ctypes binding of the depth-camera shim of libcadreco_hip.so (fealess_amd/cadreco/cadreco_depth_c.h), beside tests/cadreco_py.py,
whose table stays the table of cadreco_c.h.  Every pointer is declared, so a handle is never truncated to 32 bits."""
import ctypes as C

import numpy as np

import cadreco_py as CR

_P, _I, _D = C.c_void_p, C.c_int, C.c_double

# name -> (restype, argtypes); every function cadreco_depth_c.h declares
SIGNATURES = {
    "cadreco_set_depth_camera": (_I, [_P, _I, _I, _I, _D, _D, _D, _D, _P, _P, _I]),
    "cadreco_recognition_depth": (_I, [_P, _P, _I, _I, _P, _I, _I, _D, _D, _D, _D, _D, _P, _P, _P, _I]),
}

_bound = False


def lib():
    """libcadreco_hip.so (cadreco_py.lib()) with the signatures above set as well."""
    global _bound
    l = CR.lib()
    if not _bound:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return l


def set_depth_camera(h, on, K_depth, R, t, fill_cracks=1):
    """cadreco_set_depth_camera; K_depth = (w, h, fx, fy, cx, cy); R (3, 3) and t (3,), or None."""
    Ra = None if R is None else np.ascontiguousarray(R, np.float32).ravel()
    ta = None if t is None else np.ascontiguousarray(t, np.float32).ravel()
    return lib().cadreco_set_depth_camera(h, on, int(K_depth[0]), int(K_depth[1]), *[float(x) for x in K_depth[2:]],
                                          None if Ra is None else Ra.ctypes.data, None if ta is None else ta.ctypes.data, fill_cracks)


def recognition_depth(h, bgr, depth, K, ts=1.0):
    """cadreco_recognition_depth on one frame whose depth image has its own size; K = (fx, fy, cx, cy) of the colour image.
    Returns (code, number of results, tag of result 0, pose of result 0 as 16 floats)."""
    pose, tag, n = np.zeros(16, np.float32), C.create_string_buffer(64), C.c_int(-1)
    rc = lib().cadreco_recognition_depth(h, bgr.ctypes.data, bgr.shape[1], bgr.shape[0], depth.ctypes.data, depth.shape[1], depth.shape[0], ts,
                                         *K, C.byref(n), pose.ctypes.data, tag, 64)
    return rc, n.value, tag.value, pose
