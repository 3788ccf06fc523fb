"""tests/cadreco_py.py against fealess_amd/cadreco/cadreco_c.h and the shared object, and the refusals of the C shim that
come before anything touches the handle (so they run with a null handle and without a GPU)."""
import ctypes as C
import os
import re

import numpy as np

import cadreco_py as CR

HEADER = os.path.join(CR.ROOT, "fealess_amd", "cadreco", "cadreco_c.h")
INVALID = CR.INVALID


def _declarations():
    """name -> list of parameter strings, from the header's flat C declarations"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    out = {}
    for name, params in re.findall(r"\b(cadreco_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name not in out, name
        params = [p.strip() for p in params.split(",")]
        out[name] = [] if params == ["void"] else params
    return out


def test_the_table_is_the_header():
    decl = _declarations()
    assert len(decl) >= 24 and sorted(decl) == sorted(CR.SIGNATURES)                                 # none missing, none the header lacks
    lib = CR.lib()
    for name, params in decl.items():
        res, args = CR.SIGNATURES[name]
        assert getattr(lib, name) is not None                                        # resolves in the shared object
        assert len(args) == len(params), (name, params)
        if params and re.fullmatch(r"void\s*\*\s*h", params[0]):
            assert args[0] is C.c_void_p, name
        for p, a in zip(params, args):                                               # a pointer is never left to the int default
            assert ("*" in p) == (a in (C.c_void_p, C.c_char_p)), (name, p)
    assert CR.SIGNATURES["cadreco_create"][0] is C.c_void_p
    assert sum(1 for p in decl.values() if p and re.fullmatch(r"void\s*\*\s*h", p[0])) >= 16


def test_refusals_before_the_handle():
    lib = CR.lib()
    poses, out, tracked = np.tile(np.eye(4, dtype=np.float32).reshape(16), (2, 1)), np.zeros(2 * 11, np.int32), np.zeros(2, np.int32)
    f = CR.frame_args(np.zeros((480, 640), np.uint16), 0.0, (600.0, 600.0, 320.0, 240.0))
    p, o, t = poses.ctypes.data, out.ctypes.data, tracked.ctypes.data
    tags = (C.c_char_p * 2)(b"a", b"b")
    holed = (C.c_char_p * 2)(b"a", None)
    # n < 0
    assert lib.cadreco_track(None, *f, -1, p, t) == INVALID
    assert lib.cadreco_verify(None, *f, -1, p, 10.0, o) == INVALID
    assert lib.cadreco_verify_tagged(None, *f, -1, p, tags, 10.0, o) == INVALID
    assert lib.cadreco_arbitrate(None, *f, -1, p, tags, 10.0, 0.5, o) == INVALID
    # a null poses16 or out with n > 0
    assert lib.cadreco_track(None, *f, 2, None, t) == INVALID and lib.cadreco_track(None, *f, 2, p, None) == INVALID
    assert lib.cadreco_verify(None, *f, 2, None, 10.0, o) == INVALID and lib.cadreco_verify(None, *f, 2, p, 10.0, None) == INVALID
    assert lib.cadreco_verify_tagged(None, *f, 2, None, tags, 10.0, o) == INVALID
    assert lib.cadreco_verify_tagged(None, *f, 2, p, tags, 10.0, None) == INVALID
    assert lib.cadreco_arbitrate(None, *f, 2, None, tags, 10.0, 0.5, o) == INVALID
    assert lib.cadreco_arbitrate(None, *f, 2, p, tags, 10.0, 0.5, None) == INVALID
    # a null element in tags; null tags to the tagged entry
    assert lib.cadreco_verify_tagged(None, *f, 2, p, holed, 10.0, o) == INVALID
    assert lib.cadreco_arbitrate(None, *f, 2, p, holed, 10.0, 0.5, o) == INVALID
    assert lib.cadreco_verify_tagged(None, *f, 2, p, None, 10.0, o) == INVALID
    # a null obj_path
    assert lib.cadreco_set_tracking_mesh(None, None, 1.0) == INVALID
    assert lib.cadreco_read_obj(None, 1.0, None, None, None, None, None, None, 0, 0) == INVALID
    dist = (C.c_float * 1)(700.0)
    assert lib.cadreco_train_mesh(None, b"dir", b"id", None, 1.0, 0, 1, dist, 1, 1, 0.0, 2, (C.c_int * 2)(5, 8), None, 0) == INVALID
    # cadreco_set_tracking_meshes: n < 1, a null list, a null entry
    assert lib.cadreco_set_tracking_meshes(None, 0, tags, tags, 1.0) == INVALID
    assert lib.cadreco_set_tracking_meshes(None, -1, tags, tags, 1.0) == INVALID
    assert lib.cadreco_set_tracking_meshes(None, 2, None, tags, 1.0) == INVALID and lib.cadreco_set_tracking_meshes(None, 2, tags, None, 1.0) == INVALID
    assert lib.cadreco_set_tracking_meshes(None, 2, holed, tags, 1.0) == INVALID and lib.cadreco_set_tracking_meshes(None, 2, tags, holed, 1.0) == INVALID
    # nothing was written
    assert not out.any() and not tracked.any() and np.array_equal(poses[0], np.eye(4, dtype=np.float32).reshape(16))
