"""GPU: CadRecoTrainViews (cadreco_train_views) writes a data directory that AddObj reads and Recognition uses like the
oracle: linemod_templates.yml with one class, depth/<template_id>.png per template (a failing view gets no id), and a
pose within 1e-4 of oracle.recognition on the oracle-trained bank."""
import ctypes as C
import os

import numpy as np
import pytest

from cadreco_py import INVALID, OPEN_FAILED, lib as _lib, recognition
from fealess_amd import synth
from fealess_amd.bank import TemplateBank

pytestmark = pytest.mark.gpu


def _views():
    out = []
    for k in range(5):
        rng = np.random.default_rng(40 + k)
        R, t = synth.object_pose(tx=float(rng.uniform(-50, 50)), ty=float(rng.uniform(-30, 30)), tz=float(rng.uniform(560, 720)),
                                 yaw=float(rng.uniform(-0.8, 0.8)), tilt=float(rng.uniform(0.2, 0.5)), roll=float(rng.uniform(-0.2, 0.2)))
        depth, bgr, mask = synth.render(640, 480, R, t, seed=40 + k, noise=False, background=True)
        out.append([np.ascontiguousarray(bgr), np.ascontiguousarray(depth), np.ascontiguousarray((mask * 255).astype(np.uint8)),
                    synth.pose13(R, t).astype(np.float32)])
    out[2][0] = np.zeros((480, 640, 3), np.uint8)                             # a flat view: addTemplate returns -1
    out[2][1] = np.full((480, 640), 900, np.uint16)
    out[2][2] = None
    return out


def _train(lib, h, d, views, levels=2, T=(5, 8)):
    n = len(views)
    bp = (C.c_void_p * n)(*[v[0].ctypes.data for v in views])
    dp = (C.c_void_p * n)(*[v[1].ctypes.data for v in views])
    mp = (C.c_void_p * n)(*[None if v[2] is None else v[2].ctypes.data for v in views])
    poses = np.ascontiguousarray(np.stack([v[3] for v in views]), np.float32)
    Ta = (C.c_int * len(T))(*T)
    tov = np.full(n, -9, np.int32)
    rc = lib.cadreco_train_views(h, str(d).encode(), b"obj", n, bp, dp, mp, 640, 480, poses.ctypes.data, levels, Ta, tov.ctypes.data)
    return rc, tov


def test_train_views_then_add_obj_and_recognise(tmp_path, oracle):
    lib = _lib()
    h = C.c_void_p(lib.cadreco_create(1))                                    # EObjReco_LmICP
    assert h.value
    views = _views()
    d = tmp_path / "obj"
    rc, tov = _train(lib, h, d, views)
    assert rc == 0
    assert tov.tolist() == [0, 1, -1, 2, 3]
    lv, nc, nt, nf = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert lib.cadreco_read_linemod(str(d / "linemod_templates.yml").encode(), C.byref(lv), C.byref(nc), C.byref(nt), C.byref(nf)) == 0
    assert (lv.value, nc.value, nt.value, nf.value) == (2, 1, 4, 4 * (63 + 63 + 31 + 31))
    assert sorted(os.listdir(d / "depth")) == ["0.png", "1.png", "2.png", "3.png"]
    px = np.zeros(640 * 480, np.uint16)
    w, hh = C.c_int(), C.c_int()
    for v, tid in enumerate(tov):
        if tid < 0:
            continue
        assert lib.cadreco_read_png16(str(d / "depth" / f"{tid}.png").encode(), px.ctypes.data, px.size, C.byref(w), C.byref(hh)) == 0
        assert (w.value, hh.value) == (640, 480)
        assert np.array_equal(px.reshape(480, 640), (views[v][1].astype(np.uint32) * 10).clip(0, 65535).astype(np.uint16))

    bank = TemplateBank("obj", 2, 2)                                          # the same class, trained by the oracle
    for b, dep, m, p13 in views:
        exp = oracle.add_template(b, dep, m, 2)
        if exp is None:
            continue
        t_o, f_o, _ = exp
        bank.add_pyramid([dict(width=int(t["width"]), height=int(t["height"]), offset_x=int(t["offset_x"]),
                               offset_y=int(t["offset_y"]), pyramid_level=int(t["pyramid_level"]),
                               features=np.stack([f["x"], f["y"], f["label"]], 1)) for t, f in zip(t_o, f_o)], p13,
                         (dep.astype(np.uint32) * 10).clip(0, 65535).astype(np.uint16))
    assert bank.n_pyramids == 4

    assert lib.cadreco_add_obj(h, str(d).encode()) == 0
    for v in (1, 3):
        bgr, depth = views[v][0], views[v][1]
        rc, n, tag, pose = recognition(h, bgr, depth, (synth.FX, synth.FY, synth.CX, synth.CY))
        assert rc == 0 and n == 1 and tag == b"obj"
        exp = oracle.recognition(bgr, depth, (synth.FX, synth.FY, synth.CX, synth.CY), [5, 8], bank, 75.0, 10, 0.5, 0.01)
        assert exp["found"] == 1
        assert np.abs(pose.reshape(4, 4) - exp["pose"]).max() <= 1e-4
    lib.cadreco_destroy(h)


def test_train_views_refuses_and_writes_nothing(tmp_path):
    lib = _lib()
    h = C.c_void_p(lib.cadreco_create(1))
    views = _views()
    flat = [views[2]] * 3                                                     # no view yields a template
    d = tmp_path / "none"
    rc, tov = _train(lib, h, d, flat)
    assert rc == INVALID and not d.exists() and (tov == -9).all()
    assert _train(lib, h, tmp_path / "l0", views, levels=0, T=(5,))[0] == INVALID
    assert _train(lib, h, tmp_path / "t0", views, levels=2, T=(5, 0))[0] == INVALID
    assert not (tmp_path / "l0").exists() and not (tmp_path / "t0").exists()
    rc, _ = _train(lib, h, tmp_path / "missing" / "parent", views)
    assert rc == OPEN_FAILED
    lib.cadreco_destroy(h)
