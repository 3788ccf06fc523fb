"""GPU: fl_extract_template_batch (Detector::addTemplate for a batch of training views, linemod.cpp:1579-1615) view by view
against the oracle's orc_add_template and against fl_extract_template_pyramid, bit-exact: masks on some views only,
views that must fail in the middle of the batch, device inputs, a batch that crosses the chunk limit, odd geometry,
argument errors, and a class trained from a batch that recognises like the oracle-trained one."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from fealess_amd import _lib as L
from fealess_amd import api, synth
from fealess_amd.bank import TemplateBank

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chunk_views():
    hdr = open(os.path.join(ROOT, "include", "fealess_hip.h")).read()
    return int(re.search(r"#define FL_EXTRACT_CHUNK_VIEWS (\d+)", hdr).group(1))


def _view(seed, w=640, h=480):
    rng = np.random.default_rng(seed)
    s = w / 640.0
    R, t = synth.object_pose(tx=float(rng.uniform(-60, 60)), ty=float(rng.uniform(-40, 40)), tz=float(rng.uniform(520, 760)),
                             yaw=float(rng.uniform(-1.0, 1.0)), tilt=float(rng.uniform(0.1, 0.6)), roll=float(rng.uniform(-0.3, 0.3)))
    depth, bgr, mask = synth.render(w, h, R, t, seed=seed, noise=False, background=True, fx=synth.FX * s, fy=synth.FY * s,
                                    cx=w / 2.0, cy=h / 2.0)
    return bgr, depth, (mask * 255).astype(np.uint8), synth.pose13(R, t)


def _views(n, w=640, h=480, seed0=100, failing=True):
    """n rendered views, masks on two thirds of them; with `failing`, a flat image and a view whose mask is 4x4 pixels
    (too few candidates for 63 features) in the middle."""
    bgrs, depths, masks = [], [], []
    for k in range(n):
        b, d, m, _ = _view(seed0 + k, w, h)
        bgrs.append(b)
        depths.append(d)
        masks.append(m if k % 3 != 2 else None)
    if failing:
        tiny = np.zeros((h, w), np.uint8)
        tiny[h // 2:h // 2 + 4, w // 2:w // 2 + 4] = 255
        mid = n // 2
        bgrs[mid:mid] = [np.zeros((h, w, 3), np.uint8), bgrs[0]]
        depths[mid:mid] = [np.full((h, w), 1000, np.uint16), depths[0]]
        masks[mid:mid] = [None, tiny]
    return bgrs, depths, masks


def _same_as_oracle(got, exp):
    if exp is None:
        assert got is None
        return
    assert got is not None
    tl_g, bb_g = got
    tl_e, feats_e, bb_e = exp
    assert tuple(bb_g) == tuple(bb_e)
    assert len(tl_g) == len(tl_e)
    for k, t in enumerate(tl_g):
        for key in ("width", "height", "offset_x", "offset_y", "pyramid_level"):
            assert t[key] == int(tl_e[k][key]), (k, key)
        f = feats_e[k]
        assert np.array_equal(t["features"], np.stack([f["x"], f["y"], f["label"]], 1)), k


def _same(a, b):
    if a is None or b is None:
        assert a is None and b is None
        return
    assert tuple(a[1]) == tuple(b[1])
    assert len(a[0]) == len(b[0])
    for ta, tb in zip(a[0], b[0]):
        for key in ("width", "height", "offset_x", "offset_y", "pyramid_level"):
            assert ta[key] == tb[key]
        assert np.array_equal(ta["features"], tb["features"])


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_batch_equals_oracle_view_by_view(ctx, oracle, levels):
    bgrs, depths, masks = _views(24)
    got = ctx.extract_template_batch(bgrs, depths, masks, levels)
    assert len(got) == len(bgrs)
    mid = 24 // 2
    assert got[mid] is None and got[mid + 1] is None                        # the flat image and the 4x4 mask
    n_ok = 0
    for v in range(len(bgrs)):
        exp = oracle.add_template(bgrs[v], depths[v], masks[v], levels)
        _same_as_oracle(got[v], exp)
        n_ok += exp is not None
    assert n_ok >= 20


def test_batch_equals_single_view_calls_in_any_order(ctx):
    bgrs, depths, masks = _views(12, seed0=300)
    got = ctx.extract_template_batch(bgrs, depths, masks, 2)
    for v in range(len(bgrs)):
        _same(got[v], ctx.extract_template_pyramid(bgrs[v], depths[v], masks[v], 2))
    rev = ctx.extract_template_batch(bgrs[::-1], depths[::-1], masks[::-1], 2)
    for v in range(len(bgrs)):
        _same(rev[len(bgrs) - 1 - v], got[v])


def test_device_inputs_equal_host_inputs(ctx):
    bgrs, depths, masks = _views(8, seed0=500)
    host = ctx.extract_template_batch(bgrs, depths, masks, 2)
    db = [torch.from_numpy(b).cuda() for b in bgrs]
    dd = [torch.from_numpy(d).cuda() for d in depths]
    dm = [None if m is None else torch.from_numpy(m).cuda() for m in masks]
    torch.cuda.synchronize()
    dev = ctx.extract_template_batch(db, dd, dm, 2, mem=L.FL_MEM_DEVICE)
    for a, b in zip(host, dev):
        _same(a, b)
    assert sum(r is not None for r in dev) >= 6


def test_batch_across_the_chunk_limit(ctx, oracle):
    n = _chunk_views() + 5
    bgrs, depths, masks = _views(n, w=192, h=144, seed0=700)
    got = ctx.extract_template_batch(bgrs, depths, masks, 2)
    assert len(got) == len(bgrs)
    for v in range(len(bgrs)):
        _same(got[v], ctx.extract_template_pyramid(bgrs[v], depths[v], masks[v], 2))
    for v in (0, 1, n // 2, n // 2 + 1, n - 6, n - 1, n + 1):
        _same_as_oracle(got[v], oracle.add_template(bgrs[v], depths[v], masks[v], 2))
    assert sum(r is not None for r in got) >= n // 2


def test_odd_geometry(ctx, oracle):
    bgrs, depths, masks = _views(6, w=330, h=250, seed0=900)
    got = ctx.extract_template_batch(bgrs, depths, masks, 3)
    n_ok = 0
    for v in range(len(bgrs)):
        exp = oracle.add_template(bgrs[v], depths[v], masks[v], 3)
        _same_as_oracle(got[v], exp)
        n_ok += exp is not None
    assert n_ok >= 3


def test_class_trained_from_a_batch_recognises_like_the_oracle(ctx, oracle):
    views = [_view(1100 + k) for k in range(6)]
    bgrs, depths, masks = [v[0] for v in views], [v[1] for v in views], [v[2] for v in views]
    got = ctx.extract_template_batch(bgrs, depths, masks, 2)
    bank, bank_o = TemplateBank("obj", 2, 2), TemplateBank("obj", 2, 2)
    for v, (b, d, m, p13) in enumerate(views):
        exp = oracle.add_template(b, d, m, 2)
        assert got[v] is not None and exp is not None
        md = (d.astype(np.uint32) * 10).clip(0, 65535).astype(np.uint16)
        bank.add_pyramid(got[v][0], p13, md)
        t_o, f_o, _ = exp
        bank_o.add_pyramid([dict(width=int(t["width"]), height=int(t["height"]), offset_x=int(t["offset_x"]),
                                 offset_y=int(t["offset_y"]), pyramid_level=int(t["pyramid_level"]),
                                 features=np.stack([f["x"], f["y"], f["label"]], 1)) for t, f in zip(t_o, f_o)], p13, md)
    det = api.Detector(ctx, 2, [5, 8])
    det.add_class(bank)
    det.finalize(640, 480, max_batch=3)
    K = (synth.FX, synth.FY, 320.0, 240.0)
    frames = [1, 3, 4]
    res = det.recognize_batch([bgrs[v] for v in frames], [depths[v] for v in frames], K, 75.0, 10, 0.5, 0.01)
    for v, r in zip(frames, res):
        m, n = det.match(bgrs[v], depths[v], 75.0)
        m_o, n_o = oracle.match_images(bgrs[v], depths[v], [5, 8], [bank_o], 75.0)
        assert n == n_o and n > 0
        for k in ("x", "y", "similarity", "template_id"):
            assert np.array_equal(m[k][:n], m_o[k][:n]), k
        exp = oracle.recognition(bgrs[v], depths[v], K, [5, 8], bank_o, 75.0, 10, 0.5, 0.01)
        assert r["status"] == 0 and r["found"] == exp["found"] == 1
        assert r["n_matches"] == exp["n_matches"]
        assert r["best"]["template_id"] == exp["best"]["template_id"]
        assert r["best"]["x"] == exp["best"]["x"] and r["best"]["y"] == exp["best"]["y"]
        assert r["best"]["similarity"] == exp["best"]["similarity"]
        assert np.abs(r["pose"] - exp["pose"]).max() <= 1e-4
    det.close()


def test_argument_errors(ctx):
    lib = ctx.lib
    b, d, m, _ = _view(5)
    n = 2
    bp = (C.c_void_p * n)(b.ctypes.data, b.ctypes.data)
    dp = (C.c_void_p * n)(d.ctypes.data, d.ctypes.data)
    t = np.zeros(n * 4, dtype=[("v", "<i4", 7)])
    f = np.zeros(n * 4 * 63, dtype=[("v", "<i4", 3)])
    bb = np.full(4 * n, 77, np.int32)
    st = np.full(n, 77, np.int32)

    def call(nv=n, bgr=bp, dep=dp, mask=None, w=640, h=480, levels=2, tt=t, ff=f, b4=bb, s=st):
        return lib.fl_extract_template_batch(ctx.h, nv, bgr, dep, mask, w, h, levels, L.FL_MEM_HOST,
                                             None if tt is None else tt.ctypes.data, None if ff is None else ff.ctypes.data,
                                             None if b4 is None else b4.ctypes.data, None if s is None else s.ctypes.data)
    assert call(nv=0) == L.FL_ERR_INVALID
    assert call(nv=-3) == L.FL_ERR_INVALID
    assert call(bgr=None) == L.FL_ERR_INVALID
    assert call(dep=None) == L.FL_ERR_INVALID
    assert call(tt=None) == L.FL_ERR_INVALID
    assert call(ff=None) == L.FL_ERR_INVALID
    assert call(b4=None) == L.FL_ERR_INVALID
    assert call(s=None) == L.FL_ERR_INVALID
    assert call(w=15) == L.FL_ERR_INVALID
    assert call(levels=0) == L.FL_ERR_INVALID
    assert call(levels=5) == L.FL_ERR_INVALID
    assert call(w=40, h=40, levels=4) == L.FL_ERR_INVALID                  # 40 >> 3 = 5 < 8: too small for 4 levels
    assert call(bgr=(C.c_void_p * n)(b.ctypes.data, None)) == L.FL_ERR_INVALID
    assert call(dep=(C.c_void_p * n)(None, d.ctypes.data)) == L.FL_ERR_INVALID
    assert (st == 77).all() and (bb == 77).all() and not t["v"].any() and not f["v"].any()   # nothing written
    assert call(mask=(C.c_void_p * n)(m.ctypes.data, None)) == L.FL_OK
    assert (st == 0).all()
