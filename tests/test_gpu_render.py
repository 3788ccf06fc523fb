"""GPU: fl_render_views equals the float32 restatement of its contract (tests/raster_model.py) bit for bit -- bgr, depth,
mask and triangle index -- on the object mesh, random soups, a triangle across z = 0, edge-on triangles, a split square whose
diagonal runs through pixel positions, an empty view, an odd image size, with and without normals and colours, host and
device outputs, and a batch longer than one chunk.  Refusals write nothing.  Renders in device tensors feed
fl_extract_template_batch unchanged and give what oracle.add_template gives on host copies."""
import numpy as np
import pytest
import torch

import raster_model as RM
from fealess_amd import _lib as L
from fealess_amd import api, synth

pytestmark = pytest.mark.gpu
K0 = (synth.FX, synth.FY, synth.CX, synth.CY)


def _same(got, exp):
    for name, g, e in zip(("bgr", "depth", "mask", "tri"), got, exp):
        assert g.dtype == e.dtype and g.shape == e.shape, name
        bad = np.argwhere(g != e)
        assert len(bad) == 0, f"{name}: {len(bad)} pixels differ, first {bad[:3].tolist()}: {g[tuple(bad[0])]} vs {e[tuple(bad[0])]}"


def _poses(rng, n, tz=(560, 720), spread=1.0):
    out = []
    for _ in range(n):
        R, t = synth.object_pose(tx=float(rng.uniform(-60, 60)), ty=float(rng.uniform(-40, 40)), tz=float(rng.uniform(*tz)),
                                 yaw=float(rng.uniform(-spread, spread)), tilt=float(rng.uniform(-spread, spread)),
                                 roll=float(rng.uniform(-spread, spread)))
        out.append(synth.pose13(R, t))
    return np.array(out, np.float32)


def _check(ctx, V, T, P, K, w, h, **kw):
    got = ctx.render_views(V, T, P, K, w, h, **kw)
    exp = RM.render(V, T, P, K, w, h, **kw)
    _same(got, exp)
    return got


def test_object_mesh_bit_exact(ctx):
    m = synth.object_mesh()
    P = _poses(np.random.default_rng(1), 4)
    P = np.concatenate([P, [synth.pose13(*synth.object_pose(tx=290.0, tz=650.0))]])          # partly off the image
    got = _check(ctx, m["vertices"], m["triangles"], P, K0, 640, 480, normals=m["normals"], colors=m["colors"])
    assert (got[2] > 0).sum(axis=(1, 2)).min() > 5000
    _check(ctx, m["vertices"], m["triangles"], P[:2], K0, 640, 480)                           # face normals, grey
    _check(ctx, m["vertices"], m["triangles"], P[:2], K0, 640, 480, normals=m["normals"], light=(0.3, -0.4, 0.86), ambient=0.05)
    _check(ctx, m["vertices"], m["triangles"], P[2:4], K0, 640, 480, colors=m["colors"], light=(-1.0, 2.0, 3.0), ambient=1.0)


def test_random_soups_both_windings(ctx):
    rng = np.random.default_rng(7)
    for it in range(3):
        n = 60
        c = rng.uniform([-80, -60, 400], [80, 60, 700], (n, 1, 3))
        V = (c + rng.normal(0, 40, (n, 3, 3))).reshape(-1, 3).astype(np.float32)   # intersecting, both windings
        T = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
        Nv = rng.normal(0, 1, V.shape).astype(np.float32)
        col = rng.integers(0, 256, V.shape).astype(np.uint8)
        P = np.array([synth.pose13(np.eye(3), np.zeros(3)), synth.pose13(synth.rot_y(0.2), np.array([10.0, -5.0, 30.0]))], np.float32)
        _check(ctx, V, T, P, K0, 320, 240, normals=Nv, colors=col)
        _check(ctx, V, T, P[:1], (300.0, 310.0, 160.5, 119.25), 320, 240)


def test_triangle_across_z0_and_edge_on(ctx):
    V = np.array([[-50, -40, 600], [60, -30, -200], [0, 80, 500],          # straddles z = 0: not clipped, z > 0 hits only
                  [0, 0, 300], [0, 0, 600], [40, 30, 900],                  # its plane contains the camera: edge-on
                  [-30, 10, 0], [30, 10, 0], [0, 60, 0],                    # in the z = 0 plane
                  [-100, -100, 800], [100, -100, 800], [0, 100, -1]], np.float32)
    T = np.arange(12, dtype=np.int32).reshape(4, 3)
    P = np.array([synth.pose13(np.eye(3), np.zeros(3))], np.float32)
    K = (200.0, 200.0, 100.0, 80.0)
    bgr, depth, mask, tri = _check(ctx, V, T, P, K, 200, 160)
    assert 0 in tri and 3 in tri and 1 not in tri and 2 not in tri
    one = _check(ctx, V[3:6], np.array([[0, 1, 2]], np.int32), P, K, 200, 160)
    assert one[2].max() == 0 and (one[3] == -1).all()


def test_shared_diagonal_covered_once(ctx):
    # fronto-parallel square at z = 512 with fx = fy = 512: vertex (u, v) -> ((u - cx), (v - cy), 512), so every product
    # and sum is exact and the diagonal's pixels lie exactly on the shared edge
    K = (512.0, 512.0, 40.0, 30.0)
    uv = np.array([[10, 5], [50, 5], [50, 45], [10, 45]], np.float32)
    V = np.concatenate([uv - np.array([40, 30], np.float32), np.full((4, 1), 512, np.float32)], 1)
    P = np.array([synth.pose13(np.eye(3), np.zeros(3))], np.float32)
    for T in (np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.array([[0, 2, 3], [0, 1, 2]], np.int32),
              np.array([[2, 1, 0], [3, 2, 0]], np.int32)):                   # either order, either winding
        full = _check(ctx, V, T, P, K, 80, 64)
        a = _check(ctx, V, T[:1], P, K, 80, 64)[2][0] > 0
        b = _check(ctx, V, T[1:], P, K, 80, 64)[2][0] > 0
        diag = [(10 + k, 5 + k) for k in range(1, 40)]
        for x, y in diag:
            assert int(a[y, x]) + int(b[y, x]) == 1, (x, y)
        assert not (a & b).any()
        assert (full[2][0] > 0).sum() == a.sum() + b.sum()


def test_empty_view_and_odd_size(ctx):
    m = synth.object_mesh(2)
    behind = synth.pose13(np.eye(3), np.array([0.0, 0.0, -900.0]))
    got = _check(ctx, m["vertices"], m["triangles"], np.array([behind], np.float32), K0, 64, 48, normals=m["normals"], colors=m["colors"])
    assert got[2].max() == 0 and got[1].max() == 0 and got[0].max() == 0 and (got[3] == -1).all()
    P = _poses(np.random.default_rng(3), 3)
    _check(ctx, m["vertices"], m["triangles"], P, (401.5, 377.25, 170.3, 121.7), 333, 251, normals=m["normals"], colors=m["colors"])


def test_device_outputs_and_chunks(ctx):
    m = synth.object_mesh(2)
    n = 70                                                                  # > FL_RENDER_CHUNK_VIEWS at this size
    P = _poses(np.random.default_rng(11), n, tz=(250, 350))
    K = (300.0, 300.0, 48.0, 40.0)
    exp = RM.render(m["vertices"], m["triangles"], P, K, 96, 80, normals=m["normals"], colors=m["colors"])
    host = ctx.render_views(m["vertices"], m["triangles"], P, K, 96, 80, normals=m["normals"], colors=m["colors"])
    _same(host, exp)
    for v in (0, 63, 64, 69):                                               # per-view calls equal the batch
        _same(ctx.render_views(m["vertices"], m["triangles"], P[v:v + 1], K, 96, 80, normals=m["normals"], colors=m["colors"]),
              tuple(a[v:v + 1] for a in exp))
    dev = dict(bgr=torch.empty((n, 80, 96, 3), dtype=torch.uint8, device="cuda"), depth=torch.empty((n, 80, 96), dtype=torch.int16, device="cuda"),
               tri=torch.empty((n, 80, 96), dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    ctx.render_views(m["vertices"], m["triangles"], P, K, 96, 80, normals=m["normals"], colors=m["colors"], mem=L.FL_MEM_DEVICE, out=dev)
    ctx.synchronize()
    assert np.array_equal(dev["bgr"].cpu().numpy(), exp[0])
    assert np.array_equal(dev["depth"].cpu().numpy().view(np.uint16), exp[1])
    assert np.array_equal(dev["tri"].cpu().numpy(), exp[3])


def test_refusals_write_nothing(ctx):
    lib = ctx.lib
    import ctypes as C
    V = np.array([[0, 0, 500], [10, 0, 500], [0, 10, 500]], np.float32)
    T = np.array([[0, 1, 2]], np.int32)
    P = np.array([synth.pose13(np.eye(3), np.zeros(3))], np.float32)
    out = np.full((4, 4, 3), 7, np.uint8)
    dep = np.full((4, 4), 7, np.uint16)

    def call(V=V, nv=3, T=T, nt=1, nviews=1, K=L.Intrinsics(4, 4, 100.0, 100.0, 2.0, 2.0), prm=None, b=True, d=True):
        return lib.fl_render_views(ctx.h, V.ctypes.data, None, None, nv, T.ctypes.data, nt, nviews, P.ctypes.data, C.byref(K),
                                   None if prm is None else C.byref(prm), L.FL_MEM_HOST, out.ctypes.data if b else None,
                                   dep.ctypes.data if d else None, None, None)
    assert call() == L.FL_OK and (out == 7).sum() == 0                  # the valid call writes every output pixel
    out[:] = 7
    dep[:] = 7
    bad = [dict(nv=2), dict(nt=0), dict(nviews=0), dict(T=np.array([[0, 1, 3]], np.int32)), dict(T=np.array([[0, -1, 2]], np.int32)),
           dict(K=L.Intrinsics(0, 4, 100.0, 100.0, 2.0, 2.0)), dict(K=L.Intrinsics(4, 9000, 100.0, 100.0, 2.0, 2.0)),
           dict(K=L.Intrinsics(4, 4, 0.0, 100.0, 2.0, 2.0)), dict(K=L.Intrinsics(4, 4, 100.0, float("nan"), 2.0, 2.0)),
           dict(K=L.Intrinsics(4, 4, float("inf"), 100.0, 2.0, 2.0)), dict(K=L.Intrinsics(4, 4, -5.0, 100.0, 2.0, 2.0)),
           dict(prm=L.RenderParams((C.c_float * 3)(0, 0, 1), 1.5)), dict(prm=L.RenderParams((C.c_float * 3)(0, 0, 1), -0.1)),
           dict(prm=L.RenderParams((C.c_float * 3)(0, 0, 0), 0.2)), dict(b=False, d=False),
           dict(V=np.array([[0, 0, np.nan], [10, 0, 500], [0, 10, 500]], np.float32))]
    for kw in bad:
        assert call(**kw) == L.FL_ERR_INVALID, kw
        assert (out == 7).all() and (dep == 7).all(), kw


def test_device_route_feeds_extraction(ctx, oracle):
    m = synth.object_mesh()
    P = api.view_sphere(1, [600.0, 700.0], n_inplane=2, inplane_deg=10.0, upper_hemisphere=True)[::3][:14]
    P = np.concatenate([P, [synth.pose13(np.eye(3), np.array([0.0, 0.0, -700.0]))]]).astype(np.float32)     # an empty view
    n = len(P)
    bgr = torch.empty((n, 480, 640, 3), dtype=torch.uint8, device="cuda")
    dep = torch.empty((n, 480, 640), dtype=torch.int16, device="cuda")
    msk = torch.empty((n, 480, 640), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.render_views(m["vertices"], m["triangles"], P, K0, 640, 480, normals=m["normals"], colors=m["colors"], mem=L.FL_MEM_DEVICE,
                     out=dict(bgr=bgr, depth=dep, mask=msk))
    got = ctx.extract_template_batch([bgr[v] for v in range(n)], [dep[v] for v in range(n)], [msk[v] for v in range(n)], 2,
                                     mem=L.FL_MEM_DEVICE)
    ctx.synchronize()
    hb, hd, hm = bgr.cpu().numpy(), dep.cpu().numpy().view(np.uint16), msk.cpu().numpy()
    n_none = 0
    for v in range(n):
        exp = oracle.add_template(hb[v], hd[v], hm[v], 2)
        if exp is None:
            assert got[v] is None, v
            n_none += 1
            continue
        assert got[v] is not None, v
        t_o, f_o, bb_o = exp
        tl, bb = got[v]
        assert tuple(bb) == tuple(int(x) for x in bb_o), v
        for k, t in enumerate(tl):
            for key in ("width", "height", "offset_x", "offset_y", "pyramid_level"):
                assert t[key] == int(t_o[k][key]), (v, k, key)
            assert np.array_equal(t["features"], np.stack([f_o[k]["x"], f_o[k]["y"], f_o[k]["label"]], 1)), (v, k)
    assert n_none >= 1 and n_none < n


def test_device_outputs_are_checked_before_the_call(ctx):
    """Context.render_views refuses device outputs that cannot hold n x h x w pixels (shape, element size, contiguity,
    device) before anything is queued."""
    m = synth.object_mesh(1)
    P = _poses(np.random.default_rng(2), 2)
    ok = torch.zeros((2, 48, 64), dtype=torch.int32, device="cuda")
    for bad in (dict(tri=torch.zeros((1, 48, 64), dtype=torch.int32, device="cuda")),
                dict(tri=torch.zeros((2, 48, 64), dtype=torch.int16, device="cuda")),
                dict(tri=torch.zeros((2, 64, 48), dtype=torch.int32, device="cuda").transpose(1, 2)),
                dict(tri=torch.zeros((2, 48, 64), dtype=torch.int32)),
                dict(bgr=torch.zeros((2, 48, 64), dtype=torch.uint8, device="cuda")),
                dict(tri=ok, normals=ok)):
        with pytest.raises(ValueError):
            ctx.render_views(m["vertices"], m["triangles"], P, K0, 64, 48, mem=L.FL_MEM_DEVICE, out=bad)
    torch.cuda.synchronize()
    ctx.render_views(m["vertices"], m["triangles"], P, K0, 64, 48, mem=L.FL_MEM_DEVICE, out=dict(tri=ok))
    ctx.synchronize()
    assert np.array_equal(ok.cpu().numpy(), RM.render(m["vertices"], m["triangles"], P, K0, 64, 48)[3])
