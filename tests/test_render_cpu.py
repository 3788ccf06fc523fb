"""CPU: the float32 model of fl_render_views (tests/raster_model.py) against the analytic ray caster synth.render on the
tessellated object; fl_view_sphere (counts, rotations, the optical axis, in-plane steps, the poles, the cap query, refusals);
fealess::ReadObj through cadreco_read_obj (face forms, negative indices, polygons, normals, scale, malformed files)."""
import ctypes as C

import numpy as np
import pytest

import raster_model as RM
from cadreco_py import INVALID, OPEN_FAILED, read_obj as _read
from fealess_amd import _lib as L
from fealess_amd import api, synth

K0 = (synth.FX, synth.FY, synth.CX, synth.CY)


def _erode(m, r):
    out = m.copy()
    for _ in range(r):
        e = out.copy()
        e[1:, :] &= out[:-1, :]
        e[:-1, :] &= out[1:, :]
        e[:, 1:] &= out[:, :-1]
        e[:, :-1] &= out[:, 1:]
        out = e
    return out


def test_model_matches_the_analytic_object():
    m = synth.object_mesh()
    V, T = m["vertices"].astype(np.float64), m["triangles"]
    # tessellation bound: how far a sphere triangle's plane lies inside the sphere (the box is exact)
    sph = T[:5120]
    P0, P1, P2 = V[sph[:, 0]], V[sph[:, 1]], V[sph[:, 2]]
    n = np.cross(P1 - P0, P2 - P0)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    tess = float((60.0 - np.abs(((P0 - np.array([-35.0, 0, 0])) * n).sum(1))).max())
    assert 0 < tess < 0.1
    poses = [synth.object_pose(0, 0, 650, 0.3, 0.35, 0.1), synth.object_pose(40, -30, 560, -0.7, 0.2, 0.3),
             synth.object_pose(-60, 20, 720, 1.2, 0.6, -0.2), synth.object_pose(0, 0, 600, 0, 0, 0),
             synth.object_pose(290, 0, 650, 0.5, -0.4, 0.2)]                  # the last one leaves the image on the right
    for R, t in poses:
        bgr, dep, mk, tri = RM.render_view(m["vertices"], T, synth.pose13(R, t), K0, 640, 480, m["normals"], m["colors"])
        with np.errstate(invalid="ignore"):
            d_a, _, m_a = synth.render(640, 480, R, t, noise=False, background=False)
        a = mk > 0
        assert (a & m_a).sum() / (a | m_a).sum() >= 0.99
        # cosine of the incidence from the winning face's normal and the pixel ray
        Vc = V @ R.T + t
        fn = np.cross(Vc[T[:, 1]] - Vc[T[:, 0]], Vc[T[:, 2]] - Vc[T[:, 0]])
        fn /= np.linalg.norm(fn, axis=1, keepdims=True)
        u, v = np.meshgrid(np.arange(640.0), np.arange(480.0))
        d = np.stack([(u - K0[2]) / K0[0], (v - K0[3]) / K0[1], np.ones_like(u)], -1)
        cosi = np.abs((fn[np.maximum(tri, 0)] * d).sum(-1)) / np.linalg.norm(d, axis=-1)
        # away from the outer silhouette and from depth steps inside it (the sphere's rim over the box)
        da = d_a.astype(np.float64)
        smooth = np.ones_like(a)
        smooth[1:, :] &= np.abs(da[1:, :] - da[:-1, :]) <= 3
        smooth[:-1, :] &= np.abs(da[1:, :] - da[:-1, :]) <= 3
        smooth[:, 1:] &= np.abs(da[:, 1:] - da[:, :-1]) <= 3
        smooth[:, :-1] &= np.abs(da[:, 1:] - da[:, :-1]) <= 3
        sel = _erode(a, 2) & _erode(m_a, 2) & _erode(smooth, 2) & (cosi > 0.3)
        assert sel.sum() > 0.8 * a.sum() * (0.5 if t[0] > 200 else 1.0)
        # two rounded depths: the tessellation along the ray plus 0.5 mm of rounding on either side
        diff = dep.astype(np.float64) - d_a.astype(np.float64)
        assert (np.abs(diff[sel]) <= tess / cosi[sel] + 1.0).all(), np.abs(diff[sel]).max()
        assert (bgr[~a] == 0).all() and (dep[~a] == 0).all() and (tri[~a] == -1).all() and (tri[a] >= 0).all()


def test_model_shared_edge_and_ties():
    K = (512.0, 512.0, 40.0, 30.0)
    uv = np.array([[10, 5], [50, 5], [50, 45], [10, 45]], np.float32)
    V = np.concatenate([uv - np.array([40, 30], np.float32), np.full((4, 1), 512, np.float32)], 1)
    p = synth.pose13(np.eye(3), np.zeros(3))
    a = RM.render_view(V, np.array([[0, 1, 2]]), p, K, 80, 64)[2] > 0
    b = RM.render_view(V, np.array([[0, 2, 3]]), p, K, 80, 64)[2] > 0
    assert not (a & b).any() and (a | b).sum() == a.sum() + b.sum()
    assert all(a[5 + k, 10 + k] != b[5 + k, 10 + k] for k in range(1, 40))
    # two copies of one triangle: the lower index wins every pixel
    tri = RM.render_view(np.concatenate([V, V]), np.array([[4, 5, 6], [0, 1, 2]]), p, K, 80, 64)[3]
    assert set(np.unique(tri)) == {-1, 0}


def _sphere(*a, **k):
    return api.view_sphere(*a, **k)


def test_view_sphere_counts_and_poses():
    for s in range(4):
        assert len(_sphere(s, [500.0])) == 10 * 4 ** s + 2
        upper = 6 if s == 0 else (10 * 4 ** s + 2 + 5 * 2 ** s) // 2      # the equator's 5 * 2^s points are kept
        assert len(_sphere(s, [500.0], upper_hemisphere=True)) == upper
    assert len(_sphere(6, [1.0])) == 40962
    P = _sphere(2, [450.0, 800.0], n_inplane=5, inplane_deg=20.0)
    assert P.shape == (162 * 2 * 5, 13) and np.isfinite(P).all()
    R = P[:, :12].reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    t = P[:, :12].reshape(-1, 3, 4)[:, :, 3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6
    assert np.abs(np.linalg.det(R) - 1).max() < 1e-6
    d = np.tile(np.repeat([450.0, 800.0], 5), 162)
    assert (t[:, 0] == 0).all() and (t[:, 1] == 0).all() and (t[:, 2] == d).all() and (P[:, 12] == d).all()
    # the camera centre -R^T t lies on the sphere of radius d and the object origin on the optical axis
    centre = -np.einsum("nji,nj->ni", R, t)
    assert np.abs(np.linalg.norm(centre, axis=1) - d).max() < 1e-3
    assert np.abs(np.einsum("ni,ni->n", R[:, 2], -centre / d[:, None]) - 1).max() < 1e-6
    # consecutive in-plane poses differ by 10 degrees about the optical axis
    step = R[1::5][:, :, :] @ R[0::5].transpose(0, 2, 1)
    c, s_ = np.cos(np.radians(10.0)), np.sin(np.radians(10.0))
    assert np.abs(step - np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1]])).max() < 1e-6
    # image-up is object +z away from the poles: its image y component is negative
    mid = R[2::5]
    away = np.abs(centre[2::5, 2] / d[2::5]) < 0.99
    assert (mid[away][:, 1, 2] < 0).all()
    # the poles: finite, orthonormal, looking straight down / up
    top = _sphere(0, [300.0], n_inplane=1)[0]
    Rt = top[:12].reshape(3, 4)[:, :3]
    assert np.isfinite(top).all() and np.allclose(Rt[2], [0, 0, -1]) and np.allclose(Rt @ Rt.T, np.eye(3), atol=1e-6)


def test_view_sphere_cap_query_and_refusals():
    lib = L.load()
    d = np.array([500.0], np.float32)
    n = C.c_int(-1)
    assert lib.fl_view_sphere(1, 0, d.ctypes.data, 1, 3, 15.0, None, 0, C.byref(n)) == L.FL_OK and n.value == 126
    out = np.full((126, 13), 7, np.float32)
    n2 = C.c_int(-1)
    assert lib.fl_view_sphere(1, 0, d.ctypes.data, 1, 3, 15.0, out.ctypes.data, 125, C.byref(n2)) == L.FL_ERR_INVALID
    assert (out == 7).all() and n2.value == -1
    for args in [(-1, 0, d, 1, 1, 0.0), (7, 0, d, 1, 1, 0.0), (1, 0, d, 0, 1, 0.0), (1, 0, d, 1, 0, 0.0), (1, 0, d, 1, 2, -1.0),
                 (1, 0, d, 1, 2, 181.0), (1, 0, d, 1, 2, float("nan")), (1, 0, np.array([0.0], np.float32), 1, 1, 0.0),
                 (1, 0, np.array([np.inf], np.float32), 1, 1, 0.0)]:
        s, up, dd, nd, ni, deg = args
        assert lib.fl_view_sphere(s, up, dd.ctypes.data, nd, ni, deg, out.ctypes.data, 126, C.byref(n2)) == L.FL_ERR_INVALID, args
        assert (out == 7).all() and n2.value == -1
    assert lib.fl_view_sphere(1, 0, d.ctypes.data, 1, 3, 15.0, None, 126, C.byref(n2)) == L.FL_ERR_INVALID
    with pytest.raises(api.FealessError):
        api.view_sphere(1, [-5.0])


def test_read_obj_forms(tmp_path):
    f = tmp_path / "forms.obj"
    f.write_text("# comment\nmtllib x.mtl\no thing\nv 0 0 0 1\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0.5 1.5 0\nvt 0 0\nvt 1 0\nvt 1 1\n"
                 "g part\nusemtl m\ns 1\nf 1 2 3\nf 1/1 3/3 4/2\nf -5/1 -3 -2\nf 1 2/2 3 5 4\n")
    res = _read(f, 2.0)
    assert not isinstance(res, int), res
    V, N, T = res
    assert N is None
    assert np.array_equal(V, np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0], [1, 3, 0]], np.float32))   # scaled, file order
    assert T.tolist() == [[0, 1, 2], [0, 2, 3], [0, 2, 3], [0, 1, 2], [0, 2, 4], [0, 4, 3]]     # negative indices; fan of the pentagon


def test_read_obj_normals(tmp_path):
    f = tmp_path / "n.obj"
    f.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nvn 0 0 -1\nf 1//1 2//1 3//1\nf 1/5/2 3//2 4//2\nf -4//-2 -3//-2 -2//-2\n")
    V, N, T = _read(f)
    # distinct (position, normal) pairs in order of first use
    assert np.array_equal(V, np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32))
    assert np.array_equal(N, np.array([[0, 0, 1]] * 3 + [[0, 0, -1]] * 3, np.float32))
    assert T.tolist() == [[0, 1, 2], [3, 4, 5], [0, 1, 2]]
    g = tmp_path / "mixed.obj"                                                 # a corner without a normal: none are used
    g.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nvn 0 0 1\nf 1//1 2//1 3\n")
    V, N, T = _read(g)
    assert N is None and len(V) == 3 and T.tolist() == [[0, 1, 2]]


def test_read_obj_object_mesh_round_trip(tmp_path):
    m = synth.object_mesh(2)
    synth.write_obj(str(tmp_path / "o.obj"), m)
    V, N, T = _read(tmp_path / "o.obj")
    assert np.array_equal(V[T], m["vertices"][m["triangles"]]) and np.array_equal(N[T], m["normals"][m["triangles"]])


@pytest.mark.parametrize("body", ["v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n",
                                  "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 -4\n", "v 0 0 0\nv 1 zero 0\nv 0 1 0\nf 1 2 3\n",
                                  "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3a\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//2 2//1 3//1\n",
                                  "v 0 0 0\nv 1 0 0\nv 0 1 0\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n", "v 0 0\nf 1 1 1\n"])
def test_read_obj_refuses_malformed(tmp_path, body):
    f = tmp_path / "bad.obj"
    f.write_text(body)
    assert _read(f) == INVALID


def test_read_obj_unreadable_and_bad_scale(tmp_path):
    assert _read(tmp_path / "missing.obj") == OPEN_FAILED
    f = tmp_path / "ok.obj"
    f.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    assert _read(f, 0.0) == INVALID and _read(f, float("nan")) == INVALID
