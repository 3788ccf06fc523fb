"""GPU: CadRecoTrainMesh (cadreco_train_mesh) trains a class straight from an OBJ file: the view-sphere poses in
linemod_templates.yml, depth/<template_id>.png equal to the render x 10, and AddObj -> Recognition on composed scenes (the
mesh off the grid, another light, a textured wall, noise) within 1e-4 of oracle.recognition on a bank the oracle built from
the same renders, and close to the ground truth where the view can be told apart.  Refusals, and a failure while
writing, leave nothing behind.

Ground truth, measured on one MI355X for the ten scenes below (translation error, rotation error, the nearest grid
view's angle from the truth): 1.1 mm / 4.5 / 5.2 deg, 3.8 / 5.0 / 5.0, 1.3 / 3.8 / 3.8, 1.9 / 4.4 / 4.3, 3.5 / 3.3 / 3.5
where Recognition picks the nearest grid view; in the other five it picks another template -- one 11 deg from the truth
(3.6 mm / 11.6 deg) and four of a look-alike view 62 - 176 deg away (the object is mirror-symmetric in y and nearly
symmetric under a half turn about x, and the renders are uniformly grey).  The oracle gives the same pose in every scene.
A 30 x 20 x 20 mm tab on the box did not change that (five scenes at the nearest view, five 62 - 128 deg away): with grey
renders under another light, LINEMOD's best score often belongs to a distant view.  Asserted: every scene equals the
oracle; at least 4 of the 10 within 10 mm and within the nearest grid view's angle + 2 deg -- the ground-truth half holds
for some scenes only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cadreco_py import INVALID, OPEN_FAILED, lib as _lib, read_obj, recognition, train_mesh
from fealess_amd import api, synth
from fealess_amd.bank import TemplateBank

pytestmark = pytest.mark.gpu
K0 = (synth.FX, synth.FY, synth.CX, synth.CY)
SPHERE = dict(subdivisions=1, upper=1, distances=(600.0, 700.0), n_inplane=3, inplane_deg=10.0)


def _train(lib, h, d, obj, n_views, sphere=SPHERE, levels=2, T=(5, 8)):
    return train_mesh(h, d, obj, n_views, sphere, levels, T)


def _yaml_poses(path):
    txt = open(path).read()
    assert txt.count("class_id:") == 1
    return np.array([[float(x) for x in m.replace("\n", " ").split(",")] for m in re.findall(r"template_pose: \[(.*?)\]", txt, re.S)], np.float32)


def _angle_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1))))


def _scene(ctx, V, N, T, R, t, seed):
    """The mesh at (R, t) under a light from the upper left, over a textured wall 950 - 1010 mm away, with noise."""
    rng = np.random.default_rng(seed)
    bgr, dep, msk, _ = ctx.render_views(V, T, synth.pose13(R, t)[None], K0, 640, 480, normals=N, light=(0.35, 0.3, 0.89), ambient=0.15)
    u, v = np.meshgrid(np.arange(640.0), np.arange(480.0))
    wall_z = 950.0 + 0.06 * u + 0.04 * v
    cell = (np.floor(u / 23.0) + 2 * np.floor(v / 17.0)) % 5
    wall = (70 + 30 * cell)[..., None] * np.array([1.0, 0.9, 0.75])
    m = msk[0] > 0
    depth = np.where(m, dep[0].astype(np.float64), wall_z) + rng.integers(-1, 2, (480, 640))
    col = np.where(m[..., None], bgr[0].astype(np.float64), wall) + rng.normal(0, 1.5, (480, 640, 3))
    return (np.ascontiguousarray(np.clip(np.rint(col), 0, 255).astype(np.uint8)),
            np.ascontiguousarray(np.clip(np.rint(depth), 0, 65535).astype(np.uint16)))


def test_train_mesh_then_add_obj_and_recognise(tmp_path, ctx, oracle):
    lib = _lib()
    mesh = synth.object_mesh()
    obj = tmp_path / "object.obj"
    synth.write_obj(str(obj), mesh, with_normals=True)
    P = api.view_sphere(1, list(SPHERE["distances"]), n_inplane=3, inplane_deg=10.0, upper_hemisphere=True)
    n = len(P)
    assert n == 26 * 2 * 3
    h = C.c_void_p(lib.cadreco_create(1))
    assert h.value
    d = tmp_path / "mesh"
    rc, tov = _train(lib, h, d, obj, n)
    assert rc == 0
    ok = tov >= 0
    assert ok.sum() > n // 2 and (tov[ok] == np.arange(ok.sum())).all()     # ids count the views that gave a template, in order
    poses = _yaml_poses(d / "linemod_templates.yml")
    assert np.array_equal(poses, P[ok])
    assert sorted(os.listdir(d / "depth"), key=lambda s: int(s[:-4])) == [f"{i}.png" for i in range(ok.sum())]

    # the renders the trainer saw (the mesh as the OBJ reader gives it; no colours: FL_RENDER_GREY) and the oracle's bank
    V, N, T = read_obj(obj)
    assert N is not None and len(T) == len(mesh["triangles"])
    bgr, dep, msk, _ = ctx.render_views(V, T, P, K0, 640, 480, normals=N)
    px = np.zeros(640 * 480, np.uint16)
    w, hh = C.c_int(), C.c_int()
    bank = TemplateBank("mesh", 2, 2)
    for v in range(n):
        exp = oracle.add_template(bgr[v], dep[v], msk[v], 2)
        assert (exp is not None) == ok[v], v
        if exp is None:
            continue
        d01 = (dep[v].astype(np.uint32) * 10).clip(0, 65535).astype(np.uint16)
        assert lib.cadreco_read_png16(str(d / "depth" / f"{tov[v]}.png").encode(), px.ctypes.data, px.size, C.byref(w), C.byref(hh)) == 0
        assert (w.value, hh.value) == (640, 480) and np.array_equal(px.reshape(480, 640), d01), v
        t_o, f_o, _ = exp
        bank.add_pyramid([dict(width=int(t["width"]), height=int(t["height"]), offset_x=int(t["offset_x"]), offset_y=int(t["offset_y"]),
                               pyramid_level=int(t["pyramid_level"]), features=np.stack([f["x"], f["y"], f["label"]], 1))
                          for t, f in zip(t_o, f_o)], P[v], d01)

    assert lib.cadreco_add_obj(h, str(d).encode()) == 0
    grid = [p[:12].reshape(3, 4)[:, :3].astype(np.float64) for p in P[ok]]
    rng = np.random.default_rng(5)
    errs = []
    idx = np.flatnonzero(ok)
    for k, v in enumerate(idx[np.linspace(0, len(idx) - 1, 10).astype(int)]):
        R0, dist = P[v][:12].reshape(3, 4)[:, :3].astype(np.float64), float(P[v][12])
        R = synth.rot_x(np.radians(rng.uniform(-4, 4))) @ synth.rot_y(np.radians(rng.uniform(-4, 4))) @ synth.rot_z(np.radians(rng.uniform(-4, 4))) @ R0
        t = np.array([rng.uniform(-40, 40), rng.uniform(-30, 30), dist + rng.uniform(-20, 20)])
        bgr_s, dep_s = _scene(ctx, V, N, T, R, t, seed=100 + k)
        rc, nres, tag, pose = recognition(h, bgr_s, dep_s, K0)
        exp = oracle.recognition(bgr_s, dep_s, K0, [5, 8], bank, 75.0, 10, 0.5, 0.01)
        assert rc == 0 and nres == exp["found"] == 1 and tag == b"mesh", k
        assert np.abs(pose.reshape(4, 4) - exp["pose"]).max() <= 1e-4, k
        got = pose.reshape(4, 4).astype(np.float64)
        tid = int(exp["best"]["template_id"])
        errs.append((k, int(v), float(np.linalg.norm(got[:3, 3] - t)), _angle_deg(got[:3, :3], R), min(_angle_deg(g, R) for g in grid),
                     _angle_deg(grid[tid], R), tid, float(exp["best"]["similarity"])))
    for e in errs:
        print("scene %d view %d: dt %.2f mm, dr %.2f deg, nearest grid %.2f deg, matched template %.2f deg away (id %d, sim %.1f)" % e)
    good = [e for e in errs if e[2] <= 10.0 and e[3] <= e[4] + 2.0]
    assert len(good) >= 4, errs
    lib.cadreco_destroy(h)


def test_train_mesh_refuses_and_writes_nothing(tmp_path):
    lib = _lib()
    h = C.c_void_p(lib.cadreco_create(1))
    n = 26 * 2 * 3
    rc, tov = _train(lib, h, tmp_path / "a", tmp_path / "missing.obj", n)
    assert rc == OPEN_FAILED and not (tmp_path / "a").exists() and (tov == -9).all()
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 x\n")
    assert _train(lib, h, tmp_path / "b", bad, n)[0] == INVALID and not (tmp_path / "b").exists()
    far = tmp_path / "tiny.obj"                                                  # a speck at 600 mm: no view yields a template
    far.write_text("v 0 0 0\nv 0.5 0 0\nv 0 0.5 0\nf 1 2 3\n")
    rc, tov = _train(lib, h, tmp_path / "c", far, n)
    assert rc == INVALID and not (tmp_path / "c").exists() and (tov == -9).all()
    good = tmp_path / "good.obj"
    synth.write_obj(str(good), synth.object_mesh(1))
    assert _train(lib, h, tmp_path / "d", good, n, levels=0, T=(5,))[0] == INVALID
    assert _train(lib, h, tmp_path / "e", good, n, sphere=dict(SPHERE, subdivisions=7))[0] == INVALID
    assert _train(lib, h, tmp_path / "f", good, n, sphere=dict(SPHERE, distances=(-600.0,)))[0] == INVALID
    assert not any((tmp_path / x).exists() for x in "def")
    lib.cadreco_destroy(h)


def test_train_mesh_removes_what_it_wrote_on_a_write_error(tmp_path):
    """A PNG that cannot be written (its name is taken by a directory) fails the call after other PNGs were written: those
    go again, and so do the directories the call made; what was there before stays, and no YAML appears."""
    lib = _lib()
    h = C.c_void_p(lib.cadreco_create(1))
    good = tmp_path / "good.obj"
    synth.write_obj(str(good), synth.object_mesh(1))
    n = 26 * 2 * 3
    d = tmp_path / "dir"
    (d / "depth" / "3.png").mkdir(parents=True)
    rc, tov = _train(lib, h, d, good, n)
    assert rc == OPEN_FAILED and (tov == -9).all()
    assert sorted(os.listdir(d)) == ["depth"] and os.listdir(d / "depth") == ["3.png"]
    e = tmp_path / "fresh"
    (e / "linemod_templates.yml").mkdir(parents=True)                           # the YAML cannot be written
    rc, _ = _train(lib, h, e, good, n)
    assert rc == OPEN_FAILED and os.listdir(e) == ["linemod_templates.yml"]     # its depth/ and PNGs are gone again
    lib.cadreco_destroy(h)
