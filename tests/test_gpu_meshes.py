"""GPU: several meshes on one tracker (fl_tracker_create_meshes and the *_meshes entry points, include/fealess_hip.h).

The contract under test: the record of a track or pose whose mesh is m is, byte for byte, what the one-mesh entry point returns
for that pose and frame on a tracker created from mesh m alone -- so every test runs the multi-mesh tracker beside four
one-mesh trackers, and where the numpy models apply (tests/verify_model.py, tests/track_verified_model.py, which take the mesh
per call) against "the model with pose t's mesh" too.  The meshes and their order on the tracker (B, D, C, A) are
tests/meshes.py's; tests/test_meshes_cpu.py shows that the choice of the mesh changes a record.
"""
import ctypes as C

import numpy as np
import pytest

import cadreco_py
import clutter
import instances_model as M
import meshes as MS
import multiclass
import track_model as TM
import track_verified_model as TVM
import util
import verified_pick_model as VP
import verify_model as VM
from fealess_amd import _lib as L
from fealess_amd import api, synth
from test_gpu_track import BIG_POSE, GONE_POSE, K0, LOST_POSE, MAX_CROP, OFFSETS, POSES, _same_as_parity_model
from test_instances_cpu import MIN_DIST
from util import p13 as _p13, pose as _pose

pytestmark = pytest.mark.gpu

W, H = 640, 480
NAMES = "ABCD"
IDX = MS.INDEX
P = (75.0, 10, 0.5, 0.01)
NF = len(clutter.FRAMES)


@pytest.fixture(scope="module")
def meshes():
    return MS.all_meshes()


class Trackers:
    """A tracker of the four meshes and four one-mesh trackers, all of one size on one context."""

    def __init__(self, ctx, meshes, w, h, max_frames, max_tracks, max_crop_px):
        self.multi = api.Tracker(ctx, meshes=MS.in_order(meshes), w=w, h=h, max_frames=max_frames, max_tracks=max_tracks, max_crop_px=max_crop_px)
        self.one = {n: api.Tracker(ctx, meshes[n]["vertices"], meshes[n]["triangles"], w, h, max_frames, max_tracks, max_crop_px) for n in NAMES}

    def close(self):
        for t in [self.multi] + list(self.one.values()):
            t.close()

    def gathered(self, call, names, frame_of, poses, *args, **kw):
        """call(one-mesh tracker, frame_of, poses, ...) for every mesh over the poses that name it, back in the poses' order."""
        names, frame_of = list(names), np.asarray(frame_of)
        out = None
        for n in sorted(set(names)):
            sel = np.array([i for i, m in enumerate(names) if m == n])
            part = call(self.one[n], frame_of[sel], poses[sel], *args, **kw)
            if out is None:
                out = np.zeros(len(names), part.dtype)
            out[sel] = part
        return out


@pytest.fixture(scope="module")
def vga(ctx, meshes):
    t = Trackers(ctx, meshes, W, H, 8, 70, MAX_CROP)
    assert t.multi.num_meshes == 4 and all(o.num_meshes == 1 for o in t.one.values())
    yield t
    t.close()


def _mesh_of(names):
    return np.array([IDX[n] for n in names], np.int32)


# ---- 1. the render: every mesh at two poses, both verification paths, three image sizes ----------------------------------------
SIZES = {
    "640x480": (640, 480, K0, [(10, -5, 720, 0.30, 0.35, 0.10), (-60, 30, 690, -0.50, 0.20, 0.30)]),
    "322x250": (322, 250, K0, [(-150, -100, 700, 0.3, 0.35, 0.1), (-120, -90, 690, -0.4, 0.2, 0.2)]),      # px no multiple of eight
    # mesh D covers a few pixels; the second pose puts mesh A across the right border
    "64x48": (64, 48, (60.8, 60.8, 32.0, 24.0), [(10, -5, 720, 0.30, 0.35, 0.10), (330, 20, 700, 0.3, 0.35, 0.1)]),
}


@pytest.mark.parametrize("size", sorted(SIZES))
def test_every_mesh_renders_as_on_its_own_tracker_and_as_the_model(ctx, vga, meshes, size):
    w, h, K, ps = SIZES[size]
    scenes = [synth.render(w, h, *_pose(p), seed=11 + i, fx=K[0], fy=K[1], cx=K[2], cy=K[3])[0] for i, p in enumerate(ps)]
    names = [n for n in NAMES for _ in ps]
    frame_of = np.array([i for _ in NAMES for i in range(len(ps))], np.int32)
    poses = np.stack([_p13(ps[i]) for i in frame_of])
    model = np.concatenate([VM.verify(meshes[n], scenes, [i], poses[k:k + 1], K) for k, (n, i) in enumerate(zip(names, frame_of))])
    nm = dict(zip(zip(names, frame_of.tolist()), model["n_model"].tolist()))
    assert all(v > 0 for v in nm.values()), nm
    if size == "64x48":
        a1 = model["rect"][names.index("A") + 1]
        assert nm[("D", 0)] < 40 and a1[0] + a1[2] == w, (nm, a1)
    t = vga if size == "640x480" else Trackers(ctx, meshes, w, h, 2, 8, 1000)
    try:
        for fused in (0, 1):
            with util.options(ctx, {"verify_fused": fused}):
                got = t.multi.verify(scenes, frame_of, poses, K, mesh_of=_mesh_of(names))
                alone = t.gathered(lambda trk, f, p: trk.verify(scenes, f, p, K), names, frame_of, poses)
            assert got.tobytes() == model.tobytes(), (size, fused, got, model)
            assert got.tobytes() == alone.tobytes(), (size, fused)
    finally:
        if t is not vga:
            t.close()


# ---- 2. 70 poses cross the 64-view render chunk: mesh_of is read at the chunk's offset -----------------------------------------
def test_70_poses_cycling_through_the_meshes_cross_the_render_chunk(ctx, vga):
    scenes = [synth.render(W, H, *_pose(POSES[i], OFFSETS[2]), seed=21 + i)[0] for i in range(3)]
    names = [MS.ORDER[t % 4] for t in range(70)]
    frame_of = np.arange(70, dtype=np.int32) % 3
    base = np.stack([_p13(POSES[f]) for f in frame_of])
    base[:, 3] += np.arange(70, dtype=np.float32) - 35.0                     # every pose its own: tx moves by a millimetre per pose
    records = {}
    for fused in (0, 1):
        with util.options(ctx, {"verify_fused": fused}):
            got = vga.multi.verify(scenes, frame_of, base, K0, mesh_of=_mesh_of(names))
            alone = vga.gathered(lambda trk, f, p: trk.verify(scenes, f, p, K0), names, frame_of, base)
        assert got.tobytes() == alone.tobytes(), fused
        records[fused] = got
    assert records[0].tobytes() == records[1].tobytes() and (records[0]["n_model"] > 0).all()
    assert len({r.tobytes() for r in records[0][64:]}) > 1                   # the poses past the first chunk are not one record


# ---- 3. tracking ---------------------------------------------------------------------------------------------------------------
# (mesh, frame, pose): two frames, meshes A, B and C, a lost track, an out-of-view track, one overflowing max_crop_px
TRACKS = [("A", 0, POSES[0]), ("B", 0, POSES[0]), ("C", 0, POSES[0]), ("A", 1, POSES[1]), ("A", 1, LOST_POSE), ("B", 0, GONE_POSE),
          ("C", 1, BIG_POSE), ("C", 1, POSES[1])]
GROUPS = [0, 3, 5, 8]                                                         # the first group: meshes A, B and C on one object


@pytest.fixture(scope="module")
def tracks():
    scenes = [synth.render(W, H, *_pose(POSES[i], OFFSETS[0]), seed=40 + i)[0] for i in range(2)]
    return dict(scenes=scenes, names=[n for n, _, _ in TRACKS], frame_of=np.array([f for _, f, _ in TRACKS], np.int32),
                poses=np.stack([_p13(p) for _, _, p in TRACKS]))


@pytest.mark.parametrize("build", ["1024", "256", "256x5", "p2plane"])
def test_track_equals_the_one_mesh_trackers(ctx, vga, tracks, build):
    mode = L.FL_ICP_POINT_TO_PLANE if build == "p2plane" else L.FL_ICP_PARITY
    opts = {} if build == "p2plane" else {"icp_wide": 1 if build == "1024" else 0, "icp_occ": 5 if build == "256x5" else 0}
    s, names, fof, poses = tracks["scenes"], tracks["names"], tracks["frame_of"], tracks["poses"]
    with util.options(ctx, opts):
        got = vga.multi.track(s, fof, poses, K0, mesh_of=_mesh_of(names), icp_mode=mode)
        alone = vga.gathered(lambda trk, f, p: trk.track(s, f, p, K0, icp_mode=mode), names, fof, poses)
        assert got.tobytes() == alone.tobytes(), build
        assert got["tracked"][[0, 1, 3]].tolist() == [1, 1, 1] and got["tracked"][[4, 5, 6]].tolist() == [0, 0, 0]
        assert got["status"].tolist() == [0, 0, 0, 0, 0, 0, L.FL_ERR_OVERFLOW, 0]
        assert got[4]["rect_model"][2] > 0 and not got[5]["rect_model"].any() and got[6]["rect_model"][2] * got[6]["rect_model"][3] > MAX_CROP
        assert len({got[t].tobytes() for t in range(3)}) == 3                 # one pose, one frame, three meshes: three records
        # two passes are two chained calls
        two = vga.multi.track(s, fof, poses, K0, mesh_of=_mesh_of(names), icp_mode=mode, passes=2)
        chained = vga.multi.track(s, fof, api.poses13_of(got), K0, mesh_of=_mesh_of(names), icp_mode=mode)
        alone2 = vga.gathered(lambda trk, f, p: trk.track(s, f, p, K0, icp_mode=mode, passes=2), names, fof, poses)
    assert two.tobytes() == alone2.tobytes()
    for t in range(8):
        if got["tracked"][t]:
            a, b = two[t].copy(), chained[t].copy()
            if not b["tracked"]:                                              # lost in pass 2: the pose the CALL came in with
                a["pose"], b["pose"] = 0, 0
            assert a.tobytes() == b.tobytes(), t
        else:
            assert two[t].tobytes() == got[t].tobytes(), t


@pytest.fixture(scope="module")
def tracks_model(meshes, tracks, oracle):
    """track_verified_model with every track's own mesh, parity mode, keep_input = 1; computed once, read only."""
    out = []
    for n, f, p in zip(tracks["names"], tracks["frame_of"], tracks["poses"]):
        r = TVM.track_verified(meshes[n], tracks["scenes"], [f], p[None], K0, keep_input=1, max_crop_px=MAX_CROP, oracle=oracle, icp_mode=TM.PARITY)[0]
        r["pose_in"] = p
        out.append(r)
    return out


def _same_as_model(got, exp, keep_input):
    vin = exp["verify_in"] if keep_input and exp["icp_tracked"] else np.zeros((), VM.DTYPE)
    tracked, kept = TVM.decide(exp["icp_tracked"], exp["verify"], vin, keep_input)
    assert (got["icp_tracked"], got["track"]["tracked"], got["kept_input"]) == (exp["icp_tracked"], tracked, kept)
    assert got["verify"].tobytes() == exp["verify"].tobytes() and got["verify_in"].tobytes() == vin.tobytes(), (got, exp)
    if exp["icp_tracked"]:
        icp = np.eye(4, dtype=np.float32)
        icp[:3, :3], icp[:3, 3] = exp["track"]["det"]["R_final"], exp["track"]["det"]["T_final"]
        _same_as_parity_model(got["track"], dict(exp["track"], tracked=tracked, pose=icp if tracked and not kept else TM.pose4x4(exp["pose_in"])))
    else:
        assert got["track"]["status"] == exp["track"]["status"] and tuple(got["track"]["rect_model"]) == tuple(exp["track"]["rect_model"])


@pytest.mark.parametrize("keep", [0, 1])
def test_track_verified_equals_the_one_mesh_trackers_and_the_model(ctx, vga, tracks, tracks_model, keep):
    s, names, fof, poses = tracks["scenes"], tracks["names"], tracks["frame_of"], tracks["poses"]
    kw = dict(keep_input=keep, icp_mode=L.FL_ICP_PARITY)
    got = vga.multi.track_verified(s, fof, poses, K0, mesh_of=_mesh_of(names), **kw)
    alone = vga.gathered(lambda trk, f, p: trk.track_verified(s, f, p, K0, **kw), names, fof, poses)
    assert got.tobytes() == alone.tobytes()
    for t in range(8):
        _same_as_model(got[t], tracks_model[t], keep)
    assert got["icp_tracked"][[0, 1, 3]].tolist() == [1, 1, 1] and (got["verify"]["n_model"][[0, 1, 3]] > 1000).all()
    with util.options(ctx, {"verify_fused_px": 1024}):                        # several bands per pose
        banded = vga.multi.track_verified(s, fof, poses, K0, mesh_of=_mesh_of(names), **kw)
    assert banded.tobytes() == got.tobytes()
    # groups that mix meshes: everything but `best` is the ungrouped call's, `best` follows the exact comparison
    grouped = vga.multi.track_verified(s, fof, poses, K0, group_first=GROUPS, mesh_of=_mesh_of(names), **kw)
    best = TVM.pick(got["track"]["tracked"], got["kept_input"], got["verify"], got["verify_in"], GROUPS)
    assert grouped["best"].tolist() == best and sum(best[:3]) == 1 and got["track"]["tracked"][:3].sum() >= 2
    a, b = grouped.copy(), got.copy()
    a["best"], b["best"] = 0, 0
    assert a.tobytes() == b.tobytes()
    # mesh A on the object it is the mesh of beats the box alone and the sphere
    assert best[0] == 1, (got["verify"][:3], got["verify_in"][:3])


# ---- 4. defaults ---------------------------------------------------------------------------------------------------------------
def _old_verify(lib, trk, scenes, frame_of, poses, K):
    """fl_verify_batch itself, the entry point without mesh_of (api.Tracker.verify goes through fl_verify_batch_meshes)."""
    frames = [np.ascontiguousarray(s, np.uint16) for s in scenes]
    dp = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
    fof, p = np.ascontiguousarray(frame_of, np.int32), np.ascontiguousarray(poses, np.float32)
    k = L.Intrinsics(trk.w, trk.h, *[float(x) for x in K])
    out = np.zeros(len(fof), api.VERIFY_DTYPE)
    rc = lib.fl_verify_batch(trk.handle, len(frames), dp, L.FL_MEM_HOST, len(fof), fof.ctypes.data, p.ctypes.data, 0, None, C.byref(k), None, out.ctypes.data)
    assert rc == L.FL_OK
    return out


def test_no_mesh_of_is_mesh_0_and_the_old_entry_points_are_unchanged_around_a_multi_mesh_call(ctx, vga, tracks):
    s, fof, poses = tracks["scenes"], tracks["frame_of"], tracks["poses"]
    assert MS.ORDER[0] == "B"
    for fused in (0, 1):
        with util.options(ctx, {"verify_fused": fused}):
            before = _old_verify(ctx.lib, vga.multi, s, fof, poses, K0)
            assert vga.multi.verify(s, fof, poses, K0).tobytes() == before.tobytes() == vga.one["B"].verify(s, fof, poses, K0).tobytes()
            assert vga.multi.verify(s, fof, poses, K0, mesh_of=np.zeros(8, np.int32)).tobytes() == before.tobytes()
            vga.multi.verify(s, fof, poses, K0, mesh_of=_mesh_of(tracks["names"]))
            assert _old_verify(ctx.lib, vga.multi, s, fof, poses, K0).tobytes() == before.tobytes() and before["n_model"][0] > 1000
    t0 = vga.multi.track(s, fof, poses, K0)
    v0 = vga.multi.track_verified(s, fof, poses, K0, keep_input=1)
    assert t0.tobytes() == vga.one["B"].track(s, fof, poses, K0).tobytes()
    assert v0.tobytes() == vga.one["B"].track_verified(s, fof, poses, K0, keep_input=1).tobytes()
    vga.multi.track_verified(s, fof, poses, K0, keep_input=1, mesh_of=_mesh_of(tracks["names"]))
    assert vga.multi.track(s, fof, poses, K0).tobytes() == t0.tobytes()
    assert vga.multi.track_verified(s, fof, poses, K0, keep_input=1).tobytes() == v0.tobytes()
    # a mesh_of on a tracker of one mesh can only say 0
    assert vga.one["A"].verify(s, fof, poses, K0, mesh_of=np.zeros(8, np.int32)).tobytes() == vga.one["A"].verify(s, fof, poses, K0).tobytes()
    with pytest.raises(api.FealessError) as e:
        vga.one["A"].verify(s, fof, poses, K0, mesh_of=np.ones(8, np.int32))
    assert e.value.code == L.FL_ERR_INVALID
    with pytest.raises(api.FealessError) as e:
        vga.multi.track(s, fof, poses, K0, mesh_of=np.full(8, 4, np.int32))
    assert e.value.code == L.FL_ERR_INVALID


# ---- 5. the verified pick with a mesh per class ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three(ctx, oracle):
    """The three-class detector of tests/multiclass.py on the cluttered frames a - d, every match of every frame refined."""
    sc = clutter.build(oracle)
    bgrs, depths = [sc["frames"][f][0] for f in clutter.FRAMES], [sc["frames"][f][1] for f in clutter.FRAMES]
    det = api.Detector(ctx, 2, clutter.T)
    for b in multiclass.split(sc["bank"]):
        det.add_class(b)
    det.finalize(clutter.W, clutter.H, max_batch=NF)
    assert [b.class_id for b in det.banks] == list(multiclass.SORTED_IDS)
    lists = [m for m, _ in det.match_batch(bgrs, depths, P[0])]
    params = L.RecognitionParams(*P, L.FL_ICP_PARITY)
    refined = []
    for f, m in enumerate(lists):
        row = []
        for i0 in range(0, len(m), NF):
            part = m[i0:i0 + NF]
            res = det.refine_matches([f] * len(part), part, sc["K"], params)
            row += [api.recognition_result_to_dict(res[i]) for i in range(len(part))]
        refined.append(row)
    yield dict(det=det, K=sc["K"], bgrs=bgrs, depths=depths, lists=lists, refined=refined, wh=M.widths_heights(det.banks))
    det.close()


def _pose13_of_44(pose44):
    p = np.zeros(13, np.float32)
    p[:12] = np.ascontiguousarray(pose44, np.float32).reshape(-1)[:12]
    return p


def test_verified_pick_with_a_mesh_per_class(ctx, vga, three):
    det, K, G, h = three["det"], three["K"], 8, 4
    mesh_of_class = [IDX["A"], -1, IDX["C"]]                                  # alpha -> A, mid -> none, zeta -> C
    name_of_class = {0: "A", 2: "C"}
    got, members = det.recognize_batch_instances_verified(vga.multi, three["bgrs"], three["depths"], K, G, MIN_DIST, h, -1, True, *P,
                                                          mesh_of_class=mesh_of_class)
    plain = det.recognize_batch_instances(three["bgrs"], three["depths"], K, G, MIN_DIST, h, *P)
    assert [len(g) for g in got] == [len(g) for g in plain] and sum(len(g) for g in got) >= 6
    exp = np.zeros((NF, G, h), VM.DTYPE)
    seen = set()
    for f in range(NF):
        m, ref = three["lists"][f], three["refined"][f]
        gof, _, ng = M.group(m, three["wh"], G, MIN_DIST)
        assert ng == len(got[f])
        for g in range(ng):
            mem = [int(i) for i in np.nonzero(gof == g)[0][:h]]
            cls = int(m["class_idx"][mem[0]])
            found = [int(ref[i]["found"]) for i in mem]
            verified = cls in name_of_class
            seen.add(cls)
            live = [r for r in range(len(mem)) if found[r]] if verified else []
            if live:                                                          # Tracker.verify on the one-mesh tracker of the class's mesh
                poses = np.stack([_pose13_of_44(ref[mem[r]]["pose"]) for r in live])
                rec = vga.one[name_of_class[cls]].verify([three["depths"][f]], [0] * len(live), poses, K)
                rec["best"] = 0
                exp[f, g, live] = rec
            nms = mem.index(M.pick(ref, mem))
            pick, best = VP.pick(found, exp[f, g, :len(mem)], nms, verified)
            if best >= 0:
                exp["best"][f, g, best] = 1
            inst, t = got[f][g], (f, g)
            assert inst["verified"] == int(verified) and inst["best"]["class_idx"] == cls, t
            assert inst["rank"] == mem[pick] and inst["nms_rank"] == mem[nms] == plain[f][g]["rank"], t
            assert inst["verify"].tobytes() == (exp[f, g, pick].tobytes() if verified else bytes(64)), t
            assert inst["n_refined"] == len(mem) and inst["n_members"] == plain[f][g]["n_members"], t
            if verified and live:
                assert exp["n_model"][f, g].max() > 1000, t
    assert members.tobytes() == exp.tobytes(), (members[members != exp], exp[members != exp])
    assert seen == {0, 1, 2}                                                  # mapped and unmapped classes both occur
    # another mesh for a class is another record: class alpha against C instead of A
    other, om = det.recognize_batch_instances_verified(vga.multi, three["bgrs"], three["depths"], K, G, MIN_DIST, h, -1, True, *P,
                                                       mesh_of_class=[IDX["C"], -1, IDX["C"]])
    assert om.tobytes() != members.tobytes()


def _instances_bytes(res):
    return [[(i["rank"], i["nms_rank"], i["verified"], i["n_members"], i["n_refined"], i["verify"].tobytes(),
              np.ascontiguousarray(i["pose"], np.float32).tobytes(), i["best"]["class_idx"], i["best"]["template_id"]) for i in g] for g in res]


def test_the_maps_that_say_what_class_idx_says(vga, three):
    det, K, G, h = three["det"], three["K"], 8, 4
    args = (three["bgrs"], three["depths"], K, G, MIN_DIST, h)
    one, multi = vga.one["A"], vga.multi
    old_all, m_all = det.recognize_batch_instances_verified(one, *args, -1, True, *P)
    new_all, n_all = det.recognize_batch_instances_verified(one, *args, -1, True, *P, mesh_of_class=[0, 0, 0])
    assert m_all.tobytes() == n_all.tobytes() and _instances_bytes(old_all) == _instances_bytes(new_all) and m_all["n_model"].max() > 5000
    old_2, m_2 = det.recognize_batch_instances_verified(one, *args, 2, True, *P)
    new_2, n_2 = det.recognize_batch_instances_verified(one, *args, -1, True, *P, mesh_of_class=[-1, -1, 0])
    assert m_2.tobytes() == n_2.tobytes() and _instances_bytes(old_2) == _instances_bytes(new_2) and m_2.tobytes() != m_all.tobytes()
    # on the tracker of four meshes the same map names mesh A by its index there
    via_multi, n_m = det.recognize_batch_instances_verified(multi, *args, -1, True, *P, mesh_of_class=[-1, -1, IDX["A"]])
    assert n_m.tobytes() == m_2.tobytes() and _instances_bytes(via_multi) == _instances_bytes(old_2)
    # the call without a map on the tracker of four meshes verifies against mesh 0, the box
    box, n_b = det.recognize_batch_instances_verified(multi, *args, -1, True, *P)
    box_one, n_b1 = det.recognize_batch_instances_verified(vga.one["B"], *args, -1, True, *P)
    assert n_b.tobytes() == n_b1.tobytes() and _instances_bytes(box) == _instances_bytes(box_one) and n_b.tobytes() != m_all.tobytes()
    for bad in ([0, 0], [0, 0, 4], [-2, 0, 0]):
        with pytest.raises((api.FealessError, ValueError)):
            det.recognize_batch_instances_verified(multi, *args, -1, True, *P, mesh_of_class=bad)
    with pytest.raises(api.FealessError):
        det.recognize_batch_instances_verified(multi, *args, 1, True, *P, mesh_of_class=[0, 0, 0])


# ---- 6. the facade ---------------------------------------------------------------------------------------------------------------
def test_facade_picks_the_mesh_by_the_tag(ctx, meshes, tmp_path):
    """CadRecoSetTrackingMeshes with two class ids and two OBJ files: CadRecoVerify on a recognised result takes the mesh of the
    result's tag, and the record is the C ABI's on that mesh as the facade reads it; a tag without a mesh is refused."""
    from test_gpu_verify import FACADE_RESULT, INVALID
    cad = cadreco_py.lib()
    obj, box = str(tmp_path / "object.obj"), str(tmp_path / "box.obj")
    synth.write_obj(obj, synth.object_mesh(2))
    synth.write_obj(box, meshes["B"], with_normals=False)

    def verify(h, depth, poses16, tags):
        p = np.ascontiguousarray(poses16, np.float32)
        out = np.zeros(len(p), FACADE_RESULT)
        if tags is None:
            return cad.cadreco_verify(h, *cadreco_py.frame_args(depth, 0.0, K0), len(p), p.ctypes.data, 10.0, out.ctypes.data), out
        tg = (C.c_char_p * len(p))(*tags)
        return cad.cadreco_verify_tagged(h, *cadreco_py.frame_args(depth, 0.0, K0), len(p), p.ctypes.data, tg, 10.0, out.ctypes.data), out

    h = C.c_void_p(cad.cadreco_create(1))
    assert h.value
    one = {}
    try:
        V, N, T, depth, pose = cadreco_py.recognised_mesh_frame(h, ctx, obj, str(tmp_path / "bank"))
        Vb, _, Tb = cadreco_py.read_obj(box)
        assert len(T) == 332 and len(Tb) == 12
        poses = np.stack([pose, pose])
        ids, paths = (C.c_char_p * 2)(b"box", b"mesh"), (C.c_char_p * 2)(box.encode(), obj.encode())
        assert cad.cadreco_set_tracking_meshes(h, 2, (C.c_char_p * 2)(b"box", b"box"), paths, 1.0) == INVALID      # an id twice
        assert cad.cadreco_set_tracking_meshes(h, 0, ids, paths, 1.0) == INVALID
        assert cad.cadreco_set_tracking_meshes(h, 2, ids, paths, 1.0) == 0
        rc, got = verify(h, depth, poses, [b"mesh", b"box"])
        assert rc == 0
        one = dict(mesh=api.Tracker(ctx, V, T, W, H, 1, 2, 1000), box=api.Tracker(ctx, Vb, Tb, W, H, 1, 2, 1000))
        p44 = pose.reshape(1, 4, 4)
        want = [one["mesh"].verify([depth], [0], p44, K0)[0], one["box"].verify([depth], [0], p44, K0)[0]]
        for g, e in zip(got, want):
            assert all(g[k] == e[k] for k in FACADE_RESULT.names), (g, e)
        assert got["n_model"][0] > 5000 and got["n_model"][1] > 1000 and got["n_model"][0] != got["n_model"][1] and got["inlier_ratio"][0] > 0.9
        # a tag without a mesh, and an entry without a tag
        assert verify(h, depth, poses, [b"mesh", b"sphere"])[0] == INVALID
        assert verify(h, depth, poses, None)[0] == INVALID
        # CadRecoSetTrackingMesh keeps its meaning: one mesh whatever the tag
        assert cad.cadreco_set_tracking_mesh(h, box.encode(), 1.0) == 0
        rc, again = verify(h, depth, poses, [b"mesh", b"sphere"])
        assert rc == 0 and all(again[i][k] == want[1][k] for i in range(2) for k in FACADE_RESULT.names)
        assert verify(h, depth, poses, None)[0] == 0
    finally:
        for t in one.values():
            t.close()
        cad.cadreco_destroy(h)
