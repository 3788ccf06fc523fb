"""GPU: fl_recognize_batch_instances_verified on the cluttered frames a - d (tests/clutter.py) against the models: every job
slot's record against tests/verify_model.py at the pose fl_refine_matches returns for the slot's match (existing tests hold that
pose to the oracle) and against Tracker.verify of that pose, the pick against tests/verified_pick_model.py, bit for bit; and
k_pick_verified alone (fl_dev_pick_verified) on hand-made and random groups.

The mesh is synth.object_mesh(2), 332 triangles: the frames show the analytic object, which that mesh approximates; the records
only have to equal the model's on the same mesh.  On frame b the model says of the two picked poses: the instance that is partly
hidden has n_front = 2387 of n_model = 11558 (the hiding instance stands in front of it) and n_behind = 33, the hiding one
n_front = 19 and n_behind = 84 of 14921: the camera sees through neither, n_behind is silhouette pixels of the coarse mesh.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import cadreco_py
import clutter
import instances_model as M
import multiclass
import verified_pick_model as VP
import verify_model as VM
from fealess_amd import _lib as L
from fealess_amd import api, synth
from test_abi_cpu import write_bank_dir
from test_instances_cpu import MIN_DIST, TABLE
from test_instances_verified_cpu import CASES, REFUSED, _call, _records

pytestmark = pytest.mark.gpu


P = (75.0, 10, 0.5, 0.01)
NF = len(clutter.FRAMES)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def scene(oracle):
    sc = clutter.build(oracle)
    sc["bgrs"] = [sc["frames"][f][0] for f in clutter.FRAMES]
    sc["depths"] = [sc["frames"][f][1] for f in clutter.FRAMES]
    return sc


@pytest.fixture(scope="module")
def mesh():
    return synth.object_mesh(2)


@pytest.fixture(scope="module")
def cdet(ctx, scene):
    det = api.Detector(ctx, 2, clutter.T)
    det.add_class(scene["bank"])
    det.finalize(clutter.W, clutter.H, max_batch=NF)
    yield det
    det.close()


@pytest.fixture(scope="module")
def trk(ctx, mesh):
    t = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], clutter.W, clutter.H, NF, 128, 40000)
    yield t
    t.close()


@pytest.fixture(scope="module")
def ground(cdet, scene, mesh):
    """Per frame: the match list, fl_refine_matches of every match, and a cache of the model's renders by pose."""
    lists = [m for m, _ in cdet.match_batch(scene["bgrs"], scene["depths"], P[0])]
    params = L.RecognitionParams(*P, L.FL_ICP_PARITY)
    refined = []
    for f, m in enumerate(lists):
        row = []
        for i0 in range(0, len(m), NF):                 # at most max_batch jobs per call
            part = m[i0:i0 + NF]
            res = cdet.refine_matches([f] * len(part), part, scene["K"], params)
            row += [api.recognition_result_to_dict(res[i]) for i in range(len(part))]
        refined.append(row)
    assert [len(m) for m in lists] == [TABLE[f]["n"] for f in clutter.FRAMES]
    return dict(lists=lists, refined=refined, wh=M.widths_heights([scene["bank"]]), renders={})


def _p13(pose44):
    p = np.zeros(13, np.float32)
    p[:12] = np.ascontiguousarray(pose44, np.float32).reshape(-1)[:12]
    return p


def _expected(ground, scene, mesh, G, h, **vprm):
    """(records (NF, G, h), per frame a list of dict(members, pick, best, nms)) from the models alone."""
    rec = np.zeros((NF, G, h), VM.DTYPE)
    groups = []
    for f in range(NF):
        m, ref = ground["lists"][f], ground["refined"][f]
        gof, _, ng = M.group(m, ground["wh"], G, MIN_DIST)
        row = []
        for g in range(ng):
            mem = [int(i) for i in np.nonzero(gof == g)[0][:h]]
            found = [int(ref[i]["found"]) for i in mem]
            for r, i in enumerate(mem):
                if not found[r]:
                    continue
                p = _p13(ref[i]["pose"])
                key = p.tobytes()
                if key not in ground["renders"]:
                    ground["renders"][key] = VM.render(mesh, p, scene["K"], clutter.W, clutter.H)
                rec[f, g, r] = VM.score(ground["renders"][key], scene["depths"][f], **vprm)
            nms = mem.index(M.pick(ref, mem))
            pick, best = VP.pick(found, rec[f, g, :len(mem)], nms, True)
            rec["best"][f, g, :len(mem)] = 0
            if best >= 0:
                rec["best"][f, g, best] = 1
            row.append(dict(members=mem, pick=pick, best=best, nms=nms))
        groups.append(row)
    return rec, groups


def _check(got, members, exp_rec, exp_groups, ground, tag):
    assert members.tobytes() == exp_rec.tobytes(), (tag, members[members != exp_rec], exp_rec[members != exp_rec])
    assert [len(g) for g in got] == [len(g) for g in exp_groups], tag
    for f in range(NF):
        for g, (inst, e) in enumerate(zip(got[f], exp_groups[f])):
            t = (tag, f, g)
            rank = e["members"][e["pick"]]
            assert inst["verified"] == 1 and inst["rank"] == rank and inst["nms_rank"] == e["members"][e["nms"]], t
            assert inst["verify"].tobytes() == exp_rec[f, g, e["pick"]].tobytes(), t
            assert inst["verify"]["best"] == (1 if e["best"] >= 0 else 0), t
            ref = ground["refined"][f][rank]
            assert inst["found"] == ref["found"] and np.array_equal(_bits(inst["pose"]), _bits(ref["pose"])), t
            assert _bits(inst["det"]["icp"]["dist_mean"]) == _bits(ref["det"]["icp"]["dist_mean"]) and inst["n_refined"] == len(e["members"]), t


@pytest.mark.parametrize("h", [4, 64])
def test_member_records_and_the_pick(cdet, trk, scene, mesh, ground, h):
    exp_rec, exp_groups = _expected(ground, scene, mesh, 8, h)
    got, members = cdet.recognize_batch_instances_verified(trk, scene["bgrs"], scene["depths"], scene["K"], 8, MIN_DIST, h, -1, True, *P)
    _check(got, members, exp_rec, exp_groups, ground, h)
    assert [len(g) for g in got] == [3, 2, 2, 0] and VM.invariant(members.reshape(-1))
    # nms_rank is what fl_recognize_batch_instances picks
    plain = cdet.recognize_batch_instances(scene["bgrs"], scene["depths"], scene["K"], 8, MIN_DIST, h, *P)
    assert [[i["nms_rank"] for i in g] for g in got] == [[i["rank"] for i in g] for g in plain] == [TABLE[f]["pick64" if h == 64 else "pick4"] for f in clutter.FRAMES]
    # every live slot's record is Tracker.verify's of the same pose on the same frame
    live = [(f, g, r, i) for f in range(NF) for g, e in enumerate(exp_groups[f]) for r, i in enumerate(e["members"]) if ground["refined"][f][i]["found"]]
    assert len(live) > 10 and len(live) <= 128
    poses = np.stack([np.asarray(ground["refined"][f][i]["pose"], np.float32).reshape(4, 4) for f, g, r, i in live])
    tv = trk.verify(scene["depths"], [f for f, *_ in live], poses, scene["K"])
    for k, (f, g, r, i) in enumerate(live):
        a, b = tv[k].copy(), members[f, g, r].copy()
        a["best"] = b["best"] = 0
        assert a.tobytes() == b.tobytes(), (f, g, r)
    n_live = np.zeros((NF, 8, h), bool)
    for f, g, r, i in live:
        n_live[f, g, r] = True
    assert (members[~n_live].view(np.uint8) == 0).all()                              # absent and not-found slots are zero
    assert (exp_rec["n_model"][n_live] > 5000).all()
    # frame b: the partly hidden instance
    b = [i["verify"] for i in got[1]]
    assert max(int(v["n_front"]) for v in b) > 0, b


def test_one_instance_one_hypothesis_is_recognize_batch_and_its_verification(cdet, trk, scene):
    base = cdet.recognize_batch(scene["bgrs"], scene["depths"], scene["K"], *P)
    got = cdet.recognize_batch_instances_verified(trk, scene["bgrs"], scene["depths"], scene["K"], 1, MIN_DIST, 1, -1, False, *P)
    assert [len(g) for g in got] == [1, 1, 1, 0]
    for f in range(3):
        g, e = got[f][0], base[f]
        assert g["rank"] == g["nms_rank"] == 0 and e["found"] == g["found"] == 1 and g["best"] == e["best"], f
        assert np.array_equal(_bits(g["pose"]), _bits(e["pose"])), f
        v = trk.verify([scene["depths"][f]], [0], np.asarray(e["pose"], np.float32).reshape(1, 4, 4), scene["K"])[0]
        assert v.tobytes() == g["verify"].tobytes() and v["accepted"] == 1 and v["best"] == 1, f


def test_gates(cdet, trk, scene, mesh, ground):
    free, groups = _expected(ground, scene, mesh, 8, 4)
    live = free["n_model"] > 0
    ir, br = free["inlier_ratio"][live], free["behind_ratio"][live]
    lo, hi = (float(np.sort(ir)[len(ir) // 2 - 1]) + float(np.sort(ir)[len(ir) // 2])) / 2, (float(br.min()) + float(br.max())) / 2
    for prm in (dict(min_inlier_ratio=lo), dict(max_behind_ratio=hi), dict(min_model_px=int(free["n_model"][live].min()) + 1), dict(min_inlier_ratio=lo, max_behind_ratio=hi, tau_mm=7)):
        exp_rec, exp_groups = _expected(ground, scene, mesh, 8, 4, **prm)
        acc = exp_rec["accepted"][live]
        assert "tau_mm" in prm or 0 < acc.sum() < len(acc), prm                      # from the model alone: it rejects and it accepts
        got, members = cdet.recognize_batch_instances_verified(trk, scene["bgrs"], scene["depths"], scene["K"], 8, MIN_DIST, 4, -1, True, *P, **prm)
        _check(got, members, exp_rec, exp_groups, ground, prm)


def test_overflow_grows_and_device_frames_equal_host_frames(ctx, cdet, trk, scene):
    want, wm = cdet.recognize_batch_instances_verified(trk, scene["bgrs"], scene["depths"], scene["K"], 8, MIN_DIST, 4, -1, True, *P)
    det = api.Detector(ctx, 2, clutter.T)
    det.add_class(scene["bank"])
    det.finalize(clutter.W, clutter.H, max_batch=NF, max_candidates=64)              # every cluttered frame overflows 64 candidates
    try:
        got, gm = det.recognize_batch_instances_verified(trk, scene["bgrs"], scene["depths"], scene["K"], 8, MIN_DIST, 4, -1, True, *P)
        assert det.frame_counters(0)[2] == 0
    finally:
        det.close()
    d_b = torch.from_numpy(np.stack(scene["bgrs"])).cuda()
    d_d = torch.from_numpy(np.stack(scene["depths"]).view(np.int16)).cuda()
    torch.cuda.synchronize()
    bp = [d_b.data_ptr() + i * clutter.W * clutter.H * 3 for i in range(NF)]
    dp = [d_d.data_ptr() + i * clutter.W * clutter.H * 2 for i in range(NF)]
    dev, dm = cdet.recognize_batch_instances_verified(trk, bp, dp, scene["K"], 8, MIN_DIST, 4, -1, True, *P, mem=L.FL_MEM_DEVICE)
    for other, om, tag in ((got, gm, "grown"), (dev, dm, "device")):
        assert om.tobytes() == wm.tobytes(), tag
        for a, b in zip(other, want):
            assert [(i["rank"], i["nms_rank"], i["verify"].tobytes(), _bits(i["pose"]).tobytes()) for i in a] == \
                   [(i["rank"], i["nms_rank"], i["verify"].tobytes(), _bits(i["pose"]).tobytes()) for i in b], tag
    ms = cdet.instances_verify_ms()
    assert ms["fused"] > 0 and ms["finish"] > 0


def test_class_idx_verifies_that_class_only(ctx, trk, scene):
    """The three-class split of tests/multiclass.py (alpha, mid, zeta in class order): class_idx = 1 verifies the groups of
    class mid exactly as class_idx = -1 does; the groups of the other classes keep the NMS pick and zero records."""
    det = api.Detector(ctx, 2, clutter.T)
    for b in multiclass.split(scene["bank"]):
        det.add_class(b)
    det.finalize(clutter.W, clutter.H, max_batch=NF)
    try:
        assert [b.class_id for b in det.banks] == list(multiclass.SORTED_IDS)
        got, members = det.recognize_batch_instances_verified(trk, scene["bgrs"], scene["depths"], scene["K"], 8, MIN_DIST, 4, 1, True, *P)
        every, all_members = det.recognize_batch_instances_verified(trk, scene["bgrs"], scene["depths"], scene["K"], 8, MIN_DIST, 4, -1, True, *P)
    finally:
        det.close()
    assert [len(g) for g in got] == [len(g) for g in every] and len(got[3]) == 0
    classes = [i["best"]["class_idx"] for g in got for i in g]
    assert {0, 1, 2} == set(i["best"]["class_idx"] for i in got[0]) and classes.count(1) >= 2 and classes.count(1) < len(classes)
    for f in range(NF):
        for g, (i, e) in enumerate(zip(got[f], every[f])):
            assert e["verified"] == 1 and i["nms_rank"] == e["nms_rank"] and i["n_members"] == e["n_members"], (f, g)
            assert i["best"]["class_idx"] == e["best"]["class_idx"], (f, g)
            if e["best"]["class_idx"] == 1:
                assert i["verified"] == 1 and i["rank"] == e["rank"] and i["verify"].tobytes() == e["verify"].tobytes(), (f, g)
                assert np.array_equal(_bits(i["pose"]), _bits(e["pose"])) and members[f, g].tobytes() == all_members[f, g].tobytes(), (f, g)
                assert i["verify"]["n_model"] > 5000, (f, g)
            else:
                assert i["verified"] == 0 and i["rank"] == i["nms_rank"] and i["verify"].tobytes() == bytes(64), (f, g)
                assert (members[f, g].view(np.uint8) == 0).all() and all_members["n_model"][f, g].max() > 5000, (f, g)


def test_each_refusal_is_its_own(ctx, cdet, trk, mesh):
    """On a finalized detector and a tracker of its size and context the call of test_instances_verified_cpu.py is accepted;
    each refused argument list differs from it in one thing only.  Here the tracker's size and context are refusals of their own:
    a tracker of another size, a K of another size (which the tracker then does not have either), a tracker on a second context."""
    lib = ctx.lib
    rc, untouched, err = _call(lib, cdet, trk.handle)
    assert rc == L.FL_OK and not untouched, err
    for name, (over, text) in sorted(REFUSED.items()):
        if name == "a tracker on another context":
            continue
        rc, untouched, err = _call(lib, cdet, trk.handle, **over)
        assert rc == L.FL_ERR_INVALID and untouched, (name, rc, err)
        assert text is None or text in err, (name, err)
    half = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], 320, 240, 1, 4, 1000)
    ctx2 = api.Context(0)
    other = api.Tracker(ctx2, mesh["vertices"], mesh["triangles"], clutter.W, clutter.H, 1, 4, 1000)
    try:
        for name, over, text in (("tracker 320 x 240", dict(trk=half.handle), "is not the detector's"),
                                 ("K 320 x 240", dict(K=(320, 240, 608.0, 608.0, 320.0, 240.0)), "not K's"),
                                 ("K 640 x 481", dict(K=(640, 481, 608.0, 608.0, 320.0, 240.0)), "not K's"),
                                 ("another context", dict(trk=other.handle), "another context")):
            rc, untouched, err = _call(lib, cdet, trk.handle, **over)
            assert rc == L.FL_ERR_INVALID and untouched and text in err, (name, rc, err)
    finally:
        half.close()
        other.close()
        ctx2.close()
    rc, untouched, err = _call(lib, cdet, trk.handle)
    assert rc == L.FL_OK, err                                                         # a refused call changes nothing


def test_tracking_is_unchanged_by_a_verified_recognition_between(cdet, trk, scene):
    poses = np.stack([synth.pose13(*p) for p in scene["poses"]])
    before = trk.track(scene["depths"][:1], [0, 0, 0], poses, scene["K"])
    assert before["tracked"].any()
    cdet.recognize_batch_instances_verified(trk, scene["bgrs"], scene["depths"], scene["K"], 8, MIN_DIST, 4, -1, False, *P)
    after = trk.track(scene["depths"][:1], [0, 0, 0], poses, scene["K"])
    assert after.tobytes() == before.tobytes()


# ---- the facade ---------------------------------------------------------------------------------------------------------------
INVALID = cadreco_py.INVALID


def test_facade_verified_pick(ctx, cdet, scene, tmp_path):
    """CadRecoSetVerifiedPick on frame a: Recognition() returns the accepted instances in group order, with poses bit-equal to
    fl_recognize_batch_instances_verified's on the mesh as the facade reads it; with a gate between the instances' ratios only
    the accepted ones; switched off it returns what the multi-instance mode returned before, which is fl_recognize_batch_instances'."""
    bank = scene["bank"]
    d = tmp_path / "obj"
    write_bank_dir(d, bank, clutter.T, bank.model_depths)
    obj = str(tmp_path / "object.obj")
    synth.write_obj(obj, synth.object_mesh(2))
    lib = cadreco_py.lib()
    V, N, T = cadreco_py.read_obj(obj)
    bgr, depth = np.ascontiguousarray(scene["bgrs"][0]), np.ascontiguousarray(scene["depths"][0])
    h = C.c_void_p(lib.cadreco_create(1))
    assert h.value and lib.cadreco_add_obj(h, str(d).encode()) == 0 and lib.cadreco_set_params(h, *P, L.FL_ICP_PARITY) == 0

    def reco():
        rc, n, poses = cadreco_py.recognition_all(h, bgr, depth, scene["K"])
        assert rc == 0
        return poses[:n]
    trk = api.Tracker(ctx, V, T, clutter.W, clutter.H, 1, 4, 1000)
    try:
        # what it needs first
        assert lib.cadreco_set_verified_pick(h, 1, 10.0, 0.0, 0.0) == INVALID                      # neither the mode nor a mesh
        assert lib.cadreco_set_multi_instance(h, 8, MIN_DIST, 4) == 0
        assert lib.cadreco_set_verified_pick(h, 1, 10.0, 0.0, 0.0) == INVALID                      # no mesh
        assert lib.cadreco_set_tracking_mesh(h, obj.encode(), 1.0) == 0
        for bad in ((-1.0, 0.0, 0.0), (65536.0, 0.0, 0.0), (10.0, float("nan"), 0.0), (10.0, 0.0, float("inf"))):
            assert lib.cadreco_set_verified_pick(h, 1, *bad) == INVALID, bad
        multi = reco()
        plain = cdet.recognize_batch_instances([bgr], [depth], scene["K"], 8, MIN_DIST, 4, *P)[0]
        assert len(multi) == 3 and multi.tobytes() == np.stack([np.asarray(i["pose"], np.float32).reshape(16) for i in plain]).tobytes()
        # on, no gates: every instance is accepted
        want = cdet.recognize_batch_instances_verified(trk, [bgr], [depth], scene["K"], 8, MIN_DIST, 4, -1, False, *P)[0]
        assert len(want) == 3 and all(i["verify"]["accepted"] for i in want)
        assert lib.cadreco_set_verified_pick(h, 1, 10.0, 0.0, 0.0) == 0
        got = reco()
        assert got.tobytes() == np.stack([np.asarray(i["pose"], np.float32).reshape(16) for i in want]).tobytes()
        # a gate between the picked members' ratios, from the library's own records at no gate: fewer instances come back
        ratios = sorted(float(i["verify"]["inlier_ratio"]) for i in want)
        gate = (ratios[0] + ratios[1]) / 2
        assert ratios[0] < gate < ratios[1]
        want = cdet.recognize_batch_instances_verified(trk, [bgr], [depth], scene["K"], 8, MIN_DIST, 4, -1, False, *P, min_inlier_ratio=gate)[0]
        keep = [i for i in want if i["verify"]["accepted"]]
        assert 0 < len(keep) < 3
        assert lib.cadreco_set_verified_pick(h, 1, 10.0, gate, 0.0) == 0
        got = reco()
        assert got.tobytes() == np.stack([np.asarray(i["pose"], np.float32).reshape(16) for i in keep]).tobytes()
        # off: byte for byte the multi-instance result; leaving the multi-instance mode switches it off too
        assert lib.cadreco_set_verified_pick(h, 0, 0.0, 0.0, 0.0) == 0 and reco().tobytes() == multi.tobytes()
        assert lib.cadreco_set_verified_pick(h, 1, 10.0, gate, 0.0) == 0 and lib.cadreco_set_multi_hypothesis(h, 1, 20.0) == 0
        assert lib.cadreco_set_multi_instance(h, 8, MIN_DIST, 4) == 0 and reco().tobytes() == multi.tobytes()
    finally:
        trk.close()
        lib.cadreco_destroy(h)


# ---- k_pick_verified alone ----------------------------------------------------------------------------------------------------
JOB_DTYPE = np.dtype([("frame", "<i4"), ("match", api.MATCH_DTYPE)])
OUT_DTYPE = np.dtype([("reco", api.RESULT_DTYPE), ("rank", "<i4"), ("n_members", "<i4"), ("n_refined", "<i4"), ("reserved", "<i4"),
                      ("verify", VM.DTYPE), ("nms_rank", "<i4"), ("verified", "<i4"), ("reserved2", "<i4", 2)])


def test_pick_kernel_on_hand_made_and_random_groups(ctx):
    assert OUT_DTYPE.itemsize == C.sizeof(L.VerifiedInstanceResult) and JOB_DTYPE.itemsize == 24
    h = 6
    rng = np.random.default_rng(5)
    groups = []                                         # (found, records, class)
    for (found, rows, _, verified), _ in CASES.values():
        groups.append((list(found), _records(rows), 1 if verified else 0))
    for _ in range(3000):
        n = int(rng.integers(0, h + 1))
        nm = rng.integers(1, 40, n)
        rows = [(int(rng.integers(0, 2)), int(rng.integers(0, m + 1)), int(m)) for m in nm]
        groups.append(([int(v) for v in rng.integers(0, 2, n)], _records(rows), int(rng.integers(0, 2))))
    G = len(groups)
    res, jobs = np.zeros((G, h), api.RESULT_DTYPE), np.zeros((G, h), JOB_DTYPE)
    idx, vres = np.full((G, h), -1, np.int32), np.zeros((G, h), VM.DTYPE)
    size = np.zeros(G, np.int32)
    for g, (found, rec, cls) in enumerate(groups):
        n = len(found)
        jobs["frame"][g, n:] = -1
        jobs["match"]["class_idx"][g] = cls
        idx[g, :n] = 10 * np.arange(n) + 3
        res["found"][g, :n] = found
        res["det"]["n_points"][g, :n] = rng.integers(100, 2000, n)
        res["det"]["icp"]["dist_mean"][g, :n] = rng.uniform(0.1, 2.0, n).astype(np.float32)
        res["pose"][g, :n, 0] = np.arange(n)
        vres[g, :n] = rec
        vres["best"][g, :n] = rec["accepted"]           # as k_verify_finish leaves it
        size[g] = n + 2
    out = np.zeros(G, OUT_DTYPE)
    vin = vres.copy()
    ctx.check(L.dev(ctx.lib, "fl_dev_pick_verified")(ctx.h, G, h, 1, res.ctypes.data, jobs.ctypes.data, idx.ctypes.data, size.ctypes.data,
                                                     vres.ctypes.data, out.ctypes.data))
    picked_other = 0
    for g, (found, rec, cls) in enumerate(groups):
        n = len(found)
        nms = VP.nms_pick(found, res["det"]["n_points"][g, :n], res["det"]["icp"]["dist_mean"][g, :n])
        pick, best = VP.pick(found, rec, nms, cls == 1)
        o = out[g]
        assert o["verified"] == cls and o["n_refined"] == n and o["n_members"] == n + 2, g
        assert o["rank"] == idx[g, pick if n else 0] and o["nms_rank"] == idx[g, nms if n else 0], (g, found, rec, nms, pick)
        assert o["reco"]["pose"][0] == (pick if n else 0), g
        exp_best = vin["best"][g].copy()
        if cls == 1:
            exp_best[:n] = 0
            if best >= 0:
                exp_best[best] = 1
            e = vin[g, pick if n else 0].copy()
            e["best"] = exp_best[pick if n else 0]
            assert o["verify"].tobytes() == e.tobytes(), g
        else:
            assert o["verify"].tobytes() == bytes(64), g
        assert np.array_equal(vres["best"][g], exp_best), g
        picked_other += int(pick != nms)
    assert picked_other > 300
