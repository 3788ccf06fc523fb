"""Multi-instance recognition on the GPU: the grouping kernel alone against the numpy model (tests/instances_model.py) on
lists of every size class, and fl_recognize_batch_instances on the cluttered frames (tests/clutter.py) against the oracle's
refinement of the same matches and its nonMaximumSuppression, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import cadreco_py
import clutter
import instances_model as M
from fealess_amd import api
from fealess_amd import _lib as L
from fealess_amd.bank import MATCH_DTYPE
from test_abi_cpu import write_bank_dir
from test_instances_cpu import MIN_DIST, TABLE

pytestmark = pytest.mark.gpu

PARAMS = ((75.0, 10, 0.5, 0.01), (75.0, 20, 0.0, -3.0e38))       # those of test_gpu_clutter.py
NMS_DIST = 60.0
LDS_MAX = 16384                  # FL_GROUP_LDS_MAX: group ids in LDS up to this many matches, in global memory beyond


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the grouping kernel alone ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def banks():
    return M.small_banks()


@pytest.fixture(scope="module")
def gdet(ctx, banks):
    det = api.Detector(ctx, 2, [5, 8])
    for b in banks:
        det.add_class(b)
    det.finalize(640, 480, max_batch=1, max_candidates=64)
    yield det
    det.close()


def _group_on_device(det, m, G, dist):
    n = len(m)
    d_m = torch.from_numpy(np.frombuffer(m.tobytes() + b"\0" * 20, np.uint8).copy()).cuda()
    d_gof = torch.full((max(1, n),), -9, dtype=torch.int32, device="cuda")
    d_size = torch.full((G,), -9, dtype=torch.int32, device="cuda")
    d_ng = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    det.group_matches(d_m.data_ptr(), G, dist, mem=L.FL_MEM_DEVICE, n=n, group_of=d_gof.data_ptr(), group_size=d_size.data_ptr(),
                      n_groups=d_ng.data_ptr())
    det.ctx.synchronize()
    return d_gof.cpu().numpy()[:n], d_size.cpu().numpy(), int(d_ng.cpu()[0])


def _lists(n, banks):
    """Random and clustered lists, one where every match falls into one group, one where every match is a group of its own."""
    rng = np.random.default_rng(7 * n + 1)
    one = M.random_list(rng, n, banks, spread=20)
    one["class_idx"], one["template_id"] = 0, 0
    own = np.zeros(n, MATCH_DTYPE)
    own["x"], own["y"] = 97 * (np.arange(n) % 300), 97 * (np.arange(n) // 300)
    own["similarity"] = 90.0
    return dict(uniform=M.random_list(rng, n, banks), clustered=M.random_list(rng, n, banks, clusters=7), one_group=one, own_groups=own)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1025, LDS_MAX, LDS_MAX + 1, 70000])
def test_group_kernel_equals_model_and_host_path(gdet, banks, n):
    wh = M.widths_heights(banks)
    for name, m in _lists(n, banks).items():
        for G in (1, 3, 64):
            dist = 48
            # the sequential walk is the yardstick; above 5000 matches its statement by rounds (equal to it on every list of
            # test_instances_cpu.py) keeps the test short, with one sequential run per size
            if n <= 5000 or (name, G) == ("clustered", 64):
                e_gof, e_size, e_ng = M.group(m, wh, G, dist)
            else:
                e_gof, e_size, e_ng = M.group_rounds(m, wh, G, dist)
            gof, size, ng = _group_on_device(gdet, m, G, dist)
            tag = (n, name, G)
            assert ng == e_ng, tag
            assert np.array_equal(size, e_size), tag
            assert np.array_equal(gof, e_gof), tag
            h_gof, h_size, h_ng = gdet.group_matches(m, G, dist)
            assert h_ng == ng and np.array_equal(h_gof, gof) and np.array_equal(h_size, size), tag
            if name == "one_group" and n:
                assert ng == 1 and size[0] == n
            if name == "own_groups":
                assert ng == min(n, G) and (size[:ng] == 1).all() and int((gof == -1).sum()) == n - ng


def test_group_kernel_edge_lists(gdet, banks):
    """Exactly at the radius, coordinates at the ends of int32 with the largest radius, and matches that are not on the
    detector (the device path cannot refuse them: they get no group)."""
    wh = M.widths_heights(banks)
    big = 2 ** 31 - 1
    rows = [(50, 50, 0, 2), (53, 54, 0, 2), (53, 53, 0, 2), (-big - 1, -big - 1, 0, 0), (big, big, 1, 0), (-big, -big - 1, 0, 0), (big - 1, big, 1, 0)]
    m = np.zeros(len(rows), MATCH_DTYPE)
    for i, (x, y, c, t) in enumerate(rows):
        m[i] = (x, y, 90.0 - i, c, t)
    for dist in (5, 2 ** 30):
        e = M.group(m, wh, 8, dist)
        g = _group_on_device(gdet, m, 8, dist)
        assert g[2] == e[2] and np.array_equal(g[0], e[0]) and np.array_equal(g[1], e[1]), dist
    assert list(_group_on_device(gdet, m, 8, 5)[0][:3]) == [0, 1, 0]
    bad = m.copy()
    bad["class_idx"][1], bad["template_id"][4], bad["template_id"][5] = 2, banks[1].n_pyramids, -1
    gof, size, ng = _group_on_device(gdet, bad, 8, 5)
    keep = np.array([0, 2, 3, 6])
    e = M.group(bad[keep], wh, 8, 5)
    assert ng == e[2] and np.array_equal(gof[keep], e[0]) and np.array_equal(size, e[1]) and (gof[[1, 4, 5]] == -1).all()


@pytest.mark.parametrize("n,h", [(1, 4), (64, 4), (65, 1), (1025, 16), (LDS_MAX, 64), (LDS_MAX + 1, 64), (70000, 64)])
def test_group_kernel_places_the_first_members_in_list_order(gdet, banks, n, h):
    """The job list the grouping kernel writes for the ICP launch (fl_dev_group_jobs: the kernel with its jobs buffer on a
    caller's list): slot g * h + r holds the r-th member of group g in LIST order -- across the 64-match chunks the placing wave
    walks, with groups whose members lie thousands of matches apart, past the point where every group is full, and for lists
    whose group ids live in global memory -- and frame -1 / index -1 where a group has fewer than h members."""
    wh = M.widths_heights(banks)
    fn = L.dev(gdet.lib, "fl_dev_group_jobs")
    rng = np.random.default_rng(31 * n + h)
    late = M.random_list(rng, n, banks, clusters=5)          # a group whose second member is the list's last match
    if n > 2:
        late[0] = (5000, 5000, 99.0, 0, 0)
        late[n - 1] = (5001, 5001, 75.0, 0, 0)
    for name, m in (("clustered", M.random_list(rng, n, banks, clusters=9)), ("uniform", M.random_list(rng, n, banks)), ("late", late)):
        for G in (3, 64):
            e_gof, e_size, e_ng = M.group(m, wh, G, 48) if n <= 5000 else M.group_rounds(m, wh, G, 48)
            d_m = torch.from_numpy(np.frombuffer(m.tobytes(), np.uint8).copy()).cuda()
            d_gof = torch.full((n,), -9, dtype=torch.int32, device="cuda")
            d_size = torch.full((G,), -9, dtype=torch.int32, device="cuda")
            d_info = torch.full((4,), -9, dtype=torch.int32, device="cuda")
            d_jobs = torch.full((G * h, 6), -9, dtype=torch.int32, device="cuda")
            d_idx = torch.full((G * h,), -9, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ip = L.InstanceParams(G, 48, h)
            gdet.ctx.check(fn(gdet.h, d_m.data_ptr(), n, C.byref(ip), d_gof.data_ptr(), d_size.data_ptr(), d_info.data_ptr(), d_jobs.data_ptr(),
                              d_idx.data_ptr()))
            gdet.ctx.synchronize()
            tag = (n, h, name, G)
            assert np.array_equal(d_gof.cpu().numpy(), e_gof) and np.array_equal(d_size.cpu().numpy(), e_size), tag
            assert d_info.cpu().tolist() == [e_ng, int((e_gof == -1).sum()), 0, n], tag
            want = np.full((G, h), -1, np.int32)
            for g in range(e_ng):
                mem = np.nonzero(e_gof == g)[0][:h]
                want[g, :len(mem)] = mem
            idx = d_idx.cpu().numpy().reshape(G, h)
            assert np.array_equal(idx, want), tag
            jobs = d_jobs.cpu().numpy().reshape(G, h, 6)
            assert np.array_equal(jobs[..., 0], np.where(want >= 0, 0, -1)), tag          # FlRefineJob.frame
            sel = want >= 0
            assert np.array_equal(jobs[sel][:, 1:].copy().view(np.uint8).reshape(-1), np.frombuffer(m[want[sel]].tobytes(), np.uint8)), tag
            if name == "late" and n > 2 and G == 64 and h > 1:
                g = e_gof[0]
                assert e_gof[n - 1] == g and list(want[g, :2]) == [0, n - 1], tag


# ---- 2. - 7. the cluttered frames ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(oracle):
    sc = clutter.build(oracle)
    sc["bgrs"] = [sc["frames"][f][0] for f in clutter.FRAMES]
    sc["depths"] = [sc["frames"][f][1] for f in clutter.FRAMES]
    return sc


@pytest.fixture(scope="module")
def refined(oracle, scene):
    """Per frame: the oracle's refinement of every match (at most 64) and its nonMaximumSuppression winners."""
    return [oracle.recognition_topk(b, d, scene["K"], clutter.T, scene["bank"], 64, *PARAMS[0], nms_dist=NMS_DIST)
            for b, d in zip(scene["bgrs"], scene["depths"])]


def _detector(ctx, scene, max_candidates=0):
    det = api.Detector(ctx, 2, clutter.T)
    det.add_class(scene["bank"])
    det.finalize(clutter.W, clutter.H, max_batch=len(clutter.FRAMES), max_candidates=max_candidates)
    return det


@pytest.fixture(scope="module")
def cdet(ctx, scene):
    det = _detector(ctx, scene)
    yield det
    det.close()


def _assert_instance_is(g, e, rank, tag):
    """An instance against the oracle's refinement of match `rank`, bit for bit."""
    assert g["status"] == 0 and g["rank"] == rank and g["found"] == e["found"] == 1, tag
    assert (g["best"]["x"], g["best"]["y"], g["best"]["template_id"]) == (e["best"]["x"], e["best"]["y"], e["best"]["template_id"]), tag
    assert _bits(g["best"]["similarity"]) == _bits(e["best"]["similarity"]), tag
    assert g["det"]["n_points"] == e["det"]["n_points"], tag
    assert _bits(g["det"]["icp"]["dist_mean"]) == _bits(e["det"]["icp"]["dist_mean"]), tag
    assert np.array_equal(_bits(g["pose"]), _bits(e["pose"])), tag


def _assert_every_member_refined(got, refined, tag):
    """{8, 48, 64}: the instances are the oracle's NMS winners, in order."""
    assert [len(g) for g in got] == [3, 2, 2, 0], tag
    for i, f in enumerate(clutter.FRAMES):
        ref, win = refined[i]
        assert [g["rank"] for g in got[i]] == win == TABLE[f]["pick64"], (tag, f)
        assert [g["n_members"] for g in got[i]] == TABLE[f]["sizes"], (tag, f)
        for g, w in zip(got[i], win):
            _assert_instance_is(g, ref[w], w, (tag, f, w))
            assert g["n_matches"] == TABLE[f]["n"] and g["n_refined"] == g["n_members"], (tag, f, w)


def test_instances_equal_the_oracles_nms_winners(cdet, scene, refined):
    got, dropped = cdet.recognize_batch_instances(scene["bgrs"], scene["depths"], scene["K"], 8, MIN_DIST, 64, *PARAMS[0], with_dropped=True)
    _assert_every_member_refined(got, refined, "host")
    assert dropped == [0, 0, 0, 0]


def test_four_hypotheses_per_instance_and_the_cap(cdet, scene, refined):
    got = cdet.recognize_batch_instances(scene["bgrs"], scene["depths"], scene["K"], 8, MIN_DIST, 4, *PARAMS[0])
    for i, f in enumerate(clutter.FRAMES):
        assert [g["rank"] for g in got[i]] == TABLE[f]["pick4"], f
        for g in got[i]:
            _assert_instance_is(g, refined[i][0][g["rank"]], g["rank"], (f, g["rank"]))
            assert g["n_refined"] == min(4, g["n_members"]), f
        assert [g["n_members"] for g in got[i]] == TABLE[f]["sizes"], f
    got, dropped = cdet.recognize_batch_instances(scene["bgrs"], scene["depths"], scene["K"], 2, MIN_DIST, 1, *PARAMS[0], with_dropped=True)
    assert dropped[0] == 15 and [len(g) for g in got] == [2, 2, 2, 0]
    for g in got[0]:
        _assert_instance_is(g, refined[0][0][g["rank"]], g["rank"], ("cap", g["rank"]))


def test_one_instance_one_hypothesis_is_recognize_batch(cdet, scene):
    for p in PARAMS:
        base = cdet.recognize_batch(scene["bgrs"], scene["depths"], scene["K"], *p)
        got, dropped = cdet.recognize_batch_instances(scene["bgrs"], scene["depths"], scene["K"], 1, MIN_DIST, 1, *p, with_dropped=True)
        assert [len(g) for g in got] == [1, 1, 1, 0] and dropped[0] == 28 and dropped[3] == 0
        for i, f in enumerate(clutter.FRAMES[:3]):
            g, e = got[i][0], base[i]
            tag = (p, f)
            assert g["rank"] == 0 and g["n_refined"] == 1 and g["n_members"] == TABLE[f]["sizes"][0], tag
            assert (g["status"], g["found"], g["n_matches"]) == (e["status"], e["found"], e["n_matches"]) and e["found"] == 1, tag
            assert g["best"] == e["best"] and g["det"]["n_points"] == e["det"]["n_points"] and g["det"]["icp"]["iters"] == e["det"]["icp"]["iters"], tag
            for k in ("R", "T", "dist_mean", "px_ratio"):
                assert np.array_equal(_bits(g["det"]["icp"][k]), _bits(e["det"]["icp"][k])), (tag, k)
            assert np.array_equal(_bits(g["det"]["R_final"]), _bits(e["det"]["R_final"])) and np.array_equal(_bits(g["det"]["T_final"]), _bits(e["det"]["T_final"])), tag
            assert np.array_equal(_bits(g["pose"]), _bits(e["pose"])), tag


def test_overflowing_frames_are_grown_not_grouped(ctx, scene, refined):
    """64 candidates per frame to start with: every cluttered frame overflows, and none may be grouped from its truncated list."""
    det = _detector(ctx, scene, max_candidates=64)
    got = det.recognize_batch_instances(scene["bgrs"], scene["depths"], scene["K"], 8, MIN_DIST, 64, *PARAMS[0])
    _assert_every_member_refined(got, refined, "grown")
    assert det.frame_counters(0)[2] == 0
    det.close()


def test_device_frames_equal_host_frames(cdet, scene, refined):
    d_b = torch.from_numpy(np.stack(scene["bgrs"])).cuda()
    d_d = torch.from_numpy(np.stack(scene["depths"]).view(np.int16)).cuda()
    torch.cuda.synchronize()
    n = len(clutter.FRAMES)
    bp = [d_b.data_ptr() + i * clutter.W * clutter.H * 3 for i in range(n)]
    dp = [d_d.data_ptr() + i * clutter.W * clutter.H * 2 for i in range(n)]
    got = cdet.recognize_batch_instances(bp, dp, scene["K"], 8, MIN_DIST, 64, *PARAMS[0], mem=L.FL_MEM_DEVICE)
    _assert_every_member_refined(got, refined, "device")
    t = cdet.stage_times()
    assert t["icp_launches"] == 1 and 0.0 < t["group_ms"] < t["icp_ms"] <= t["total_ms"]


def test_facade_returns_every_instance(tmp_path, scene, refined):
    """CadRecoSetMultiInstance(8, 48, 4) through the C++ facade: three results on frame a, in group order."""
    bank = scene["bank"]
    d = tmp_path / "obj"
    write_bank_dir(d, bank, clutter.T, bank.model_depths)
    lib = cadreco_py.lib()
    h = C.c_void_p(lib.cadreco_create(1))
    assert h.value and lib.cadreco_add_obj(h, str(d).encode()) == 0
    bad = C.c_int(0x80000001).value
    for args in ((0, 48, 4), (65, 48, 4), (8, 0, 4), (8, 48, 0), (8, 48, 65)):
        assert lib.cadreco_set_multi_instance(h, *args) == bad, args
    bgr, depth = np.ascontiguousarray(scene["bgrs"][0]), np.ascontiguousarray(scene["depths"][0])
    poses = np.zeros((8, 16), np.float32)

    def reco():
        rc, n, poses[:] = cadreco_py.recognition_all(h, bgr, depth, scene["K"])
        assert rc == 0
        return n
    ref = refined[0][0]
    assert reco() == 1 and np.abs(poses[0].reshape(4, 4) - ref[0]["pose"]).max() <= 1e-4          # the default: matches[0]
    assert lib.cadreco_set_multi_instance(h, 8, MIN_DIST, 4) == 0
    assert reco() == 3
    for i, r in enumerate(TABLE["a"]["pick4"]):
        assert np.abs(poses[i].reshape(4, 4) - ref[r]["pose"]).max() <= 1e-4, r
    assert lib.cadreco_set_multi_hypothesis(h, 2, 20.0) == 0                                      # clears the multi-instance mode
    assert reco() <= 2
    assert lib.cadreco_set_multi_instance(h, 8, MIN_DIST, 4) == 0 and reco() == 3                 # and the other way round
    assert lib.cadreco_set_multi_instance(h, 1, MIN_DIST, 1) == 0                                 # the default again
    assert reco() == 1 and np.abs(poses[0].reshape(4, 4) - ref[0]["pose"]).max() <= 1e-4
    lib.cadreco_destroy(h)
