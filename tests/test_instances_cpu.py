"""Multi-instance grouping without a GPU: fl_group_matches(FL_MEM_HOST) against the numpy model (tests/instances_model.py)
on hand-made and random lists, the model's two statements of the rule against each other, the argument checks, and -- with
the oracle alone -- the model's grouping and pick on the refined match lists of the cluttered frames (tests/clutter.py),
which must give the groups and picks the GPU tests expect of fl_recognize_batch_instances."""
import ctypes as C

import numpy as np
import pytest

import clutter
import instances_model as M
from fealess_amd import api
from fealess_amd import _lib as L
from fealess_amd.bank import MATCH_DTYPE

# frames a - d with min_dist_px = 48: group sizes, and the picks (indices in the match list) with 64 and with 4 hypotheses
# per instance
MIN_DIST = 48
TABLE = {"a": dict(n=41, sizes=[13, 13, 15], pick64=[3, 1, 16], pick4=[3, 1, 10]),
         "b": dict(n=22, sizes=[14, 8], pick64=[0, 13], pick4=[0, 13]),
         "c": dict(n=28, sizes=[13, 15], pick64=[2, 11], pick4=[2, 7]),
         "d": dict(n=0, sizes=[], pick64=[], pick4=[])}


@pytest.fixture(scope="module")
def banks():
    return M.small_banks()


@pytest.fixture(scope="module")
def det(banks):
    d = api._host_only_detector(2, [5, 8])     # no GPU, never finalized
    for b in banks:
        d.add_class(b)
    yield d
    d.close()


def _matches(rows):
    m = np.zeros(len(rows), MATCH_DTYPE)
    for i, (x, y, c, t) in enumerate(rows):
        m[i] = (x, y, 90.0 - i, c, t)
    return m


def _check(det, banks, m, G, dist):
    gof, size, ng = det.group_matches(m, G, dist)
    e_gof, e_size, e_ng = M.group(m, M.widths_heights(banks), G, dist)
    assert ng == e_ng and np.array_equal(gof, e_gof) and np.array_equal(size, e_size), (len(m), G, dist)
    return gof, size, ng


def test_hand_made_lists(det, banks):
    # two classes at the same place stay apart (template 0 of each; the boxes differ, the rule only looks at the class)
    gof, size, ng = _check(det, banks, _matches([(100, 100, 0, 0), (100, 100, 1, 0), (101, 100, 0, 0), (101, 101, 1, 0)]), 8, 50)
    assert list(gof) == [0, 1, 0, 1] and ng == 2 and list(size[:2]) == [2, 2]
    # within the radius of two leaders: the older one; distances go to the LEADER (match 3 is near member 2, not near leader 0
    # or 1, and founds its own group)
    rows = [(100, 100, 0, 1), (160, 100, 0, 1), (130, 100, 0, 1), (130, 139, 0, 1)]
    gof, _, ng = _check(det, banks, _matches(rows), 8, 40)
    assert list(gof) == [0, 1, 0, 2] and ng == 3
    # exactly at the radius is outside: (3, 4) pixels apart with min_dist 5; (3, 3) is inside
    gof, _, _ = _check(det, banks, _matches([(50, 50, 0, 2), (53, 54, 0, 2), (53, 53, 0, 2), (55, 50, 0, 2), (54, 50, 0, 2)]), 8, 5)
    assert list(gof) == [0, 1, 0, 1, 0]
    # the cap: with two groups allowed the third place is dropped, and counted
    rows = [(0, 0, 0, 0), (300, 0, 0, 0), (0, 300, 0, 0), (1, 1, 0, 0), (301, 1, 0, 0), (2, 301, 0, 0)]
    gof, size, ng = _check(det, banks, _matches(rows), 2, 20)
    assert list(gof) == [0, 1, -1, 0, 1, -1] and ng == 2 and int((gof == -1).sum()) == 2 and list(size) == [2, 2]
    gof, size, ng = _check(det, banks, _matches(rows), 1, 20)
    assert list(gof) == [0, -1, -1, 0, -1, -1] and ng == 1 and list(size) == [2]
    # coordinates at the ends of int32 and the largest radius: 64-bit arithmetic throughout
    big = 2 ** 31 - 1
    rows = [(-big - 1, -big - 1, 0, 0), (big, big, 0, 0), (-big, -big - 1, 0, 0), (big - 1, big, 0, 0), (0, 0, 0, 0)]
    for dist in (1, 2, 2 ** 30):
        _check(det, banks, _matches(rows), 8, dist)
    assert list(_check(det, banks, _matches(rows), 8, 2)[0]) == [0, 1, 0, 1, 2]
    assert list(_check(det, banks, _matches(rows), 8, 2 ** 30)[0]) == [0, 1, 0, 1, 2]


@pytest.mark.parametrize("n", [0, 1, 2, 65, 5000])
def test_random_lists(det, banks, n):
    wh = M.widths_heights(banks)
    for seed in range(3):
        rng = np.random.default_rng(100 * n + seed)
        for clusters in (0, 5):
            m = M.random_list(rng, n, banks, clusters=clusters)
            for G, dist in ((1, 40), (3, 25), (8, 48), (64, 10), (64, 300)):
                _check(det, banks, m, G, dist)
                a, b = M.group(m, wh, G, dist), M.group_rounds(m, wh, G, dist)      # the rule's two statements agree
                assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (n, seed, clusters, G, dist)


def test_argument_checks(det, banks):
    lib = L.load()
    m = M.random_list(np.random.default_rng(1), 4, banks)
    gof, size, ng = np.zeros(4, np.int32), np.zeros(64, np.int32), C.c_int32(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(mm=m, n=4, mem=L.FL_MEM_HOST, ip=(8, 48, 4), d=det.h, g=p(gof), s=p(size), k=C.byref(ng)):
        ipp = C.byref(L.InstanceParams(*ip)) if ip is not None else None
        return lib.fl_group_matches(d, p(mm) if mm is not None else None, n, mem, ipp, g, s, k)
    assert call() == L.FL_OK
    assert call(d=None) == L.FL_ERR_INVALID and call(mm=None) == L.FL_ERR_INVALID and call(n=-1) == L.FL_ERR_INVALID
    assert call(g=None) == L.FL_ERR_INVALID and call(s=None) == L.FL_ERR_INVALID and call(k=None) == L.FL_ERR_INVALID
    assert call(ip=None) == L.FL_ERR_INVALID and call(mem=2) == L.FL_ERR_INVALID
    for ip in ((0, 48, 4), (65, 48, 4), (8, 0, 4), (8, -3, 4), (8, 2 ** 30 + 1, 4), (8, 48, 0), (8, 48, 65)):
        assert call(ip=ip) == L.FL_ERR_INVALID, ip
    assert call(ip=(64, 2 ** 30, 64)) == L.FL_OK and call(ip=(1, 1, 1)) == L.FL_OK
    assert call(mm=None, n=0, g=None) == L.FL_OK and ng.value == 0          # an empty list needs no arrays
    for field, v in (("class_idx", 2), ("class_idx", -1), ("template_id", banks[0].n_pyramids + banks[1].n_pyramids), ("template_id", -1)):
        bad = m.copy()
        bad[field][2] = v
        gof[:] = -7
        assert call(mm=bad) == L.FL_ERR_INVALID and (gof == -7).all(), field     # not on the detector: nothing written
    assert call(mem=L.FL_MEM_DEVICE) == L.FL_ERR_STATE                        # the device path needs a finalized detector
    with pytest.raises(api.FealessError):
        det.finalize(640, 480)                                                # and a host-only detector cannot become one


def test_clutter_groups_and_picks_with_the_oracle(oracle):
    """The model on the oracle's refined lists of frames a - d: the groups and picks of the table, the picks with every member
    refined equal to the oracle's NMS winners, and the counts of dropped matches with fewer groups allowed."""
    sc = clutter.build(oracle)
    wh = M.widths_heights([sc["bank"]])
    for name in clutter.FRAMES:
        bgr, depth = sc["frames"][name]
        t = TABLE[name]
        m, n = oracle.match_images(bgr, depth, clutter.T, [sc["bank"]], 75.0)
        assert n == t["n"], name
        if n == 0:
            assert M.instances(m, wh, [], 8, MIN_DIST, 64) == ([], 0)
            continue
        ref, win = oracle.recognition_topk(bgr, depth, sc["K"], clutter.T, sc["bank"], 64, 75.0, 10, 0.5, 0.01, nms_dist=60.0)
        assert len(ref) == n
        for dist in (24, MIN_DIST, 96):
            inst, dropped = M.instances(m, wh, ref, 8, dist, 64)
            assert [i["n_members"] for i in inst] == t["sizes"] and dropped == 0, (name, dist)
            assert [i["rank"] for i in inst] == t["pick64"] == win, (name, dist)
        inst, _ = M.instances(m, wh, ref, 8, MIN_DIST, 4)
        assert [i["rank"] for i in inst] == t["pick4"] and [i["n_refined"] for i in inst] == [4] * len(inst), name
        gof = M.group(m, wh, 8, MIN_DIST)[0]
        for r in t["pick64"]:                    # the winner is among the first five members of its group
            assert r in np.nonzero(gof == gof[r])[0][:5], name
        if name == "a":
            assert M.instances(m, wh, ref, 2, MIN_DIST, 1)[1] == 15 and M.instances(m, wh, ref, 1, MIN_DIST, 1)[1] == 28
