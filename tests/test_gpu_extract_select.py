"""GPU: the sort (k_pad_keys, k_bitonic_local, k_bitonic_step) and the scattered selection (k_select_scattered) of template
extraction on candidate lists of chosen length, order and ties, through fl_dev_extract_select, which runs the launch sequence
fl_extract_template_batch runs.  Every feature (x, y, label) equals the oracle's orc_select_scattered_list on the list in
raster order, the sorted keys equal the lexsort (score descending, raster ascending), and what the kernels must not write
comes back untouched.  tests/test_extract_model_cpu.py holds the oracle entry to the plain model and to the image-driven
oracle on the same lists."""
import numpy as np
import pytest

import extract_model as M
from fealess_amd import _lib as L

pytestmark = pytest.mark.gpu
FILL = -7
_expected = {}


def _exp(job):
    if job["name"] not in _expected:
        _expected[job["name"]] = M.job_expected(job)
    return _expected[job["name"]]


def _check_one(job, got):
    n_out, feats, keys = got
    exp, exp_keys = _exp(job)
    nf, n = job["num_features"], len(job["raster"])
    print(job["name"], "candidates", n, "start distance", float(M.job_distance(job)), "n_out", n_out)
    if n < nf:
        assert exp is None
        assert n_out == -1 and (feats == FILL).all() and (keys == np.int64(FILL).astype(np.uint64)).all(), job["name"]
        return
    assert np.array_equal(keys, exp_keys), (job["name"], "sort")
    assert n_out == nf, job["name"]
    assert np.array_equal(feats[:nf], exp), (job["name"], "selection")
    assert (feats[nf:] == FILL).all(), job["name"]
    if n <= 700:                                             # and the plain model, where it is fast
        x, y, label = M.job_xyl(job)
        o = np.argsort(job["raster"], kind="stable")
        assert np.array_equal(feats[:nf], M.select_model(x[o], y[o], label[o], job["score"][o], nf, M.job_distance(job))[0]), job["name"]


def _check(ctx, jobs):
    got = ctx.dev_extract_select(jobs, fill=FILL)
    assert len(got) == len(jobs)
    for j, g in zip(jobs, got):
        _check_one(j, g)
    return got


@pytest.mark.parametrize("nf", [63, 31, 15, 7])
def test_counts_around_the_rule(ctx, nf):
    jobs = M.rule_jobs(nf)
    assert [len(j["raster"]) for j in jobs] == [nf - 1, nf, nf + 1, 2 * nf - 1, 2 * nf]
    for j in jobs:
        _check(ctx, [j])
    _check(ctx, jobs)


@pytest.mark.parametrize("dist", ["distinct", "three", "equal"])
@pytest.mark.parametrize("n", M.SORT_COUNTS)
def test_counts_around_the_sort(ctx, n, dist):
    for order in ("raster", "reversed", "shuffled"):
        j = M.sort_job(n, dist, order)
        assert len(j["raster"]) == n and len(np.unique(j["score"])) == {"distinct": n, "three": 3, "equal": 1}[dist]
        _check(ctx, [j])


def _same_results(a, b):
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_mixed_jobs_in_one_call_equal_each_job_alone(ctx):
    jobs = M.mixed_jobs()
    assert [len(j["raster"]) for j in jobs] == [0, 62, 63, 64, 2048, 2049, 8193, 20000]
    alone = [_check(ctx, [j])[0] for j in jobs]
    for order in (list(range(8)), [7, 0, 4, 2, 6, 1, 5, 3]):       # the longest job last, then first among shorter ones
        got = _check(ctx, [jobs[k] for k in order])
        for k, g in zip(order, got):
            _same_results(g, alone[k])


@pytest.mark.parametrize("counts", [(0, 62, 63, 64, 100, 1000, 2047), (700, 63, 0, 64, 62, 513)])
def test_mixed_jobs_below_one_sort_chunk(ctx, counts):
    jobs = M.mixed_jobs(counts)
    assert max(len(j["raster"]) for j in jobs) < 2048
    alone = [_check(ctx, [j])[0] for j in jobs]
    for g, a in zip(_check(ctx, jobs), alone):
        _same_results(g, a)


def test_deep_relaxation(ctx):
    jobs = M.deep_jobs()
    relax = []
    for j in jobs:
        x, y, label = M.job_xyl(j)
        o = np.argsort(j["raster"], kind="stable")
        relax.append(M.select_walk(x[o], y[o], label[o], j["score"][o], 63, M.job_distance(j))[1]["relaxations"])
    print("relaxations", relax)
    assert relax[0] >= 93 and relax[1] >= 90 and relax[2] >= 1
    # n = nf: every candidate is chosen, the last sorted one among them, and the walk wraps after it
    exp, _ = _exp(jobs[2])
    x, y, _ = M.job_xyl(jobs[2])
    assert sorted(map(tuple, exp[:, :2])) == sorted(zip(x.tolist(), y.tolist()))
    for j in jobs:
        _check(ctx, [j])


def test_depth_rule(ctx):
    jobs = M.depth_jobs()
    assert [j["area"] for j in jobs if j["depth_mode"] == 2 and j["num_features"] == 63][:8] == [251, 252, 253, 1574, 1575, 1576, 279, 280]
    assert jobs[0]["depth_mode"] == 1 and jobs[0]["area"] == 0
    for j in jobs:
        assert len(j["raster"]) < 200 or len(np.unique(j["score"])) < len(j["score"]) // 4          # ties everywhere
    by = {j["name"]: j for j in jobs}
    # the float-versus-int compare: 279 and 280 start either side of the squared distance 13 and select differently
    d279, d280 = (M.job_distance(by[f"depth-mode2-area{a}"]) for a in (279, 280))
    assert d279 * d279 < 13 < d280 * d280
    for j in jobs:
        _check(ctx, [j])
    _check(ctx, jobs)


def test_coordinates(ctx):
    wide, wide_d, w17 = M.coordinate_jobs()
    assert (wide["w"], wide["h"]) == (4096, 64) and {0, 4095, 63 * 4096, 64 * 4096 - 1} <= set(wide["raster"].tolist())
    exp, _ = _exp(wide)
    assert {(0, 0), (4095, 0), (0, 63), (4095, 63)} <= set(map(tuple, exp[:, :2]))     # dx^2 = 4095^2 is computed
    for j in (wide, wide_d, w17):
        _check(ctx, [j])
    _check(ctx, [w17, wide_d, wide])


def test_refusals(ctx):
    fn = L.dev(ctx.lib, "fl_dev_extract_select")
    good = M.rule_jobs(15)[2]
    keep = []

    def record(j, **nulls):
        raster, score, labels = (np.ascontiguousarray(j[k]) for k in ("raster", "score", "labels"))
        n_out, feats, keys = np.full(1, FILL, np.int32), np.full((64, 3), FILL, np.int32), np.full(max(len(raster), 1), 77, np.uint64)
        keep.append((raster, score, labels, n_out, feats, keys))
        p = dict(raster=raster.ctypes.data, score=score.ctypes.data, labels=labels.ctypes.data, n_out=n_out.ctypes.data,
                 features=feats.ctypes.data, sorted_keys=keys.ctypes.data)
        p.update(nulls)
        return L.DevSelectJob(j["w"], j.get("total_px", j["w"] * j["h"]), j["num_features"], j["depth_mode"], j["area"],
                              j.get("n_cand", len(raster)), p["raster"], p["score"], p["labels"], p["n_out"], p["features"], p["sorted_keys"])

    def call(second, n_jobs=2, h=ctx.h):
        arr = (L.DevSelectJob * 2)(record(good), second)       # a good job first: nothing of it may run either
        return fn(h, n_jobs, arr)

    def bad(**kw):
        j = dict(good)
        j.update(kw)
        return j
    r = good["raster"].copy()
    cases = [record(good, **{k: None}) for k in ("raster", "score", "labels", "n_out", "features", "sorted_keys")]
    cases += [record(bad(num_features=0)), record(bad(num_features=64)), record(bad(num_features=-1)), record(bad(n_cand=-1)),
              record(bad(depth_mode=3)), record(bad(depth_mode=-1)), record(bad(area=-1)), record(bad(w=0)), record(bad(total_px=41))]
    for pos, v in ((0, -1), (5, 40 * 30), (len(r) - 1, 1 << 30)):
        rr = r.copy()
        rr[pos] = v
        cases.append(record(bad(raster=rr)))
    s = good["score"].copy()
    s[3] = 0.0
    cases.append(record(bad(score=s)))
    rr = r.copy()
    rr[4] = rr[9]
    cases.append(record(bad(raster=rr, depth_mode=2, area=100)))        # a repeated pixel in a depth job
    for c in cases:
        assert call(c) == L.FL_ERR_INVALID
    assert call(record(good), n_jobs=0) == L.FL_ERR_INVALID
    assert call(record(good), n_jobs=-2) == L.FL_ERR_INVALID
    assert call(record(good), h=None) == L.FL_ERR_INVALID
    assert fn(ctx.h, 1, None) == L.FL_ERR_INVALID
    for raster, score, labels, n_out, feats, keys in keep:                # nothing written
        assert n_out[0] == FILL and (feats == FILL).all() and (keys == 77).all()
    _check(ctx, [good])                                                    # and the context still works
