"""CPU: the plain selection model, the oracle's orc_select_scattered_list and the image-driven oracle entry points agree on
the candidate lists tests/test_gpu_extract_select.py feeds the kernels, and extract_model.candidate_counts predicts
exactly which of the threshold views of tests/test_gpu_extract_edges.py the oracle's add_template refuses."""
import numpy as np
import pytest

import extract_model as M

JOBS = M.all_select_jobs()
MODEL_MAX = 2049            # the candidate-by-candidate loop stays under about a second up to here


def _raster_order(job):
    x, y, label = M.job_xyl(job)
    o = np.argsort(job["raster"], kind="stable")
    return x[o], y[o], label[o], job["score"][o]


def test_generated_jobs_are_the_cases_the_gpu_tests_name():
    names = [j["name"] for j in JOBS]
    assert len(set(names)) == len(names)
    by = {j["name"]: j for j in JOBS}
    for nf in (63, 31, 15, 7):
        assert [len(j["raster"]) for j in M.rule_jobs(nf)] == [nf - 1, nf, nf + 1, 2 * nf - 1, 2 * nf]
    assert [len(by[f"mixed-{n}"]["raster"]) for n in M.MIXED_COUNTS] == list(M.MIXED_COUNTS)
    assert len(np.unique(by["deep-6300-equal"]["score"])) == 1 and len(by["deep-6300-equal"]["raster"]) == 6300
    assert len(np.unique(by["deep-6400-five"]["score"])) == 5 and len(by["deep-6400-five"]["raster"]) == 6400
    for j in JOBS:                                             # depth jobs never repeat a pixel; every score is positive
        assert (j["score"] > 0).all()
        assert j["depth_mode"] == 0 or len(np.unique(j["raster"])) == len(j["raster"])
        assert j["w"] <= 160 and j["h"] <= 120 or j["name"].startswith("wide-4096x64")


@pytest.mark.parametrize("job", [j for j in JOBS if len(j["raster"]) <= MODEL_MAX], ids=lambda j: j["name"])
def test_model_equals_oracle_list(oracle, job):
    x, y, label, score = _raster_order(job)
    d = M.job_distance(job)
    exp, _ = M.job_expected(job)
    got, stats = M.select_model(x, y, label, score, job["num_features"], d)
    walk, wstats = M.select_walk(x, y, label, score, job["num_features"], d)
    if len(x) < job["num_features"]:
        assert exp is None and got is None and walk is None
        return
    assert np.array_equal(got, exp) and np.array_equal(walk, exp)
    assert stats["relaxations"] == wstats["relaxations"]
    if len(x) == job["num_features"] and job["depth_mode"] == 0:
        # every candidate is chosen, so the last sorted one is, and the walk wraps right after taking it
        assert stats["wraps_after_take"] >= 1 and sorted(map(tuple, got[:, :2])) == sorted(zip(x.tolist(), y.tolist()))
    # an arrival order other than the raster order changes the reference's tie-breaks, and the model follows it there too
    xa, ya, la = M.job_xyl(job)
    fa = oracle.select_scattered_list(xa, ya, la, job["score"], job["num_features"], d)
    ma, _ = M.select_model(xa, ya, la, job["score"], job["num_features"], d)
    assert np.array_equal(ma, np.stack([fa["x"], fa["y"], fa["label"]], 1))


@pytest.mark.parametrize("job", [j for j in JOBS if len(j["raster"]) > MODEL_MAX], ids=lambda j: j["name"])
def test_walk_equals_oracle_list_on_the_long_lists(job):
    x, y, label, score = _raster_order(job)
    exp, _ = M.job_expected(job)
    walk, _ = M.select_walk(x, y, label, score, job["num_features"], M.job_distance(job))
    assert np.array_equal(walk, exp)


def test_deep_lists_relax_dozens_of_times():
    by = {j["name"]: j for j in JOBS}
    for name, least in (("deep-6300-equal", 93), ("deep-6400-five", 90), ("mixed-20000", 100)):
        j = by[name]
        x, y, label, score = _raster_order(j)
        assert M.select_walk(x, y, label, score, 63, M.job_distance(j))[1]["relaxations"] >= least, name


def test_sorted_keys_are_the_stable_sort_of_the_raster_order():
    """(score descending, raster ascending) is what std::stable_sort with Candidate::operator< gives a list met in raster order."""
    for j in JOBS[::7]:
        o = np.argsort(j["raster"], kind="stable")
        r, s = j["raster"][o], j["score"][o]
        so = M.sort_order(s)
        assert np.array_equal(M.sorted_keys(j["raster"], j["score"]), M.pack_keys(r[so], s[so])), j["name"]


@pytest.mark.parametrize("job", [j for j in JOBS if j["depth_mode"] == 0 and len(np.unique(j["raster"])) == len(j["raster"])][::3],
                         ids=lambda j: j["name"])
def test_list_equals_image_driven_colour_extraction(oracle, job):
    """The list at its pixels of an otherwise empty image: q > 0 and magnitude = score there (every score is above 55^2)."""
    w, h, nf = job["w"], job["h"], job["num_features"]
    q, mag = np.zeros((h, w), np.uint8), np.zeros((h, w), np.float32)
    x, y, label = M.job_xyl(job)
    q[y, x] = job["labels"][y, x]
    mag[y, x] = job["score"]
    f = oracle.extract_template_color(q, mag, None, 55.0, nf)
    exp, _ = M.job_expected(job)
    assert (f is None) == (exp is None) == (len(x) < nf)
    if f is not None:
        assert np.array_equal(np.stack([f["x"], f["y"], f["label"]], 1), exp)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("level", [0, 1])
def test_list_equals_image_driven_depth_extraction(oracle, level, masked):
    """The depth candidates of a tilted-patch view as a list, with the depth rule's distance from the mask's area (or the
    pixel count), against orc_extract_template_depth on the image."""
    sc = M.edge_scene(0)
    mask = sc.mask_pyramid(M.rect_mask(M.W, M.H, 6, 5, 70, 48) if masked else None)[level]
    normal, nf, thr = sc.normal[level], 63 >> level, 2 >> level
    cand, dist, area = M.depth_candidates(normal, mask, thr)
    ys, xs = np.nonzero(cand)                                  # raster order
    label = np.log2(normal[ys, xs].astype(np.float64)).astype(np.int32)
    score = (dist[ys, xs] / np.bincount(label, minlength=8)[label].astype(np.float32)).astype(np.float32)
    assert len(xs) > 4 * nf and len(np.unique(score)) < len(score) // 4          # ties everywhere
    got = oracle.select_scattered_list(xs, ys, label, score, nf, M.depth_distance(area, nf))
    exp = oracle.extract_template_depth(normal, mask, thr, nf)
    assert exp is not None and np.array_equal(got, exp)


@pytest.mark.parametrize("job,target", M.THRESHOLD_CASES)
def test_candidate_counts_predict_add_template(oracle, job, target):
    case = M.threshold_case(job, target)
    assert case is not None, "the search found no view for this count"
    counts = M.candidate_counts(case["bgr"], case["depth"], case["mask"], M.LEVELS)
    th = M.thresholds(M.LEVELS)
    assert counts == case["counts"] and counts[job] == target
    assert all(counts[k] >= th[k] + M.MARGIN for k in range(4) if k != job)
    exp = oracle.add_template(case["bgr"], case["depth"], case["mask"], M.LEVELS)
    assert (exp is None) == (target < th[job]) == (not M.predicts_template(counts))
