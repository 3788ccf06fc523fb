"""The cases of tests/test_gpu_extract_candidates.py can fail: the numpy model of extraction's candidate stage
(tests/extract_candidate_cases.expected) equals the oracle's stage functions and scipy on every case, each case sits on the
path it is named for, and every mutant of the model -- one operator changed -- changes the expected output of the cases
CAUGHT_BY names for it.  No GPU."""
import numpy as np
import pytest

import extract_candidate_cases as XC

CASES = XC.by_name()


@pytest.mark.parametrize("name", list(CASES))
def test_model_equals_the_oracle_and_scipy(oracle, name):
    case = CASES[name]
    exp, orc = XC.expected(case), XC.oracle_products(case)
    for k in ("local", "cand", "score", "area", "features"):
        a, b = exp[k], orc[k]
        assert (a is None) == (b is None) and (a is None or np.array_equal(np.asarray(a), np.asarray(b))), (name, k)
    assert exp["n_cand"] == int(orc["cand"].sum()) and (exp["features"] is None) == (exp["n_cand"] < case["nf"]), name
    if case["modality"] == 1:
        inside = np.ones(case["q"].shape, bool) if exp["local"] is None else exp["local"] != 0
        assert np.array_equal(np.where(exp["cand"], XC.scipy_distances(case["q"], inside), 0), exp["score"]), name
        lab = np.log2(case["q"][exp["cand"]].astype(np.float64)).astype(np.int64)
        assert np.array_equal(np.bincount(lab, minlength=8), exp["label_counts"]), name


def test_cases_sit_on_the_paths_they_are_named_for(oracle):
    e = {n: XC.expected(c) for n, c in CASES.items()}
    # shapes: no multiple of the 64 x 4 tile; 55^2 and 55^2 + 1 both on labelled pixels inside the local mask
    for c in XC.shape_cases():
        h, w = c["q"].shape
        assert w % 64 and (h % 4 or w < 64), c["name"]
        if c["modality"] == 0:
            inside = np.ones(c["q"].shape, bool) if c["mask"] is None else e[c["name"]]["local"] != 0
            for m in (3025.0, 3026.0):
                assert (inside & (c["q"] > 0) & (c["mag"] == m)).any(), (c["name"], m)
    taken = [c["name"] for c in XC.shape_cases() if e[c["name"]]["features"] is not None]
    assert {(n.split("_")[0], n.split("_")[-1]) for n in taken} == {(m, k) for m in ("color", "depth") for k in ("mask", "nomask")}, taken
    # one label everywhere: every distance is the cap, one score, the features in raster order
    one = e["depth_one_label_128x96"]
    assert one["n_cand"] == 12288 and (one["score"] == 8192).all() and len(np.unique(one["keys"] >> np.uint64(32))) == 1
    r = one["features"][:, 1] * 128 + one["features"][:, 0]
    assert len(r) == 63 and (np.diff(r) > 0).all()
    far = e["depth_one_label_far_corner_128x96"]
    assert far["n_cand"] == 12284 and far["score"][0, 0] == 127 == max(128 - 1, 96 - 1)
    assert e["depth_blocks_192x128_thr1"]["n_cand"] == 23625 > 16384           # k_depth_keys: 64 blocks of 256 threads per trip
    for n, count in (("color_8192_of_128x64", 8192), ("color_8191_of_128x64", 8191), ("depth_8192_of_128x64", 8192), ("depth_8191_of_128x64", 8191)):
        assert e[n]["n_cand"] == count, n
    full_c, full_d = e["color_full_mask_8x8"], e["depth_full_mask_8x8"]
    assert (full_c["local"] == 0).all() and full_c["n_cand"] == 0 and full_c["features"] is None
    assert (full_d["local"] == 255).all() and full_d["area"] == 64
    for c in XC.rule_cases():
        exact = int(c["name"].split("_")[1])
        assert e[c["name"]]["n_cand"] == exact and (e[c["name"]]["features"] is None) == (exact < c["nf"]), c["name"]
    # several views: differing content, masks on views 0 and 2 only
    for tag, views in XC.multi_view_cases().items():
        assert len(views) == 3 and [v["mask"] is not None for v in views] == ([True, False, True] if "masks_0_2" in tag else [False] * 3)
        for i in range(3):
            assert e[views[i]["name"]]["features"] is not None, views[i]["name"]
            for j in range(i):
                assert not np.array_equal(views[i]["q"], views[j]["q"]) and not np.array_equal(e[views[i]["name"]]["features"], e[views[j]["name"]]["features"])


@pytest.mark.parametrize("mutant", XC.MUTANTS)
def test_every_mutant_is_caught_by_its_named_cases(oracle, mutant):
    assert set(XC.CAUGHT_BY) == set(XC.MUTANTS) and len(XC.CAUGHT_BY[mutant]) >= 1
    for name in XC.CAUGHT_BY[mutant]:
        assert XC.differs(XC.expected(CASES[name]), XC.expected(CASES[name], mutant)) is not None, (mutant, name)
