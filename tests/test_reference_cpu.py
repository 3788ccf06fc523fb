"""The oracle against the reference's own compiled code (oracle/ref: the reference's linemod.cpp built against a
container-only opencv2/ stand-in), bit for bit, stage by stage, in its scalar and in its SSE2/SSE3/SSSE3 build, and against
the outputs recorded from it (tests/golden/reference_linemod.npz), which run on any checkout.  Cases: tests/reference_cases.py.

No case is dropped at run time: what a build cannot take (the SSE2 spread needs w % 16 == 0) is decided by the case alone when
the tests are collected, and inputs that would make the reference's behaviour undefined are built so that they cannot.  Quirk
Q2 (reads past the last grid row of a linear memory) is DEFINED BY THE STAND-IN'S ALLOCATOR, UB IN THE REFERENCE: its cases
(names starting with q2_) are a group of their own in every list below.

The ICP half the same way: the oracle in the reference's float32 arithmetic (accum64 = False), on its kd-tree and on its
brute-force search, against the reference's compiled ICP.cpp, common.cpp, depth_to_3d.cpp, detection.cpp and NMS.cpp
(oracle/_ref/libfealess_ref_icp.so) and against tests/golden/reference_icp.npz.  Every comparison is equality of bit patterns
or of ints: R, T, dist_mean and px_ratio of every prefix icp_it_thr = 0 .. N (the prefixes are the per-iteration states), `iter`
on exit, n_points, the helpers' clouds and pair lists, the back-projected clouds, the NMS winners.  Exact nearest-neighbour ties
(names starting with tie_) are DEFINED BY THE STAND-IN'S RULE (lowest index), UNSPECIFIED IN FLANN, and a group of their own.

Template extraction the same way (RC.extract_groups; tests/golden/reference_extract.npz): the sort and scattered selection on
lists, the two extractTemplate methods on given images, quantizedOrientations with its magnitude, Detector::addTemplate.  Both
builds compile the same text there (it has no SSE branch), and both are compared.  Pinned: the reference's comparisons, start
distances, relaxation loop, stable sort, score division, channel choice and cropping.  NOT pinned: GaussianBlur, Sobel, phase,
pyrDown, resize, erode and distanceTransform, which the stand-in delegates to the oracle (oracle/ref/ref_harness.cpp).
"""
import numpy as np
import pytest

import reference_cases as RC
import reference_py as R
from util import golden

GROUPS = RC.groups()
LIVE = [pytest.param(simd, g, name, id=f"{'simd' if simd else 'scalar'}-{name}") for simd in (False, True)
        for g, (cases, _) in GROUPS.items() for name, c in cases if not simd or RC.simd_takes(g, c)]
ALL = [pytest.param(g, name, id=name) for g, (cases, _) in GROUPS.items() for name, _ in cases]
EXTRACT_GROUPS = RC.extract_groups()
EXTRACT_ALL = [pytest.param(g, name, id=name) for g, (cases, _) in EXTRACT_GROUPS.items() for name, _ in cases]
EXTRACT_LIVE = [pytest.param(simd, g, name, id=f"{'simd' if simd else 'scalar'}-{name}") for simd in (False, True)
                for g, (cases, _) in EXTRACT_GROUPS.items() for name, _ in cases]
ICP_GROUPS = RC.icp_groups()
ICP_ALL = [pytest.param(kd, g, name, id=f"{'kdtree' if kd else 'brute'}-{name}") for kd in (True, False)
           for g, (cases, _) in ICP_GROUPS.items() for name, _ in cases]


def _case(g, name):
    cases, fn = GROUPS[g]
    return dict(cases)[name], fn


@pytest.mark.parametrize("simd,group,name", LIVE)
def test_oracle_equals_compiled_reference(oracle, simd, group, name):
    case, fn = _case(group, name)
    ref = RC.ReferenceBackend(R.require(simd))
    a, b = fn(RC.OracleBackend(oracle), case), fn(ref, case)
    assert RC.same(a, b) is None, (name, RC.same(a, b))


@pytest.mark.parametrize("group,name", ALL)
def test_oracle_equals_recorded_reference(oracle, group, name):
    case, fn = _case(group, name)
    rec = golden("reference_linemod.npz")
    out = fn(RC.OracleBackend(oracle), case)
    keys = sorted(k.split("/", 2)[2] for k in rec.files if k.startswith(f"{group}/{name}/") and not k.endswith("/full"))
    assert keys == sorted(out), (keys, sorted(out))
    for k, v in out.items():
        assert np.array_equal(RC.digest(v), rec[f"{group}/{name}/{k}"]) if k != "__in__" else np.array_equal(v, rec[f"{group}/{name}/{k}"]), (name, k)
        if f"{group}/{name}/{k}/full" in rec.files:
            assert RC.matches_equal(v, rec[f"{group}/{name}/{k}/full"]), (name, k)


def _icp_case(g, name):
    cases, fn = ICP_GROUPS[g]
    return dict(cases)[name], fn


@pytest.mark.parametrize("use_kdtree,group,name", ICP_ALL)
def test_icp_oracle_equals_compiled_reference(oracle, use_kdtree, group, name):
    case, fn = _icp_case(group, name)
    ref = RC.ReferenceIcpBackend(R.require_icp())
    a, b = fn(RC.OracleIcpBackend(oracle, use_kdtree), case), fn(ref, case)
    assert RC.same(a, b) is None, (name, RC.same(a, b))


@pytest.mark.parametrize("use_kdtree,group,name", ICP_ALL)
def test_icp_oracle_equals_recorded_reference(oracle, use_kdtree, group, name):
    case, fn = _icp_case(group, name)
    out = fn(RC.OracleIcpBackend(oracle, use_kdtree), case)
    assert RC.same_as_record(out, golden("reference_icp.npz"), group, name) is None, (name, RC.same_as_record(out, golden("reference_icp.npz"), group, name))


def test_icp_record_holds_exactly_the_case_list():
    rec = golden("reference_icp.npz")
    assert sorted(rec.files) == sorted(f"{g}/{name}" for g, (cases, _) in ICP_GROUPS.items() for name, _ in cases)


def _extract_case(g, name):
    cases, fn = EXTRACT_GROUPS[g]
    return dict(cases)[name], fn


@pytest.mark.parametrize("simd,group,name", EXTRACT_LIVE)
def test_extract_oracle_equals_compiled_reference(oracle, simd, group, name):
    case, fn = _extract_case(group, name)
    a, b = fn(RC.OracleExtractBackend(oracle), case), fn(R.require(simd), case)
    assert RC.same(a, b) is None, (name, RC.same(a, b))


@pytest.mark.parametrize("group,name", EXTRACT_ALL)
def test_extract_oracle_equals_recorded_reference(oracle, group, name):
    case, fn = _extract_case(group, name)
    diff = RC.same_as_record(fn(RC.OracleExtractBackend(oracle), case), golden("reference_extract.npz"), group, name, RC.is_image)
    assert diff is None, (name, diff)


def test_extract_record_holds_exactly_the_case_list():
    rec = golden("reference_extract.npz")
    assert sorted(rec.files) == sorted(f"{g}/{name}" for g, (cases, _) in EXTRACT_GROUPS.items() for name, _ in cases)
    # a refusal is part of the record: two members, the input digest and the one byte of `refused`
    refused = [k for k in rec.files if RC.record_lengths(rec[k]) == [32, 1]]
    assert len(refused) >= 12 and all("refused" in k or "_of_" in k or k.startswith("select/rule-") for k in refused), refused
    full = [k for k in rec.files if k.startswith(("select/", "extract_")) and k not in refused]
    assert all(RC.record_lengths(rec[k])[1] % 12 == 0 and RC.record_lengths(rec[k])[1] >= 7 * 12 for k in full)   # feature lists in full


@pytest.mark.parametrize("group", ["spread", "lut", "linearize", "similarity", "local", "total", "match"])
def test_scalar_and_simd_builds_agree(group):
    """The functions with SSE branches, on every case both builds take."""
    cases, fn = GROUPS[group]
    s, v = RC.ReferenceBackend(R.require(False)), RC.ReferenceBackend(R.require(True))
    n = 0
    for name, c in cases:
        if RC.simd_takes(group, c):
            assert RC.same(fn(s, c), fn(v, c)) is None, name
            n += 1
    assert n > 0


def test_inputs_keep_the_reference_defined(oracle):
    """The properties of the INPUTS that keep the reference's behaviour defined (and Q2 and tie_ cases in their own groups)."""
    for c in RC.similarity_cases():
        RC.check_similarity_case(c)
    for c in RC.local_cases():
        RC.check_local_case(c)
    assert sum(c[0].startswith("q2_") for c in RC.similarity_cases() + RC.local_cases()) >= 4
    for c in RC.normals_cases():
        assert not RC.normals_unsafe(RC.normals_input(c), c[4], c[5]).any(), c[0]
    for c in RC.hysteresis_cases():
        assert RC.angles_unambiguous(RC.hysteresis_input(c)[1]), c[0]
    assert RC.angles_unambiguous(RC.edge_angles()) and not RC.angles_unambiguous(RC.AMBIGUOUS_ANGLES)
    for c in RC.crop_cases():
        RC.check_crop_case(c)
    for g in ("spread", "linearize"):
        assert any(not RC.simd_takes(g, c) for _, c in GROUPS[g][0]) and any(RC.simd_takes(g, c) for _, c in GROUPS[g][0])
    # the ICP half: n_model <= n_ref, no exact nearest-neighbour tie at any search the loop performs outside the tie_ group,
    # crops of one size inside the frame (or the recorded refusal), NMS distances exact in any order of evaluation
    for c in RC.icp_cases():
        RC.check_icp_case(oracle, c)
    assert sum(c[0].startswith("tie_") for c in RC.icp_cases()) >= 2
    for c in RC.detection_cases():
        RC.check_detection_case(oracle, c)
    for c in RC.nms_cases():
        RC.check_nms_case(c)
    for c in RC.depth3d_cases():
        d = RC.depth3d_input(c)
        assert d.shape == (c[2], c[1]) and {0, 1, 65535} <= set(d.ravel().tolist()), c[0]
    # template extraction: every case is on the edge it is named for, and none leaves the reference undefined (one check per
    # case, from tests/extract_model.py and the oracle's stage functions: reference_cases.check_extract_cases)
    RC.check_extract_cases()


@pytest.mark.parametrize("simd", [False, True], ids=["scalar", "simd"])
@pytest.mark.parametrize("name", list(RC.match_cases()))
def test_reference_final_list(oracle, simd, name):
    """Detector::match's own list: std::sort is unstable and std::unique drops adjacent repeats only, so it is one of several
    valid outcomes.  Checked: the same set of (x, y, similarity bits, class) keys as the oracle's list, the same first
    similarity and template id, non-increasing in (similarity, -template_id); and the intended lists are not empty."""
    case = RC.match_cases()[name]
    ref, orc = RC.ReferenceBackend(R.require(simd)), RC.OracleBackend(oracle)
    total = 0
    for thr in case["thresholds"]:
        fin, raw = ref.match_lists(case, thr)
        exp = orc.match(case, thr)
        assert RC.matches_equal(RC.canonical(raw), exp), thr
        key = lambda m: set(zip(m["x"].tolist(), m["y"].tolist(), m["similarity"].view(np.uint32).tolist(), m["class_idx"].tolist()))
        assert key(fin) == key(exp), thr
        if len(exp):
            assert fin[0]["similarity"] == exp[0]["similarity"] and fin[0]["template_id"] == exp[0]["template_id"]
            s, t = fin["similarity"], fin["template_id"]
            assert np.all((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (t[:-1] <= t[1:])))
        total = max(total, len(exp))
    assert total >= case["min_matches"], (total, case["min_matches"])
