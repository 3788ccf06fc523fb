"""The OpenCV-typed caller (tests/dropin/tu_cv_caller.cpp), the parts that need no GPU.

oracle/_ref/ref_cv_caller is that caller compiled against the reference's own headers and linked to its compiled linemod.cpp,
linemod_if.cpp and ICP sources, all on the stand-in containers of oracle/ref/opencv2.  tests/golden/reference_cv_caller.npz
records what it writes on the cases of tests/cv_caller_cases.py.  Here: the record is what the reference gives today, the cases
are where they are meant to be, the adapter build of the same caller compiles without a warning and links, and its
drawResponse cases (host code only) equal the record.  tests/test_gpu_cv_caller.py runs everything else of the adapter build.
"""
import os

import numpy as np
import pytest

import cv_caller_cases as CC
import reference_cases as RC
import reference_py as R
from util import golden


@pytest.fixture(scope="module")
def cases(tmp_path_factory, oracle):
    d = str(tmp_path_factory.mktemp("cv_cases"))
    groups, inputs = CC.write_case_dir(d, oracle)
    return dict(dir=d, groups=groups, inputs=inputs, names=[n for g in groups.values() for n in g])


@pytest.fixture(scope="module")
def adapter_build(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cv_adapter") / "adapter_cv_caller")
    return exe, CC.compile_adapter_caller(exe)


def test_reference_caller_run_live_equals_the_record(cases, tmp_path):
    exe = R._require(CC.REF_CALLER, lambda: CC.REF_CALLER)
    live = CC.recorded(CC.run_caller(exe, cases["dir"], str(tmp_path / "out")))
    rec = dict(golden("reference_cv_caller.npz"))
    assert sorted(live) == sorted(rec)
    assert CC.same(live, rec, cases["names"]) is None


def test_record_holds_every_case_and_the_long_list(cases):
    rec = golden("reference_cv_caller.npz")
    assert {k.split("/")[0] for k in rec.files} == set(cases["names"])
    assert int(rec[CC.LONG + "/matches/count"][0]) > 65536
    assert len(rec[CC.LONG + "/matches/head"]) == 64 and len(rec[CC.LONG + "/matches/tail"]) == 64


def test_cases_are_where_they_are_meant_to_be(cases, oracle):
    """What the reference did on the cases that are there for one path: its return values and throws, lists that are not
    empty where something is compared, both classes in the two-class lists; and the short lists equal the oracle's, which are
    made from the list BEFORE the unstable sort -- so no outcome of that sort is baked into the record."""
    rec = dict(golden("reference_cv_caller.npz"))
    st = lambda n: CC.status(rec, n)
    n_of = lambda n: int(rec[n + "/matches/count"][0])
    for n in ("two_one_mask_for_two", "two_one_mask_for_two_quantized", "two_one_source", "two_one_source_quantized", "one_two_sources"):
        assert st(n) == ("returned", -1) and n_of(n) == 0, n
    assert rec["two_one_source_quantized/n_quantized"][0] == 4 and rec["two_one_mask_for_two_quantized/n_quantized"][0] == 4
    assert rec["two_one_source/n_quantized"][0] == 0
    assert all(rec[f"two_one_source_quantized/quantized{i}_dims"].tolist() == [0, 0, -1] for i in range(4))
    for n in ("detection_rect_leaves_image_cont", "detection_rect_leaves_image_roi", "depth3d_23x17_K_3x4"):
        assert st(n) == ("threw", "StsAssert"), n
    for n in cases["names"]:
        if st(n)[0] == "threw" or st(n) == ("returned", -1):
            continue
        assert st(n) == ("returned", 0), n
        if n + "/matches/count" in rec and n != "two_filter_nope":
            assert n_of(n) > 0, n
    assert n_of("two_filter_nope") == 0
    plain = rec["two_plain/matches"]
    assert set(plain["class_idx"].tolist()) == {0, 1}                       # zeta (inserted first) and alpha both match
    assert set(rec["two_filter_alpha/matches"]["class_idx"].tolist()) == {1}
    assert RC.matches_equal(rec["two_filter_zeta_zeta/matches"], plain[plain["class_idx"] == 0])
    assert n_of("seq_72") > 0 and RC.matches_equal(rec["seq_160_first/matches"], rec["seq_160_again/matches"])
    # a ROI of the colour image changes nothing, a ROI of the depth image does: quantizedNormals ignores the step (linemod.cpp:600-622)
    assert not RC.matches_equal(rec["two_roi/matches"], plain)
    # the pose table is global: row t is the t-th pose in file order, whatever the class
    T, M, banks = cases["inputs"]["dets"]["two"]
    poses = np.concatenate([b.arrays()[2] for b in banks])
    got = rec["two_templates/poses"].reshape(-1, 14)
    assert np.array_equal(got[:, 0], RC.fbits(np.full(len(poses), 13.0))) and np.array_equal(got[:, 1:], RC.fbits(poses))
    assert bytes(rec["two_templates/class_ids"]).decode() == "alpha\nzeta\n"
    assert rec["two_templates/info"].tolist() == [2, len(poses), 2, 5, 8]
    # the oracle's lists (class_idx = index in the order given = the bank file's order)
    b, d = cases["inputs"]["big"]
    mk = cases["inputs"]["masks"]
    for n, flt, masks in (("two_plain", None, None), ("two_filter_alpha", [1], None), ("two_masks_both", None, ("mask_box.u8", "mask_half.u8")),
                          ("two_mask_first_only", None, ("mask_half.u8", None)), ("two_masks_speckled", None, ("mask_speckle0.u8", "mask_speckle1.u8"))):
        exp, _ = oracle.match_images(b, d, T, banks, 70.0, masks=None if masks is None else [None if m is None else mk[m] for m in masks])
        exp = RC.canonical(exp)
        if flt is not None:
            exp = exp[np.isin(exp["class_idx"], flt)]
        assert RC.matches_equal(rec[n + "/matches"], exp), n


def test_adapter_build_compiles_without_warnings_and_links(adapter_build):
    exe, r = adapter_build
    assert r.returncode == 0, r.stdout
    assert "warning" not in r.stdout, r.stdout
    assert os.path.exists(exe)


def test_adapter_draw_response_equals_the_record(cases, adapter_build, tmp_path):
    """Both drawResponse overloads are host code: dst's bytes and cv::circle's calls (centre, radius, colour, thickness, in
    order), against what the reference's linemod_if.cpp left.  The six-argument overload draws no circle."""
    exe, r = adapter_build
    assert r.returncode == 0, r.stdout
    got = CC.recorded(CC.run_caller(exe, cases["dir"], str(tmp_path / "out"), kind="draw"))
    rec = dict(golden("reference_cv_caller.npz"))
    names = cases["groups"]["draw"]
    assert len(names) == 6 and CC.same(got, rec, names) is None, CC.same(got, rec, names)
    assert len(rec["draw_five_T5/circles"]) == 6 * 8 and all(len(rec[n + "/circles"]) == 0 for n in names if n.startswith("draw_six"))
    dst0 = np.fromfile(os.path.join(cases["dir"], "draw_five_T5.dst.u8"), np.uint8)
    changed = {n: int((rec[n + "/dst"] != dst0).sum()) for n in names}
    assert changed["draw_five_T5"] == 0 and changed["draw_six_all_black"] == 0
    assert all(changed[n] > 0 for n in ("draw_six_box_inside", "draw_six_box_touches_row_0", "draw_six_box_touches_last_row_and_column"))
