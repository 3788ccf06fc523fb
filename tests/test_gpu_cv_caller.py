"""include/fealess_opencv_adapter.hpp, RUN: the caller tests/dropin/tu_cv_caller.cpp, written against the reference's names
only, compiled against the adapter header and libfealess_hip.so, on the cases of tests/cv_caller_cases.py; every output against
what the same caller gave when it was compiled against the reference's own headers and compiled code
(tests/golden/reference_cv_caller.npz), bit for bit, match lists in the project's canonical order -- and, where
oracle/_ref/ref_cv_caller is present, against a live run of it on the same directory.  Both run on the stand-in containers of
oracle/ref/opencv2, not on OpenCV.

One g++ compile, one case directory and ONE child process (one HIP context) serve the module.
"""
import os

import pytest

import cv_caller_cases as CC
from util import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(tmp_path_factory, oracle):
    tmp = tmp_path_factory.mktemp("cv_caller")
    exe = str(tmp / "adapter_cv_caller")
    r = CC.compile_adapter_caller(exe)
    assert r.returncode == 0, r.stdout
    case_dir = str(tmp / "in")
    groups, _ = CC.write_case_dir(case_dir, oracle)
    got = CC.recorded(CC.run_caller(exe, case_dir, str(tmp / "out"), timeout=120))       # a fresh child; any failure ends the module here
    live = None
    if os.path.exists(CC.REF_CALLER):
        live = CC.recorded(CC.run_caller(CC.REF_CALLER, case_dir, str(tmp / "ref"), timeout=120))
    return dict(groups=groups, got=got, rec=dict(golden("reference_cv_caller.npz")), live=live)


GROUPS = ["match_two", "match_masks", "match_sizes", "match_quantized", "match_roi", "templates", "match_one", "match_sequence", "match_long",
          "detection", "icp", "depth3d", "draw"]


def test_group_list_is_the_case_list(run):
    assert sorted(run["groups"]) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_adapter_equals_the_compiled_reference(run, group):
    names = run["groups"][group]
    assert CC.same(run["got"], run["rec"], names) is None, CC.same(run["got"], run["rec"], names)
    if run["live"] is not None:
        assert CC.same(run["got"], run["live"], names) is None, CC.same(run["got"], run["live"], names)
