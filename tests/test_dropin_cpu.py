"""Compile-time check of the drop-in claim.

`tests/golden/cadreco_reference_abi.txt` records what a small C++ caller (tests/dropin/tu_reference_caller.cpp) sees when it is
compiled against the reference's own `CadReco/obj_reco_temp.h` / `lotus_common.h` (`make_golden.py --reference`; nothing is
copied): sizeof / offsetof of every type that crosses the facade, the vtable slot of every virtual method, enum values and error
codes, and the mangled symbols it links.  The same caller compiled against `fealess_amd/cadreco/fealess_cadreco.h` must print
the same table, `libcadreco_hip.so` must export every one of those symbols, and the calls -- Create / AddObj / Recognition /
Destroy through a `CObjRecoCAD*` -- must behave (vtable order, enum values, error codes) without a GPU: the documented error codes.
"""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAD = os.path.join(ROOT, "fealess_amd", "cadreco")
SRC = os.path.join(ROOT, "tests", "dropin")
REF_ABI = os.path.join(ROOT, "tests", "golden", "cadreco_reference_abi.txt")


def _run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)


def test_reference_caller_links_and_layouts_agree(tmp_path):
    lib = os.path.join(CAD, "libcadreco_hip.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    ref = [l for l in open(REF_ABI).read().splitlines() if l and not l.startswith("#")]
    cut = ref.index("--symbols")
    ref_layout, ref_symbols = ref[:cut], ref[cut + 1:]
    assert len(ref_layout) == 44 and len(ref_symbols) == 3
    cad = C.CDLL(lib)
    missing = [s for s in ref_symbols if not hasattr(cad, s)]
    assert not missing, f"libcadreco_hip.so does not export what the reference's headers make a caller link: {missing}"
    refc = str(tmp_path / "tu_ref")
    r = _run(["g++", "-std=c++14", "-O1", "-I", CAD, "-I", SRC, os.path.join(SRC, "tu_reference_caller.cpp"), "-o", refc,
              "-L", CAD, "-lcadreco_hip", "-Wl,-rpath," + CAD, "-Wl,-rpath," + os.path.join(ROOT, "fealess_amd", "csrc")])
    assert r.returncode == 0, r.stdout
    out = _run([refc, str(tmp_path / "no_such_bank")])
    assert out.returncode == 0, out.stdout
    lines = out.stdout.strip().splitlines()
    cut = lines.index("--calls")
    assert lines[:cut] == ref_layout, "layout of the facade types differs between the reference's headers and fealess_cadreco.h"
    calls = dict(l.split(" ", 1) for l in lines[cut + 1:])
    assert calls["create_unsupported"] == "1" and calls["create"] == "1"
    assert calls["version"].startswith("CAD-based 3D Object Recog")
    assert int(calls["addobj_missing"]) != 0                # ERROR_OPEN_FILE_FAILED with a GPU, ERROR_UNKNOW without one
    assert calls["clearobj"] == "0" and calls["setadvanced"] == "0"          # no-ops returning 0 (obj_reco_lmicp.cpp:76-84,206-209)
    rc, n = calls["recognition_no_object"].split()
    assert int(rc) == -2147483647 and n == "0"              # ERROR_INVALID_PARAM: no object loaded
    assert int(calls["recognition_bad_image"]) == -2147483647
    assert calls["destroyed"] == "1"


def test_opencv_adapter_header_is_well_formed():
    """include/fealess_opencv_adapter.hpp (readLinemod / Detector::match / detection / icpCloudToCloud_Ex / depthTo3d with the
    reference's OpenCV-typed signatures) cannot be built here -- there is no OpenCV in the image -- so it gets a syntax-only
    pass against a declarations-only stand-in of <opencv2/core.hpp> (tests/dropin/opencv_stub), every entry point used."""
    r = _run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-I", os.path.join(SRC, "opencv_stub"), "-I", os.path.join(ROOT, "include"),
              "-I", CAD, os.path.join(SRC, "tu_adapter_syntax.cpp")])
    assert r.returncode == 0, r.stdout
    assert "warning" not in r.stdout, r.stdout


def test_cxx_caller_of_the_multi_gpu_host_compiles_and_links(tmp_path):
    """include/fealess_mg.h from C++ (north_star: "host code stays C++"): a translation unit that uses every entry point compiles
    with g++ against the header alone and links libfealess_mg.so (which brings in librccl and libfealess_hip.so); run here it
    only reaches the argument checks -- the collectives run on the GPU box (tests/test_gpu_configs.py)."""
    exe = str(tmp_path / "tu_mg")
    MG = os.path.join(ROOT, "fealess_amd", "mg")
    r = _run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), os.path.join(SRC, "tu_mg_caller.cpp"), "-o", exe,
              "-L", MG, "-lfealess_mg", "-Wl,-rpath," + MG, "-Wl,-rpath," + os.path.join(ROOT, "fealess_amd", "csrc"), "-Wl,-rpath,/opt/rocm/lib"])
    assert r.returncode == 0, r.stdout
    out = _run([exe])
    assert out.returncode == 0, out.stdout
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().splitlines() if " " in l)
    assert lines["create_null_detector"] == "-1 1" and lines["unique_id_short_buffer"] == "-1" and lines["recognize_null_group"] == "-1"
    assert lines["sizeof_result"] == "92"
