#!/usr/bin/env python3
"""Generates the golden fixtures under tests/golden/ from the ORACLE (oracle/liboracle.so).

The reference ships no golden vectors, known-answer tests or fixtures for this path and cannot
be built or run here (OpenCV 3.x is absent), so these vectors pin the oracle *restatement*
against regressions and give the HIP path a data-only target that travels to the GPU box --
they do NOT pin the oracle to the reference; reference_linemod.npz and reference_icp.npz (--reference, below) do that for the
LINEMOD half and for the ICP half.
Run:  python tests/golden/make_golden.py     (inputs are seeded; output is deterministic)

`--reference DIR` instead records what the CPU tests compare against the reference's own sources, as data, so that the
tests need no copy of the reference: the two tables of DIR/linemod (reference_tables.npz) and the layout table and linked
symbols of a CadReco caller compiled against DIR/CadReco's headers (cadreco_reference_abi.txt; needs build() first), and
the outputs of DIR/linemod/linemod.cpp, compiled against the stand-in of oracle/ref, on the cases of tests/reference_cases.py
(reference_linemod.npz), and those of DIR/ICP's ICP.cpp, common.cpp, depth_to_3d.cpp, detection.cpp and NMS.cpp, compiled the same
way, on the ICP cases of that module (reference_icp.npz: results only, written with fixed time stamps so that a second run gives
the same bytes), and those of linemod.cpp's template extraction on the extraction cases (reference_extract.npz, same writer),
and those of the OpenCV-typed caller tests/dropin/tu_cv_caller.cpp built against DIR's headers and compiled code on the cases of
tests/cv_caller_cases.py (reference_cv_caller.npz, same writer).
"""
import io
import os
import re
import shutil
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_py as O  # noqa: E402
from fealess_amd import synth  # noqa: E402


def bank_arrays(bank):
    t, f, p = bank.arrays()
    return dict(templates=t, features=f, poses=p)


def linemod_fixture():
    rng = np.random.default_rng(20261003)
    w0, h0, T = 320, 160, [5, 8]
    qs = [synth.random_quantized(rng, w0 >> l, h0 >> l, 0.04) for l in range(2) for _ in range(2)]
    bank = synth.make_bank("obj", 24, 2, 2, w0, h0, seed=5, qs=qs, planted_frac=0.3, bbox=64)
    matches, n = O.match_quantized(qs, w0, h0, T, [bank], 60.0)
    lms = [O.build_linear_memories(qs[2 + m], 8) for m in range(2)]
    sims = np.stack([O.total_similarity(lms, bank, g, 160, 80, 8) for g in range(bank.n_pyramids)])
    lm0 = O.build_linear_memories(qs[0], 5)
    np.savez_compressed(os.path.join(HERE, "linemod_320x160.npz"), w0=w0, h0=h0, T=np.array(T), q0=qs[0], q1=qs[1], q2=qs[2],
                        q3=qs[3], matches=matches, n_matches=n, sims=sims, lm_level0_mod0_crc=np.array([int(lm0.astype(np.uint64).sum()),
                                                                                                       int((lm0.astype(np.uint64) * (np.arange(lm0.size, dtype=np.uint64).reshape(lm0.shape) % 251)).sum())]),
                        threshold=60.0, **bank_arrays(bank))
    print("linemod fixture:", n, "matches")


def frontend_fixture():
    R, t = synth.object_pose(tx=-15, ty=8, tz=640, yaw=0.25)
    depth, bgr, _ = synth.render(640, 480, R, t, seed=11)
    d = np.ascontiguousarray(depth[150:342, 200:456])       # 256 x 192 window around the object
    b = np.ascontiguousarray(bgr[150:342, 200:456])
    qo = O.quantized_orientations(b, 10.0)
    qn = O.quantized_normals(d)
    pd = O.pyrdown_bgr(b)
    qo1 = O.quantized_orientations(pd, 10.0)
    np.savez_compressed(os.path.join(HERE, "frontend_256x192.npz"), bgr=b, depth=d, qo=qo, qn=qn, pyrdown=pd, qo1=qo1)
    print("frontend fixture: non-zero", int((qo != 0).sum()), int((qn != 0).sum()))


def icp_fixture():
    rng = np.random.default_rng(7)
    R, t = synth.object_pose(tz=650.0)
    depth, _, mask = synth.render(640, 480, R, t, seed=3, noise=True, background=False)
    ys, xs = np.nonzero(mask)
    sel = np.sort(rng.choice(len(ys), size=1500, replace=False))
    z = depth[ys[sel], xs[sel]].astype(np.float32)
    ref = np.stack([(xs[sel] - 320.0) / 608.0 * z, (ys[sel] - 240.0) / 608.0 * z, z], 1).astype(np.float32)
    dR = synth.rot_z(0.02) @ synth.rot_x(-0.015) @ synth.rot_y(0.01)
    c = ref.mean(0)
    model = ((ref - c) @ dR.T + c + np.array([1.5, -2.0, 1.0])).astype(np.float32)
    model += rng.normal(0, 0.3, model.shape).astype(np.float32)
    r32 = O.icp(ref, model, 12, 0.0, -3.0e38, accum64=False, trace=True)
    r64 = O.icp(ref, model, 12, 0.0, -3.0e38, accum64=True)
    rdef = O.icp(ref, model, 10, 0.5, 0.01)
    np.savez_compressed(os.path.join(HERE, "icp_1500.npz"), ref=ref, model=model, R32=r32["R"], T32=r32["T"], dm32=r32["dist_mean"],
                        trace32=r32["trace"], R64=r64["R"], T64=r64["T"], Rdef=rdef["R"], Tdef=rdef["T"], iters_def=rdef["iters"])
    print("icp fixture: iters", r32["iters"], "default-threshold iters", rdef["iters"])


def recognition_fixture():
    sc = synth.recognition_scene(lambda b, d, l: O.quantize_pyramid(b, d, l), levels=2, seed=21, n_views=3, n_random=5)
    res = O.recognition(sc["bgr"], sc["depth"], sc["K"], [5, 8], sc["bank"], 75.0, 10, 0.5, 0.01)
    res20 = O.recognition(sc["bgr"], sc["depth"], sc["K"], [5, 8], sc["bank"], 75.0, 20, -1.0, -3.0e38)
    md = np.stack(sc["bank"].model_depths)
    np.savez_compressed(os.path.join(HERE, "recognition_vga.npz"), bgr=sc["bgr"], depth=sc["depth"], K=np.array(sc["K"]),
                        model_depths=md, pose=res["pose"], best=np.array([res["best"]["x"], res["best"]["y"], res["best"]["template_id"]]),
                        best_sim=res["best"]["similarity"], n_matches=res["n_matches"], n_points=res["det"]["n_points"],
                        iters=res["det"]["icp"]["iters"], pose20=res20["pose"], **bank_arrays(sc["bank"]))
    print("recognition fixture: found", res["found"], "tid", res["best"]["template_id"], "iters", res["det"]["icp"]["iters"])


def reference_fixtures(ref):
    src = open(os.path.join(ref, "linemod", "linemod.cpp"), errors="replace").read()
    line = [l for l in src.splitlines() if l.startswith("CV_DECL_ALIGNED(16) static const unsigned char SIMILARITY_LUT")][0]
    sim = np.array([int(v) for v in re.findall(r"\d+", line[line.index("{"):])], np.uint8)
    txt = open(os.path.join(ref, "linemod", "normal_lut.i")).read()
    nrm = np.array([int(v) for v in re.findall(r"\d+", txt[txt.index("{"):])][:8000], np.uint8)
    assert sim.size == 256 and nrm.size == 8000
    np.savez_compressed(os.path.join(HERE, "reference_tables.npz"), similarity_lut=sim, normal_lut=nrm)

    cad, dropin = os.path.join(ROOT, "fealess_amd", "cadreco"), os.path.join(ROOT, "tests", "dropin")
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "tu_reference_caller")
    try:
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-w", "-DFL_REFERENCE_HEADERS", "-I", os.path.join(ref, "CadReco"), "-I", dropin,
                               os.path.join(dropin, "tu_reference_caller.cpp"), "-o", exe, "-L", cad, "-lcadreco_hip",
                               "-Wl,-rpath," + cad, "-Wl,-rpath," + os.path.join(ROOT, "fealess_amd", "csrc")])
        out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
        syms = subprocess.run(["nm", "-u", exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    finally:
        shutil.rmtree(tmp)
    layout = out[:out.index("--calls")]
    syms = sorted(s for s in syms if "CObjRecoCAD" in s)
    with open(os.path.join(HERE, "cadreco_reference_abi.txt"), "w") as f:
        f.write("# tests/dropin/tu_reference_caller.cpp compiled against the reference's CadReco headers "
                "(tests/golden/make_golden.py --reference):\n# its layout table, then the library symbols it links\n")
        f.write("\n".join(layout + ["--symbols"] + syms) + "\n")
    print("reference fixtures:", len(layout), "layout rows,", len(syms), "symbols")
    reference_linemod_fixture(ref)
    reference_icp_fixture(ref)
    reference_extract_fixture(ref)
    reference_cv_caller_fixture(ref)


def reference_linemod_fixture(ref):
    """Outputs of the reference's COMPILED linemod.cpp (oracle/ref, built here from `ref`) on the case list of
    tests/reference_cases.py -> reference_linemod.npz.  Data only: a sha256 digest of every output and of every case's inputs
    (the inputs are regenerated from seeds), and the match lists in full.  Both builds must agree before anything is written."""
    import reference_cases as RC
    import reference_py as R
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "ref")], env=dict(os.environ, FEALESS_REFERENCE_ROOT=os.path.abspath(ref)))
    scalar, simd = RC.ReferenceBackend(R.lib(False)), RC.ReferenceBackend(R.lib(True))
    rec = {}
    for g, (cases, fn) in RC.groups().items():
        for name, c in cases:
            out = fn(scalar, c)
            if RC.simd_takes(g, c):
                assert RC.same(out, fn(simd, c)) is None, name
            for k, v in out.items():
                rec[f"{g}/{name}/{k}"] = v if k == "__in__" else RC.digest(v)
                if k.startswith("matches_"):
                    rec[f"{g}/{name}/{k}/full"] = v
    path = os.path.join(HERE, "reference_linemod.npz")
    np.savez_compressed(path, **rec)
    print("reference linemod fixture:", len(rec), "entries,", os.path.getsize(path) // 1024, "KiB")


def save_npz_reproducibly(path, arrays):
    """np.savez_compressed with the members in sorted order and a fixed time stamp: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def reference_icp_fixture(ref):
    """Outputs of the reference's COMPILED ICP sources (oracle/ref/icp_harness.cpp, built here from `ref`) on the ICP case
    list of tests/reference_cases.py -> reference_icp.npz.  Results only: a digest of every case's inputs (regenerated from
    seeds), the float results as bit patterns, the ints, and a digest in place of every large array, one member per case
    (RC.recorded)."""
    import reference_cases as RC
    import reference_py as R
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "ref")], env=dict(os.environ, FEALESS_REFERENCE_ROOT=os.path.abspath(ref)))
    B = RC.ReferenceIcpBackend(R.icp_lib())
    rec = {}
    for g, (cases, fn) in RC.icp_groups().items():
        for name, c in cases:
            rec[f"{g}/{name}"] = RC.recorded(fn(B, c))
    path = os.path.join(HERE, "reference_icp.npz")
    save_npz_reproducibly(path, rec)
    print("reference icp fixture:", len(rec), "entries,", os.path.getsize(path) // 1024, "KiB")


def reference_extract_fixture(ref):
    """Outputs of the reference's COMPILED template extraction (linemod.cpp through oracle/ref/ref_harness.cpp, built here from
    `ref`) on the extraction case list of tests/reference_cases.py -> reference_extract.npz.  One member per case (RC.recorded
    with RC.is_image): a digest of the inputs, the feature lists, templates and bounding boxes in full, refusals as such,
    images as digests.  Both builds must agree before anything is written."""
    import reference_cases as RC
    import reference_py as R
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "ref")], env=dict(os.environ, FEALESS_REFERENCE_ROOT=os.path.abspath(ref)))
    scalar, simd = R.lib(False), R.lib(True)
    rec = {}
    for g, (cases, fn) in RC.extract_groups().items():
        for name, c in cases:
            out = fn(scalar, c)
            assert RC.same(out, fn(simd, c)) is None, name
            rec[f"{g}/{name}"] = RC.recorded(out, RC.is_image)
    path = os.path.join(HERE, "reference_extract.npz")
    save_npz_reproducibly(path, rec)
    print("reference extract fixture:", len(rec), "entries,", os.path.getsize(path) // 1024, "KiB")


def reference_cv_caller_fixture(ref):
    """Outputs of tests/dropin/tu_cv_caller.cpp compiled against the reference's own headers and compiled code
    (oracle/_ref/ref_cv_caller, built here from `ref`) on the case list of tests/cv_caller_cases.py -> reference_cv_caller.npz.
    Case outputs only (cv_caller_cases.recorded): match lists in canonical order, the long one as count, first and last 64
    entries and a digest; images above 8 KiB as digests; everything else in full."""
    import cv_caller_cases as CC
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "ref")], env=dict(os.environ, FEALESS_REFERENCE_ROOT=os.path.abspath(ref)))
    tmp = tempfile.mkdtemp()
    try:
        CC.write_case_dir(os.path.join(tmp, "in"), O)
        rec = CC.recorded(CC.run_caller(CC.REF_CALLER, os.path.join(tmp, "in"), os.path.join(tmp, "out")))
    finally:
        shutil.rmtree(tmp)
    path = os.path.join(HERE, "reference_cv_caller.npz")
    save_npz_reproducibly(path, rec)
    print("reference cv caller fixture:", len(rec), "entries,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--reference":
        reference_fixtures(sys.argv[2])
        sys.exit(0)
    linemod_fixture()
    frontend_fixture()
    icp_fixture()
    recognition_fixture()
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(HERE, f)) // 1024, "KiB")
