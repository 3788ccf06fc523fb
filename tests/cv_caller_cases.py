"""The cases of tests/dropin/tu_cv_caller.cpp: ONE list, used by the record (tests/golden/make_golden.py --reference ->
reference_cv_caller.npz), by tests/test_cv_caller_cpu.py and by tests/test_gpu_cv_caller.py.

write_case_dir(path) writes a case directory (manifest.txt, raw arrays, and per detector linemod_templates.yml + bank.bin);
read_outputs(out_dir) reads what a build of the caller wrote; recorded(outputs) is what goes into the record (large arrays as
digests, the long list as count / head / tail / digest); same(got, exp, names) compares two sets of outputs.

Every shape is small: 160 x 160 with T = {5, 8} (and {4, 2} where one detector has to serve two sizes), 72 x 64 with
T = {4, 2}; all satisfy linearize's asserts (linemod.cpp:981, :1062-1063).

Match lists: Detector::match ends in an UNSTABLE std::sort and a std::unique on adjacent entries, so the reference's list is
one of several valid ones.  Both sides are put through reference_cases.canonical (the project's canonical order within ties of
Match::operator<, then the adjacent unique) before they are compared, bit for bit.  That is exact as long as no two templates
OF ONE CLASS reach the same (x, y, similarity): otherwise which of the two survives std::unique depends on the sort.  The
long list is therefore made of many classes with one template each; the short lists are checked against the oracle's list
(tests/test_cv_caller_cpu.py), which is made from the list before the sort.
"""
import hashlib
import os
import struct

import numpy as np

import reference_cases as RC
from fealess_amd import synth
from fealess_amd.bank import MATCH_DTYPE, TemplateBank
from test_abi_cpu import write_linemod_yaml

W, H, T_MAIN = 160, 160, [5, 8]
SW, SH, T_SMALL = 72, 64, [4, 2]
CV_32F, CV_64F = 5, 6
LONG = "long_list"                     # the case whose list is longer than 65536
DIGEST_ABOVE = 8192                    # bytes: larger outputs are recorded as sha256 digests


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _K(w, h):
    s = w / 640.0
    return dict(fx=synth.FX * s, fy=synth.FY * s, cx=w / 2.0, cy=h / 2.0)


def _scene(w, h, seed):
    """A cluttered frame: two instances of the object in front of the textured, stepped background."""
    rng = np.random.default_rng(seed)
    s = w / 640.0
    poses = [synth.object_pose(tx=float(rng.uniform(-60, 60)) * s, ty=float(rng.uniform(-40, 40)) * s, tz=float(rng.uniform(600, 700)),
                               yaw=float(rng.uniform(-0.8, 0.8)), tilt=float(rng.uniform(0.1, 0.6))) for _ in range(2)]
    d, b, _ = synth.render_clutter(w, h, poses, seed=seed, **_K(w, h))
    return np.ascontiguousarray(b, np.uint8), np.ascontiguousarray(d, np.uint16)


def _pyr(hd, feats, M):
    keep = range(len(hd)) if M == 2 else range(0, len(hd), 2)          # colour only: the templates [l * 2 + 0]
    return [dict(width=int(hd[k]["width"]), height=int(hd[k]["height"]), offset_x=int(hd[k]["offset_x"]), offset_y=int(hd[k]["offset_y"]),
                 pyramid_level=int(hd[k]["pyramid_level"]), features=np.stack([feats[k]["x"], feats[k]["y"], feats[k]["label"]], 1).astype(np.int32))
            for k in keep]


def _trained(O, class_id, frame, windows, M, rng, n_planted, bbox):
    """Templates trained by the oracle (Detector::addTemplate restated) on windows of the frame, as tests/test_gpu_batch_frontend.py
    does, and pyramids planted from the frame's own quantised images; each with 13 pose floats of its own."""
    b, d = frame
    h, w = d.shape
    bank = TemplateBank(class_id, 2, M)
    for (x, y, ww, hh) in windows:
        mk = np.zeros((h, w), np.uint8)
        mk[y:y + hh, x:x + ww] = 255
        ex = O.add_template(b, d, mk, 2)
        if ex is not None:
            bank.add_pyramid(_pyr(ex[0], ex[1], M), rng.normal(0, 100, 13).astype(np.float32))
    q = O.quantize_pyramid(b, d, 2)
    qs = q if M == 2 else [q[0], q[2]]
    for _ in range(n_planted):
        tl = synth.planted_pyramid(rng, qs, 2, M, w, h, bbox=bbox)
        assert tl is not None
        bank.add_pyramid(tl, rng.normal(0, 100, 13).astype(np.float32))
    return bank


def _row_pyramid(rng, qs, M, w, h):
    """A two-level pyramid planted on ONE image row, 8 pixels wide: the only kind the reference can refine inside a 72 x 64
    frame (see refinable)."""
    for _ in range(2000):
        x0, y0 = int(rng.integers(2, (w - 12) // 2)) * 2, int(rng.integers(2, (h - 4) // 2)) * 2
        tl = []
        for l in range(2):
            s = 8 >> l
            for m in range(M):
                row = qs[l * M + m][y0 >> l, (x0 >> l):(x0 >> l) + s + 1]
                nz = np.nonzero(row)[0]
                if len(nz) >= 4 - 2 * l:
                    tl.append(dict(width=s, height=0, offset_x=x0 >> l, offset_y=y0 >> l, pyramid_level=l,
                                   features=np.array([(int(dx), 0, int(np.log2(row[dx]))) for dx in nz], np.int32)))
        if len(tl) == 2 * M:
            return tl
    raise AssertionError("no row of the frame holds a template")


def refinable(bank, T, w, h):
    """The reference refines a coarse match in a window of 16 x 16 grid cells that it clamps to [8 T, size - template - 8 T]
    (linemod.cpp:1515-1534).  Where that interval is empty the window starts at a negative cell and similarityLocal reads in
    front of the linear memory: undefined.  True when every template of the bank leaves the interval non-empty at w x h."""
    t, _, _ = bank.arrays()
    fine = t[t["pyramid_level"] < bank.levels - 1]
    return all(w - int(hd["width"]) - 8 * T[hd["pyramid_level"]] >= 8 * T[hd["pyramid_level"]] and
               h - int(hd["height"]) - 8 * T[hd["pyramid_level"]] >= 8 * T[hd["pyramid_level"]] for hd in fine)


def detectors(O):
    """name -> (T, M, [banks in the order they are inserted / written])."""
    big, small = _scene(W, H, 71), _scene(SW, SH, 72)
    rng = np.random.default_rng(7100)
    zeta = _trained(O, "zeta", big, [(8, 8, 72, 72), (70, 60, 72, 72)], 2, rng, 3, 48)
    alpha = _trained(O, "alpha", big, [(40, 30, 64, 72), (10, 70, 72, 64)], 2, rng, 4, 48)
    assert zeta.n_pyramids >= 4 and alpha.n_pyramids >= 5 and zeta.n_pyramids != alpha.n_pyramids
    assert refinable(zeta, T_MAIN, W, H) and refinable(alpha, T_MAIN, W, H)
    qb, qs = O.quantize_pyramid(*big, 2), O.quantize_pyramid(*small, 2)
    one = TemplateBank("obj", 2, 1)                      # colour only, 72 x 64
    for _ in range(5):
        one.add_pyramid(_row_pyramid(rng, [qs[0], qs[2]], 1, SW, SH), rng.normal(0, 100, 13).astype(np.float32))
    seq = TemplateBank("obj", 2, 2)                      # one detector at both sizes: templates that both can refine
    for q, (w, h) in ((qb, (W, H)), (qs, (SW, SH)), (qb, (W, H)), (qs, (SW, SH)), (qs, (SW, SH))):
        seq.add_pyramid(_row_pyramid(rng, q, 2, w, h), rng.normal(0, 100, 13).astype(np.float32))
    assert refinable(one, T_SMALL, SW, SH) and refinable(seq, T_SMALL, SW, SH) and refinable(seq, T_SMALL, W, H)
    many = []                                            # one level, one template per class, inserted out of alphabetical order:
    for k in rng.permutation(16):                        # every one of the 80 x 80 grid positions can be a match of its own
        bk = TemplateBank(f"c{k:02d}", 1, 2)
        bk.add_pyramid(synth.random_pyramid(rng, 1, 2, W, H, bbox=16, nf0=20), rng.normal(0, 100, 13).astype(np.float32))
        many.append(bk)
    return {"two": (T_MAIN, 2, [zeta, alpha]), "one": (T_SMALL, 1, [one]), "seq": (T_SMALL, 2, [seq]), "many": ([2], 2, many)}, big, small


def _bank_words(T, M, banks):
    w = [M, len(T)] + list(T) + [len(banks)]
    for b in banks:
        t, f, p = b.arrays()
        LM = b.levels * b.modalities
        w += [len(b.class_id)] + [ord(c) for c in b.class_id] + [b.n_pyramids]
        for i in range(b.n_pyramids):
            w += np.asarray(p[i], np.float32).view(np.int32).tolist()
            w += _template_words(t[i * LM:(i + 1) * LM], f)
    return np.array(w, np.int32)


def _template_words(hdrs, feats):
    w = []
    for hd in hdrs:
        fr = feats[hd["feat_begin"]:hd["feat_begin"] + hd["feat_count"]]
        w += [int(hd[k]) for k in ("width", "height", "offset_x", "offset_y", "pyramid_level")] + [len(fr)]
        w += np.stack([fr["x"], fr["y"], fr["label"]], 1).ravel().tolist()
    return w


def _f32(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def _f64(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


class _Dir:
    def __init__(self, path):
        self.path, self.lines, self.groups = path, [], {}
        os.makedirs(path, exist_ok=True)

    def put(self, name, a):
        np.ascontiguousarray(a).tofile(os.path.join(self.path, name))

    def case(self, group, kind, name, **kv):
        self.lines.append(" ".join([kind, name] + [f"{k}={v}" for k, v in kv.items()]))
        self.groups.setdefault(group, []).append(name)

    def close(self):
        with open(os.path.join(self.path, "manifest.txt"), "w") as f:
            f.write("\n".join(self.lines) + "\n")


def hand_templates():
    """Two modalities' worth of hand-made templates for drawResponse: (headers, features) in the bank's layout."""
    feats = [[(3, 4, 1), (10, 2, 5), (0, 0, 7), (17, 9, 2)], [(5, 5, 2), (7, 1, 0)]]
    w = []
    for m, fs in enumerate(feats):
        w += [20, 12, 2, 4, 0, len(fs)] + [v for f in fs for v in f]
    return np.array(w, np.int32)


def write_case_dir(path, O):
    """Writes the case directory; returns {group: [case names]} and what the tests need of the inputs."""
    D = _Dir(path)
    dets, big, small = detectors(O)
    for name, (T, M, banks) in dets.items():
        os.makedirs(os.path.join(path, name), exist_ok=True)
        write_linemod_yaml(os.path.join(path, name, "linemod_templates.yml"), banks, T)
        D.put(os.path.join(name, "bank.bin"), _bank_words(T, M, banks))
    rng = np.random.default_rng(7200)
    for stem, (b, d) in (("big", big), ("small", small)):
        D.put(stem + ".bgr", b)
        D.put(stem + ".d16", d)
    full = np.zeros((H, W), np.uint8)
    full[20:150, 10:140] = 255
    half = np.zeros((H, W), np.uint8)
    half[:, :90] = 255
    masks = {"mask_box.u8": full, "mask_half.u8": half, "mask_speckle0.u8": (rng.random((H, W)) < 0.7).astype(np.uint8) * 255,
             "mask_speckle1.u8": (rng.random((H, W)) < 0.7).astype(np.uint8) * 255,
             "mask_small.u8": (rng.random((SH, SW)) < 0.8).astype(np.uint8) * 255}
    for k, v in masks.items():
        D.put(k, v)
    thr = _f32(70.0)
    two = dict(det="two", w=W, h=H, src="big", thr=thr)
    # ---- match, two modalities: classes inserted as zeta then alpha
    D.case("match_two", "match", "two_plain", **two)
    D.case("match_two", "match", "two_filter_alpha", filter="alpha", **two)
    D.case("match_two", "match", "two_filter_nope", filter="nope", **two)
    D.case("match_two", "match", "two_filter_zeta_zeta", filter="zeta,zeta", **two)
    D.case("match_masks", "match", "two_masks_both", nmask=2, mask0="mask_box.u8", mask1="mask_half.u8", **two)
    D.case("match_masks", "match", "two_mask_first_only", nmask=2, mask0="mask_half.u8", mask1="-", **two)
    D.case("match_masks", "match", "two_mask_second_only", nmask=2, mask0="-", mask1="mask_box.u8", **two)
    D.case("match_masks", "match", "two_masks_speckled", nmask=2, mask0="mask_speckle0.u8", mask1="mask_speckle1.u8", **two)
    D.case("match_sizes", "match", "two_one_mask_for_two", nmask=1, mask0="mask_box.u8", **two)
    D.case("match_sizes", "match", "two_one_mask_for_two_quantized", nmask=1, mask0="mask_box.u8", quant=1, **two)
    D.case("match_sizes", "match", "two_one_source", nsrc=1, **two)
    D.case("match_sizes", "match", "two_one_source_quantized", nsrc=1, quant=1, **two)
    D.case("match_quantized", "match", "two_quantized", quant=1, **two)
    D.case("match_quantized", "match", "two_quantized_masked", quant=1, nmask=2, mask0="mask_speckle0.u8", mask1="mask_box.u8", **two)
    D.case("match_roi", "match", "two_roi", roi=1, **two)
    D.case("match_roi", "match", "two_roi_masks_quantized", roi=1, quant=1, nmask=2, mask0="mask_box.u8", mask1="mask_speckle1.u8", **two)
    # ---- getTemplates / getPoseInfo / classIds after a match
    D.case("templates", "match", "two_templates", tpl=1, **two)
    D.case("templates", "match", "two_templates_alpha", tpl=1, filter="alpha", **two)
    # ---- one modality
    one = dict(det="one", w=SW, h=SH, src="small", thr=thr)
    D.case("match_one", "match", "one_plain", nsrc=1, tpl=1, **one)
    D.case("match_one", "match", "one_quantized_masked", nsrc=1, quant=1, nmask=1, mask0="mask_small.u8", **one)
    D.case("match_one", "match", "one_two_sources", nsrc=2, **one)
    # ---- one detector object at 160 x 160, 72 x 64, 160 x 160 (T = {4, 2} divides both): the adapter's ensure()
    D.case("match_sequence", "match", "seq_160_first", det="seq", w=W, h=H, src="big", thr=thr, quant=1)
    D.case("match_sequence", "match", "seq_72", det="seq", w=SW, h=SH, src="small", thr=thr, quant=1)
    D.case("match_sequence", "match", "seq_160_again", det="seq", w=W, h=H, src="big", thr=thr, quant=1)
    # ---- a list longer than 65536 (16 classes of one one-level template, T = 2: every grid position with a score passes -100 %)
    D.case("match_long", "match", LONG, det="many", w=W, h=H, src="big", thr=_f32(-100.0), tpl=1)
    D.case("match_long", "match", "many_filtered", det="many", w=W, h=H, src="big", thr=_f32(-40.0), filter="c07,c15,c03")

    # ---- detection(): four cases of reference_cases.icp_groups, continuous and as ROIs
    dcases = {c[0]: c for c in RC.detection_cases()}
    picks = [("ordinary", "det_64x4"), ("runs_to_icp_it_thr", "det_65x5"), ("icp_refuses", "det_two_valid_pairs_64x4"),
             ("invalid_depth", "det_no_valid_pair_63x3"), ("rect_leaves_image", "det_refused_rect_leaves_frame")]

    def det_case(name, c, model, scene, r_match, t_match, roi):
        _, seed, rm, rr, K, holes, it, a, b, rotated = c
        D.put(name + ".model.d16", model)
        D.put(name + ".scene.d16", scene)
        D.put(name + ".rt.f32", np.concatenate([np.asarray(r_match, np.float32).ravel(), np.asarray(t_match, np.float32)]))
        kv = dict(mw=model.shape[1], mh=model.shape[0], sw=scene.shape[1], sh=scene.shape[0], roi=roi, it=it, dist_mean_thr=_f32(a),
                  dist_diff_thr=_f32(b), fx=_f64(K[0]), fy=_f64(K[1]), cx=_f64(K[2]), cy=_f64(K[3]))
        kv.update({f"rm{i}": rm[i] for i in range(4)})
        kv.update({f"rr{i}": rr[i] for i in range(4)})
        D.case("detection", "detection", name, **kv)

    for tag, cname in picks:
        c = dcases[cname]
        model, scene, r_match, t_match = RC.detection_input(c)
        for roi in (0, 1):
            det_case(f"detection_{tag}_{'roi' if roi else 'cont'}", c, model, scene, r_match, t_match, roi)
    c = dcases["det_64x4"]                                  # images of different sizes: the model image cut down around its crop
    model, scene, r_match, t_match = RC.detection_input(c)
    rm = c[2]
    det_case("detection_sizes_differ", c, model[:rm[1] + rm[3] + 2, :rm[0] + rm[2] + 3], scene, r_match, t_match, 0)
    det_case("detection_sizes_differ_scene_smaller", c, np.pad(model, ((0, 9), (0, 14))), scene, r_match, t_match, 0)

    # ---- icpCloudToCloud_Ex
    icases = {c[0]: c for c in RC.icp_cases()}
    for tag, cname in (("3_points", "icp_clean_3"), ("256_points", "icp_clean_256"), ("nan_points", "icp_nan_valid_model_65"),
                       ("invalid_points", "icp_invalid_both_257")):
        c = icases[cname]
        ref, model = RC.icp_input(c)
        D.put(f"icp_{tag}.ref.f32", ref)
        D.put(f"icp_{tag}.model.f32", model)
        D.case("icp", "icp", f"icp_{tag}", it=c[5], dist_mean_thr=_f32(c[6]), dist_diff_thr=_f32(c[7]))
    ref, model = RC.icp_input(icases["icp_clean_256"])
    D.put("icp_default_arguments.ref.f32", ref)
    D.put("icp_default_arguments.model.f32", model)
    D.case("icp", "icp", "icp_default_arguments")
    for tag, (nr, nm) in (("empty", (0, 0)), ("2_points", (2, 2))):
        D.put(f"icp_{tag}.ref.f32", ref[:nr])
        D.put(f"icp_{tag}.model.f32", model[:nm])
        D.case("icp", "icp", f"icp_{tag}", it=4, dist_mean_thr=_f32(0.0), dist_diff_thr=_f32(0.0))

    # ---- cup_d2pc::depthTo3d
    for (w, h) in ((23, 17), (64, 48)):
        d = rng.integers(0, 65536, (h, w)).astype(np.uint16)
        d[rng.random((h, w)) < 0.2] = 0
        d.ravel()[[0, 1, 2, w - 1, w * h - 1]] = (0, 1, 65535, 65535, 1)
        K = np.array([[RC.SCENE_K[0], 0, RC.SCENE_K[2]], [0, RC.SCENE_K[1], RC.SCENE_K[3]], [0, 0, 1]], np.float64)
        for tag, kv, Km in ((f"K64", dict(ktype=CV_64F), K), ("K32", dict(ktype=CV_32F), K), ("K64_roi", dict(ktype=CV_64F, roi=1), K),
                            ("K_3x4", dict(ktype=CV_64F), np.pad(K, ((0, 0), (0, 1))))):
            if tag == "K_3x4" and w != 23:
                continue
            name = f"depth3d_{w}x{h}_{tag}"
            D.put(name + ".depth.d16", d)
            D.put(name + ".K.f64", Km)
            D.case("depth3d", "depth3d", name, w=w, h=h, krows=Km.shape[0], kcols=Km.shape[1], **kv)

    # ---- drawResponse, both overloads (no GPU).  Every paste stays inside dst: a paste that leaves it is undefined behaviour
    # in the reference (dst.at<> out of range) and is kept out of the cases
    tw = hand_templates()
    dst = rng.integers(0, 256, (40, 48, 3), dtype=np.uint8)

    def box(r0, r1, c0, c1):
        ct = np.zeros((20, 24, 3), np.uint8)
        px = rng.integers(0, 256, (r1 - r0, c1 - c0, 3), dtype=np.uint8)
        px[rng.random(px.shape) < 0.3] = 0                     # pixels with some, and some with all, channels zero inside the box
        px[0, :, 1] = 9
        px[-1, :, 2] = 9
        px[:, 0, 0] = 9
        px[:, -1, 0] = 9                                          # the box's outline is non-black: its extent is what is intended
        ct[r0:r1, c0:c1] = px
        return ct

    draws = [("draw_five_T5", dict(m=2, t=5), None), ("draw_five_T8_one_modality", dict(m=1, t=8), None),
             ("draw_six_box_inside", dict(m=2, t=5), box(4, 11, 3, 12)), ("draw_six_box_touches_row_0", dict(m=2, t=5), box(0, 6, 3, 10)),
             ("draw_six_box_touches_last_row_and_column", dict(m=2, t=8), box(15, 20, 18, 24)), ("draw_six_all_black", dict(m=2, t=5), np.zeros((20, 24, 3), np.uint8))]
    for name, kv, ct in draws:
        D.put(name + ".dst.u8", dst)
        D.put(name + ".templates.i32", tw)
        if ct is not None:
            D.put(name + ".ct.u8", ct)
            kv = dict(kv, six=1, ctrows=ct.shape[0], ctcols=ct.shape[1])
        D.case("draw", "draw", name, rows=dst.shape[0], cols=dst.shape[1], offx=6, offy=5, ntempl=2, **kv)
    D.close()
    return D.groups, dict(dets=dets, big=big, small=small, masks=masks)


# ---- running a build of the caller ---------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CALLER = os.path.join(ROOT, "oracle", "_ref", "ref_cv_caller")


def compile_adapter_caller(exe):
    """tests/dropin/tu_cv_caller.cpp against include/fealess_opencv_adapter.hpp on the stand-in's containers; returns g++'s
    CompletedProcess (the callers assert on it)."""
    import subprocess
    cad, csrc, orc = (os.path.join(ROOT, *p) for p in (("fealess_amd", "cadreco"), ("fealess_amd", "csrc"), ("oracle",)))
    return subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "oracle", "ref"), "-I", os.path.join(ROOT, "include"),
                           "-I", cad, os.path.join(ROOT, "tests", "dropin", "tu_cv_caller.cpp"), "-o", exe, "-L", cad, "-lcadreco_hip",
                           "-L", csrc, "-lfealess_hip", "-Wl,-rpath," + cad, "-Wl,-rpath," + csrc],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def run_caller(exe, case_dir, out_dir, kind=None, timeout=120):
    """One fresh child process; a non-zero status, a signal or the timeout is an AssertionError.  Returns read_outputs(out_dir)."""
    import subprocess
    os.makedirs(out_dir, exist_ok=True)
    r = subprocess.run([exe, case_dir, out_dir] + ([kind] if kind else []), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:])
    return read_outputs(out_dir)


# ---- outputs -----------------------------------------------------------------------------------------------------------
_DTYPES = {"i32": np.int32, "u8": np.uint8, "f32": np.uint32, "f64": np.float64}     # f32 as bit patterns


def read_outputs(out_dir):
    """{'<case>/<key>': array}; float32 outputs as uint32 bit patterns with every NaN as the one quiet NaN."""
    out = {}
    for f in sorted(os.listdir(out_dir)):
        name, key, ext = f.rsplit(".", 2)
        a = np.fromfile(os.path.join(out_dir, f), _DTYPES[ext])
        if ext == "f32":
            a = RC.fbits(a.view(np.float32))
        out[f"{name}/{key}"] = a
    return out


def match_list(a):
    """The caller's (n, 5) int32 rows as MATCH_DTYPE in canonical order.  class_idx is the index in the bank file's order."""
    a = np.asarray(a, np.int32).reshape(-1, 5)
    m = np.zeros(len(a), MATCH_DTYPE)
    m["x"], m["y"], m["class_idx"], m["template_id"] = a[:, 0], a[:, 1], a[:, 3], a[:, 4]
    m["similarity"] = a[:, 2].copy().view(np.float32)
    return RC.canonical(m)


def _digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def recorded(outputs):
    """What the record keeps of a set of outputs: match lists in canonical order (the long one as count, first and last 64
    entries and a digest of all of it), arrays above DIGEST_ABOVE bytes as sha256 digests, everything else in full."""
    rec = {}
    for k, v in outputs.items():
        if k.endswith("/matches"):
            m = match_list(v)
            rec[k + "/count"] = np.array([len(m)], np.int64)
            if len(m) > 4096:
                rec[k + "/head"], rec[k + "/tail"], rec[k + "/sha256"] = m[:64], m[-64:], _digest(m)
            else:
                rec[k] = m
        elif v.nbytes > DIGEST_ABOVE:
            rec[k + "/sha256"] = _digest(v)
        else:
            rec[k] = v
    return rec


def same(got, exp, names):
    """None, or what differs between two recorded() dicts on the cases `names` (every key of every case, both ways)."""
    names = set(names)
    keys = lambda d: sorted(k for k in d if k.split("/")[0] in names)
    if keys(got) != keys(exp):
        return f"outputs differ: {sorted(set(keys(got)) ^ set(keys(exp)))}"
    for k in keys(exp):
        a, b = np.asarray(got[k]), np.asarray(exp[k])
        if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
            return f"{k}: {a[:8] if a.ndim else a} != {b[:8] if b.ndim else b} (shapes {a.shape}, {b.shape})"
    return None


def status(outputs, name):
    s = outputs[name + "/status"]
    return ("threw", "StsAssert" if s[1] else "other") if s[0] else ("returned", int(s[1]))
