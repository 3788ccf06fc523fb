"""GPU parity with the REFERENCE ITSELF, bit for bit: the HIP kernels against the outputs recorded from the reference's compiled
linemod.cpp (tests/golden/reference_linemod.npz; always run) and against the compiled reference live (oracle/_ref/, which
travels with the tree; tests/reference_py.require decides what its absence means), on seeded cases placed on the kernels'
dispatch edges as fl_linmem.hip, fl_scan.hip and fl_refine.hip state them.  Neither part reads a reference source tree.

The ICP half the same way (tests/golden/reference_icp.npz and oracle/_ref/libfealess_ref_icp.so, the reference's compiled ICP.cpp,
common.cpp, depth_to_3d.cpp, detection.cpp and NMS.cpp): FL_ICP_PARITY under every build of the ICP kernels that test_gpu_icp.py's
`width` fixture selects, on cloud sizes on the wave and workgroup strides of those builds; ctx.detection, ctx.depth_to_3d and
fl_nms.  Every comparison is equality of bit patterns or of ints.

Template extraction the same way (tests/golden/reference_extract.npz, RC.extract_groups), every group on the kernels:
fl_dev_extract_select on the `select` cases; fl_dev_extract_quantized -- the candidate kernels, sort and selection of one level
on quantized images from the caller, through the launch functions extract_chunk calls -- on the `extract_color` and
`extract_depth` cases (magnitude exactly 55^2 against 55^2 + 1, q == 0 under a huge magnitude, labels 0 and 255,
extract_threshold 2 / 1 / 0, distance exactly at the threshold, equal scores across labels, absent labels, mask values other
than 255, masks flush with the border, a hole, a one-pixel line); ctx.quantized_orientations (k_color_quantize<false, *>) and
fl_dev_quantized_orientations_mag (k_color_quantize<true, *>, labels and magnitude) on the `orientations` cases;
ctx.extract_template_pyramid and extract_template_batch on the `add_template` cases.  tests/test_gpu_extract_candidates.py holds
the intermediate products of the candidate stage to plain references.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import reference_cases as RC
import reference_py as R
from fealess_amd import _lib as L
from fealess_amd import api, synth
from test_gpu_icp import width  # noqa: F401  (the fixture that forces each build of the ICP kernels in turn)
from util import golden

pytestmark = pytest.mark.gpu
GROUPS = RC.groups()
ICP_GROUPS = RC.icp_groups()
EXTRACT_GROUPS = RC.extract_groups()


def _detector(ctx, case):
    det = api.Detector(ctx, case["M"], case["T"])
    for b in case["banks"]:
        det.add_class(b)
    det.finalize(case["w0"], case["h0"])
    det.set_class_filter(case["class_ids"])
    return det


# ---- against the recorded reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, c in GROUPS["linearize"][0]])
def test_linear_memories_equal_recorded_reference(ctx, name):
    """The reference's CV_Asserts (rows * cols % 16, linemod.cpp:981; rows, cols % T, :1062-1063) are part of the record:
    where it refused, the kernel's entry point must refuse too."""
    case = dict(GROUPS["linearize"][0])[name]
    rec = golden("reference_linemod.npz")
    q, _ = RC.linearize_input(case)
    if f"linearize/{name}/lm_refused" in rec.files:
        with pytest.raises(api.FealessError) as e:
            ctx.build_linear_memories(q, case[3])
        assert e.value.code == -3
        return
    got = ctx.build_linear_memories(q, case[3])
    assert np.array_equal(RC.digest(got), rec[f"linearize/{name}/lm"])


@pytest.mark.parametrize("name", list(RC.match_cases()))
def test_match_and_similarity_maps_equal_recorded_reference(ctx, name):
    case = RC.match_cases()[name]
    rec = golden("reference_linemod.npz")
    det = _detector(ctx, case)
    for thr in case["thresholds"]:
        exp = rec[f"match/{name}/matches_{thr:g}/full"]
        got, n = det.match_quantized(case["qs"], thr, cap=1 << 18)
        assert n == len(exp), (thr, n, len(exp))
        assert RC.matches_equal(got, exp), thr
    if len(case["banks"]) == 1:        # fl_similarity_maps indexes the pyramids of the whole detector; one class: no ordering to assume
        assert np.array_equal(RC.digest(det.similarity_maps(0, case["banks"][0].n_pyramids)), rec[f"match/{name}/sims"])
    det.close()


@pytest.mark.parametrize("name", [c[0] for c in RC.normals_cases()])
def test_quantized_normals_equal_recorded_reference(ctx, name):
    case = dict(GROUPS["normals"][0])[name]
    rec = golden("reference_linemod.npz")
    got = ctx.quantized_normals(RC.normals_input(case), case[4], case[5])
    assert np.array_equal(RC.digest(got), rec[f"normals/{name}/qn"])


# ---- against the compiled reference, live, on the dispatch edges -------------------------------------------------------
# fl_launch_build_lm takes k_build_lm when w % 4 == 0 and W % 4 == 0 and 2 <= T <= 8 and the strip of k*T rows fits:
# lds = 2 * (k*T + T-1) * (w+16) + 2048, k from 6 down while lds > 60 KiB, refused above 64 KiB even at k = 1.
LM_EDGES = [(150, 80, 5),      # w % 4 != 0                                   -> generic
            (80, 48, 8),       # w % 4 == 0, W = 10: W % 4 != 0               -> generic
            (96, 48, 8),       # W = 12                                       -> k_build_lm, k = 6
            (64, 48, 16),      # T > 8                                        -> generic
            (64, 48, 2),       # T = 2, the lower bound                       -> k_build_lm
            (512, 64, 8),      # 2*55*528+2048 = 60128 <= 61440: still k = 6
            (544, 64, 8),      # 2*55*560+2048 = 63648 > 61440: k drops to 5
            (2080, 64, 8),     # only k = 1 fits: 2*15*2096+2048 = 64928 <= 65536
            (2560, 64, 8)]     # 2*15*2576+2048 = 79328 > 64 KiB: not even k = 1 -> generic although w % 4 == W % 4 == 0


@pytest.mark.parametrize("w,h,T", LM_EDGES)
@pytest.mark.parametrize("density", [0.05, 0.9])
def test_linear_memories_equal_live_reference_on_dispatch_edges(ctx, w, h, T, density):
    ref = R.require(False)
    q = synth.random_quantized(np.random.default_rng(w * 31 + T), w, h, density)
    got = ctx.build_linear_memories(q, T)
    assert np.array_equal(got, ref.build_linear_memories(q, T, got.shape[1]))


def _edge_case(w0, h0, T, M, counts, seed, density, bbox):
    levels = len(T)
    qs = RC._pyramid(np.random.default_rng(seed), w0, h0, levels, M, density)
    planted = synth.make_bank("obj", 6, levels, M, w0, h0, seed=seed + 1, qs=qs, planted_frac=0.5, bbox=bbox)
    counted = RC._count_bank("cnt", levels, M, counts, w0, h0, seed + 2, bbox=bbox)
    return dict(qs=qs, w0=w0, h0=h0, T=T, M=M, banks=[planted, counted], class_ids=(), thresholds=[])


# k_scan chunks the W*H positions by 1024 and pads the features to groups of 8; k_refine clamps its 16x16 window at the
# borders; k_spread takes strips of k = 4 rows of T while 2*(k*T+T-1)*(w+16) <= 60 KiB (w = 1280, T = 5: k drops to 3) and
# needs w % 4 == 0 (650: generic, and 325 % 4 != 0 sends level 1 to the generic linear-memory kernel)
SCAN_EDGES = [("wh_992", 256, 248, [8], 1), ("wh_1024", 256, 256, [8], 1), ("wh_1056", 256, 264, [8], 2),
              ("refine_T5_T8", 320, 240, [5, 8], 2), ("refine_T4_T8", 320, 240, [4, 8], 1), ("three_levels", 640, 480, [5, 8, 4], 2),
              ("spread_k_drops_1280", 1280, 720, [5, 8], 1), ("spread_generic_650", 650, 480, [5, 5], 1)]


@pytest.mark.parametrize("name,w0,h0,T,M", SCAN_EDGES)
def test_match_equals_live_reference_on_scan_and_refine_edges(ctx, name, w0, h0, T, M):
    ref = RC.ReferenceBackend(R.require(False))
    case = _edge_case(w0, h0, T, M, [1, 7, 8, 9, 63], 11000 + w0 + h0, 0.25, 48)
    det = _detector(ctx, case)
    seen = 0
    for thr in (-100.0, 40.0, 70.0):
        exp = ref.match(case, thr)
        for prune, mid in ((1, 0), (1, 0xFF), (0, 0)):
            ctx.set_option("scan_prune", prune)
            ctx.set_option("scan_prune_mid", mid)
            try:
                got, n = det.match_quantized(case["qs"], thr, cap=1 << 20)
            finally:
                ctx.set_option("scan_prune", 1)
                ctx.set_option("scan_prune_mid", 0)
            assert n == len(exp), (thr, prune, mid, n, len(exp))
            assert RC.matches_equal(got, exp), (thr, prune, mid)
        seen += len(exp)
    assert seen > 0
    det.close()


@pytest.mark.parametrize("n_live", [0, 1, 2047, 2048, 2049])
def test_sort_unique_equals_live_reference_at_exact_list_sizes(ctx, n_live):
    """k_sort_unique around its switch from the LDS to the HBM bitonic path (2048 live matches).  n_live isolated pixels of
    one label at multiples of T, one 1-feature template of that label, threshold 70 (raw score 4 > 3): exactly n_live matches, all tied in
    similarity and template id."""
    ref = RC.ReferenceBackend(R.require(False))
    q = np.zeros((480, 640), np.uint8)
    cells = np.random.default_rng(12100 + n_live).permutation(80 * 60)[:n_live]
    q[(cells // 80) * 8, (cells % 80) * 8] = 1 << 3
    bank = RC.TemplateBank("obj", 1, 1)
    bank.add_pyramid([dict(width=1, height=1, offset_x=0, offset_y=0, pyramid_level=0, features=np.array([[0, 0, 3]], np.int32))])
    case = dict(qs=[q], w0=640, h0=480, T=[8], M=1, banks=[bank], class_ids=(), thresholds=[])
    exp = ref.match(case, 70.0)
    assert len(exp) == n_live
    det = _detector(ctx, case)
    got, n = det.match_quantized([q], 70.0, cap=1 << 16)
    assert n == n_live and RC.matches_equal(got, exp)
    det.close()


def test_sort_unique_equals_live_reference_above_20000(ctx):
    """The HBM bitonic path well above the switch, with many ties: 2- to 5-feature templates on a dense image."""
    ref = RC.ReferenceBackend(R.require(False))
    qs = RC._pyramid(np.random.default_rng(12000), 640, 480, 1, 1, 0.6)
    bank = RC._count_bank("obj", 1, 1, [2, 2, 3, 2, 5, 2], 640, 480, 12001, bbox=24)
    case = dict(qs=qs, w0=640, h0=480, T=[8], M=1, banks=[bank], class_ids=(), thresholds=[])
    exp = ref.match(case, 75.0)
    assert len(exp) > 20000
    det = _detector(ctx, case)
    got, n = det.match_quantized(qs, 75.0, cap=1 << 20)
    assert n == len(exp) and RC.matches_equal(got, exp)
    det.close()


# ---- the ICP half --------------------------------------------------------------------------------------------------------
class KernelIcpBackend:
    """The HIP entry points under the method names of reference_cases.ReferenceIcpBackend, in FL_ICP_PARITY."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.depth_to_3d = ctx.depth_to_3d

    def icp(self, ref, model, it, a, b):
        return self.ctx.icp_cloud_to_cloud_ex(ref, model, it, a, b, L.FL_ICP_PARITY)

    def detection(self, model, scene, K, rm, rr, it, a, b, r_match, t_match):
        try:
            return self.ctx.detection(model, scene, K, rm, rr, it, a, b, r_match, t_match, L.FL_ICP_PARITY)
        except api.FealessError as e:
            assert e.code == -3                             # FL_ERR_ASSERT: the reference's CV_Assert on the ROI
            raise AssertionError("reference CV_Assert")

    def nms(self, t, n_points, icp_dist, th_obj_dist):
        n = len(n_points)
        objs = (L.RecognitionResult * max(1, n))()
        for i in range(n):
            objs[i].det.T_final[:] = [float(v) for v in t[i]]
            objs[i].det.n_points = int(n_points[i])
            objs[i].det.icp.dist_mean = float(icp_dist[i])
        win = (C.c_int * max(1, n))()
        nw = C.c_int(0)
        self.ctx.check(self.ctx.lib.fl_nms(objs, n, th_obj_dist, win, C.byref(nw)))
        return [int(win[i]) for i in range(nw.value)]


def _icp_case(group, name):
    cases, fn = ICP_GROUPS[group]
    return dict(cases)[name], fn


def _names(group):
    return [n for n, _ in ICP_GROUPS[group][0]]


@pytest.mark.parametrize("name", _names("icp"))
def test_icp_parity_equals_recorded_reference(ctx, width, name):
    """R, T, dist_mean and px_ratio of every prefix icp_it_thr = 0 .. N, and `iter` on exit, under each build."""
    case, fn = _icp_case("icp", name)
    diff = RC.same_as_record(fn(KernelIcpBackend(ctx), case), golden("reference_icp.npz"), "icp", name)
    assert diff is None, (name, width, diff)


@pytest.mark.parametrize("name", _names("detection"))
def test_detection_equals_recorded_reference(ctx, width, name):
    """R_final, T_final, the ICP result inside, n_points and `iter`; a crop that leaves the frame is refused on both sides."""
    case, fn = _icp_case("detection", name)
    diff = RC.same_as_record(fn(KernelIcpBackend(ctx), case), golden("reference_icp.npz"), "detection", name)
    assert diff is None, (name, width, diff)


@pytest.mark.parametrize("group,name", [(g, n) for g in ("depth3d", "nms") for n in _names(g)])
def test_depth_to_3d_and_nms_equal_recorded_reference(ctx, group, name):
    case, fn = _icp_case(group, name)
    diff = RC.same_as_record(fn(KernelIcpBackend(ctx), case), golden("reference_icp.npz"), group, name)
    assert diff is None, (name, diff)


@pytest.mark.parametrize("group", ["icp", "detection", "depth3d", "nms"])
def test_icp_half_equals_live_reference(ctx, group):
    """The same cases against the compiled reference itself, under the build the library picks for one job."""
    ref = RC.ReferenceIcpBackend(R.require_icp())
    cases, fn = ICP_GROUPS[group]
    for name, case in cases:
        diff = RC.same(fn(KernelIcpBackend(ctx), case), fn(ref, case))
        assert diff is None, (name, diff)


# ---- template extraction ---------------------------------------------------------------------------------------------------
FILL = -7


class KernelExtractBackend:
    """The HIP entry points under the method names of reference_py.Ref, for the groups the kernels have an entry for."""

    def __init__(self, ctx):
        self.ctx = ctx

    def select_job(self, job):
        """fl_dev_extract_select on one job, candidates in the job's own arrival order: the features, or None (refused)."""
        n_out, feats, keys = self.ctx.dev_extract_select([job], fill=FILL)[0]
        if n_out == -1:
            assert (feats == FILL).all()
            return None
        assert n_out == job["num_features"] and (feats[n_out:] == FILL).all()
        return feats[:n_out]

    @staticmethod
    def as_record(got):
        """(templates, features per template, bb) of reference_cases.add_template_record from a kernel result."""
        if got is None:
            return None
        tl, bb = got
        t = {k: np.array([d[k] for d in tl], np.int32) for k in ("width", "height", "offset_x", "offset_y", "pyramid_level")}
        t["feat_count"] = np.array([len(d["features"]) for d in tl], np.int32)
        return t, [np.asarray(d["features"], np.int32).reshape(-1, 3) for d in tl], bb

    def add_template(self, bgr, depth, mask, levels):
        return self.as_record(self.ctx.extract_template_pyramid(bgr, depth, mask, levels))

    def _extract_quantized(self, modality, quantized, magnitude, mask, threshold, num_features):
        """fl_dev_extract_quantized on one view: the features, or None (refused: nothing sorted, nothing written)."""
        g = self.ctx.dev_extract_quantized(modality, [quantized], [magnitude], None if mask is None else [mask], threshold, num_features, fill=FILL)[0]
        assert g["tails_unwritten"]
        if g["n_out"] == -1:
            assert g["n_cand"] < num_features and g["keys"] is None and (g["features"] == FILL).all()
            return None
        assert g["n_out"] == num_features <= g["n_cand"] and (g["features"][num_features:] == FILL).all()
        return g["features"][:num_features]

    def extract_template_color(self, quantized, magnitude, mask, strong_threshold, num_features):
        return self._extract_quantized(0, quantized, magnitude, mask, strong_threshold, num_features)

    def extract_template_depth(self, normal, mask, extract_threshold, num_features):
        return self._extract_quantized(1, normal, None, mask, extract_threshold, num_features)

    def quantized_orientations_mag(self, bgr, weak_threshold=10.0):
        """k_color_quantize<true, *>, the build extraction launches: (labels, squared magnitude)."""
        q, mag = self.ctx.dev_quantized_orientations_mag([bgr], weak_threshold)
        return q[0], mag[0]


def _extract_names(group):
    return [n for n, _ in EXTRACT_GROUPS[group][0]]


def _extract_case(group, name):
    return dict(EXTRACT_GROUPS[group][0])[name]


def _against_extract_record(out, group, name):
    diff = RC.same_as_record(out, golden("reference_extract.npz"), group, name, RC.is_image)
    assert diff is None, (name, diff)


@pytest.mark.parametrize("name", _extract_names("select"))
def test_extract_select_equals_recorded_reference(ctx, name):
    """std::stable_sort + selectScatteredFeatures: the features, or the refusal where the list is shorter than num_features."""
    job = _extract_case("select", name)
    _against_extract_record(RC.select_record(job, KernelExtractBackend(ctx).select_job(job)), "select", name)


@pytest.mark.parametrize("name", _extract_names("orientations"))
def test_quantized_orientations_equal_recorded_reference(ctx, name):
    """quantizedOrientations: the quantized image from both builds of the colour quantiser, the public entry point's (it returns
    no magnitude) and extraction's, and the magnitude image from extraction's."""
    case = _extract_case("orientations", name)
    rec = RC.record_parts(golden("reference_extract.npz"), "orientations", name, ["__in__", "img_mag", "img_q"])
    bgr = RC.orientation_input(case)
    assert RC._with_inputs({}, bgr)["__in__"].tobytes() == rec["__in__"]
    assert RC.digest(ctx.quantized_orientations(bgr, 10.0)).tobytes() == rec["img_q"]
    q, mag = KernelExtractBackend(ctx).quantized_orientations_mag(bgr, 10.0)
    assert RC.digest(q).tobytes() == rec["img_q"]
    assert RC.digest(RC.fbits(mag)).tobytes() == rec["img_mag"]
    _against_extract_record(RC.compute_orientations(KernelExtractBackend(ctx), case), "orientations", name)


@pytest.mark.parametrize("group,name", [(g, n) for g in ("extract_color", "extract_depth") for n in _extract_names(g)])
def test_extract_candidates_equal_recorded_reference(ctx, group, name):
    """The two extractTemplate methods on given quantized images: the features in full, or the refusal."""
    _against_extract_record(EXTRACT_GROUPS[group][1](KernelExtractBackend(ctx), _extract_case(group, name)), group, name)


@pytest.mark.parametrize("name", _extract_names("add_template"))
def test_extract_template_pyramid_equals_recorded_reference(ctx, name):
    """Detector::addTemplate: templates, features and bounding box in full, or the refusal."""
    _against_extract_record(RC.compute_add_template(KernelExtractBackend(ctx), _extract_case("add_template", name)), "add_template", name)


def _batches():
    """The add_template cases by frame size and level count: one fl_extract_template_batch call takes one of each."""
    out = {}
    for name, c in EXTRACT_GROUPS["add_template"][0]:
        out.setdefault((c["depth"].shape[1], c["depth"].shape[0], c["levels"]), []).append((name, c))
    return out


@pytest.mark.parametrize("mem", ["host", "device"])
def test_extract_template_batch_equals_recorded_reference(ctx, mem):
    """Every add_template case of one geometry in one call, the refused views among the others, from host and from device frames."""
    seen = refused_among_others = 0
    for (w, h, levels), cases in _batches().items():
        bgrs, depths, masks = ([c[k] for _, c in cases] for k in ("bgr", "depth", "mask"))
        if mem == "device":
            bgrs, depths = [torch.from_numpy(b).cuda() for b in bgrs], [torch.from_numpy(d).cuda() for d in depths]
            masks = [None if m is None else torch.from_numpy(m).cuda() for m in masks]
            torch.cuda.synchronize()
        got = ctx.extract_template_batch(bgrs, depths, masks, levels, mem=L.FL_MEM_DEVICE if mem == "device" else L.FL_MEM_HOST)
        assert len(got) == len(cases)
        for (name, c), g in zip(cases, got):
            _against_extract_record(RC.add_template_record(c, KernelExtractBackend.as_record(g)), "add_template", name)
        none = [g is None for g in got]
        refused_among_others += any(none[i] and not none[i - 1] and not none[i + 1] for i in range(1, len(none) - 1))
        seen += len(cases)
    assert seen == len(EXTRACT_GROUPS["add_template"][0]) and refused_among_others >= 1


@pytest.mark.parametrize("group", ["select", "orientations", "add_template", "extract_color", "extract_depth"])
def test_extraction_equals_live_reference(ctx, group):
    """The same cases against the compiled reference itself."""
    ref, K = R.require(False), KernelExtractBackend(ctx)
    for name, case in EXTRACT_GROUPS[group][0]:
        if group == "select":
            a, b = RC.select_record(case, K.select_job(case)), RC.compute_select(ref, case)
        elif group == "orientations":
            b = RC.compute_orientations(ref, case)
            a = {"img_q": ctx.quantized_orientations(RC.orientation_input(case), 10.0)}
            assert RC.same(a, {"img_q": b["img_q"]}) is None, (name, "img_q of the public entry point")
            a = RC.compute_orientations(K, case)               # extraction's build: labels and magnitude
        elif group == "add_template":
            a, b = RC.compute_add_template(K, case), RC.compute_add_template(ref, case)
        else:
            fn = EXTRACT_GROUPS[group][1]
            a, b = fn(K, case), fn(ref, case)
        assert RC.same(a, b) is None, (name, RC.same(a, b))
