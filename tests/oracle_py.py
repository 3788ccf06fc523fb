"""ctypes binding of oracle/liboracle.so -- the CPU restatement of the reference hot path.

TEST INFRASTRUCTURE.  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
import this module; the product (fealess_amd) never does.  Its LINEMOD half and its ICP half are compared bit for bit with the
reference's own compiled code through tests/reference_py.py, the twin of this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
LIB_PATH = os.path.join(ORACLE_DIR, "liboracle.so")

MATCH_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("similarity", "<f4"), ("class_idx", "<i4"),
                        ("template_id", "<i4")])


class OrcBank(C.Structure):
    _fields_ = [("n_pyramids", C.c_int32), ("levels", C.c_int32), ("modalities", C.c_int32),
                ("templates", C.c_void_p), ("features", C.c_void_p)]


class OrcIcpResult(C.Structure):
    _fields_ = [("R", C.c_float * 9), ("T", C.c_float * 3), ("dist_mean", C.c_float), ("px_ratio", C.c_float),
                ("iters", C.c_int32), ("n_corr_last", C.c_int32)]


class OrcDetectionResult(C.Structure):
    _fields_ = [("R_final", C.c_float * 9), ("T_final", C.c_float * 3), ("icp", OrcIcpResult), ("n_points", C.c_int32)]


class OrcMatch(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("similarity", C.c_float), ("class_idx", C.c_int32),
                ("template_id", C.c_int32)]


class OrcRecognitionResult(C.Structure):
    _fields_ = [("found", C.c_int32), ("best", OrcMatch), ("pose", C.c_float * 16), ("det", OrcDetectionResult),
                ("n_matches", C.c_int32)]


_lib = None


def build():
    subprocess.check_call(["make", "-s", "-C", ORACLE_DIR])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        _lib = C.CDLL(LIB_PATH)
        _lib.orc_lm_label_stride.restype = C.c_size_t
        _lib.orc_fast_atan2.restype = C.c_float
        _lib.orc_fast_atan2.argtypes = [C.c_float, C.c_float]
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def similarity_lut():
    out = np.zeros(256, np.uint8)
    lib().orc_similarity_lut(_p(out))
    return out


def normal_lut():
    out = np.zeros(8000, np.uint8)
    lib().orc_normal_lut(_p(out))
    return out


def spread(q, T):
    q = np.ascontiguousarray(q, np.uint8)
    out = np.zeros_like(q)
    lib().orc_spread(_p(q), q.shape[1], q.shape[0], T, _p(out))
    return out


def response_maps(s):
    s = np.ascontiguousarray(s, np.uint8)
    out = np.zeros((8,) + s.shape, np.uint8)
    if lib().orc_response_maps(_p(s), s.shape[1], s.shape[0], _p(out)):
        raise AssertionError("reference CV_Assert")
    return out


def build_linear_memories(q, T):
    q = np.ascontiguousarray(q, np.uint8)
    h, w = q.shape
    stride = lib().orc_lm_label_stride(w, h, T)
    out = np.zeros(8 * stride, np.uint8)
    rc = lib().orc_build_linear_memories(_p(q), w, h, T, _p(out))
    if rc:
        raise AssertionError("reference CV_Assert")
    return out.reshape(8, stride)


def _banks(banks):
    """banks: list of fealess_amd.bank.TemplateBank (sorted by class id) -> (OrcBank array, keepalive)"""
    arr = (OrcBank * len(banks))()
    keep = []
    for i, b in enumerate(banks):
        t, f, p = b.arrays()
        keep.append((t, f, p))
        arr[i] = OrcBank(b.n_pyramids, b.levels, b.modalities, t.ctypes.data, f.ctypes.data)
    return arr, keep


def total_similarity(lms, bank, pyramid, w, h, T):
    """lms: list over modalities of (8, stride) arrays of the coarsest level."""
    arr, keep = _banks([bank])
    ptrs = (C.c_void_p * len(lms))(*[l.ctypes.data for l in lms])
    out = np.zeros((h // T, w // T), np.uint16)
    rc = lib().orc_total_similarity(ptrs, C.byref(arr[0]), pyramid, w, h, T, _p(out))
    if rc:
        raise AssertionError("reference CV_Assert")
    return out


def match_quantized(quantized, w0, h0, T_pyramid, banks, threshold, cap=1 << 20):
    qs = [np.ascontiguousarray(q, np.uint8) for q in quantized]
    levels = len(T_pyramid)
    M = len(qs) // levels
    ptrs = (C.c_void_p * len(qs))(*[q.ctypes.data for q in qs])
    T = (C.c_int * levels)(*T_pyramid)
    arr, keep = _banks(banks)
    out = np.zeros(cap, MATCH_DTYPE)
    nt = C.c_int(0)
    n = lib().orc_match_quantized(ptrs, w0, h0, levels, M, T, arr, len(banks), C.c_float(threshold), _p(out), cap,
                                  C.byref(nt))
    if n < 0:
        raise AssertionError("reference CV_Assert")
    return out[:n], nt.value


def quantized_normals(depth, distance_threshold=2000, difference_threshold=50):
    d = np.ascontiguousarray(depth, np.uint16)
    out = np.zeros(d.shape, np.uint8)
    lib().orc_quantized_normals(_p(d), d.shape[1], d.shape[0], distance_threshold, difference_threshold, _p(out))
    return out


def quantized_orientations(bgr, weak_threshold=10.0):
    b = np.ascontiguousarray(bgr, np.uint8)
    out = np.zeros(b.shape[:2], np.uint8)
    lib().orc_quantized_orientations(_p(b), b.shape[1], b.shape[0], C.c_float(weak_threshold), _p(out), None)
    return out


def pyrdown_bgr(bgr):
    b = np.ascontiguousarray(bgr, np.uint8)
    h, w = b.shape[:2]
    out = np.zeros((h // 2, w // 2, 3), np.uint8)
    lib().orc_pyrdown_bgr(_p(b), w, h, _p(out))
    return out


def resize_nn_half(q):
    q = np.ascontiguousarray(q, np.uint8)
    h, w = q.shape
    out = np.zeros((h // 2, w // 2), np.uint8)
    lib().orc_resize_nn_half(_p(q), w, h, _p(out))
    return out


def resize_linear_u8(img, dw, dh):
    a = np.ascontiguousarray(img, np.uint8)
    sh, sw = a.shape[:2]
    cn = 1 if a.ndim == 2 else a.shape[2]
    out = np.zeros((dh, dw) + (() if a.ndim == 2 else (cn,)), np.uint8)
    lib().orc_resize_linear_u8(_p(a), sw, sh, cn, _p(out), dw, dh)
    return out


def resize_linear_u16(img, dw, dh):
    a = np.ascontiguousarray(img, np.uint16)
    sh, sw = a.shape
    out = np.zeros((dh, dw), np.uint16)
    lib().orc_resize_linear_u16(_p(a), sw, sh, _p(out), dw, dh)
    return out


def erode_rect(mask, iterations):
    m = np.ascontiguousarray(mask, np.uint8)
    out = np.zeros_like(m)
    lib().orc_erode_rect(_p(m), m.shape[1], m.shape[0], iterations, _p(out))
    return out


def distance_transform_c3(img):
    m = np.ascontiguousarray(img, np.uint8)
    out = np.zeros(m.shape, np.float32)
    lib().orc_distance_transform_c3(_p(m), m.shape[1], m.shape[0], _p(out))
    return out


FEAT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("label", "<i4")])
TEMPL_DTYPE = np.dtype([("width", "<i4"), ("height", "<i4"), ("offset_x", "<i4"), ("offset_y", "<i4"),
                        ("pyramid_level", "<i4"), ("feat_begin", "<i4"), ("feat_count", "<i4")])


def extract_template_color(quantized, magnitude, mask, strong_threshold, num_features):
    q = np.ascontiguousarray(quantized, np.uint8)
    mg = np.ascontiguousarray(magnitude, np.float32)
    mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    out = np.zeros(num_features, FEAT_DTYPE)
    ok = lib().orc_extract_template_color(_p(q), _p(mg), None if mk is None else _p(mk), q.shape[1], q.shape[0],
                                          C.c_float(strong_threshold), num_features, _p(out))
    return out if ok else None


def extract_template_depth(normal, mask, extract_threshold, num_features):
    q = np.ascontiguousarray(normal, np.uint8)
    mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    out = np.zeros(num_features, FEAT_DTYPE)
    ok = lib().orc_extract_template_depth(_p(q), None if mk is None else _p(mk), q.shape[1], q.shape[0], extract_threshold,
                                          num_features, _p(out))
    return out if ok else None


def select_scattered_list(x, y, label, score, num_features, distance):
    """stable sort by Candidate::operator< + selectScatteredFeatures on a candidate list in arrival order; None when the
    list is shorter than num_features."""
    x, y, label = (np.ascontiguousarray(a, np.int32) for a in (x, y, label))
    score = np.ascontiguousarray(score, np.float32)
    out = np.zeros(num_features, FEAT_DTYPE)
    ok = lib().orc_select_scattered_list(_p(x), _p(y), _p(label), _p(score), len(x), num_features, C.c_float(distance), _p(out))
    return out if ok else None


def sobel3_bgr(bgr, vertical):
    """cv::Sobel(CV_16S, ksize 3, BORDER_REPLICATE) of an (h, w, 3) u8 image: d/dx (vertical = False) or d/dy, int16."""
    b = np.ascontiguousarray(bgr, np.uint8)
    out = np.zeros(b.shape, np.int16)
    lib().orc_sobel3_bgr(_p(b), b.shape[1], b.shape[0], int(bool(vertical)), _p(out))
    return out


def quantized_orientations_mag(bgr, weak_threshold=10.0):
    b = np.ascontiguousarray(bgr, np.uint8)
    out = np.zeros(b.shape[:2], np.uint8)
    mag = np.zeros(b.shape[:2], np.float32)
    lib().orc_quantized_orientations(_p(b), b.shape[1], b.shape[0], C.c_float(weak_threshold), _p(out), _p(mag))
    return out, mag


def add_template(bgr, depth, mask, levels):
    """Detector::addTemplate: returns (templates[levels*2] TEMPL_DTYPE, features list per template, bb) or None."""
    b = np.ascontiguousarray(bgr, np.uint8)
    d = np.ascontiguousarray(depth, np.uint16)
    mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    h, w = d.shape
    t = np.zeros(levels * 2, TEMPL_DTYPE)
    f = np.zeros(levels * 2 * 63, FEAT_DTYPE)
    bb = (C.c_int * 4)()
    rc = lib().orc_add_template(_p(b), _p(d), None if mk is None else _p(mk), w, h, levels, _p(t), _p(f), bb)
    if rc:
        return None
    feats = [f[t[k]["feat_begin"]:t[k]["feat_begin"] + t[k]["feat_count"]].copy() for k in range(levels * 2)]
    return t, feats, tuple(bb)


def quantize_pyramid(bgr, depth, levels):
    """The two default modalities' quantized images per level, order [l*2 + m]."""
    out = []
    src = np.ascontiguousarray(bgr, np.uint8)
    qn = quantized_normals(depth)
    for l in range(levels):
        if l > 0:
            src = pyrdown_bgr(src)
            qn = resize_nn_half(qn)
        out.append(quantized_orientations(src))
        out.append(qn)
    return out


def match_images(bgr, depth, T_pyramid, banks, threshold, cap=1 << 20, masks=None):
    b = np.ascontiguousarray(bgr, np.uint8)
    d = np.ascontiguousarray(depth, np.uint16)
    h, w = d.shape
    levels = len(T_pyramid)
    T = (C.c_int * levels)(*T_pyramid)
    arr, keep = _banks(banks)
    out = np.zeros(cap, MATCH_DTYPE)
    nt = C.c_int(0)
    mks = [None, None]
    if masks is not None:
        mks = [None if m is None else np.ascontiguousarray(m, np.uint8) for m in masks]
    n = lib().orc_match_images_masked(_p(b), _p(d), w, h, levels, T, arr, len(banks), C.c_float(threshold),
                                      None if mks[0] is None else _p(mks[0]), None if mks[1] is None else _p(mks[1]),
                                      _p(out), cap, C.byref(nt), None)
    if n < 0:
        raise AssertionError("reference CV_Assert")
    return out[:n], nt.value


def depth_to_3d(depth, fx, fy, cx, cy):
    d = np.ascontiguousarray(depth, np.uint16)
    out = np.zeros(d.shape + (3,), np.float32)
    lib().orc_depth_to_3d(_p(d), d.shape[1], d.shape[0], C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy),
                          _p(out))
    return out


def svd3(A):
    A = np.ascontiguousarray(A, np.float32)
    w = np.zeros(3, np.float32)
    u = np.zeros((3, 3), np.float32)
    vt = np.zeros((3, 3), np.float32)
    lib().orc_svd3(_p(A), _p(w), _p(u), _p(vt))
    return w, u, vt


def _icp_dict(r):
    return dict(R=np.array(r.R, np.float32).reshape(3, 3), T=np.array(r.T, np.float32), dist_mean=np.float32(r.dist_mean),
                px_ratio=np.float32(r.px_ratio), iters=int(r.iters), n_corr_last=int(r.n_corr_last))


def icp(ref, model, icp_it_thr=4, dist_mean_thr=0.0, dist_diff_thr=0.0, accum64=False, use_kdtree=True, trace=False):
    ref = np.ascontiguousarray(ref, np.float32).reshape(-1, 3)
    model = np.ascontiguousarray(model, np.float32).reshape(-1, 3)
    res = OrcIcpResult()
    tr = np.full((max(icp_it_thr, 1), 23), np.nan, np.float32)
    rc = lib().orc_icp(_p(ref), len(ref), _p(model), len(model), icp_it_thr, C.c_float(dist_mean_thr),
                       C.c_float(dist_diff_thr), int(accum64), int(use_kdtree), C.byref(res),
                       _p(tr) if trace else None, icp_it_thr if trace else 0)
    d = _icp_dict(res)
    d["rc"] = rc
    if trace:
        d["trace"] = tr
    return d


def detection(model_depth_mm, scene_depth_mm, K, rect_model, rect_ref, icp_it_thr, dist_mean_thr, dist_diff_thr,
              r_match, t_match, accum64=False, use_kdtree=True):
    md = np.ascontiguousarray(model_depth_mm, np.uint16)
    sd = np.ascontiguousarray(scene_depth_mm, np.uint16)
    h, w = sd.shape
    rm = (C.c_int * 4)(*[int(v) for v in rect_model])
    rr = (C.c_int * 4)(*[int(v) for v in rect_ref])
    rmat = (C.c_float * 9)(*np.asarray(r_match, np.float32).ravel())
    tvec = (C.c_float * 3)(*np.asarray(t_match, np.float32).ravel())
    res = OrcDetectionResult()
    rc = lib().orc_detection(_p(md), _p(sd), w, h, C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]),
                             rm, rr, icp_it_thr, C.c_float(dist_mean_thr), C.c_float(dist_diff_thr), rmat, tvec,
                             int(accum64), int(use_kdtree), C.byref(res))
    return dict(rc=rc, R_final=np.array(res.R_final, np.float32).reshape(3, 3), T_final=np.array(res.T_final, np.float32),
                icp=_icp_dict(res.icp), n_points=int(res.n_points))


def recognition(bgr, depth, K, T_pyramid, bank, threshold=75.0, icp_it_thr=10, dist_mean_thr=0.5, dist_diff_thr=0.01,
                accum64=False, use_kdtree=True):
    b = np.ascontiguousarray(bgr, np.uint8)
    d = np.ascontiguousarray(depth, np.uint16)
    h, w = d.shape
    levels = len(T_pyramid)
    T = (C.c_int * levels)(*T_pyramid)
    arr, keep = _banks([bank])
    t, f, p = keep[0]
    zero = np.zeros((h, w), np.uint16)    # pyramids without a depth render (bank.py): an empty render here; the product reports
                                          # FL_ERR_STATE for them, and refine_match / recognition_banks say no_render
    mds = [zero if m is None else np.ascontiguousarray(m, np.uint16) for m in bank.model_depths]
    mds = mds + [zero] * (bank.n_pyramids - len(mds))
    mptr = (C.c_void_p * len(mds))(*[m.ctypes.data for m in mds])
    res = OrcRecognitionResult()
    rc = lib().orc_recognition(_p(b), _p(d), w, h, C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]),
                               levels, T, C.byref(arr[0]), _p(p), mptr, C.c_float(threshold), icp_it_thr,
                               C.c_float(dist_mean_thr), C.c_float(dist_diff_thr), int(accum64), int(use_kdtree),
                               C.byref(res))
    return dict(rc=rc, found=int(res.found), n_matches=int(res.n_matches),
                best=dict(x=res.best.x, y=res.best.y, similarity=np.float32(res.best.similarity),
                          class_idx=res.best.class_idx, template_id=res.best.template_id),
                pose=np.array(res.pose, np.float32).reshape(4, 4),
                det=dict(R_final=np.array(res.det.R_final, np.float32).reshape(3, 3),
                         T_final=np.array(res.det.T_final, np.float32), icp=_icp_dict(res.det.icp),
                         n_points=int(res.det.n_points)))


def last_stage_ms():
    """(linemod_ms, icp_ms) of the calling thread's last recognition(): the reference's own timer points
    ("Time of linemod" / "Time of ICP", CadReco/obj_reco_lmicp.cpp:125,202)."""
    out = (C.c_double * 2)()
    lib().orc_last_stage_ms(out)
    return float(out[0]), float(out[1])


def _reco_dict(res, rc=0):
    return dict(rc=rc, found=int(res.found), n_matches=int(res.n_matches),
                best=dict(x=res.best.x, y=res.best.y, similarity=np.float32(res.best.similarity),
                          class_idx=res.best.class_idx, template_id=res.best.template_id),
                pose=np.array(res.pose, np.float32).reshape(4, 4),
                det=dict(R_final=np.array(res.det.R_final, np.float32).reshape(3, 3),
                         T_final=np.array(res.det.T_final, np.float32), icp=_icp_dict(res.det.icp),
                         n_points=int(res.det.n_points)))


def recognition_topk(bgr, depth, K, T_pyramid, bank, k, threshold=75.0, icp_it_thr=10, dist_mean_thr=0.5, dist_diff_thr=0.01,
                     nms_dist=None, accum64=False):
    """First k matches refined like Recognition() does for matches[0]; with nms_dist also the NMS winners."""
    b = np.ascontiguousarray(bgr, np.uint8)
    d = np.ascontiguousarray(depth, np.uint16)
    h, w = d.shape
    levels = len(T_pyramid)
    T = (C.c_int * levels)(*T_pyramid)
    arr, keep = _banks([bank])
    t, f, p = keep[0]
    zero = np.zeros((h, w), np.uint16)    # pyramids without a depth render (bank.py): an empty render here; the product reports
                                          # FL_ERR_STATE for them, and refine_match / recognition_banks say no_render
    mds = [zero if m is None else np.ascontiguousarray(m, np.uint16) for m in bank.model_depths]
    mds = mds + [zero] * (bank.n_pyramids - len(mds))
    mptr = (C.c_void_p * len(mds))(*[m.ctypes.data for m in mds])
    res = (OrcRecognitionResult * k)()
    n = lib().orc_recognition_topk(_p(b), _p(d), w, h, C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]),
                                   levels, T, C.byref(arr[0]), _p(p), mptr, C.c_float(threshold), icp_it_thr,
                                   C.c_float(dist_mean_thr), C.c_float(dist_diff_thr), int(accum64), 1, k, res)
    if n < 0:
        raise AssertionError("reference CV_Assert")
    out = [_reco_dict(res[i]) for i in range(n)]
    if nms_dist is None:
        return out
    win = (C.c_int * max(1, n))()
    nw = lib().orc_nms(res, n, C.c_float(nms_dist), win)
    return out, [int(win[i]) for i in range(nw)]


def _refine_into(res, depth, K, bank, match, icp_it_thr, dist_mean_thr, dist_diff_thr, accum64):
    """orc_recognition_refine of `match` (template_id local to `bank`) into the OrcRecognitionResult `res`.  Returns False,
    with res zero but for `best`, where the pyramid has no depth render: the reference finds no depth/<id>.png to read."""
    d = np.ascontiguousarray(depth, np.uint16)
    h, w = d.shape
    tid = int(match["template_id"])
    m = OrcMatch(int(match["x"]), int(match["y"]), float(match["similarity"]), int(match["class_idx"]), tid)
    if not 0 <= tid < bank.n_pyramids:
        raise IndexError("template %d is not in bank %r" % (tid, bank.class_id))
    md = bank.model_depths[tid] if tid < len(bank.model_depths) else None
    if md is None:
        C.memset(C.byref(res), 0, C.sizeof(res))
        res.best = m
        return False
    md = np.ascontiguousarray(md, np.uint16)
    assert md.shape == (h, w)
    arr, keep = _banks([bank])
    p = keep[0][2]
    mptr = (C.c_void_p * bank.n_pyramids)()          # recognition_refine reads the named pyramid's render only
    mptr[tid] = md.ctypes.data
    lib().orc_recognition_refine(C.byref(m), _p(d), w, h, C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]),
                                 C.byref(arr[0]), _p(p), mptr, icp_it_thr, C.c_float(dist_mean_thr), C.c_float(dist_diff_thr),
                                 int(accum64), 1, C.byref(res))
    return True


def refine_match(depth, K, bank, match, icp_it_thr=10, dist_mean_thr=0.5, dist_diff_thr=0.01, accum64=False, n_matches=0):
    """The part of Recognition() behind the choice of the match, for a match the caller names: `match` is a MATCH_DTYPE
    record (or a dict with its fields) whose template_id is local to `bank`, the bank of its class; class_idx is carried
    along untouched.  A result dict as recognition_topk's, plus no_render: True (and found = 0) where the pyramid has no
    depth render, which the reference cannot refine."""
    res = OrcRecognitionResult()
    ok = _refine_into(res, depth, K, bank, match, icp_it_thr, dist_mean_thr, dist_diff_thr, accum64)
    res.n_matches = n_matches
    return dict(_reco_dict(res), no_render=not ok)


def recognition_banks(bgr, depth, K, T_pyramid, banks, k, threshold=75.0, icp_it_thr=10, dist_mean_thr=0.5, dist_diff_thr=0.01,
                      nms_dist=None, accum64=False, class_ids=()):
    """Recognition() over several classes on one detector: Detector::match over `banks` in the order of their class ids
    (std::map order), restricted to class_ids when that is not empty (a set; unknown ids match nothing, linemod.cpp:1418-1434),
    then refine_match of the first k matches.  class_idx is the index in the FULL sorted list whatever the filter.  A list of
    result dicts (n_matches = the length of the whole match list); with nms_dist also orc_nms's winners among them."""
    full = sorted(banks, key=lambda b: b.class_id)
    sel = [i for i, b in enumerate(full) if not class_ids or b.class_id in set(class_ids)]
    if sel:
        m, n_total = match_images(bgr, depth, T_pyramid, [full[i] for i in sel], threshold)
    else:
        m, n_total = np.zeros(0, MATCH_DTYPE), 0
    m = m[:k].copy()
    m["class_idx"] = np.asarray(sel, np.int32)[m["class_idx"]] if len(m) else m["class_idx"]
    res = (OrcRecognitionResult * max(1, len(m)))()
    out = []
    for r in range(len(m)):
        ok = _refine_into(res[r], depth, K, full[int(m["class_idx"][r])], m[r], icp_it_thr, dist_mean_thr, dist_diff_thr, accum64)
        res[r].n_matches = n_total
        out.append(dict(_reco_dict(res[r]), no_render=not ok))
    if nms_dist is None:
        return out
    win = (C.c_int * max(1, len(m)))()
    nw = lib().orc_nms(res, len(m), C.c_float(nms_dist), win)
    return out, [int(win[i]) for i in range(nw)]


def gaussian7_bgr(bgr):
    b = np.ascontiguousarray(bgr, np.uint8)
    out = np.zeros_like(b)
    lib().orc_gaussian7_bgr(_p(b), b.shape[1], b.shape[0], _p(out))
    return out


def median5(img):
    m = np.ascontiguousarray(img, np.uint8)
    out = np.zeros_like(m)
    lib().orc_median5(_p(m), m.shape[1], m.shape[0], _p(out))
    return out


# ---- stage entry points that tests/reference_py.py mirrors one to one ----------------------------------------------------
def linearize(response_map, T):
    """(T*T, (w/T)*(h/T)) linear memories of one response map; AssertionError where the reference's CV_Assert refuses."""
    m = np.ascontiguousarray(response_map, np.uint8)
    h, w = m.shape
    out = np.zeros((T * T, (w // T) * (h // T)), np.uint8)
    if lib().orc_linearize(_p(m), w, h, T, _p(out)):
        raise AssertionError("reference CV_Assert")
    return out


def similarity(lm8, templ, feats, w, h, T):
    """lm8: (8, stride) from build_linear_memories; templ: one TEMPL_DTYPE record; feats: FEAT_DTYPE array."""
    t = np.ascontiguousarray(np.atleast_1d(templ), TEMPL_DTYPE)
    f = np.ascontiguousarray(feats, FEAT_DTYPE)
    out = np.zeros((h // T, w // T), np.uint8)
    if lib().orc_similarity(_p(lm8), _p(t), _p(f), w, h, T, _p(out)):
        raise AssertionError("reference CV_Assert")
    return out


def similarity_local(lm8, templ, feats, w, h, T, cx, cy):
    t = np.ascontiguousarray(np.atleast_1d(templ), TEMPL_DTYPE)
    f = np.ascontiguousarray(feats, FEAT_DTYPE)
    out = np.zeros((16, 16), np.uint8)
    if lib().orc_similarity_local(_p(lm8), _p(t), _p(f), w, h, T, cx, cy, _p(out)):
        raise AssertionError("reference CV_Assert")
    return out


def hysteresis_gradient(magnitude, angle, threshold):
    mg = np.ascontiguousarray(magnitude, np.float32)
    ag = np.ascontiguousarray(angle, np.float32)
    out = np.zeros(mg.shape, np.uint8)
    lib().orc_hysteresis_gradient(_p(mg), _p(ag), mg.shape[1], mg.shape[0], C.c_float(threshold), _p(out))
    return out


def crop_templates(templates, feats):
    """cropTemplates on TEMPL_DTYPE / FEAT_DTYPE arrays: returns (templates, features, (x, y, w, h)), inputs untouched."""
    t = np.array(templates, TEMPL_DTYPE)
    f = np.array(feats, FEAT_DTYPE)
    bb = (C.c_int * 4)()
    lib().orc_crop_templates(_p(t), len(t), _p(f), bb)
    return t, f, tuple(bb)


# ---- ICP helpers and NMS under the signatures tests/reference_py.RefIcp mirrors one to one ------------------------------------
def _cloud(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def get_mean(pts):
    pts = _cloud(pts)
    out = np.zeros(3, np.float32)
    lib().orc_get_mean(_p(pts), len(pts), _p(out))
    return out


def l2dist_clouds(model, ref, dist_thr=np.finfo(np.float32).max):
    """getL2distClouds: (inlier ratio, dist_mean) as float32."""
    model, ref = _cloud(model), _cloud(ref)
    assert len(ref) >= len(model)
    lib().orc_l2dist_clouds.restype = C.c_float
    dm = C.c_float(0)
    ratio = lib().orc_l2dist_clouds(_p(model), len(model), _p(ref), C.c_float(dist_thr), C.byref(dm))
    return np.float32(ratio), np.float32(dm.value)


def copy_points(src):
    src = _cloud(src)
    out = np.full_like(src, 7.0)
    lib().orc_copy_points(_p(src), len(src), _p(out))
    return out


def transform_points(src, R, T, in_place):
    src = _cloud(src)
    out = np.full_like(src, 7.0)
    R, T = np.ascontiguousarray(R, np.float32), np.ascontiguousarray(T, np.float32)
    lib().orc_transform_points(_p(src), len(src), _p(R), _p(T), _p(out), int(in_place))
    return out


def points_corresponding(ref, model, dist_thr, use_kdtree=True):
    """PointsCorresponding on a prebuilt index: (cor_ref, cor_model)."""
    ref, model = _cloud(ref), _cloud(model)
    cr, cm = np.zeros_like(model), np.zeros_like(model)
    n = lib().orc_points_corresponding(_p(ref), len(ref), _p(model), len(model), C.c_float(dist_thr), int(use_kdtree), _p(cr), _p(cm))
    return cr[:n].copy(), cm[:n].copy()


def nn_tie_count(ref, queries):
    """Queries with two or more reference points at exactly the smallest float32 squared distance."""
    ref, q = _cloud(ref), _cloud(queries)
    return int(lib().orc_nn_tie_count(_p(ref), len(ref), _p(q), len(q)))


def nms(t, n_points, icp_dist, th_obj_dist):
    """nonMaximumSuppression over objects given by their translation, model point count and ICP distance: the winners."""
    n = len(n_points)
    res = (OrcRecognitionResult * max(1, n))()
    for i in range(n):
        res[i].det.T_final[:] = [float(v) for v in np.asarray(t, np.float32).reshape(-1, 3)[i]]
        res[i].det.n_points = int(n_points[i])
        res[i].det.icp.dist_mean = float(icp_dist[i])
    win = (C.c_int * max(1, n))()
    nw = lib().orc_nms(res, n, C.c_float(th_obj_dist), win)
    return [int(win[i]) for i in range(nw)]
