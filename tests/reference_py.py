"""ctypes binding of oracle/_ref/libfealess_ref{,_simd}.so -- the reference's own linemod.cpp -- and of
oracle/_ref/libfealess_ref_icp.so -- its ICP sources (ICP.cpp, common.cpp, depth_to_3d.cpp, detection.cpp, NMS.cpp) --, both compiled
against the container-only opencv2/ stand-in of oracle/ref/ (the twin of tests/oracle_py.py, entry point for entry point).

TEST INFRASTRUCTURE.  The libraries are built by `make -C oracle/ref` (which __graft_entry__.build() runs when a reference
tree is there) and never committed; a machine without the reference tree receives them ready built or does without.
"""
import ctypes as C
import os

import numpy as np

from oracle_py import FEAT_DTYPE, MATCH_DTYPE, TEMPL_DTYPE, OrcBank, OrcDetectionResult, OrcIcpResult, _banks, _cloud, _icp_dict, _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")


def reference_root():
    """FEALESS_REFERENCE_ROOT, or a reference/ directory beside the repository root."""
    return os.environ.get("FEALESS_REFERENCE_ROOT") or os.path.join(os.path.dirname(ROOT), "reference")


def reference_present():
    return os.path.exists(os.path.join(reference_root(), "linemod", "linemod.cpp"))


def lib_path(simd=False):
    return os.path.join(REF_DIR, "libfealess_ref_simd.so" if simd else "libfealess_ref.so")


class Ref:
    """One loaded build of the compiled reference."""

    def __init__(self, simd):
        self.simd = bool(simd)
        self.l = C.CDLL(lib_path(simd))
        assert self.l.ref_is_simd() == int(self.simd)

    def spread(self, q, T):
        q = np.ascontiguousarray(q, np.uint8)
        out = np.zeros_like(q)
        self._ok(self.l.ref_spread(_p(q), q.shape[1], q.shape[0], T, _p(out)))
        return out

    def response_maps(self, s):
        s = np.ascontiguousarray(s, np.uint8)
        out = np.zeros((8,) + s.shape, np.uint8)
        self._ok(self.l.ref_response_maps(_p(s), s.shape[1], s.shape[0], _p(out)))
        return out

    def linearize(self, response_map, T):
        m = np.ascontiguousarray(response_map, np.uint8)
        h, w = m.shape
        out = np.zeros((T * T, (w // T) * (h // T)), np.uint8)
        self._ok(self.l.ref_linearize(_p(m), w, h, T, _p(out)))
        return out

    def build_linear_memories(self, q, T, stride):
        """spread -> computeResponseMaps -> linearize, laid out like oracle_py.build_linear_memories: (8, stride), the
        T*T linear memories of a label back to back and zeros behind them."""
        maps = self.response_maps(self.spread(q, T))
        out = np.zeros((8, stride), np.uint8)
        for l in range(8):
            lin = self.linearize(maps[l], T)
            out[l, :lin.size] = lin.ravel()
        return out

    def similarity(self, lm8, templ, feats, w, h, T):
        t = np.ascontiguousarray(np.atleast_1d(templ), TEMPL_DTYPE)
        f = np.ascontiguousarray(feats, FEAT_DTYPE)
        lm8 = np.ascontiguousarray(lm8, np.uint8)
        out = np.zeros((h // T, w // T), np.uint8)
        self._ok(self.l.ref_similarity(_p(lm8), C.c_size_t(lm8.shape[1]), _p(t), _p(f), w, h, T, _p(out)))
        return out

    def similarity_local(self, lm8, templ, feats, w, h, T, cx, cy):
        t = np.ascontiguousarray(np.atleast_1d(templ), TEMPL_DTYPE)
        f = np.ascontiguousarray(feats, FEAT_DTYPE)
        lm8 = np.ascontiguousarray(lm8, np.uint8)
        out = np.zeros((16, 16), np.uint8)
        self._ok(self.l.ref_similarity_local(_p(lm8), C.c_size_t(lm8.shape[1]), _p(t), _p(f), w, h, T, cx, cy, _p(out)))
        return out

    def add_similarities(self, sims):
        sims = [np.ascontiguousarray(s, np.uint8) for s in sims]
        ptrs = (C.c_void_p * len(sims))(*[s.ctypes.data for s in sims])
        out = np.zeros(sims[0].shape, np.uint16)
        self._ok(self.l.ref_add_similarities(ptrs, len(sims), sims[0].shape[0], sims[0].shape[1], _p(out)))
        return out

    def match_quantized(self, quantized, w0, h0, T_pyramid, banks, threshold, class_ids=()):
        """banks: TemplateBanks in the order they are to be inserted (any order; the reference keeps them in a std::map).
        Returns (final, raw): Detector::match's own list and the list before std::sort / std::unique, both with
        class_idx = index into `banks`."""
        qs = [np.ascontiguousarray(q, np.uint8) for q in quantized]
        levels = len(T_pyramid)
        M = len(qs) // levels
        ptrs = (C.c_void_p * len(qs))(*[q.ctypes.data for q in qs])
        T = (C.c_int * levels)(*T_pyramid)
        arr, keep = _banks(banks)
        names = (C.c_char_p * len(banks))(*[b.class_id.encode() for b in banks])
        flt = (C.c_char_p * max(1, len(class_ids)))(*[c.encode() for c in class_ids])
        cap = 1 << 16
        while True:
            fin, raw = np.zeros(cap, MATCH_DTYPE), np.zeros(cap, MATCH_DTYPE)
            nf, nr = C.c_int(0), C.c_int(0)
            self._ok(self.l.ref_match_quantized(ptrs, w0, h0, levels, M, T, arr, names, len(banks), flt, len(class_ids),
                                                C.c_float(threshold), _p(fin), cap, C.byref(nf), _p(raw), cap, C.byref(nr)))
            if max(nf.value, nr.value) <= cap:
                return fin[:nf.value], raw[:nr.value]
            cap = max(nf.value, nr.value)

    def quantized_normals(self, depth, distance_threshold=2000, difference_threshold=50):
        d = np.ascontiguousarray(depth, np.uint16)
        out = np.zeros(d.shape, np.uint8)
        self._ok(self.l.ref_quantized_normals(_p(d), d.shape[1], d.shape[0], distance_threshold, difference_threshold, _p(out)))
        return out

    def hysteresis_gradient(self, magnitude, angle, threshold):
        mg = np.ascontiguousarray(magnitude, np.float32)
        ag = np.ascontiguousarray(angle, np.float32)
        out = np.zeros(mg.shape, np.uint8)
        self._ok(self.l.ref_hysteresis_gradient(_p(mg), _p(ag), mg.shape[1], mg.shape[0], C.c_float(threshold), _p(out)))
        return out

    def crop_templates(self, templates, feats):
        t = np.array(templates, TEMPL_DTYPE)
        f = np.array(feats, FEAT_DTYPE)
        bb = (C.c_int * 4)()
        self._ok(self.l.ref_crop_templates(_p(t), len(t), _p(f), bb))
        return t, f, tuple(bb)

    # ---- template extraction: 1 = features, 0 = refused (too few candidates), -1 = the reference threw ----
    def _taken(self, rc, out):
        if rc < 0:
            raise AssertionError("reference CV_Assert")
        return out if rc else None

    def select_scattered_list(self, x, y, label, score, num_features, distance):
        x, y, label = (np.ascontiguousarray(a, np.int32) for a in (x, y, label))
        score = np.ascontiguousarray(score, np.float32)
        out = np.zeros(num_features, FEAT_DTYPE)
        return self._taken(self.l.ref_select_scattered_list(_p(x), _p(y), _p(label), _p(score), len(x), num_features, C.c_float(distance),
                                                            _p(out)), out)

    def extract_template_color(self, quantized, magnitude, mask, strong_threshold, num_features):
        q = np.ascontiguousarray(quantized, np.uint8)
        mg = np.ascontiguousarray(magnitude, np.float32)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        out = np.zeros(num_features, FEAT_DTYPE)
        return self._taken(self.l.ref_extract_template_color(_p(q), _p(mg), None if mk is None else _p(mk), q.shape[1], q.shape[0],
                                                             C.c_float(strong_threshold), num_features, _p(out)), out)

    def extract_template_depth(self, normal, mask, extract_threshold, num_features):
        q = np.ascontiguousarray(normal, np.uint8)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        out = np.zeros(num_features, FEAT_DTYPE)
        return self._taken(self.l.ref_extract_template_depth(_p(q), None if mk is None else _p(mk), q.shape[1], q.shape[0], extract_threshold,
                                                             num_features, _p(out)), out)

    def quantized_orientations_mag(self, bgr, weak_threshold=10.0):
        b = np.ascontiguousarray(bgr, np.uint8)
        out, mag = np.zeros(b.shape[:2], np.uint8), np.zeros(b.shape[:2], np.float32)
        self._ok(self.l.ref_quantized_orientations(_p(b), b.shape[1], b.shape[0], C.c_float(weak_threshold), _p(out), _p(mag)))
        return out, mag

    def add_template(self, bgr, depth, mask, levels):
        """As oracle_py.add_template: (templates, features per template, bb), or None where addTemplate returned -1."""
        b = np.ascontiguousarray(bgr, np.uint8)
        d = np.ascontiguousarray(depth, np.uint16)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        h, w = d.shape
        t = np.zeros(levels * 2, TEMPL_DTYPE)
        f = np.zeros(levels * 2 * 63, FEAT_DTYPE)
        bb = (C.c_int * 4)()
        if self.l.ref_add_template(_p(b), _p(d), None if mk is None else _p(mk), w, h, levels, _p(t), _p(f), bb):
            return None
        return t, [f[t[k]["feat_begin"]:t[k]["feat_begin"] + t[k]["feat_count"]].copy() for k in range(levels * 2)], tuple(bb)

    @staticmethod
    def _ok(rc):
        if rc:
            raise AssertionError("reference CV_Assert")


ICP_LIB_PATH = os.path.join(REF_DIR, "libfealess_ref_icp.so")


class RefIcp:
    """The loaded build of the reference's ICP sources, under the names and result layouts of oracle_py."""

    def __init__(self):
        self.l = C.CDLL(ICP_LIB_PATH)
        self.l.ref_l2dist_clouds.restype = C.c_float

    def icp(self, ref, model, icp_it_thr=4, dist_mean_thr=0.0, dist_diff_thr=0.0):
        """As oracle_py.icp; n_corr_last is not observable in the reference (-1)."""
        ref, model = _cloud(ref), _cloud(model)
        res = OrcIcpResult()
        rc = self.l.ref_icp(_p(ref), len(ref), _p(model), len(model), icp_it_thr, C.c_float(dist_mean_thr), C.c_float(dist_diff_thr),
                            C.byref(res))
        d = _icp_dict(res)
        d["rc"] = rc
        return d

    def get_mean(self, pts):
        pts = _cloud(pts)
        out = np.zeros(3, np.float32)
        self.l.ref_get_mean(_p(pts), len(pts), _p(out))
        return out

    def l2dist_clouds(self, model, ref, dist_thr=np.finfo(np.float32).max):
        model, ref = _cloud(model), _cloud(ref)
        assert len(ref) >= len(model)
        dm = C.c_float(0)
        ratio = self.l.ref_l2dist_clouds(_p(model), len(model), _p(ref), len(ref), C.c_float(dist_thr), C.byref(dm))
        return np.float32(ratio), np.float32(dm.value)

    def copy_points(self, src):
        src = _cloud(src)
        out = np.full_like(src, 7.0)
        self.l.ref_copy_points(_p(src), len(src), _p(out))
        return out

    def transform_points(self, src, R, T, in_place):
        src = _cloud(src)
        out = np.full_like(src, 7.0)
        R, T = np.ascontiguousarray(R, np.float32), np.ascontiguousarray(T, np.float32)
        self.l.ref_transform_points(_p(src), len(src), _p(R), _p(T), _p(out), int(in_place))
        return out

    def points_corresponding(self, ref, model, dist_thr, use_kdtree=True):
        ref, model = _cloud(ref), _cloud(model)
        cr, cm = np.zeros_like(model), np.zeros_like(model)
        n = self.l.ref_points_corresponding(_p(ref), len(ref), _p(model), len(model), C.c_float(dist_thr), _p(cr), _p(cm))
        return cr[:n].copy(), cm[:n].copy()

    def depth_to_3d(self, depth, fx, fy, cx, cy):
        d = np.ascontiguousarray(depth, np.uint16)
        out = np.zeros(d.shape + (3,), np.float32)
        if self.l.ref_depth_to_3d(_p(d), d.shape[1], d.shape[0], C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy), _p(out)):
            raise AssertionError("reference CV_Assert")
        return out

    def detection(self, model_depth_mm, scene_depth_mm, K, rect_model, rect_ref, icp_it_thr, dist_mean_thr, dist_diff_thr, r_match, t_match):
        md = np.ascontiguousarray(model_depth_mm, np.uint16)
        sd = np.ascontiguousarray(scene_depth_mm, np.uint16)
        h, w = sd.shape
        rm = (C.c_int * 4)(*[int(v) for v in rect_model])
        rr = (C.c_int * 4)(*[int(v) for v in rect_ref])
        rmat = (C.c_float * 9)(*np.asarray(r_match, np.float32).ravel())
        tvec = (C.c_float * 3)(*np.asarray(t_match, np.float32).ravel())
        res = OrcDetectionResult()
        rc = self.l.ref_detection(_p(md), _p(sd), w, h, C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]), rm, rr,
                                  icp_it_thr, C.c_float(dist_mean_thr), C.c_float(dist_diff_thr), rmat, tvec, C.byref(res))
        return dict(rc=rc, R_final=np.array(res.R_final, np.float32).reshape(3, 3), T_final=np.array(res.T_final, np.float32),
                    icp=_icp_dict(res.icp), n_points=int(res.n_points))

    def nms(self, t, n_points, icp_dist, th_obj_dist):
        n = len(n_points)
        t = np.ascontiguousarray(np.asarray(t, np.float32).reshape(-1, 3))
        npts = np.ascontiguousarray(n_points, np.int32)
        dist = np.ascontiguousarray(icp_dist, np.float32)
        win = np.zeros(max(1, n), np.int32)
        nw = self.l.ref_nms(_p(t), _p(npts), _p(dist), n, C.c_float(th_obj_dist), _p(win))
        return [int(v) for v in win[:nw]]


_libs = {}


def lib(simd=False):
    """The loaded scalar (simd=False) or SSE2/SSE3/SSSE3 (simd=True) build; OSError when it is not built."""
    if simd not in _libs:
        _libs[simd] = Ref(simd)
    return _libs[simd]


def icp_lib():
    """The loaded build of the ICP sources; OSError when it is not built."""
    if "icp" not in _libs:
        _libs["icp"] = RefIcp()
    return _libs["icp"]


def _require(path, load):
    import pytest
    if os.path.exists(path):
        return load()
    if not reference_present():
        pytest.skip(f"{os.path.relpath(path, ROOT)} is not built and there is no reference tree at "
                    f"{reference_root()} to build it from")
    pytest.fail(f"{os.path.relpath(path, ROOT)} is missing although the reference tree is at {reference_root()}: "
                "build first (python -c 'import __graft_entry__ as g; g.build()' or make -C oracle/ref)")


def require(simd=False):
    """lib(simd) for a test.  A missing library means: skip where there is no reference tree to build it from, fail where
    there is one (the build was forgotten)."""
    return _require(lib_path(simd), lambda: lib(simd))


def require_icp():
    """icp_lib() for a test, with require()'s meaning of a missing library."""
    return _require(ICP_LIB_PATH, icp_lib)
