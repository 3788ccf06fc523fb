"""ctypes binding of oracle/_ref/libfealess_ref{,_simd}.so -- the reference's own linemod.cpp, compiled against the
container-only opencv2/ stand-in of oracle/ref/ (the twin of tests/oracle_py.py, entry point for entry point).

TEST INFRASTRUCTURE.  The libraries are built by `make -C oracle/ref` (which __graft_entry__.build() runs when a reference
tree is there) and never committed; a machine without the reference tree receives them ready built or does without.
"""
import ctypes as C
import os

import numpy as np

from oracle_py import FEAT_DTYPE, MATCH_DTYPE, TEMPL_DTYPE, OrcBank, _banks, _p

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

    @staticmethod
    def _ok(rc):
        if rc:
            raise AssertionError("reference CV_Assert")


_libs = {}


def lib(simd=False):
    """The loaded scalar (simd=False) or SSE2/SSE3/SSSE3 (simd=True) build; OSError when it is not built."""
    if simd not in _libs:
        _libs[simd] = Ref(simd)
    return _libs[simd]


def require(simd=False):
    """lib(simd) for a test.  A missing library means: skip where there is no reference tree to build it from, fail where
    there is one (the build was forgotten)."""
    import pytest
    if os.path.exists(lib_path(simd)):
        return lib(simd)
    if not reference_present():
        pytest.skip(f"{os.path.relpath(lib_path(simd), ROOT)} is not built and there is no reference tree at "
                    f"{reference_root()} to build it from")
    pytest.fail(f"{os.path.relpath(lib_path(simd), ROOT)} is missing although the reference tree is at {reference_root()}: "
                "build first (python -c 'import __graft_entry__ as g; g.build()' or make -C oracle/ref)")
