"""Host-side Python mirror of the reference's operator surface, on top of the C ABI.

This is harness code (tests, bench.py); the product is libfealess_hip.so and the C++ adapter in
fealess_amd/cadreco.  Names follow the reference: Detector.match (linemod.cpp:1356),
quantized_orientations (:230), quantized_normals (:595), depth_to_3d (depth_to_3d.cpp:190),
icp_cloud_to_cloud_ex (ICP.cpp:617), detection (detection.cpp:11), Recognizer.recognition
(obj_reco_lmicp.cpp:86).
"""
import ctypes as C
import numpy as np

from . import _lib as L
from .bank import MATCH_DTYPE, TemplateBank


# numpy view of fl_recognition_result (include/fealess_hip.h), for bulk access to result arrays
_ICP_DT = np.dtype([("R", "<f4", 9), ("T", "<f4", 3), ("dist_mean", "<f4"), ("px_ratio", "<f4"), ("iters", "<i4"), ("n_corr_last", "<i4")])
_DET_DT = np.dtype([("R_final", "<f4", 9), ("T_final", "<f4", 3), ("icp", _ICP_DT), ("n_points", "<i4"), ("status", "<i4")])
RESULT_DTYPE = np.dtype([("status", "<i4"), ("found", "<i4"), ("n_matches", "<i4"), ("best", MATCH_DTYPE), ("pose", "<f4", 16), ("det", _DET_DT)])
assert RESULT_DTYPE.itemsize == C.sizeof(L.RecognitionResult)
# numpy view of fl_track_result
TRACK_DTYPE = np.dtype([("status", "<i4"), ("tracked", "<i4"), ("rect_model", "<i4", 4), ("rect_ref", "<i4", 4), ("pose", "<f4", 16),
                        ("det", _DET_DT)])
assert TRACK_DTYPE.itemsize == C.sizeof(L.TrackResult)
# numpy view of fl_verify_result
VERIFY_DTYPE = np.dtype([("status", "<i4"), ("accepted", "<i4"), ("best", "<i4"), ("rect", "<i4", 4), ("n_model", "<i4"), ("n_missing", "<i4"),
                         ("n_inlier", "<i4"), ("n_front", "<i4"), ("n_behind", "<i4"), ("sum_abs_inlier", "<i8"), ("inlier_ratio", "<f4"),
                         ("behind_ratio", "<f4")])
assert VERIFY_DTYPE.itemsize == C.sizeof(L.VerifyResult) == 64
# numpy view of fl_verified_track_result
VERIFIED_TRACK_DTYPE = np.dtype([("track", TRACK_DTYPE), ("verify", VERIFY_DTYPE), ("verify_in", VERIFY_DTYPE), ("icp_tracked", "<i4"),
                                 ("kept_input", "<i4"), ("best", "<i4"), ("reserved", "<i4")])
assert VERIFIED_TRACK_DTYPE.itemsize == C.sizeof(L.VerifiedTrackResult) == 368
# numpy view of fl_scene_result
SCENE_DTYPE = np.dtype([("verify", VERIFY_DTYPE), ("kept", "<i4"), ("order", "<i4"), ("rival", "<i4"), ("n_shared", "<i4")])
assert SCENE_DTYPE.itemsize == C.sizeof(L.SceneResult) == 80


class FealessError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"fealess_hip error {code}: {msg}")
        self.code = code


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _pyramid_dicts(t, f):
    """One extracted pyramid (templates t, feat_begin into f) as the dicts TemplateBank.add_pyramid takes."""
    out = []
    for k in range(len(t)):
        fb, fc = int(t[k]["feat_begin"]), int(t[k]["feat_count"])
        feats = np.stack([f["x"][fb:fb + fc], f["y"][fb:fb + fc], f["label"][fb:fb + fc]], axis=1).astype(np.int32)
        out.append(dict(width=int(t[k]["width"]), height=int(t[k]["height"]), offset_x=int(t[k]["offset_x"]),
                        offset_y=int(t[k]["offset_y"]), pyramid_level=int(t[k]["pyramid_level"]), features=feats))
    return out


class Context:
    def __init__(self, device=0):
        self.lib = L.load()
        h = C.c_void_p()
        rc = self.lib.fl_context_create(device, C.byref(h))
        if rc != L.FL_OK:
            raise FealessError(rc, "fl_context_create failed (no HIP device? there is no CPU fallback)")
        self.h = h
        self.device = device

    def check(self, rc):
        if rc != L.FL_OK:
            raise FealessError(rc, self.lib.fl_last_error(self.h).decode(errors="replace"))

    def set_stream(self, stream_handle):
        self.check(self.lib.fl_context_set_stream(self.h, C.c_void_p(stream_handle)))

    def synchronize(self):
        self.check(self.lib.fl_context_synchronize(self.h))

    def set_option(self, name, value):
        """Development / comparison switch (fl_context_set_option): speed only, results identical."""
        self.check(self.lib.fl_context_set_option(self.h, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_long()
        self.check(self.lib.fl_context_get_option(self.h, name.encode(), C.byref(v)))
        return int(v.value)

    def close(self):
        if self.h:
            self.lib.fl_context_destroy(self.h)
            self.h = None

    # ---- stage entry points (host numpy arrays in/out) ----
    def quantized_orientations(self, bgr, weak_threshold=10.0):
        bgr = np.ascontiguousarray(bgr, np.uint8)
        h, w = bgr.shape[:2]
        out = np.empty((h, w), np.uint8)
        self.check(self.lib.fl_quantized_orientations(self.h, _ptr(bgr), w, h, weak_threshold, _ptr(out), L.FL_MEM_HOST))
        return out

    def quantized_normals(self, depth, distance_threshold=2000, difference_threshold=50):
        depth = np.ascontiguousarray(depth, np.uint16)
        h, w = depth.shape
        out = np.empty((h, w), np.uint8)
        self.check(self.lib.fl_quantized_normals(self.h, _ptr(depth), w, h, distance_threshold, difference_threshold,
                                                 _ptr(out), L.FL_MEM_HOST))
        return out

    def pyrdown_bgr(self, bgr):
        bgr = np.ascontiguousarray(bgr, np.uint8)
        h, w = bgr.shape[:2]
        out = np.empty((h // 2, w // 2, 3), np.uint8)
        self.check(self.lib.fl_pyrdown_bgr(self.h, _ptr(bgr), w, h, _ptr(out), L.FL_MEM_HOST))
        return out

    def resize_linear(self, img, dw, dh):
        """cv::resize(INTER_LINEAR) of PrepareInputData (obj_reco_lmicp.cpp:39-45): (h, w, 3) u8 or (h, w) u16."""
        if img.dtype == np.uint16:
            a = np.ascontiguousarray(img, np.uint16)
            out = np.empty((dh, dw), np.uint16)
            self.check(self.lib.fl_resize_linear_u16(self.h, _ptr(a), a.shape[1], a.shape[0], _ptr(out), dw, dh, L.FL_MEM_HOST))
        else:
            a = np.ascontiguousarray(img, np.uint8)
            out = np.empty((dh, dw, 3), np.uint8)
            self.check(self.lib.fl_resize_linear_bgr8(self.h, _ptr(a), a.shape[1], a.shape[0], _ptr(out), dw, dh, L.FL_MEM_HOST))
        return out

    def extract_template_pyramid(self, bgr, depth, mask, levels):
        """Detector::addTemplate's extraction (linemod.cpp:1579-1615), default modalities.  Returns (templates, bb):
        templates = levels * 2 dicts ordered [l * 2 + m], ready for TemplateBank.add_pyramid, bb = (x, y, w, h);
        None where the reference returns -1 (too few candidate features)."""
        from .bank import FEATURE_DTYPE, TEMPLATE_DTYPE
        bgr = np.ascontiguousarray(bgr, np.uint8)
        depth = np.ascontiguousarray(depth, np.uint16)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        h, w = depth.shape
        t = np.zeros(levels * 2, TEMPLATE_DTYPE)
        f = np.zeros(levels * 2 * 63, FEATURE_DTYPE)
        bb = (C.c_int * 4)()
        rc = self.lib.fl_extract_template_pyramid(self.h, _ptr(bgr), _ptr(depth), None if mk is None else _ptr(mk), w, h, levels,
                                                  L.FL_MEM_HOST, _ptr(t), _ptr(f), bb)
        if rc == L.FL_ERR_NO_TEMPLATE:
            return None
        self.check(rc)
        return _pyramid_dicts(t, f), tuple(bb)

    def extract_template_batch(self, bgrs, depths, masks, levels, mem=L.FL_MEM_HOST):
        """fl_extract_template_batch: extract_template_pyramid for every view in one call.  masks: None, or one mask or
        None per view.  mem=FL_MEM_HOST: numpy arrays; FL_MEM_DEVICE: device tensors (torch, anything with data_ptr()
        and shape).  Returns one entry per view: (templates, bb), or None where the reference returns -1."""
        from .bank import FEATURE_DTYPE, TEMPLATE_DTYPE
        n = len(bgrs)
        masks = [None] * n if masks is None else list(masks)
        if mem == L.FL_MEM_HOST:
            bgrs = [np.ascontiguousarray(b, np.uint8) for b in bgrs]
            depths = [np.ascontiguousarray(d, np.uint16) for d in depths]
            masks = [None if m is None else np.ascontiguousarray(m, np.uint8) for m in masks]

            def addr(a):
                return a.ctypes.data
        else:
            def addr(a):
                return a.data_ptr()
        h, w = depths[0].shape[:2]
        bp = (C.c_void_p * n)(*[addr(b) for b in bgrs])
        dp = (C.c_void_p * n)(*[addr(d) for d in depths])
        mp = None if all(m is None for m in masks) else (C.c_void_p * n)(*[None if m is None else addr(m) for m in masks])
        J = levels * 2
        t = np.zeros(n * J, TEMPLATE_DTYPE)
        f = np.zeros(n * J * 63, FEATURE_DTYPE)
        bb = np.zeros(4 * n, np.int32)
        st = np.zeros(n, np.int32)
        self.check(self.lib.fl_extract_template_batch(self.h, n, bp, dp, mp, w, h, levels, mem, _ptr(t), _ptr(f), _ptr(bb), _ptr(st)))
        return [None if st[v] != L.FL_OK else (_pyramid_dicts(t[v * J:(v + 1) * J], f), tuple(int(x) for x in bb[4 * v:4 * v + 4]))
                for v in range(n)]

    def dev_extract_select(self, jobs, fill=-7):
        """DEVELOPMENT ONLY (fl_dev_extract_select, not part of the C ABI): extraction's sort and scattered selection on
        candidate lists, all jobs in one call.  jobs: dicts with w, h, num_features, depth_mode, area, raster (int32, in
        arrival order), score (float32), labels ((h, w) uint8).  Returns per job (n_out, features (64, 3) int32 with
        `fill` wherever the kernel wrote nothing, sorted keys (uint64, `fill` as uint64 if the job was not sorted))."""
        n = len(jobs)
        arr = (L.DevSelectJob * n)()
        keep = []
        for k, j in enumerate(jobs):
            raster = np.ascontiguousarray(j["raster"], np.int32)
            score = np.ascontiguousarray(j["score"], np.float32)
            labels = np.ascontiguousarray(j["labels"], np.uint8)
            assert len(raster) == len(score) and labels.shape == (j["h"], j["w"])
            n_out = np.full(1, fill, np.int32)
            feats = np.full((64, 3), fill, np.int32)
            keys = np.full(max(len(raster), 1), np.int64(fill).astype(np.uint64), np.uint64)
            keep.append((raster, score, labels, n_out, feats, keys))
            arr[k] = L.DevSelectJob(j["w"], j["w"] * j["h"], j["num_features"], j["depth_mode"], j["area"], len(raster),
                                    raster.ctypes.data, score.ctypes.data, labels.ctypes.data, n_out.ctypes.data,
                                    feats.ctypes.data, keys.ctypes.data)
        self.check(L.dev(self.lib, "fl_dev_extract_select")(self.h, n, arr))
        return [(int(k[3][0]), k[4], k[5][:len(k[0])]) for k in keep]

    def dev_extract_quantized(self, modality, quantized, magnitudes, masks, threshold, num_features, fill=-7, w=None, h=None):
        """DEVELOPMENT ONLY (fl_dev_extract_quantized, not part of the C ABI): the candidate kernels, the sort and the selection
        of one pyramid level on caller-supplied quantized images, all views in one call.  modality 0 (colour; threshold =
        strong_threshold, magnitudes = one (h, w) float32 image per view) or 1 (depth; threshold = extract_threshold, magnitudes
        ignored); masks: None, or per view a mask or None.  w, h: sizes to pass instead of the images' own (refusal tests).
        Returns per view a dict: local ((h, w) uint8, None without a mask), n_cand, label_counts (8), area, n_out, raster /
        score (the n_cand candidates before the sort, in arrival order), keys (the sorted segment, None if the view was not
        sorted), features ((64, 3) int32), tails_unwritten (the lists hold `fill` behind their n_cand entries); `fill` (its low byte
        in `local`) wherever nothing was written.  A refusal's FealessError carries the untouched buffers as `buffers`."""
        n = len(quantized)
        masks = [None] * n if masks is None else list(masks)
        qs = [np.ascontiguousarray(q, np.uint8) for q in quantized]
        ih, iw = qs[0].shape
        px = iw * ih
        arr = (L.DevExtractView * n)()
        kfill = np.int64(fill).astype(np.uint64)
        keep = []
        for v in range(n):
            mg = None if modality != 0 else np.ascontiguousarray(magnitudes[v], np.float32)
            mk = None if masks[v] is None else np.ascontiguousarray(masks[v], np.uint8)
            assert qs[v].shape == (ih, iw) and (mg is None or mg.shape == (ih, iw)) and (mk is None or mk.shape == (ih, iw))
            local = np.full((ih, iw), fill & 0xFF, np.uint8)
            cnt = np.full(11, fill, np.int32)
            raster, score = np.full(px, fill, np.int32), np.full(px, float(fill), np.float32)
            keys = np.full(px, kfill, np.uint64)
            feats = np.full((64, 3), fill, np.int32)
            keep.append((qs[v], mg, mk, local, cnt, raster, score, keys, feats))
            arr[v] = L.DevExtractView(qs[v].ctypes.data, None if mg is None else mg.ctypes.data, None if mk is None else mk.ctypes.data,
                                      local.ctypes.data, cnt.ctypes.data, raster.ctypes.data, score.ctypes.data, keys.ctypes.data,
                                      feats.ctypes.data)
        strong, ext = (float(threshold), 0) if modality == 0 else (0.0, int(threshold))
        rc = L.dev(self.lib, "fl_dev_extract_quantized")(self.h, n, arr, iw if w is None else w, ih if h is None else h, modality, strong,
                                                         ext, num_features)
        try:
            self.check(rc)
        except FealessError as e:                                # a refusal writes nothing: the caller may look
            e.buffers = [dict(local=k[3], counters=k[4], raster=k[5], score=k[6], keys=k[7], features=k[8]) for k in keep]
            raise
        out = []
        for (_, _, mk, local, cnt, raster, score, keys, feats) in keep:
            nc = int(cnt[0])
            unwritten = bool((raster[nc:] == fill).all() and (score[nc:] == float(fill)).all() and (keys[nc:] == kfill).all())
            was_sorted = nc > 0 and bool((keys[:nc] != kfill).any())
            out.append(dict(local=None if mk is None else local, n_cand=nc, label_counts=cnt[1:9].copy(), area=int(cnt[9]), n_out=int(cnt[10]),
                            raster=raster[:nc], score=score[:nc], keys=keys[:nc] if was_sorted else None, features=feats,
                            tails_unwritten=unwritten))
        return out

    def dev_quantized_orientations_mag(self, bgrs, weak_threshold=10.0, fill=0xEE):
        """DEVELOPMENT ONLY (fl_dev_quantized_orientations_mag, not part of the C ABI): k_color_quantize<true, *>, the build
        template extraction launches, on packed frames of one size.  Returns (quantized (n, h, w) uint8, magnitude (n, h, w)
        float32); bytes the kernel did not write hold `fill`."""
        b = np.ascontiguousarray(np.stack(bgrs), np.uint8)
        n, h, w = b.shape[:3]
        q = np.full((n, h, w), fill, np.uint8)
        mag = np.full((n, h, w), fill * 0x01010101, np.uint32).view(np.float32)
        self.check(L.dev(self.lib, "fl_dev_quantized_orientations_mag")(self.h, _ptr(b), n, w, h, weak_threshold, _ptr(q), _ptr(mag)))
        return q, mag

    def dev_front_images(self, bgrs, depths, levels):
        """DEVELOPMENT ONLY (fl_dev_front_images, not part of the C ABI): the launches of an eager batch's front-end on frames
        of any size, also those no detector can be finalized for.  Returns per frame a list over the levels of dicts with the
        quantised colour image `q0`, the quantised normals `q1` and, from level 1 on, the colour image `bgr`."""
        n = len(bgrs)
        b = np.ascontiguousarray(np.stack(bgrs), np.uint8)
        d = np.ascontiguousarray(np.stack(depths), np.uint16)
        h, w = d.shape[1:]
        sizes = [(w >> l, h >> l) for l in range(levels)]
        per = sum(lw * lh * (5 if l else 2) for l, (lw, lh) in enumerate(sizes))
        out = np.zeros(n * per, np.uint8)
        self.check(L.dev(self.lib, "fl_dev_front_images")(self.h, _ptr(b), _ptr(d), n, w, h, levels, _ptr(out), out.nbytes))
        frames, o = [], 0
        for _ in range(n):
            lv = []
            for l, (lw, lh) in enumerate(sizes):
                px = lw * lh
                e = dict(q0=out[o:o + px].reshape(lh, lw), q1=out[o + px:o + 2 * px].reshape(lh, lw))
                if l:
                    e["bgr"] = out[o + 2 * px:o + 5 * px].reshape(lh, lw, 3)
                o += (5 if l else 2) * px
                lv.append(e)
            frames.append(lv)
        return frames

    def render_views(self, vertices, triangles, poses13, K, w, h, normals=None, colors=None, light=None, ambient=None,
                     mem=L.FL_MEM_HOST, out=None):
        """fl_render_views: views of a triangle mesh (vertices (n, 3) mm, triangles (m, 3) 0-based) at poses13 (k, 13),
        K = (fx, fy, cx, cy), w x h.  normals (n, 3) / colors (n, 3) u8 BGR: optional per-vertex.  light / ambient: None =
        the library's defaults (a headlight and FL_RENDER_AMBIENT).  mem=FL_MEM_HOST: returns numpy (bgr (k, h, w, 3),
        depth (k, h, w) u16 mm, mask (k, h, w) u8, tri (k, h, w) int32).  FL_MEM_DEVICE: `out` is a dict of device tensors
        under some of the keys bgr / depth / mask / tri (contiguous, those shapes and dtypes); the work is queued on this
        context's stream and `out` is returned."""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
        p = np.ascontiguousarray(poses13, np.float32).reshape(-1, 13)
        nv = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        cv = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
        for a in (nv, cv):
            if a is not None and len(a) != len(v):
                raise ValueError("normals / colors need one row per vertex")
        k = L.Intrinsics(w, h, *[float(x) for x in K])
        prm = None
        if light is not None or ambient is not None:
            prm = L.RenderParams((C.c_float * 3)(*(light if light is not None else (0.0, 0.0, 1.0))),
                                 L.FL_RENDER_AMBIENT if ambient is None else float(ambient))
        n = len(p)
        if mem == L.FL_MEM_HOST:
            res = dict(bgr=np.empty((n, h, w, 3), np.uint8), depth=np.empty((n, h, w), np.uint16), mask=np.empty((n, h, w), np.uint8),
                       tri=np.empty((n, h, w), np.int32))
            ptrs = [_ptr(res[key]) for key in ("bgr", "depth", "mask", "tri")]
        else:
            res = dict(out or {})
            # the kernel writes n * h * w pixels into each output: refuse a tensor that cannot hold them, before the call
            shapes = dict(bgr=((n, h, w, 3), 1), depth=((n, h, w), 2), mask=((n, h, w), 1), tri=((n, h, w), 4))
            for key, tns in res.items():
                if key not in shapes:
                    raise ValueError(f"render_views: unknown output {key!r}")
                shape, size = shapes[key]
                if (tns.device.type != "cuda" or tns.device.index != self.device or not tns.is_contiguous()
                        or tns.element_size() != size or tuple(tns.shape) != shape):
                    raise ValueError(f"render_views: out[{key!r}] must be a contiguous tensor on cuda:{self.device} of shape {shape} "
                                     f"with {size}-byte elements")
            ptrs = [C.c_void_p(res[key].data_ptr()) if key in res else None for key in ("bgr", "depth", "mask", "tri")]
        self.check(self.lib.fl_render_views(self.h, _ptr(v), None if nv is None else _ptr(nv), None if cv is None else _ptr(cv), len(v),
                                            _ptr(t), len(t), n, _ptr(p), C.byref(k), None if prm is None else C.byref(prm), mem, *ptrs))
        if mem == L.FL_MEM_HOST:
            return res["bgr"], res["depth"], res["mask"], res["tri"]
        return res

    def register_depth(self, depths, K_depth, K_color, R, t, fill_cracks=1, mem=L.FL_MEM_HOST, out=None):
        """fl_register_depth_batch: raw depth frames re-expressed in the colour camera.  K_depth, K_color = (w, h, fx, fy, cx,
        cy) of the two cameras; R (3, 3) and t (3,) take a point of the depth camera to the colour camera, X_colour = R X_depth
        + t in mm.  mem=FL_MEM_HOST: depths are (hd, wd) u16 numpy arrays in mm and the result is an (n, hc, wc) u16 array (`out`,
        when given, is that array to fill).  FL_MEM_DEVICE: depths and `out` are lists of device pointers (ints, or anything
        with data_ptr()) to frames of wd * hd and wc * hc u16; the work is queued on this context's stream and `out` is returned."""
        kd = L.Intrinsics(int(K_depth[0]), int(K_depth[1]), *[float(x) for x in K_depth[2:]])
        kc = L.Intrinsics(int(K_color[0]), int(K_color[1]), *[float(x) for x in K_color[2:]])
        Ra, ta = np.ascontiguousarray(R, np.float32).ravel(), np.ascontiguousarray(t, np.float32).ravel()
        if Ra.size != 9 or ta.size != 3:
            raise ValueError("register_depth: R is 3 x 3 and t has 3 entries")
        ext = L.Extrinsics((C.c_float * 9)(*Ra), (C.c_float * 3)(*ta))
        prm = L.RegisterParams(int(fill_cracks))
        n = len(depths)
        if not all(0 < v <= L.FL_RENDER_MAX_DIM for v in (kd.width, kd.height, kc.width, kc.height)):     # what the library refuses, before np.empty meets it
            raise FealessError(L.FL_ERR_INVALID, f"register_depth: image sizes must be 1..{L.FL_RENDER_MAX_DIM}")
        if mem == L.FL_MEM_HOST:
            frames = [np.ascontiguousarray(d, np.uint16) for d in depths]
            for d in frames:
                if d.shape != (kd.height, kd.width):
                    raise ValueError(f"register_depth: frames must be {kd.height} x {kd.width}")
            res = np.empty((n, kc.height, kc.width), np.uint16) if out is None else out
            if res.dtype != np.uint16 or res.shape != (n, kc.height, kc.width) or not res.flags.c_contiguous:
                raise ValueError(f"register_depth: out must be a contiguous ({n}, {kc.height}, {kc.width}) uint16 array")
            ip = [d.ctypes.data for d in frames]
            op = [res[i].ctypes.data for i in range(n)]
        else:
            if out is None or len(out) != n:
                raise ValueError("register_depth: with FL_MEM_DEVICE `out` holds one device pointer per frame")
            res = out
            ip = [d.data_ptr() if hasattr(d, "data_ptr") else int(d) for d in depths]
            op = [d.data_ptr() if hasattr(d, "data_ptr") else int(d) for d in out]
        self.check(self.lib.fl_register_depth_batch(self.h, n, (C.c_void_p * max(1, n))(*ip), mem, C.byref(kd), C.byref(kc), C.byref(ext),
                                                    C.byref(prm), (C.c_void_p * max(1, n))(*op)))
        return res

    def build_linear_memories(self, quantized, T):
        q = np.ascontiguousarray(quantized, np.uint8)
        h, w = q.shape
        stride = self.lib.fl_lm_label_stride(w, h, T)
        out = np.empty(8 * stride, np.uint8)
        self.check(self.lib.fl_build_linear_memories(self.h, _ptr(q), w, h, T, _ptr(out), L.FL_MEM_HOST))
        return out.reshape(8, stride)

    def depth_to_3d(self, depth, fx, fy, cx, cy):
        depth = np.ascontiguousarray(depth, np.uint16)
        h, w = depth.shape
        out = np.empty((h, w, 3), np.float32)
        self.check(self.lib.fl_depth_to_3d(self.h, _ptr(depth), w, h, fx, fy, cx, cy, _ptr(out), L.FL_MEM_HOST))
        return out

    def icp_cloud_to_cloud_ex(self, ref, model, icp_it_thr=4, dist_mean_thr=0.0, dist_diff_thr=0.0,
                              mode=L.FL_ICP_PARITY):
        ref = np.ascontiguousarray(ref, np.float32).reshape(-1, 3)
        model = np.ascontiguousarray(model, np.float32).reshape(-1, 3)
        res = L.IcpResult()
        self.check(self.lib.fl_icp(self.h, _ptr(ref), len(ref), _ptr(model), len(model), icp_it_thr, dist_mean_thr,
                                   dist_diff_thr, mode, L.FL_MEM_HOST, C.byref(res)))
        return icp_result_to_dict(res)

    def icp_point_to_plane(self, ref, ref_normals, model, icp_it_thr=4, dist_mean_thr=0.0, dist_diff_thr=0.0):
        """FL_ICP_POINT_TO_PLANE on caller-supplied clouds (no reference counterpart)."""
        ref = np.ascontiguousarray(ref, np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(ref_normals, np.float32).reshape(-1, 3)
        if len(nrm) != len(ref):
            raise ValueError("ref_normals must have one normal per reference point")
        model = np.ascontiguousarray(model, np.float32).reshape(-1, 3)
        res = L.IcpResult()
        self.check(self.lib.fl_icp_point_to_plane(self.h, _ptr(ref), _ptr(nrm), len(ref), _ptr(model), len(model),
                                                  icp_it_thr, dist_mean_thr, dist_diff_thr, L.FL_MEM_HOST, C.byref(res)))
        return icp_result_to_dict(res)

    def dev_scene_normals(self, depth_mm, K, xs, ys):
        """DEVELOPMENT ONLY (fl_dev_scene_normals, not part of the C ABI): the unit normals FL_ICP_POINT_TO_PLANE gives the scene
        pixels (xs[i], ys[i]) of a u16 depth image (mm) with intrinsics K = (fx, fy, cx, cy); (0, 0, 0) where it gives none."""
        fn = self.lib.fl_dev_scene_normals
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_void_p]
        d = np.ascontiguousarray(depth_mm, np.uint16)
        h, w = d.shape
        xy = np.ascontiguousarray(np.stack([np.asarray(xs).ravel(), np.asarray(ys).ravel()], 1), np.int32)
        out = np.zeros((len(xy), 3), np.float32)
        self.check(fn(_ptr(d), w, h, *[float(v) for v in K], _ptr(xy), len(xy), _ptr(out)))
        return out

    def detection(self, model_depth_mm, scene_depth_mm, K, rect_model, rect_ref, icp_it_thr, dist_mean_thr,
                  dist_diff_thr, r_match, t_match, mode=L.FL_ICP_PARITY):
        md = np.ascontiguousarray(model_depth_mm, np.uint16)
        sd = np.ascontiguousarray(scene_depth_mm, np.uint16)
        h, w = sd.shape
        k = L.Intrinsics(w, h, *K)
        rm = (C.c_int * 4)(*[int(v) for v in rect_model])
        rr = (C.c_int * 4)(*[int(v) for v in rect_ref])
        rmat = (C.c_float * 9)(*np.asarray(r_match, np.float32).ravel())
        tvec = (C.c_float * 3)(*np.asarray(t_match, np.float32).ravel())
        res = L.DetectionResult()
        self.check(self.lib.fl_detection(self.h, _ptr(md), _ptr(sd), w, h, C.byref(k), rm, rr, icp_it_thr, dist_mean_thr,
                                         dist_diff_thr, rmat, tvec, mode, L.FL_MEM_HOST, C.byref(res)))
        return detection_result_to_dict(res)


def icp_result_to_dict(r):
    return dict(R=np.array(r.R, np.float32).reshape(3, 3), T=np.array(r.T, np.float32), dist_mean=np.float32(r.dist_mean),
                px_ratio=np.float32(r.px_ratio), iters=int(r.iters), n_corr_last=int(r.n_corr_last))


def detection_result_to_dict(r):
    return dict(R_final=np.array(r.R_final, np.float32).reshape(3, 3), T_final=np.array(r.T_final, np.float32),
                icp=icp_result_to_dict(r.icp), n_points=int(r.n_points), status=int(r.status))


def recognition_result_to_dict(r):
    return dict(status=int(r.status), found=int(r.found), n_matches=int(r.n_matches),
                best=dict(x=r.best.x, y=r.best.y, similarity=np.float32(r.best.similarity), class_idx=r.best.class_idx,
                          template_id=r.best.template_id),
                pose=np.array(r.pose, np.float32).reshape(4, 4), det=detection_result_to_dict(r.det))


class _HostOnlyContext:
    """What a host-only Detector needs of a Context: the library and the error text of the detector's own context."""

    def __init__(self):
        self.lib = L.load()
        self.h = None

    def check(self, rc):
        if rc != L.FL_OK:
            raise FealessError(rc, self.lib.fl_last_error(self.h).decode(errors="replace") if self.h else "")


def _host_only_detector(modalities, T_pyramid):
    """Test aid (fl_dev_detector_create_host, not part of the ABI): a Detector that holds its bank on the host only.  It needs
    no GPU, cannot be finalized and serves the host-only entry points (group_matches with FL_MEM_HOST)."""
    return Detector(_HostOnlyContext(), modalities, T_pyramid, _host_only=True)


class Detector:
    """cup_linemod::Detector resident on one GPU (linemod.hpp:292-412)."""

    def __init__(self, ctx, modalities, T_pyramid, _host_only=False):
        self.ctx = ctx
        self.lib = ctx.lib
        self.M = modalities
        self.T = list(T_pyramid)
        self.L = len(self.T)
        h = C.c_void_p()
        arr = (C.c_int * self.L)(*self.T)
        if _host_only:
            ctx.check(L.dev(self.lib, "fl_dev_detector_create_host")(modalities, self.L, arr, C.byref(h)))
            ctx.h = C.c_void_p(self.lib.fl_detector_get_context(h))
        else:
            ctx.check(self.lib.fl_detector_create(ctx.h, modalities, self.L, arr, C.byref(h)))
        self.h = h
        self.banks = []
        self.w0 = self.h0 = 0

    def add_class(self, bank: TemplateBank):
        assert bank.levels == self.L and bank.modalities == self.M
        t, f, p = bank.arrays()
        self.ctx.check(self.lib.fl_detector_add_class(self.h, bank.class_id.encode(), bank.n_pyramids, _ptr(t), _ptr(f),
                                                      len(f), _ptr(p) if len(p) else None))
        self.banks.append(bank)
        self.banks.sort(key=lambda b: b.class_id)

    def set_class_filter(self, class_ids=()):
        """Detector::match's class_ids (linemod.cpp:1418-1434): () = all classes."""
        ids = [c.encode() for c in class_ids]
        arr = (C.c_char_p * max(1, len(ids)))(*ids) if ids else None
        self.ctx.check(self.lib.fl_detector_set_class_filter(self.h, arr, len(ids)))

    def finalize(self, w0, h0, max_batch=1, max_candidates=0):
        # model depth renders first (class order = sorted class ids)
        for ci, b in enumerate(self.banks):
            # render i belongs to pyramid i (bank.py); pyramids without one (None / behind the list's end) get none and
            # cannot be refined (FL_ERR_STATE in the result).  One upload per run of consecutive renders.
            i, n = 0, len(b.model_depths)
            while i < n:
                if b.model_depths[i] is None:
                    i += 1
                    continue
                j = i
                while j < n and b.model_depths[j] is not None:
                    j += 1
                d = np.ascontiguousarray(np.stack(b.model_depths[i:j]), np.uint16)
                self.ctx.check(self.lib.fl_detector_set_model_depths(self.h, ci, i, j - i, _ptr(d), d.shape[2], d.shape[1],
                                                                     L.FL_MEM_HOST))
                i = j
        self.ctx.check(self.lib.fl_detector_finalize(self.h, w0, h0, max_batch, max_candidates))
        self.w0, self.h0, self.max_batch = w0, h0, max_batch

    def num_templates(self):
        return self.lib.fl_detector_num_templates(self.h)

    def match_quantized(self, quantized, threshold, cap=65536):
        """quantized: list [l*M+m] of (h_l, w_l) uint8 arrays (the pass-through modality)."""
        qs = [np.ascontiguousarray(q, np.uint8) for q in quantized]
        ptrs = (C.c_void_p * len(qs))(*[q.ctypes.data for q in qs])
        out = np.zeros(cap, MATCH_DTYPE)
        n = C.c_int(0)
        self.ctx.check(self.lib.fl_match_quantized(self.h, ptrs, L.FL_MEM_HOST, threshold, _ptr(out), cap, C.byref(n)))
        return out[:min(n.value, cap)], n.value

    def match(self, bgr, depth, threshold, cap=65536, masks=None):
        """Detector::match (linemod.hpp:319-327); masks: None or one u8 image (or None) per modality."""
        bgr = np.ascontiguousarray(bgr, np.uint8)
        depth = np.ascontiguousarray(depth, np.uint16) if depth is not None else None
        out = np.zeros(cap, MATCH_DTYPE)
        n = C.c_int(0)
        mp = None
        if masks is not None:
            if len(masks) != self.M:
                raise FealessError(L.FL_ERR_INVALID, "masks.size() != modalities.size() (linemod.cpp:1365)")
            mk = [None if m is None else np.ascontiguousarray(m, np.uint8) for m in masks]
            mp = (C.c_void_p * self.M)(*[None if m is None else m.ctypes.data for m in mk])
        self.ctx.check(self.lib.fl_match_frame_masked(self.h, _ptr(bgr), _ptr(depth) if depth is not None else None, mp,
                                                      L.FL_MEM_HOST, threshold, _ptr(out), cap, C.byref(n)))
        return out[:min(n.value, cap)], n.value

    def match_batch_submit(self, bgr_ptrs, depth_ptrs, threshold, mem=L.FL_MEM_DEVICE):
        """Detector::match of a batch of frames (raw pointers, device memory by default); queued, not waited for."""
        n = len(bgr_ptrs)
        bp = (C.c_void_p * n)(*bgr_ptrs)
        dp = (C.c_void_p * n)(*depth_ptrs) if depth_ptrs is not None else None
        self.ctx.check(self.lib.fl_match_batch_submit(self.h, n, bp, dp, mem, threshold))

    def match_batch_collect(self, frame, cap=65536):
        out = np.zeros(cap, MATCH_DTYPE)
        n = C.c_int(0)
        self.ctx.check(self.lib.fl_match_batch_collect(self.h, frame, _ptr(out), cap, C.byref(n)))
        return out[:min(n.value, cap)], n.value

    def match_batch(self, bgrs, depths, threshold, cap=65536):
        """Host arrays in: list of (matches, n_total) per frame."""
        bs = [np.ascontiguousarray(b, np.uint8) for b in bgrs]
        ds = [np.ascontiguousarray(d, np.uint16) for d in depths]
        self.match_batch_submit([b.ctypes.data for b in bs], [d.ctypes.data for d in ds], threshold, L.FL_MEM_HOST)
        return [self.match_batch_collect(i, cap) for i in range(len(bs))]

    def similarity_maps(self, first, count):
        g = self.T[-1]
        w, h = self.w0 >> (self.L - 1), self.h0 >> (self.L - 1)
        W, H = w // g, h // g
        out = np.zeros((count, H, W), np.uint16)
        self.ctx.check(self.lib.fl_similarity_maps(self.h, first, count, _ptr(out)))
        return out

    def last_quantized(self):
        sizes = [((self.h0 >> l), (self.w0 >> l)) for l in range(self.L) for _ in range(self.M)]
        buf = np.zeros(sum(a * b for a, b in sizes), np.uint8)
        self.ctx.check(self.lib.fl_last_quantized(self.h, _ptr(buf)))
        out, o = [], 0
        for a, b in sizes:
            out.append(buf[o:o + a * b].reshape(a, b).copy())
            o += a * b
        return out

    def dev_frame_image(self, frame, kind, level, modality=0):
        """DEVELOPMENT ONLY (fl_dev_frame_image, not part of the C ABI): frame `frame`'s workspace image of the last batch, as
        it is (lazy batches included).  kind 0: quantised (h, w) u8; 1: pyrDown BGR (h, w, 3) of a level >= 1; 2: spread (h, w)
        of a fine level; 3: the coarsest level's linear memories (8, fl_lm_label_stride)."""
        fn = self.lib.fl_dev_frame_image
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        h, w = self.h0 >> level, self.w0 >> level
        if kind == 3:
            shape = (8, self.lib.fl_lm_label_stride(w, h, self.T[level]))
        else:
            shape = (h, w, 3) if kind == 1 else (h, w)
        out = np.empty(shape, np.uint8)
        n = C.c_size_t(0)
        self.ctx.check(fn(self.h, frame, kind, level, modality, _ptr(out), out.nbytes, C.byref(n)))
        assert n.value == out.nbytes
        return out

    def _params(self, threshold, icp_it_thr, dist_mean_thr, dist_diff_thr, mode):
        return L.RecognitionParams(threshold, icp_it_thr, dist_mean_thr, dist_diff_thr, mode)

    def recognize_batch(self, bgrs, depths, K, threshold=75.0, icp_it_thr=10, dist_mean_thr=0.5, dist_diff_thr=0.01,
                        mode=L.FL_ICP_PARITY):
        """Host arrays in, list of result dicts out (CObjRecoLmICP::Recognition per frame)."""
        n = len(bgrs)
        bs = [np.ascontiguousarray(b, np.uint8) for b in bgrs]
        ds = [np.ascontiguousarray(d, np.uint16) for d in depths]
        bp = (C.c_void_p * n)(*[b.ctypes.data for b in bs])
        dp = (C.c_void_p * n)(*[d.ctypes.data for d in ds])
        k = L.Intrinsics(self.w0, self.h0, *K)
        p = self._params(threshold, icp_it_thr, dist_mean_thr, dist_diff_thr, mode)
        res = (L.RecognitionResult * n)()
        self.ctx.check(self.lib.fl_recognize_batch(self.h, n, bp, dp, L.FL_MEM_HOST, C.byref(k), C.byref(p), res))
        return [recognition_result_to_dict(r) for r in res]

    def recognize_batch_zoom(self, bgrs, depths, K, threshold=75.0, icp_it_thr=10, dist_mean_thr=0.5, dist_diff_thr=0.01,
                             mode=L.FL_ICP_PARITY, mem=L.FL_MEM_HOST, src_size=None):
        """PrepareInputData's zoom + Recognition (fl_recognize_batch_zoom): sources of one size, resized (INTER_LINEAR) on the
        device to the finalized size; K is the finalized size's.  Host arrays in, or with mem=FL_MEM_DEVICE lists of device
        pointers and src_size = (w, h).  List of result dicts."""
        if mem == L.FL_MEM_HOST:
            bs = [np.ascontiguousarray(b, np.uint8) for b in bgrs]
            ds = [np.ascontiguousarray(d, np.uint16) for d in depths]
            sw, sh = ds[0].shape[1], ds[0].shape[0]
            bptrs, dptrs = [b.ctypes.data for b in bs], [d.ctypes.data for d in ds]
        else:
            (sw, sh), bptrs, dptrs = src_size, bgrs, depths
        n = len(bptrs)
        bp = (C.c_void_p * n)(*bptrs)
        dp = (C.c_void_p * n)(*dptrs)
        k = L.Intrinsics(self.w0, self.h0, *K)
        p = self._params(threshold, icp_it_thr, dist_mean_thr, dist_diff_thr, mode)
        res = (L.RecognitionResult * n)()
        self.ctx.check(self.lib.fl_recognize_batch_zoom(self.h, n, bp, dp, sw, sh, mem, C.byref(k), C.byref(p), res))
        return [recognition_result_to_dict(r) for r in res]

    def recognize_topk(self, bgr, depth, K, k, threshold=75.0, icp_it_thr=10, dist_mean_thr=0.5, dist_diff_thr=0.01,
                       mode=L.FL_ICP_PARITY):
        """Refinement of the first k matches of one frame; list of result dicts."""
        b = np.ascontiguousarray(bgr, np.uint8)
        d = np.ascontiguousarray(depth, np.uint16)
        kk = L.Intrinsics(self.w0, self.h0, *K)
        p = self._params(threshold, icp_it_thr, dist_mean_thr, dist_diff_thr, mode)
        res = (L.RecognitionResult * k)()
        n = C.c_int(0)
        self.ctx.check(self.lib.fl_recognize_topk(self.h, _ptr(b), _ptr(d), L.FL_MEM_HOST, C.byref(kk), C.byref(p), k, res, C.byref(n)))
        self._last_topk = res
        return [recognition_result_to_dict(res[i]) for i in range(n.value)]

    def recognize_batch_topk(self, bgrs, depths, K, k, threshold=75.0, icp_it_thr=10, dist_mean_thr=0.5, dist_diff_thr=0.01,
                             mode=L.FL_ICP_PARITY):
        """recognize_topk for a batch: list (per frame) of lists of result dicts (n_frames * k ICP workgroups, one launch)."""
        n = len(bgrs)
        bs = [np.ascontiguousarray(b, np.uint8) for b in bgrs]
        ds = [np.ascontiguousarray(d, np.uint16) for d in depths]
        bp = (C.c_void_p * n)(*[b.ctypes.data for b in bs])
        dp = (C.c_void_p * n)(*[d.ctypes.data for d in ds])
        kk = L.Intrinsics(self.w0, self.h0, *K)
        p = self._params(threshold, icp_it_thr, dist_mean_thr, dist_diff_thr, mode)
        res = (L.RecognitionResult * (n * k))()
        cnt = (C.c_int * n)()
        self.ctx.check(self.lib.fl_recognize_batch_topk(self.h, n, bp, dp, L.FL_MEM_HOST, C.byref(kk), C.byref(p), k, res, cnt))
        return [[recognition_result_to_dict(res[f * k + r]) for r in range(cnt[f])] for f in range(n)]

    def group_matches(self, matches, max_instances, min_dist_px, hyp_per_instance=1, mem=L.FL_MEM_HOST, n=None, group_of=None,
                      group_size=None, n_groups=None):
        """fl_group_matches: the multi-instance grouping alone.  Host: `matches` is a MATCH_DTYPE array; returns
        (group_of, group_size, n_groups).  Device (mem=FL_MEM_DEVICE): matches, group_of, group_size and n_groups are device
        pointers and n the number of matches; queued on the context's stream, returns None."""
        ip = L.InstanceParams(max_instances, min_dist_px, hyp_per_instance)
        if mem == L.FL_MEM_DEVICE:
            self.ctx.check(self.lib.fl_group_matches(self.h, C.c_void_p(matches), n, mem, C.byref(ip), C.c_void_p(group_of),
                                                     C.c_void_p(group_size), C.c_void_p(n_groups)))
            return None
        m = np.ascontiguousarray(matches, MATCH_DTYPE)
        gof = np.full(max(1, len(m)), -9, np.int32)
        gsize = np.full(max(1, max_instances), -9, np.int32)
        ng = C.c_int32(-9)
        self.ctx.check(self.lib.fl_group_matches(self.h, _ptr(m), len(m), mem, C.byref(ip), _ptr(gof), _ptr(gsize), C.byref(ng)))
        return gof[:len(m)], gsize, ng.value

    def recognize_batch_instances(self, bgrs, depths, K, max_instances, min_dist_px, hyp_per_instance, threshold=75.0, icp_it_thr=10,
                                  dist_mean_thr=0.5, dist_diff_thr=0.01, mode=L.FL_ICP_PARITY, mem=L.FL_MEM_HOST, with_dropped=False):
        """fl_recognize_batch_instances: every instance in each frame.  Host arrays in (or, with mem=FL_MEM_DEVICE, lists of
        device pointers); a list per frame of result dicts (recognition_result_to_dict plus rank, n_members, n_refined), in
        group order.  with_dropped: also the per-frame counts of matches that found no group."""
        if mem == L.FL_MEM_HOST:
            bs = [np.ascontiguousarray(b, np.uint8) for b in bgrs]
            ds = [np.ascontiguousarray(d, np.uint16) for d in depths]
            bptrs, dptrs = [b.ctypes.data for b in bs], [d.ctypes.data for d in ds]
        else:
            bptrs, dptrs = bgrs, depths
        n = len(bptrs)
        bp = (C.c_void_p * n)(*bptrs)
        dp = (C.c_void_p * n)(*dptrs)
        kk = L.Intrinsics(self.w0, self.h0, *K)
        p = self._params(threshold, icp_it_thr, dist_mean_thr, dist_diff_thr, mode)
        ip = L.InstanceParams(max_instances, min_dist_px, hyp_per_instance)
        G = max(1, max_instances)
        res = (L.InstanceResult * (n * G))()
        cnt = (C.c_int32 * n)()
        drop = (C.c_int32 * n)()
        self.ctx.check(self.lib.fl_recognize_batch_instances(self.h, n, bp, dp, mem, C.byref(kk), C.byref(p), C.byref(ip), res, cnt, drop))
        out = []
        for f in range(n):
            out.append([dict(recognition_result_to_dict(res[f * G + g].reco), rank=int(res[f * G + g].rank),
                             n_members=int(res[f * G + g].n_members), n_refined=int(res[f * G + g].n_refined)) for g in range(cnt[f])])
        return (out, [int(v) for v in drop]) if with_dropped else out

    def recognize_batch_instances_verified(self, tracker, bgrs, depths, K, max_instances, min_dist_px, hyp_per_instance, class_idx=-1,
                                           member_records=False, threshold=75.0, icp_it_thr=10, dist_mean_thr=0.5, dist_diff_thr=0.01,
                                           mode=L.FL_ICP_PARITY, mem=L.FL_MEM_HOST, mesh_of_class=None, **verify):
        """fl_recognize_batch_instances_verified: recognize_batch_instances whose pick among a group's members is the
        verification's, against `tracker`'s mesh (a Tracker of the detector's frame size on the same context; only its mesh is
        used).  verify: the fields of fl_verify_params (tau_mm, min_model_px, min_inlier_ratio, max_behind_ratio), the rest at
        the library's defaults; class_idx >= 0: only that class's groups are verified.  mesh_of_class (then class_idx stays -1;
        fl_recognize_batch_instances_verified_meshes): one entry per class of the detector, the mesh of `tracker` its groups are
        verified against or -1 for none.  A list per frame of result dicts as
        recognize_batch_instances returns them, plus verify (a VERIFY_DTYPE record), nms_rank and verified, in group order.
        member_records: also a VERIFY_DTYPE array of shape (n_frames, max_instances, hyp_per_instance), every job slot's record."""
        unknown = set(verify) - set(_VERIFY_DEFAULTS)
        if unknown:
            raise TypeError(f"recognize_batch_instances_verified: unknown parameters {sorted(unknown)}")
        if mem == L.FL_MEM_HOST:
            bs = [np.ascontiguousarray(b, np.uint8) for b in bgrs]
            ds = [np.ascontiguousarray(d, np.uint16) for d in depths]
            bptrs, dptrs = [b.ctypes.data for b in bs], [d.ctypes.data for d in ds]
        else:
            bptrs, dptrs = bgrs, depths
        n = len(bptrs)
        bp = (C.c_void_p * n)(*bptrs)
        dp = (C.c_void_p * n)(*dptrs)
        kk = L.Intrinsics(self.w0, self.h0, *K)
        p = self._params(threshold, icp_it_thr, dist_mean_thr, dist_diff_thr, mode)
        ip = L.InstanceParams(max_instances, min_dist_px, hyp_per_instance)
        vp = L.InstanceVerifyParams(L.VerifyParams(**dict(_VERIFY_DEFAULTS, **verify)), class_idx, 0)
        G, h = max(1, max_instances), max(1, hyp_per_instance)
        res = (L.VerifiedInstanceResult * (n * G))()
        cnt = (C.c_int32 * n)()
        drop = (C.c_int32 * n)()
        members = np.zeros((n, G, h), VERIFY_DTYPE) if member_records else None
        trk_h, mem_p = None if tracker is None else tracker.handle, None if members is None else _ptr(members)
        if mesh_of_class is None:
            self.ctx.check(self.lib.fl_recognize_batch_instances_verified(self.h, trk_h, n, bp, dp, mem, C.byref(kk), C.byref(p), C.byref(ip),
                                                                          C.byref(vp), res, cnt, drop, mem_p))
        else:
            moc = np.ascontiguousarray(mesh_of_class, np.int32).ravel()
            if len(moc) != self.lib.fl_detector_num_classes(self.h):
                raise ValueError("recognize_batch_instances_verified: mesh_of_class has one entry per class of the detector")
            self.ctx.check(self.lib.fl_recognize_batch_instances_verified_meshes(self.h, trk_h, n, bp, dp, mem, C.byref(kk), C.byref(p), C.byref(ip),
                                                                                 C.byref(vp), _ptr(moc), res, cnt, drop, mem_p))
        out = []
        for f in range(n):
            row = []
            for g in range(cnt[f]):
                r = res[f * G + g]
                row.append(dict(recognition_result_to_dict(r.inst.reco), rank=int(r.inst.rank), n_members=int(r.inst.n_members),
                                n_refined=int(r.inst.n_refined), verify=np.frombuffer(bytes(r.verify), VERIFY_DTYPE)[0],
                                nms_rank=int(r.nms_rank), verified=int(r.verified)))
            out.append(row)
        return (out, members) if member_records else out

    def instances_verify_ms(self):
        """DEVELOPMENT ONLY (fl_dev_instances_verify_ms, not part of the C ABI): device time of the verification stage of the
        last recognize_batch_instances_verified: dict(fused, finish) in ms."""
        out = (C.c_float * 2)()
        self.ctx.check(L.dev(self.lib, "fl_dev_instances_verify_ms")(self.h, out))
        return dict(fused=float(out[0]), finish=float(out[1]))

    def nms(self, n, th_obj_dist):
        """nonMaximumSuppression (ICP/NMS.cpp:6-40) over the first n hypotheses of the last recognize_topk call."""
        win = (C.c_int * max(1, n))()
        nw = C.c_int(0)
        self.ctx.check(self.lib.fl_nms(self._last_topk, n, th_obj_dist, win, C.byref(nw)))
        return [int(win[i]) for i in range(nw.value)]

    def recognize_submit_device(self, bgr_ptrs, depth_ptrs, K, params):
        n = len(bgr_ptrs)
        bp = (C.c_void_p * n)(*bgr_ptrs)
        dp = (C.c_void_p * n)(*depth_ptrs)
        k = L.Intrinsics(self.w0, self.h0, *K)
        self.ctx.check(self.lib.fl_recognize_submit(self.h, n, bp, dp, L.FL_MEM_DEVICE, C.byref(k), C.byref(params)))

    def recognize_submit_host(self, bgr_ptrs, depth_ptrs, K, params):
        """Same as recognize_submit_device with host (ideally pinned) frame pointers: the upload is part of the call."""
        n = len(bgr_ptrs)
        bp = (C.c_void_p * n)(*bgr_ptrs)
        dp = (C.c_void_p * n)(*depth_ptrs)
        k = L.Intrinsics(self.w0, self.h0, *K)
        self.ctx.check(self.lib.fl_recognize_submit(self.h, n, bp, dp, L.FL_MEM_HOST, C.byref(k), C.byref(params)))

    def recognize_collect(self, n):
        res = (L.RecognitionResult * n)()
        self.ctx.check(self.lib.fl_recognize_collect(self.h, n, res))
        return res

    def recognize_collect_previous(self, n):
        """The results of the batch submitted before the latest recognize_submit_*, waiting for that batch only: with
        submit(i + 1); collect_previous(i) two batches stay in flight.  FL_ERR_STATE when there is no such batch."""
        res = (L.RecognitionResult * n)()
        self.ctx.check(self.lib.fl_recognize_collect_previous(self.h, n, res))
        return res

    def frame_counters(self, frame):
        """fl_frame_counters: (coarse candidates, matches after sort/unique, overflow flag, marked level-0 tiles or -1)."""
        out = (C.c_int32 * 4)()
        self.ctx.check(self.lib.fl_frame_counters(self.h, frame, out))
        return tuple(int(v) for v in out)

    def stage_times(self):
        t = L.StageTimes()
        self.ctx.check(self.lib.fl_last_stage_times(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in L.StageTimes._fields_}

    def export_topk(self, frame, k, template_id_base, dev_ptr):
        self.ctx.check(self.lib.fl_export_topk(self.h, frame, k, template_id_base, C.c_void_p(dev_ptr)))

    def export_topk_batch(self, n_frames, k, template_id_base, dev_ptr):
        self.ctx.check(self.lib.fl_export_topk_batch(self.h, n_frames, k, template_id_base, C.c_void_p(dev_ptr)))

    def refine_matches(self, frames, matches, K, params):
        """fl_refine_matches: `matches` is a MATCH_DTYPE array with class-local template ids of THIS detector."""
        n = len(frames)
        fr = (C.c_int32 * n)(*[int(f) for f in frames])
        m = np.ascontiguousarray(matches, MATCH_DTYPE)
        k = L.Intrinsics(self.w0, self.h0, *K)
        res = (L.RecognitionResult * n)()
        self.ctx.check(self.lib.fl_refine_matches(self.h, n, fr, _ptr(m), C.byref(k), C.byref(params), res))
        return res

    def grow_candidates(self, n_frames):
        """fl_detector_grow_candidates: after a queued batch reported an overflow; returns the capacity afterwards."""
        cap = C.c_int(0)
        self.ctx.check(self.lib.fl_detector_grow_candidates(self.h, n_frames, C.byref(cap)))
        return cap.value

    def select_best_batch(self, dev_gathered, n_ranks, n_frames, k, tid_first, tid_count, dev_best):
        """fl_select_best_batch: per frame matches[0] of the global sort over the ranks' all-gathered records (device
        pointers in and out); this rank's refinement jobs stay in the detector."""
        self.ctx.check(self.lib.fl_select_best_batch(self.h, C.c_void_p(dev_gathered), n_ranks, n_frames, k, tid_first, tid_count,
                                                     C.c_void_p(dev_best)))

    def refine_selected(self, n_frames, K, params, dev_rows, depth_base=None, depth_stride=0):
        """fl_refine_selected: ICP of the selected jobs, {found, 4x4 pose} rows (float32 [n_frames, 17]) written to dev_rows."""
        k = L.Intrinsics(self.w0, self.h0, *K)
        self.ctx.check(self.lib.fl_refine_selected(self.h, n_frames, C.byref(k), C.byref(params),
                                                   C.c_void_p(depth_base) if depth_base else None, depth_stride, C.c_void_p(dev_rows)))

    def close(self):
        if self.h:
            self.lib.fl_detector_destroy(self.h)
            self.h = None


class MgGroup:
    """One rank of a template-sharded group driven by the C++ host (libfealess_mg.so, include/fealess_mg.h): RCCL
    all-gather of the top-k records, winner selection and refinement on the device, int32 all-reduce of the pose rows."""

    @staticmethod
    def unique_id():
        lib = L.load_mg()
        buf = C.create_string_buffer(L.FL_MG_ID_BYTES)
        rc = lib.fl_mg_unique_id(buf, L.FL_MG_ID_BYTES)
        if rc != L.FL_OK:
            raise FealessError(rc, "fl_mg_unique_id (ncclGetUniqueId) failed")
        return buf.raw

    def __init__(self, det, unique_id, n_ranks, rank, tid_first, tid_count, k):
        self.lib = L.load_mg()
        self.det = det
        h = C.c_void_p()
        rc = self.lib.fl_mg_create(det.h, C.c_char_p(unique_id), n_ranks, rank, tid_first, tid_count, k, C.byref(h))
        if rc != L.FL_OK:
            raise FealessError(rc, "fl_mg_create (ncclCommInitRank) failed")
        self.h = h

    def recognize_batch(self, bgr_ptrs, depth_ptrs, K, params, mem=L.FL_MEM_DEVICE):
        n = len(bgr_ptrs)
        bp = (C.c_void_p * n)(*bgr_ptrs)
        dp = (C.c_void_p * n)(*depth_ptrs)
        k = L.Intrinsics(self.det.w0, self.det.h0, *K)
        res = (L.MgResult * n)()
        rc = self.lib.fl_mg_recognize_batch(self.h, n, bp, dp, mem, C.byref(k), C.byref(params), res)
        if rc != L.FL_OK:
            raise FealessError(rc, self.lib.fl_mg_last_error(self.h).decode(errors="replace"))
        return res

    def stats(self):
        a, g, r = C.c_int32(), C.c_size_t(), C.c_size_t()
        self.lib.fl_mg_last_stats(self.h, C.byref(a), C.byref(g), C.byref(r))
        return dict(attempts=a.value, allgather_bytes=g.value, allreduce_bytes=r.value)

    def close(self):
        if self.h:
            self.lib.fl_mg_destroy(self.h)
            self.h = None


def view_sphere(subdivisions, distances_mm, n_inplane=1, inplane_deg=0.0, upper_hemisphere=False):
    """fl_view_sphere: camera poses around the object origin, (n, 13) float32 in the bank's pose layout."""
    lib = L.load()
    d = np.ascontiguousarray(np.atleast_1d(distances_mm), np.float32)
    n = C.c_int()
    args = (int(subdivisions), int(bool(upper_hemisphere)), _ptr(d), len(d), int(n_inplane), float(inplane_deg))
    rc = lib.fl_view_sphere(*args, None, 0, C.byref(n))
    if rc != L.FL_OK:
        raise FealessError(rc, "fl_view_sphere: invalid arguments")
    out = np.zeros((n.value, 13), np.float32)
    rc = lib.fl_view_sphere(*args, _ptr(out), n.value, C.byref(n))
    if rc != L.FL_OK:
        raise FealessError(rc, "fl_view_sphere")
    return out


def merge_topk_batch(gathered, n_ranks, n_frames, k, cap):
    """fl_merge_topk_batch: gathered[(rank * n_frames + frame) * k + i] -> (out[n_frames, cap], n_out[n_frames])."""
    lib = L.load()
    rec = np.ascontiguousarray(gathered, MATCH_DTYPE)
    assert rec.size == n_ranks * n_frames * k
    out = np.zeros((n_frames, cap), MATCH_DTYPE)
    n_out = (C.c_int * n_frames)()
    rc = lib.fl_merge_topk_batch(_ptr(rec), n_ranks, n_frames, k, _ptr(out), cap, n_out)
    if rc < 0:
        raise FealessError(rc, "fl_merge_topk_batch")
    return out, np.array(n_out[:], np.int32)


def merge_topk(records, cap):
    """Host merge of all-gathered top-k records (fl_merge_topk): numpy MATCH_DTYPE in/out."""
    lib = L.load()
    rec = np.ascontiguousarray(records, MATCH_DTYPE)
    out = np.zeros(cap, MATCH_DTYPE)
    n = lib.fl_merge_topk(_ptr(rec), len(rec), _ptr(out), cap)
    if n < 0:
        raise FealessError(n, "fl_merge_topk")
    return out[:n]


def _poses13(poses):
    """(n, 13) float32 from (n, 13) or (n, 4, 4) poses."""
    p = np.asarray(poses, np.float32)
    if p.ndim == 3 and p.shape[1:] == (4, 4):
        p = np.concatenate([p[:, :3, :].reshape(-1, 12), np.zeros((len(p), 1), np.float32)], 1)
    return np.ascontiguousarray(p, np.float32).reshape(-1, 13)


# what a field holds when only some keywords are given: the library's own defaults (k_track_defaults, k_verify_defaults)
_TRACK_DEFAULTS = dict(margin_px=12, passes=1, icp_it_thr=10, dist_mean_thr=0.5, dist_diff_thr=0.01, icp_mode=L.FL_ICP_POINT_TO_PLANE,
                       max_dist_mean=0.0, min_px_ratio=0.0)
_VERIFY_DEFAULTS = dict(tau_mm=10, min_model_px=1, min_inlier_ratio=0.0, max_behind_ratio=0.0)


def _params_struct(who, struct, defaults, params):
    """A parameter struct from keyword arguments, the fields not named from `defaults`; None (the library's defaults) when no
    keyword is given.  TypeError for a keyword that is no field of the struct."""
    if not params:
        return None
    unknown = set(params) - {f[0] for f in struct._fields_}
    if unknown:
        raise TypeError(f"{who}: unknown parameters {sorted(unknown)}")
    return struct(**dict(defaults, **params))


_SCENE_DEFAULTS = dict(_VERIFY_DEFAULTS, max_shared_ratio=0.5, min_shared_px=1)    # k_scene_defaults


def _scene_params(who, params):
    """fl_scene_params from keyword arguments (the fields of fl_verify_params, max_shared_ratio, min_shared_px), the fields not
    named at the library's defaults; None when no keyword is given."""
    if not params:
        return None
    unknown = set(params) - set(_SCENE_DEFAULTS)
    if unknown:
        raise TypeError(f"{who}: unknown parameters {sorted(unknown)}")
    P = dict(_SCENE_DEFAULTS, **params)
    return L.SceneParams(L.VerifyParams(*[P[k] for k in _VERIFY_DEFAULTS]), P["max_shared_ratio"], P["min_shared_px"])


def scene_pick(records, scene_first, shared, **params):
    """fl_scene_pick, host only: the order and the suppression of Tracker.verify_scene alone, on a VERIFY_DTYPE array, the
    scenes and the compact shared array (None where no scene has a pair).  Returns a SCENE_DTYPE array."""
    lib = L.load()
    rec = np.ascontiguousarray(records, VERIFY_DTYPE).ravel()
    sf = np.ascontiguousarray(scene_first, np.int32).ravel()
    sh = None if shared is None else np.ascontiguousarray(shared, np.int32).ravel()
    m = np.diff(sf.astype(np.int64))
    if len(sf) < 2 or (sh is not None and len(sh) < int((m * (m - 1) // 2).sum())):
        raise ValueError("scene_pick: scene_first has n_scenes + 1 entries, shared one entry per pair")
    prm = _scene_params("scene_pick", params)
    out = np.zeros(max(1, len(rec)), SCENE_DTYPE)
    rc = lib.fl_scene_pick(_ptr(rec) if len(rec) else _ptr(np.zeros(1, VERIFY_DTYPE)), len(rec), len(sf) - 1, _ptr(sf), None if sh is None else _ptr(sh),
                           None if prm is None else C.byref(prm), _ptr(out))
    if rc != L.FL_OK:
        raise FealessError(rc, "fl_scene_pick")
    return out[:len(rec)]


def scene_of_instances(results, n_instances, mesh_of_class):
    """What Tracker.verify_scene takes, from the output of Detector.recognize_batch_instances_verified: results, a list per
    frame of result dicts; n_instances, the number of instances of every frame (None: all of each list); mesh_of_class, the
    mesh of every class or -1.  Returns (frame_of_pose, poses13, scene_first, mesh_of) over the instances with found == 1 whose
    class has a mesh, in list order, one scene per frame (a frame without such an instance: an empty scene)."""
    frame_of, poses, mesh_of, scene_first = [], [], [], [0]
    for f, row in enumerate(results):
        for r in row[:len(row) if n_instances is None else int(n_instances[f])]:
            m = int(mesh_of_class[int(r["best"]["class_idx"])]) if r["found"] == 1 else -1
            if m >= 0:
                frame_of.append(f)
                poses.append(np.asarray(r["pose"], np.float32).reshape(4, 4))
                mesh_of.append(m)
        scene_first.append(len(frame_of))
    p = _poses13(np.stack(poses)) if poses else np.zeros((0, 13), np.float32)
    return np.array(frame_of, np.int32), p, np.array(scene_first, np.int32), np.array(mesh_of, np.int32)


class Tracker:
    """fl_tracker: follows objects from frame to frame against their CAD mesh (render at the previous pose, crop, detection()
    from that pose).  Owns its device memory: the mesh, max_frames depth frames of w x h, max_tracks renders and ICP workspaces
    for crops of up to max_crop_px pixels.  Tracker(ctx, vertices, triangles, w, ...) holds one mesh; Tracker(ctx,
    meshes=[(vertices, triangles), ...], w=..., ...) holds several (fl_tracker_create_meshes), which share everything but the
    mesh itself: track(), verify() and track_verified() then take mesh_of, the mesh of every track or pose."""

    def __init__(self, ctx, vertices=None, triangles=None, w=None, h=None, max_frames=None, max_tracks=None, max_crop_px=None, meshes=None):
        self.ctx = ctx
        self.lib = ctx.lib
        if (meshes is None) == (vertices is None) or (meshes is None and triangles is None):
            raise TypeError("Tracker: give vertices and triangles, or meshes=[(vertices, triangles), ...]")
        if None in (w, h, max_frames, max_tracks, max_crop_px):
            raise TypeError("Tracker: w, h, max_frames, max_tracks and max_crop_px are required")
        self.w, self.h, self.max_frames, self.max_tracks, self.max_crop_px = w, h, max_frames, max_tracks, max_crop_px
        h_ = C.c_void_p()
        if meshes is None:
            v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
            t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
            ctx.check(self.lib.fl_tracker_create(ctx.h, _ptr(v), len(v), _ptr(t), len(t), w, h, max_frames, max_tracks, max_crop_px, C.byref(h_)))
        else:
            keep = [(np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(t, np.int32).reshape(-1, 3)) for v, t in meshes]
            arr = (L.Mesh * max(1, len(keep)))(*[L.Mesh(v.ctypes.data, t.ctypes.data, len(v), len(t)) for v, t in keep])
            ctx.check(self.lib.fl_tracker_create_meshes(ctx.h, arr, len(keep), w, h, max_frames, max_tracks, max_crop_px, C.byref(h_)))
        self.handle = h_

    @property
    def num_meshes(self):
        """fl_tracker_num_meshes: the number of meshes the tracker holds."""
        return int(self.lib.fl_tracker_num_meshes(self.handle))

    @staticmethod
    def _mesh_of(who, mesh_of, n):
        """The mesh_of argument of a call over n poses: None, or an int32 array of n mesh indices."""
        if mesh_of is None:
            return None
        m = np.ascontiguousarray(mesh_of, np.int32).ravel()
        if len(m) != n:
            raise ValueError(f"{who}: one mesh index per pose")
        return m

    def _frames(self, depths, who):
        """(n, pointer array, device?) of a list of frames: (h, w) u16 numpy arrays, or device tensors, all of one kind.  The
        pointer array's owner keeps the (possibly converted) frames alive through its _frames attribute."""
        depths = list(depths)
        device = len(depths) > 0 and hasattr(depths[0], "data_ptr")
        if device:
            for d in depths:
                if d.numel() != self.w * self.h or d.element_size() != 2 or not d.is_contiguous():
                    raise ValueError(f"{who}: device frames must be contiguous {self.h} x {self.w} 16-bit tensors")
            ptrs = [d.data_ptr() for d in depths]
        else:
            depths = [np.ascontiguousarray(d, np.uint16) for d in depths]
            for d in depths:
                if d.shape != (self.h, self.w):
                    raise ValueError(f"{who}: frames must be {self.h} x {self.w}")
            ptrs = [d.ctypes.data for d in depths]
        dp = (C.c_void_p * max(1, len(ptrs)))(*ptrs)
        dp._frames = depths
        return len(ptrs), dp, device

    def _batch(self, who, what, depths, frame_of, poses, K, dtype):
        """What track() and verify() hand the library alike: (n_frames, frame pointers, mem, n, frame_of, poses13) to pass on as
        they are, then the Intrinsics and the zeroed output array."""
        n_frames, dp, device = self._frames(depths, who)
        fof = np.ascontiguousarray(frame_of, np.int32).ravel()
        p = _poses13(poses)
        if len(p) != len(fof):
            raise ValueError(f"{who}: one pose per {what}")
        k = L.Intrinsics(self.w, self.h, *[float(x) for x in K])
        return (n_frames, dp, L.FL_MEM_DEVICE if device else L.FL_MEM_HOST, len(fof), fof, p), k, np.zeros(max(1, len(fof)), dtype)

    def track(self, depths, frame_of_track, poses13, K, mesh_of=None, **params):
        """One step of every track (fl_track_batch_meshes; mesh_of: the mesh of every track on a tracker of several, None:
        mesh 0).  depths: the frames, (h, w) u16 numpy arrays in mm, or device tensors
        (anything with data_ptr(): all of one kind); frame_of_track: the frame each track looks at; poses13: (n_tracks, 13)
        or (n_tracks, 4, 4) poses to start from; K = (fx, fy, cx, cy) of the scene camera.  params: the fields of
        fl_track_params (margin_px, passes, icp_it_thr, dist_mean_thr, dist_diff_thr, icp_mode, max_dist_mean, min_px_ratio);
        none given = the library's defaults.  Returns a TRACK_DTYPE array, one record per track; feed its poses back in
        (poses13_of) for the next frame."""
        (n_frames, dp, mem, n, fof, p), k, out = self._batch("Tracker.track", "track", depths, frame_of_track, poses13, K, TRACK_DTYPE)
        prm = _params_struct("Tracker.track", L.TrackParams, _TRACK_DEFAULTS, params)
        mo = self._mesh_of("Tracker.track", mesh_of, n)
        self.ctx.check(self.lib.fl_track_batch_meshes(self.handle, n_frames, dp, mem, n, _ptr(fof), None if mo is None else _ptr(mo), _ptr(p),
                                                      C.byref(k), None if prm is None else C.byref(prm), _ptr(out)))
        return out[:n]

    def verify(self, depths, frame_of_pose, poses, K, group_first=None, mesh_of=None, **params):
        """Hypothesis verification (fl_verify_batch_meshes; mesh_of: the mesh of every pose, None: mesh 0): the mesh rendered at every pose with the scene camera K = (fx, fy, cx, cy)
        and laid over the pose's depth frame.  depths, frame_of_pose and poses ((n, 13) or (n, 4, 4): the `pose` fields of
        recognize_instances / track results feed straight in) are as track() takes them.  group_first: None (every pose is its
        own group, best = accepted) or n_groups + 1 non-decreasing indices from 0 to n; one pose per group at most comes back
        with best = 1.  params: the fields of fl_verify_params (tau_mm, min_model_px, min_inlier_ratio, max_behind_ratio); none
        given = the library's defaults.  Returns a VERIFY_DTYPE array, one record per pose."""
        (n_frames, dp, mem, n, fof, p), k, out = self._batch("Tracker.verify", "frame index", depths, frame_of_pose, poses, K, VERIFY_DTYPE)
        gf = None
        if group_first is not None:
            gf = np.ascontiguousarray(group_first, np.int32).ravel()
            if len(gf) < 2:
                raise ValueError("Tracker.verify: group_first has n_groups + 1 entries")
        prm = _params_struct("Tracker.verify", L.VerifyParams, _VERIFY_DEFAULTS, params)
        mo = self._mesh_of("Tracker.verify", mesh_of, n)
        self.ctx.check(self.lib.fl_verify_batch_meshes(self.handle, n_frames, dp, mem, n, _ptr(fof), None if mo is None else _ptr(mo), _ptr(p),
                                                       0 if gf is None else len(gf) - 1, None if gf is None else _ptr(gf), C.byref(k),
                                                       None if prm is None else C.byref(prm), _ptr(out)))
        return out[:n]

    def track_verified(self, depths, frame_of_track, poses13, K, group_first=None, keep_input=0, tau_mm=10, min_model_px=1,
                       min_inlier_ratio=0.0, max_behind_ratio=0.0, mesh_of=None, **track_params):
        """One step of every track whose `tracked` is the verification's (fl_track_batch_verified): track()'s passes, then on
        the device the pose each tracked track came out with rendered at the scene camera and laid over its frame, as verify()
        does it; a track whose pose is not accepted comes back lost.  keep_input = 1: the pose a track came in with is verified
        too and kept where it verifies strictly better.  group_first: None, or verify()'s groups over the tracks (several start
        poses for one object); one track per group at most comes back with best = 1.  tau_mm .. max_behind_ratio: the fields of
        fl_verify_params; mesh_of: the mesh of every track (None: mesh 0); track_params: the fields of fl_track_params.  Returns a VERIFIED_TRACK_DTYPE array, one record per
        track; poses13_of(result["track"]) feeds the next frame."""
        who = "Tracker.track_verified"
        (n_frames, dp, mem, n, fof, p), k, out = self._batch(who, "track", depths, frame_of_track, poses13, K, VERIFIED_TRACK_DTYPE)
        gf = None
        if group_first is not None:
            gf = np.ascontiguousarray(group_first, np.int32).ravel()
            if len(gf) < 2:
                raise ValueError(f"{who}: group_first has n_groups + 1 entries")
        prm = _params_struct(who, L.TrackParams, _TRACK_DEFAULTS, track_params)
        vp = L.TrackVerifyParams(L.VerifyParams(int(tau_mm), int(min_model_px), float(min_inlier_ratio), float(max_behind_ratio)), int(keep_input), 0)
        mo = self._mesh_of(who, mesh_of, n)
        self.ctx.check(self.lib.fl_track_batch_verified_meshes(self.handle, n_frames, dp, mem, n, _ptr(fof), None if mo is None else _ptr(mo),
                                                               _ptr(p), 0 if gf is None else len(gf) - 1, None if gf is None else _ptr(gf),
                                                               C.byref(k), None if prm is None else C.byref(prm), C.byref(vp), _ptr(out)))
        return out[:n]

    def verify_scene(self, depths, frame_of_pose, poses, K, scene_first, mesh_of=None, **params):
        """Scene arbitration (fl_verify_scene_batch): every pose verified as verify() verifies it (mesh_of: the mesh of every
        pose, None: mesh 0), then per scene -- the poses scene_first[s] .. scene_first[s + 1] - 1, all on one frame, 64 at the
        most -- the accepted poses in the order of their n_inlier, a pose suppressed when a kept pose before it shares at least
        min_shared_px and max_shared_ratio of its supporting pixels.  params: the fields of fl_verify_params (tau_mm,
        min_model_px, min_inlier_ratio, max_behind_ratio) and max_shared_ratio (0.5), min_shared_px (1); none given = the
        library's defaults.  Returns a SCENE_DTYPE array, one record per pose: verify (verify()'s record), kept, order, rival,
        n_shared."""
        who = "Tracker.verify_scene"
        (n_frames, dp, mem, n, fof, p), k, out = self._batch(who, "frame index", depths, frame_of_pose, poses, K, SCENE_DTYPE)
        sf = np.ascontiguousarray(scene_first, np.int32).ravel()
        if len(sf) < 2:
            raise ValueError(f"{who}: scene_first has n_scenes + 1 entries")
        prm = _scene_params(who, params)
        mo = self._mesh_of(who, mesh_of, n)
        self.ctx.check(self.lib.fl_verify_scene_batch(self.handle, n_frames, dp, mem, n, _ptr(fof), None if mo is None else _ptr(mo), _ptr(p),
                                                      len(sf) - 1, _ptr(sf), C.byref(k), None if prm is None else C.byref(prm), _ptr(out)))
        return out[:n]

    def dev_scene_shared(self):
        """DEVELOPMENT ONLY (fl_dev_tracker_scene_shared, not part of the C ABI): the compact shared array of the last
        verify_scene(), int32: the pair of local indices i < j of scene s at pair_first(s) + j (j - 1) / 2 + i."""
        fn = L.dev(self.lib, "fl_dev_tracker_scene_shared")
        n = C.c_int(0)
        rc = fn(self.handle, None, 0, C.byref(n))
        if rc != L.FL_ERR_OVERFLOW:
            self.ctx.check(rc)
        out = np.zeros(max(1, n.value), np.int32)
        self.ctx.check(fn(self.handle, _ptr(out), n.value, C.byref(n)))
        return out[:n.value]

    def scene_ms(self):
        """DEVELOPMENT ONLY (fl_dev_tracker_scene_ms, not part of the C ABI): device time of the last verify_scene() by stage:
        dict(copy, render, score, finish, overlap, pick) in ms."""
        out = (C.c_float * 6)()
        self.ctx.check(L.dev(self.lib, "fl_dev_tracker_scene_ms")(self.handle, out))
        return dict(zip(("copy", "render", "score", "finish", "overlap", "pick"), [float(v) for v in out]))

    def track_verified_ms(self):
        """DEVELOPMENT ONLY (fl_dev_tracker_track_verified_ms, not part of the C ABI): device time of the stages the last
        track_verified() ran after its passes: dict(fused, finish) in ms; stage_ms() has the passes."""
        out = (C.c_float * 2)()
        self.ctx.check(L.dev(self.lib, "fl_dev_tracker_track_verified_ms")(self.handle, out))
        return dict(zip(("fused", "finish"), [float(v) for v in out]))

    def verify_ms(self):
        """DEVELOPMENT ONLY (fl_dev_tracker_verify_ms, not part of the C ABI): device time of the last verify() by stage:
        dict(copy, render, score, finish) in ms."""
        out = (C.c_float * 4)()
        self.ctx.check(L.dev(self.lib, "fl_dev_tracker_verify_ms")(self.handle, out))
        return dict(zip(("copy", "render", "score", "finish"), [float(v) for v in out]))

    def stage_ms(self):
        """DEVELOPMENT ONLY (fl_dev_tracker_stage_ms, not part of the C ABI): device time of the last track() by stage, summed
        over its passes: dict(copy, render, rects, icp, finish) in ms."""
        out = (C.c_float * 5)()
        self.ctx.check(L.dev(self.lib, "fl_dev_tracker_stage_ms")(self.handle, out))
        return dict(zip(("copy", "render", "rects", "icp", "finish"), [float(v) for v in out]))

    def close(self):
        if self.handle:
            self.lib.fl_tracker_destroy(self.handle)
            self.handle = None


def poses13_of(track_results):
    """The (n, 13) pose array that feeds a TRACK_DTYPE result array (Tracker.track's, or the "track" part of
    Tracker.track_verified's) back into either."""
    r = np.atleast_1d(track_results)
    out = np.zeros((len(r), 13), np.float32)
    out[:, :12] = r["pose"][:, :12]
    return out
