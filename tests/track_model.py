"""numpy statement of one tracking step (fl_track_batch, include/fealess_hip.h), test infrastructure only.

The rectangle rule, the x10 / rint(d * 0.1f) round trip of the model image and the lost rule are written here from the header's
text, not by calling the library; the render is tests/raster_model.py (the float32 restatement fl_render_views is tested against)
and detection() is the oracle's (FL_ICP_PARITY, bit for bit) or tests/p2plane_model.py's (FL_ICP_POINT_TO_PLANE).
"""
import numpy as np

import raster_model as RM

f32 = np.float32
MODEL_K = (608.0, 608.0, 320.0, 240.0)       # initInternalMat (ICP/common.cpp:358): what detection() back-projects the model with
SHIFT_MAX = 2.0 ** 20
PARITY, FAST, POINT_TO_PLANE = 0, 1, 2
OK, OVERFLOW = 0, -4
DEFAULTS = dict(margin_px=12, passes=1, icp_it_thr=10, dist_mean_thr=0.5, dist_diff_thr=0.01, icp_mode=POINT_TO_PLANE,
                max_dist_mean=0.0, min_px_ratio=0.0)


def bounding_box(depth):
    """Inclusive (x0, x1, y0, y1) of the non-zero pixels, or None."""
    ys, xs = np.nonzero(depth)
    if len(xs) == 0:
        return None
    return int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())


def shift(K, t):
    """(dx, dy) of rect_ref against rect_model, or None where it is not finite or beyond 2^20 pixels.  fp64, one operation
    per operator; t = the pose's translation as float32 values."""
    fx, fy, cx, cy = (np.float64(v) for v in K)
    tx, ty, tz = (np.float64(f32(v)) for v in t)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sx = (fx - np.float64(608.0)) * (tx / tz) + (cx - np.float64(320.0))
        sy = (fy - np.float64(608.0)) * (ty / tz) + (cy - np.float64(240.0))
    if not (abs(sx) <= SHIFT_MAX and abs(sy) <= SHIFT_MAX):
        return None
    return int(np.rint(sx)), int(np.rint(sy))


def rects_from_box(box, w, h, margin, d):
    """The rule on a bounding box (x0, x1, y0, y1) and a shift d = (dx, dy): (rect_model, rect_ref) as (x, y, w, h), or None
    (out of view)."""
    if box is None or d is None:
        return None
    x0, x1, y0, y1 = box
    mx0, my0 = max(x0 - margin, 0), max(y0 - margin, 0)
    mx1, my1 = min(x1 + margin, w - 1), min(y1 + margin, h - 1)
    dx, dy = d
    cx0, cy0 = max(mx0 + dx, 0), max(my0 + dy, 0)
    cx1, cy1 = min(mx1 + dx, w - 1), min(my1 + dy, h - 1)
    if cx1 < cx0 or cy1 < cy0:
        return None
    rr = (cx0, cy0, cx1 - cx0 + 1, cy1 - cy0 + 1)
    return (cx0 - dx, cy0 - dy, rr[2], rr[3]), rr


def rects(render_mm, pose13, K, margin):
    h, w = render_mm.shape
    p = np.asarray(pose13, f32)
    return rects_from_box(bounding_box(render_mm), w, h, margin, shift(K, (p[3], p[7], p[11])))


def times10(depth_mm):
    """The render in 0.1 mm, saturating, as k_track_rects leaves it inside rect_model."""
    return np.minimum(depth_mm.astype(np.uint32) * 10, 65535).astype(np.uint16)


def back_to_mm(depth_01mm):
    """What the recognition branch of the ICP kernel makes of a 0.1 mm model image: rint(d * 0.1f), clamped to u16
    (convertTo(CV_16UC1, 0.1), obj_reco_lmicp.cpp:188)."""
    v = np.rint(depth_01mm.astype(f32) * f32(0.1))
    return np.clip(v, 0, 65535).astype(np.uint16)


def is_lost(found, dist_mean, px_ratio, max_dist_mean=0.0, min_px_ratio=0.0):
    return bool(not found or dist_mean < 0 or (max_dist_mean > 0 and dist_mean > max_dist_mean) or
                (min_px_ratio > 0 and px_ratio < min_px_ratio))


def pose4x4(pose13):
    m = np.zeros((4, 4), f32)
    m[:3, :] = np.asarray(pose13, f32)[:12].reshape(3, 4)
    m[3, 3] = 1
    return m


def render(mesh, pose13, w, h):
    return RM.render_view(mesh["vertices"], mesh["triangles"], np.asarray(pose13, f32), MODEL_K, w, h)[1]


def step(mesh, pose13, scene_mm, K, max_crop_px=None, oracle=None, **params):
    """One pass of one track.  Returns dict(status, tracked, rect_model, rect_ref, pose (4, 4) f32, det or None); det is the
    detection() dict of oracle_py (parity; `oracle` = that module) or p2plane_model (point-to-plane)."""
    P = dict(DEFAULTS, **params)
    h, w = scene_mm.shape
    p13 = np.asarray(pose13, f32)
    out = dict(status=OK, tracked=0, rect_model=(0, 0, 0, 0), rect_ref=(0, 0, 0, 0), pose=pose4x4(p13), det=None)
    rend = render(mesh, p13, w, h)
    r = rects(rend, p13, K, P["margin_px"])
    if r is None:
        return out
    out["rect_model"], out["rect_ref"] = r
    if max_crop_px is not None and r[0][2] * r[0][3] > max_crop_px:
        out["status"] = OVERFLOW
        return out
    model = back_to_mm(times10(rend))
    Rm, tm = p13[:12].reshape(3, 4)[:, :3], p13[:12].reshape(3, 4)[:, 3]
    args = (model, scene_mm, K, r[0], r[1], P["icp_it_thr"], P["dist_mean_thr"], P["dist_diff_thr"], Rm, tm)
    if P["icp_mode"] == PARITY:
        det = oracle.detection(*args)
    elif P["icp_mode"] == POINT_TO_PLANE:
        import p2plane_model as PM
        ref, _, _, _ = PM.crop_pairs(model, scene_mm, K, r[0], r[1])
        if len(ref) < 3:                            # icpCloudToCloud_Ex returns -1 below three points
            det = dict(R_final=Rm.copy(), T_final=tm.copy(), n_points=len(ref),
                       icp=dict(R=np.eye(3, dtype=f32), T=np.zeros(3, f32), dist_mean=-1.0, px_ratio=0.0, iters=0, n_corr_last=0))
        else:
            det = PM.detection_point_to_plane(*args)
    else:
        raise ValueError("track_model.step: parity or point-to-plane")
    out["det"] = det
    ic = det["icp"]
    if is_lost(1, float(ic["dist_mean"]), float(ic["px_ratio"]), P["max_dist_mean"], P["min_px_ratio"]):
        return out
    out["tracked"] = 1
    m = np.zeros((4, 4), f32)
    m[:3, :3] = det["R_final"]
    m[:3, 3] = det["T_final"]
    m[3, 3] = 1
    out["pose"] = m
    return out


def pose13_of(pose4):
    p = np.zeros(13, f32)
    p[:12] = np.asarray(pose4, f32)[:3, :].ravel()
    p[12] = np.linalg.norm(p[[3, 7, 11]])
    return p


def pose_error(pose4, R_true, t_true):
    """(rotation error in degrees, translation error in mm) of a 4x4 pose against ground truth."""
    M = np.asarray(pose4, np.float64)[:3, :3] @ np.asarray(R_true, np.float64).T
    s = 0.5 * np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])      # atan2: accurate for small angles too
    return float(np.degrees(np.arctan2(s, (np.trace(M) - 1) / 2))), float(np.linalg.norm(np.asarray(pose4, np.float64)[:3, 3] - t_true))
