"""numpy statement of hypothesis verification (fl_verify_batch, include/fealess_hip.h), test infrastructure only.

Written from the header's text, not by calling the library: the render is tests/raster_model.py (the float32 restatement
fl_render_views is tested against) at the SCENE camera, the counts are sums of boolean masks over int64 images, each ratio is
one np.float32 division and the pick is a plain loop with Python's integers.
"""
import numpy as np

import raster_model as RM

f32 = np.float32
DEFAULTS = dict(tau_mm=10, min_model_px=1, min_inlier_ratio=0.0, max_behind_ratio=0.0)
# the layout of fl_verify_result
DTYPE = np.dtype([("status", "<i4"), ("accepted", "<i4"), ("best", "<i4"), ("rect", "<i4", 4), ("n_model", "<i4"), ("n_missing", "<i4"),
                  ("n_inlier", "<i4"), ("n_front", "<i4"), ("n_behind", "<i4"), ("sum_abs_inlier", "<i8"), ("inlier_ratio", "<f4"),
                  ("behind_ratio", "<f4")])
COUNTS = ("n_model", "n_missing", "n_inlier", "n_front", "n_behind")


def render(mesh, pose13, K, w, h):
    """The mesh at one pose, depth only, in mm, at the scene camera K = (fx, fy, cx, cy) (float32 inside the rasteriser)."""
    return RM.render_view(mesh["vertices"], mesh["triangles"], np.asarray(pose13, f32), K, w, h)[1]


def score(render_mm, scene_mm, **params):
    """One pose's record (best left 0) from its render and its frame, both (h, w) u16 in mm."""
    P = dict(DEFAULTS, **params)
    tau = int(P["tau_mm"])
    out = np.zeros((), DTYPE)
    r, s = render_mm.astype(np.int64), scene_mm.astype(np.int64)
    model = r != 0
    if not model.any():                         # an empty render: FL_OK, not accepted, everything zero
        return out
    d = s - r
    missing = model & (s == 0)
    seen = model & (s != 0)
    inlier = seen & (np.abs(d) <= tau)
    front = seen & (d < -tau)
    behind = seen & (d > tau)
    ys, xs = np.nonzero(model)
    x0, x1, y0, y1 = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())
    out["rect"] = (x0, y0, x1 - x0 + 1, y1 - y0 + 1)
    n_model, n_inlier, n_behind = int(model.sum()), int(inlier.sum()), int(behind.sum())
    out["n_model"], out["n_missing"], out["n_inlier"] = n_model, int(missing.sum()), n_inlier
    out["n_front"], out["n_behind"] = int(front.sum()), n_behind
    out["sum_abs_inlier"] = int(np.abs(d)[inlier].sum())
    out["inlier_ratio"] = f32(n_inlier) / f32(n_model)
    out["behind_ratio"] = f32(n_behind) / f32(n_model)
    lo, hi = f32(P["min_inlier_ratio"]), f32(P["max_behind_ratio"])
    out["accepted"] = int(n_model >= int(P["min_model_px"]) and (lo <= 0 or out["inlier_ratio"] >= lo) and
                          (hi <= 0 or out["behind_ratio"] <= hi))
    return out


def pick(records, group_first=None):
    """Sets `best` in a DTYPE array: per group the accepted pose with the largest n_inlier / n_model, compared exactly, a tie
    to the lower index; no groups: best = accepted."""
    records["best"] = 0
    if group_first is None:
        records["best"] = records["accepted"]
        return records
    gf = [int(v) for v in group_first]
    for g in range(len(gf) - 1):
        best = -1
        for i in range(gf[g], gf[g + 1]):
            if not records["accepted"][i]:
                continue
            if best < 0 or int(records["n_inlier"][i]) * int(records["n_model"][best]) > int(records["n_inlier"][best]) * int(records["n_model"][i]):
                best = i
        if best >= 0:
            records["best"][best] = 1
    return records


def verify(mesh, scenes, frame_of_pose, poses13, K, group_first=None, renders=None, **params):
    """fl_verify_batch: a DTYPE array, one record per pose.  renders: the poses' renders where the caller has them already."""
    poses13 = np.asarray(poses13, f32).reshape(-1, 13)
    out = np.zeros(len(poses13), DTYPE)
    for i, p in enumerate(poses13):
        scene = np.asarray(scenes[int(frame_of_pose[i])])
        h, w = scene.shape
        out[i] = score(render(mesh, p, K, w, h) if renders is None else renders[i], scene, **params)
    return pick(out, group_first)


def invariant(records):
    r = np.atleast_1d(records)
    return bool((r["n_model"] == r["n_missing"] + r["n_inlier"] + r["n_front"] + r["n_behind"]).all())
