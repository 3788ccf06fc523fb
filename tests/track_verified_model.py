"""numpy / Python statement of verified tracking (fl_track_batch_verified, include/fealess_hip.h), test infrastructure only.

Composed from the two models it joins: track_model.step iterated over the passes, verify_model.verify at the SCENE camera on the
pose the passes returned (and on the input pose with keep_input), then the decision and the pick as loops over Python integers,
written from the header's text.
"""
import numpy as np

import track_model as TM
import verify_model as VM

f32 = np.float32
_ICP_DT = np.dtype([("R", "<f4", 9), ("T", "<f4", 3), ("dist_mean", "<f4"), ("px_ratio", "<f4"), ("iters", "<i4"), ("n_corr_last", "<i4")])
_DET_DT = np.dtype([("R_final", "<f4", 9), ("T_final", "<f4", 3), ("icp", _ICP_DT), ("n_points", "<i4"), ("status", "<i4")])
# the layout of fl_track_result and of fl_verified_track_result
TRACK_DTYPE = np.dtype([("status", "<i4"), ("tracked", "<i4"), ("rect_model", "<i4", 4), ("rect_ref", "<i4", 4), ("pose", "<f4", 16),
                        ("det", _DET_DT)])
DTYPE = np.dtype([("track", TRACK_DTYPE), ("verify", VM.DTYPE), ("verify_in", VM.DTYPE), ("icp_tracked", "<i4"), ("kept_input", "<i4"),
                  ("best", "<i4"), ("reserved", "<i4")])
VERIFY_KEYS = ("tau_mm", "min_model_px", "min_inlier_ratio", "max_behind_ratio")


def decide(icp_tracked, verify, verify_in, keep_input):
    """(tracked, kept_input) of one track from its two records (anything indexable by field name)."""
    if not icp_tracked:
        return 0, 0
    a = bool(verify["accepted"])
    b = bool(keep_input) and bool(verify_in["accepted"])
    if not a and not b:
        return 0, 0
    if b and (not a or int(verify_in["n_inlier"]) * int(verify["n_model"]) > int(verify["n_inlier"]) * int(verify_in["n_model"])):
        return 1, 1
    return 1, 0


def pick(tracked, kept_input, verify, verify_in, group_first=None):
    """`best` per track: per group the tracked track whose chosen record (verify_in where kept_input, else verify) has the
    largest n_inlier / n_model, compared exactly, a tie to the lower index; no groups: best = tracked."""
    n = len(tracked)
    if group_first is None:
        return [int(bool(t)) for t in tracked]
    best = [0] * n
    chosen = [(verify_in if kept_input[i] else verify)[i] for i in range(n)]
    gf = [int(v) for v in group_first]
    for g in range(len(gf) - 1):
        b = -1
        for i in range(gf[g], gf[g + 1]):
            if not tracked[i]:
                continue
            if b < 0 or int(chosen[i]["n_inlier"]) * int(chosen[b]["n_model"]) > int(chosen[b]["n_inlier"]) * int(chosen[i]["n_model"]):
                b = i
        if b >= 0:
            best[b] = 1
    return best


def track_passes(mesh, pose13, scene_mm, K, passes=1, **kw):
    """fl_track_batch on one track: track_model.step `passes` times, each from the pose of the one before; a pass that loses the
    track ends it, with that pass's record and the pose the call came in with."""
    p_in = np.asarray(pose13, f32)
    p, out = p_in, None
    for _ in range(passes):
        out = TM.step(mesh, p, scene_mm, K, **kw)
        if not out["tracked"]:
            out["pose"] = TM.pose4x4(p_in)
            return out
        p = TM.pose13_of(out["pose"])
    return out


def track_verified(mesh, scenes, frame_of_track, poses13, K, group_first=None, keep_input=0, **params):
    """fl_track_batch_verified.  params: fl_verify_params' fields go to the verification, everything else to track_passes
    (fl_track_params' fields, max_crop_px, oracle).  Returns one dict per track: track (track_passes' dict, with tracked and pose
    by the decision), verify and verify_in (verify_model records), icp_tracked, kept_input, best."""
    vp = {k: params.pop(k) for k in VERIFY_KEYS if k in params}
    poses13 = np.asarray(poses13, f32).reshape(-1, 13)
    out = []
    for t, p in enumerate(poses13):
        scene = np.asarray(scenes[int(frame_of_track[t])])
        trk = track_passes(mesh, p, scene, K, **params)
        rec = dict(track=trk, verify=np.zeros((), VM.DTYPE), verify_in=np.zeros((), VM.DTYPE), icp_tracked=int(trk["tracked"]), kept_input=0, best=0)
        if rec["icp_tracked"]:
            rec["verify"] = VM.verify(mesh, [scene], [0], TM.pose13_of(trk["pose"])[None], K, **vp)[0]
            if keep_input:
                rec["verify_in"] = VM.verify(mesh, [scene], [0], p[None], K, **vp)[0]
        trk["tracked"], rec["kept_input"] = decide(rec["icp_tracked"], rec["verify"], rec["verify_in"], keep_input)
        if not trk["tracked"] or rec["kept_input"]:
            trk["pose"] = TM.pose4x4(p)
        out.append(rec)
    best = pick([r["track"]["tracked"] for r in out], [r["kept_input"] for r in out], [r["verify"] for r in out], [r["verify_in"] for r in out],
                group_first)
    for r, b in zip(out, best):
        r["best"] = b
    return out
