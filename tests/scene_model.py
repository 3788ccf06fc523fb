"""numpy statement of scene arbitration (fl_verify_scene_batch and fl_scene_pick, include/fealess_hip.h), test infrastructure only.

Written from the header's text, not by calling the library: a pose's record and its support mask come from
tests/verify_model.py's render and score rule, shared(a, b) is the sum of mask_a & mask_b, the order and the suppression are
plain loops over Python integers with one np.float32 division.
"""
import numpy as np

import verify_model as VM

f32 = np.float32
MAX_POSES = 64
DEFAULTS = dict(VM.DEFAULTS, max_shared_ratio=0.5, min_shared_px=1)
# the layout of fl_scene_result
DTYPE = np.dtype([("verify", VM.DTYPE), ("kept", "<i4"), ("order", "<i4"), ("rival", "<i4"), ("n_shared", "<i4")])


def _split(params):
    unknown = set(params) - set(DEFAULTS)
    assert not unknown, unknown
    P = dict(DEFAULTS, **params)
    return {k: P[k] for k in VM.DEFAULTS}, f32(P["max_shared_ratio"]), int(P["min_shared_px"])


def support(render_mm, scene_mm, tau_mm):
    """The pixels that support a pose: the ones its record counts in n_inlier."""
    r, s = render_mm.astype(np.int64), scene_mm.astype(np.int64)
    return (r != 0) & (s != 0) & (np.abs(s - r) <= int(tau_mm))


def pair_first(scene_first):
    m = np.diff(np.asarray(scene_first, np.int64))
    return np.concatenate([[0], np.cumsum(m * (m - 1) // 2)]).astype(np.int64)


def compact(matrix, scene_first):
    """The compact shared array of a full symmetric (n, n) matrix: local i < j of scene s at pair_first(s) + j (j - 1) / 2 + i."""
    sf, pf = [int(v) for v in scene_first], pair_first(scene_first)
    out = np.zeros(int(pf[-1]), np.int32)
    for s in range(len(sf) - 1):
        for j in range(sf[s + 1] - sf[s]):
            for i in range(j):
                out[pf[s] + j * (j - 1) // 2 + i] = matrix[sf[s] + i, sf[s] + j]
    return out


def before(ra, a, rb, b):
    """Pose a stands before pose b (both accepted verify records)."""
    na, nb, ma, mb = int(ra["n_inlier"]), int(rb["n_inlier"]), int(ra["n_model"]), int(rb["n_model"])
    if na != nb:
        return na > nb
    if na * mb != nb * ma:
        return na * mb > nb * ma
    return a < b


def pick(records, scene_first, shared, **params):
    """fl_scene_pick: DTYPE records from verify records (VM.DTYPE), the scenes and the COMPACT shared array."""
    _, ratio, min_px = _split(params)
    sf, pf = [int(v) for v in scene_first], pair_first(scene_first)
    out = np.zeros(len(records), DTYPE)
    out["verify"] = records
    out["order"], out["rival"] = -1, -1
    for s in range(len(sf) - 1):
        first, m = sf[s], sf[s + 1] - sf[s]
        assert 0 <= m <= MAX_POSES

        def sh(a, b):
            i, j = min(a, b) - first, max(a, b) - first
            return int(shared[pf[s] + j * (j - 1) // 2 + i])

        acc = [t for t in range(first, first + m) if records["accepted"][t]]
        order = sorted(acc, key=lambda t: sum(before(records[u], u, records[t], t) for u in acc if u != t))
        kept = []
        for place, b in enumerate(order):
            out["order"][b] = place
            rival, n_shared, keep = -1, 0, 1
            for a in kept:
                n = sh(a, b)
                if n >= min_px and f32(n) / f32(int(records["n_inlier"][b])) >= ratio:
                    rival, n_shared, keep = a, n, 0
                    break
                if n > n_shared:
                    rival, n_shared = a, n
            if keep:
                kept.append(b)
            out["kept"][b], out["rival"][b], out["n_shared"][b] = keep, rival, n_shared
    return out


def masks_and_records(meshes, scenes, frame_of_pose, poses13, K, mesh_of=None, **verify_params):
    """Per pose the verify record (best = accepted) and the support mask.  meshes: a list of mesh dicts, mesh_of an index per
    pose (None: mesh 0)."""
    poses13 = np.asarray(poses13, f32).reshape(-1, 13)
    P = dict(VM.DEFAULTS, **verify_params)
    rec, masks = np.zeros(len(poses13), VM.DTYPE), []
    for t, p in enumerate(poses13):
        scene = np.asarray(scenes[int(frame_of_pose[t])])
        h, w = scene.shape
        r = VM.render(meshes[0 if mesh_of is None else int(mesh_of[t])], p, K, w, h)
        rec[t] = VM.score(r, scene, **P)
        masks.append(support(r, scene, P["tau_mm"]))
    rec["best"] = rec["accepted"]
    return rec, masks


def shared_matrix(rec, masks, scene_first):
    """(n, n) int64: shared(a, b) for two accepted poses of one scene, 0 elsewhere (the diagonal included)."""
    n, sf = len(rec), [int(v) for v in scene_first]
    M = np.zeros((n, n), np.int64)
    for s in range(len(sf) - 1):
        for a in range(sf[s], sf[s + 1]):
            for b in range(a + 1, sf[s + 1]):
                if rec["accepted"][a] and rec["accepted"][b]:
                    M[a, b] = M[b, a] = int((masks[a] & masks[b]).sum())
    return M


def verify_scene(meshes, scenes, frame_of_pose, poses13, K, scene_first, mesh_of=None, **params):
    """fl_verify_scene_batch: (DTYPE records, the compact shared array, the full matrix)."""
    vp, _, _ = _split(params)
    sf = [int(v) for v in scene_first]
    for s in range(len(sf) - 1):
        assert len({int(frame_of_pose[t]) for t in range(sf[s], sf[s + 1])}) <= 1
    rec, masks = masks_and_records(meshes, scenes, frame_of_pose, poses13, K, mesh_of, **vp)
    M = shared_matrix(rec, masks, scene_first)
    sh = compact(M, scene_first)
    return pick(rec, scene_first, sh, **params), sh, M
