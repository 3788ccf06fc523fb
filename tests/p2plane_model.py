"""numpy/scipy model of FL_ICP_POINT_TO_PLANE (fealess_amd/csrc/fl_icp.hip), test infrastructure only.

The mode has no counterpart in the reference, so there is no oracle
for it: this file restates the kernel's arithmetic (float32 points, fp64 sums, the same gates and
loop control) so the GPU tests can check the kernel against an independent implementation, and
the tests then judge both against the ground-truth pose of a synthetic scene.
"""
import numpy as np
from scipy.spatial import cKDTree

NRM_R = 3


def scene_normals(depth, K, xs, ys):
    """Least-squares depth-gradient normals at pixels (xs, ys) of a u16 depth image (mm)."""
    fx, fy, cx, cy = K
    h, w = depth.shape
    d = depth.astype(np.float32)
    out = np.zeros((len(xs), 3), np.float32)
    r = NRM_R
    s2 = np.float32((2 * r + 1) * r * (r + 1) * (2 * r + 1) // 3)
    du, dv = np.meshgrid(np.arange(-r, r + 1, dtype=np.float32), np.arange(-r, r + 1, dtype=np.float32))
    for k, (x, y) in enumerate(zip(xs, ys)):
        if x < r or y < r or x + r >= w or y + r >= h:
            continue
        win = d[y - r:y + r + 1, x - r:x + r + 1]
        zc = d[y, x]
        gate = np.float32(0.02) * zc + np.float32(2.0)
        if zc <= 0 or (win <= 0).any() or (np.abs(win - zc) > gate).any():
            continue
        zu = np.float32((du * win).sum(dtype=np.float64)) / s2
        zv = np.float32((dv * win).sum(dtype=np.float64)) / s2
        X = np.float32((x - cx) / fx)
        Y = np.float32((y - cy) / fy)
        pu = np.array([zc / fx + X * zu, Y * zu, zu], np.float64)
        pv = np.array([X * zv, zc / fy + Y * zv, zv], np.float64)
        c = np.cross(pu, pv)
        n = np.linalg.norm(c)
        if n > 0:
            out[k] = (c / n).astype(np.float32)
    return out


def _l2dist(mod, ref, thr):
    ok = (ref[:, 2] <= 900) & (mod[:, 2] <= 900)
    d = np.sqrt(((mod.astype(np.float64) - ref.astype(np.float64)) ** 2).sum(1)).astype(np.float32)
    inl = ok & (d <= thr)
    counter = int(ok.sum())
    if counter == 0:
        return np.float32(np.finfo(np.float32).max), 0.0
    return np.float32(d[inl].astype(np.float64).sum() / max(int(inl.sum()), 1)) if inl.sum() else np.float32(np.nan), inl.sum() / counter


def rodrigues(w):
    t2 = float(w @ w)
    t = np.sqrt(t2)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    sa = np.sin(t) / t if t > 1e-9 else 1 - t2 / 6
    sb = (1 - np.cos(t)) / t2 if t > 1e-9 else 0.5 - t2 / 24
    return np.eye(3) + sa * K + sb * (K @ K)


def icp_point_to_plane(ref, nrm, model, it_thr, dmt, ddt):
    """ref/model index-paired float32 clouds (len(ref) >= len(model)); returns dict like fl_icp_result."""
    ref = np.asarray(ref, np.float32)
    nrm = np.asarray(nrm, np.float32)
    mod = np.array(model, np.float32)
    n = len(mod)
    mod[~(mod[:, 2] <= 900)] = 0
    R = np.eye(3, dtype=np.float32)
    T = np.zeros(3, np.float32)
    tree = cKDTree(ref.astype(np.float64))
    dist_mean, px = _l2dist(mod, ref[:n], np.float32(np.finfo(np.float32).max))
    dist_diff = np.float32(np.finfo(np.float32).max)
    it = 0
    n_corr = 0
    while dist_mean > dmt and dist_diff > ddt and it < it_thr:
        it += 1
        gate = np.float32(3) * dist_mean
        thr = gate * gate
        d, j = tree.query(mod.astype(np.float64))
        d2 = ((mod - ref[j]) ** 2).sum(1, dtype=np.float32)
        keep = d2 <= thr
        n_corr = int(keep.sum())
        if n_corr < 3:
            it = it_thr
            continue
        m = mod[keep].astype(np.float64)
        r = ref[j[keep]].astype(np.float64)
        nn = nrm[j[keep]].astype(np.float64)
        J = np.concatenate([np.cross(m, nn), nn], 1)
        e = (nn * (m - r)).sum(1)
        A = J.T @ J
        b = -(J.T @ e)
        tr = np.trace(A)
        A = A + 1e-12 * tr * np.eye(6)
        try:
            Lc = np.linalg.cholesky(A)
            if (np.diag(Lc) ** 2 <= 1e-13 * tr).any():
                raise np.linalg.LinAlgError
        except np.linalg.LinAlgError:
            continue
        x = np.linalg.solve(A, b)
        Ro = rodrigues(x[:3]).astype(np.float32)
        To = x[3:].astype(np.float32)
        valid = mod[:, 2] <= 900
        new = (mod @ Ro.T + To).astype(np.float32)
        mod = np.where(valid[:, None], new, mod)
        old = dist_mean
        dist_mean, px = _l2dist(mod, ref[:n], np.float32(3) * old)
        dist_diff = old - dist_mean
        T = (Ro @ T + To).astype(np.float32)
        R = (Ro @ R).astype(np.float32)
    return dict(R=R, T=T, dist_mean=float(dist_mean), px_ratio=float(px), iters=it, n_corr_last=n_corr)


def crop_pairs(model_depth, scene_depth, K, rect_model, rect_ref):
    """detection()'s paired-valid compaction (ICP/common.cpp:382-405): returns ref, mod clouds (mm) and the
    scene pixel coordinates of the kept pairs."""
    fx, fy, cx, cy = K
    mx0, my0, cw, ch = rect_model
    sx0, sy0 = rect_ref[:2]
    ys, xs = np.mgrid[0:ch, 0:cw]
    sx, sy, mx, my = sx0 + xs, sy0 + ys, mx0 + xs, my0 + ys
    zs = scene_depth[sy, sx].astype(np.float32)
    zm = model_depth[my, mx].astype(np.float32)
    A = np.stack([(sx - cx) / fx * zs, (sy - cy) / fy * zs, zs], -1).astype(np.float32)
    B = np.stack([(mx - 320.0) / 608.0 * zm, (my - 240.0) / 608.0 * zm, zm], -1).astype(np.float32)
    keep = (zs > 0) & (zm > 0) & (zs <= 900) & (zm <= 900)
    return A[keep], B[keep], sx[keep], sy[keep]


def detection_point_to_plane(model_depth, scene_depth, K, rect_model, rect_ref, it_thr, dmt, ddt, r_match, t_match):
    ref, mod, sx, sy = crop_pairs(model_depth, scene_depth, K, rect_model, rect_ref)
    nrm = scene_normals(scene_depth, K, sx, sy)
    t_tmp = (ref.astype(np.float64).mean(0) - mod.astype(np.float64).mean(0)).astype(np.float32)
    mod = (mod + t_tmp).astype(np.float32)
    t_init = t_tmp + np.asarray(t_match, np.float32)
    icp = icp_point_to_plane(ref, nrm, mod, it_thr, dmt, ddt)
    Rf = icp["R"] @ np.asarray(r_match, np.float32).reshape(3, 3)
    Tf = icp["R"] @ t_init + icp["T"]
    return dict(R_final=Rf, T_final=Tf, icp=icp, n_points=len(ref), normals=nrm)


# ---- fp64 restatements with error bounds: the yardsticks of the kernel's normals and of one point-to-plane iteration --------
F32_EPS = float(np.finfo(np.float32).eps) / 2          # unit roundoff u of float32 (2^-24)


def scene_normals_fp64(depth, K, xs, ys):
    """scene_normal (fl_icp.hip) in fp64, with the bound on the float32 kernel's distance from it.

    The border and depth-step rules are definitions, so they are evaluated exactly as the kernel does (the gate
    0.02f * zc + 2.0f in float32; z - zc of two u16 depths is exact in float32).  Everything after them is fp64 on the
    float32 intrinsics the kernel receives.  Returns (normals (n, 3) float64, zero (n,) bool, bound (n,) float64):
    `zero` marks the pixels whose normal is 0 by the rules, `bound` is a first-order bound on |n_f32 - n_fp64| per
    component for the others, from the float32 roundings the kernel performs (see _normal_bound)."""
    fx, fy, cx, cy = (float(np.float32(v)) for v in K)
    h, w = depth.shape
    r = NRM_R
    s2 = float((2 * r + 1) * r * (r + 1) * (2 * r + 1) // 3)
    du, dv = np.meshgrid(np.arange(-r, r + 1, dtype=np.float64), np.arange(-r, r + 1, dtype=np.float64))
    n = len(xs)
    out = np.zeros((n, 3), np.float64)
    zero = np.ones(n, bool)
    bound = np.zeros(n, np.float64)
    for k, (x, y) in enumerate(zip(xs, ys)):
        x, y = int(x), int(y)
        if x < r or y < r or x + r >= w or y + r >= h:
            continue
        win = depth[y - r:y + r + 1, x - r:x + r + 1].astype(np.float64)
        zc = float(depth[y, x])
        gate = np.float32(np.float32(0.02) * np.float32(zc)) + np.float32(2.0)
        if zc <= 0 or (win <= 0).any() or (np.abs(win - zc) > float(gate)).any():
            continue
        zu = (du * win).sum() / s2                   # the sums are integers below 2^24: exact in float32 too
        zv = (dv * win).sum() / s2
        X, Y = (x - cx) / fx, (y - cy) / fy
        pu = np.array([zc / fx + X * zu, Y * zu, zu])
        pv = np.array([X * zv, zc / fy + Y * zv, zv])
        c = np.cross(pu, pv)
        ln = float(np.linalg.norm(c))
        if not ln > 0:
            continue
        out[k] = c / ln
        zero[k] = False
        # magnitudes of the terms each component of Pu, Pv is formed from (their rounding errors scale with these)
        tu = np.array([abs(zc / fx) + abs(X * zu), abs(Y * zu), abs(zu)])
        tv = np.array([abs(X * zv), abs(zc / fy) + abs(Y * zv), abs(zv)])
        bound[k] = _normal_bound(tu, tv, ln)
    return out, zero, bound


def _normal_bound(tu, tv, ln):
    """First-order bound on a component of n = c / |c|, c = Pu x Pv, computed in float32 as scene_normal does.

    Pu, Pv: zu = su / 196 (su exact) is one rounding; X = (x - cx) / fx two; X * zu, Y * zu one more each, Pu_x a sum:
    |dPu_i| <= 5 u tu_i, |dPv_i| <= 5 u tv_i.  c_i = Pu_j Pv_k - Pu_k Pv_j: 10 u from the inputs, two products and a
    difference 3 u, so |dc_i| <= 13 u (tu_j tv_k + tu_k tv_j).  n_i = c_i / |c|: |dn_i| <= |dc| (1 + |n_i|) / |c| + 4 u (the
    sum of squares, the root, the division).  Doubled for the second-order terms and a last-place difference in the
    device's sqrt and division."""
    u = F32_EPS
    dc = np.array([tu[1] * tv[2] + tu[2] * tv[1], tu[2] * tv[0] + tu[0] * tv[2], tu[0] * tv[1] + tu[1] * tv[0]]) * 13 * u
    return 2.0 * (2.0 * float(np.linalg.norm(dc)) / ln + 4 * u)


def _plane_terms32(m, r, n):
    """The 27 terms of a kept pair as pair_sums (fl_icp.hip) forms them: float32, one IEEE operation per operator."""
    m, r, n = (np.asarray(a, np.float32) for a in (m, r, n))
    J = [m[:, 1] * n[:, 2] - m[:, 2] * n[:, 1], m[:, 2] * n[:, 0] - m[:, 0] * n[:, 2], m[:, 0] * n[:, 1] - m[:, 1] * n[:, 0],
         n[:, 0], n[:, 1], n[:, 2]]
    e = (n[:, 0] * (m[:, 0] - r[:, 0]) + n[:, 1] * (m[:, 1] - r[:, 1])) + n[:, 2] * (m[:, 2] - r[:, 2])
    t = [J[a] * J[b] for a in range(6) for b in range(a, 6)] + [J[a] * e for a in range(6)]
    return np.stack(t, 1)


def _plane_terms64(m, r, n):
    m, r, n = (np.asarray(a, np.float64) for a in (m, r, n))
    J = np.concatenate([np.cross(m, n), n], 1)
    e = (n * (m - r)).sum(1)
    return np.stack([J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)] + [J[:, a] * e for a in range(6)], 1)


def _plane_solve(s):
    """(R, T) of one iteration from the 27 sums, as the kernel solves it (fp64 Cholesky of the regularised system, Rodrigues),
    rounded to float32; None where the kernel skips the iteration."""
    A = np.zeros((6, 6))
    q = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = s[q]
            q += 1
    b = -np.asarray(s[21:27], np.float64)
    tr = np.trace(A)
    A = A + 1e-12 * tr * np.eye(6)
    try:
        Lc = np.linalg.cholesky(A)
        if (np.diag(Lc) ** 2 <= 1e-13 * tr).any():
            return None
    except np.linalg.LinAlgError:
        return None
    x = np.linalg.solve(A, b)
    return rodrigues(x[:3]).astype(np.float32), x[3:].astype(np.float32)


def crop_clouds_f32(model_depth, scene_depth, K, rect_model, rect_ref):
    """crop_pairs with the float32 arithmetic of detection()'s back-projection (crop_clouds in fl_icp.hip, after
    depth_to_3d.cpp and rescaleDepth): ((u - cx) * (1 / fx)) * (z * 0.001f) * 1000 per coordinate.  The points differ from
    crop_pairs' by up to an ulp, which moves one iteration's (R, T) by more than its summation noise floor."""
    f = np.float32
    fx, fy, cx, cy = (f(v) for v in K)
    mx0, my0, cw, ch = rect_model
    sx0, sy0 = rect_ref[:2]
    ys, xs = np.mgrid[0:ch, 0:cw]
    sx, sy, mx, my = sx0 + xs, sy0 + ys, mx0 + xs, my0 + ys
    ds, dm = scene_depth[sy, sx].astype(f), model_depth[my, mx].astype(f)
    with np.errstate(invalid="ignore"):
        zs = np.where(ds == 0, f(np.nan), ds * f(1 / 1000.0)).astype(f)
        zm = np.where(dm == 0, f(np.nan), dm * f(1 / 1000.0)).astype(f)
        A = np.stack([(((sx.astype(f) - cx) * (f(1) / fx)) * zs) * f(1000), (((sy.astype(f) - cy) * (f(1) / fy)) * zs) * f(1000),
                      zs * f(1000)], -1)
        B = np.stack([(((mx.astype(f) - f(320)) * (f(1) / f(608))) * zm) * f(1000), (((my.astype(f) - f(240)) * (f(1) / f(608))) * zm) * f(1000),
                      zm * f(1000)], -1)
        keep = (A[..., 2] <= 900) & (B[..., 2] <= 900)
    return A[keep].astype(f), B[keep].astype(f), sx[keep], sy[keep]


def first_iteration_pairs(ref, mod):
    """The pairs of iteration 1 of icp_point_to_plane, with how close the closest call was: the smallest relative gap
    between a kept or dropped pair's squared distance and the gate, and between a point's nearest and second-nearest
    reference distance (a near-tie there lets float rounding pick another partner)."""
    ref = np.asarray(ref, np.float32)
    mod = np.array(mod, np.float32)
    n = len(mod)
    mod[~(mod[:, 2] <= 900)] = 0
    dist_mean, _ = _l2dist(mod, ref[:n], np.float32(np.finfo(np.float32).max))
    gate = np.float32(3) * dist_mean
    thr = gate * gate
    d, j = cKDTree(ref.astype(np.float64)).query(mod.astype(np.float64), k=2)
    j = j[:, 0]
    d2 = ((mod - ref[j]) ** 2).sum(1, dtype=np.float32)
    keep = d2 <= thr
    gate_gap = float(np.min(np.abs(d2.astype(np.float64) - float(thr)) / float(thr)))
    tie_gap = float(np.min((d[:, 1] - d[:, 0]) / np.maximum(d[:, 1], 1e-30)))
    return dict(mod=mod, keep=keep, j=j, thr=thr, gate_gap=gate_gap, tie_gap=tie_gap)


def one_iteration_noise_floor(ref, nrm, mod, bs, n_partitions=8, seed=0):
    """One point-to-plane iteration (icp_it_thr = 1) in fp64 and the float32 summation noise floor of the kernel's result.

    The kernel forms each pair's 27 terms in float32, sums them per thread in float32 (a thread takes about n / bs pairs)
    and adds the threads' partials in fp64.  Which pairs share a thread depends on the build and the search order, so the
    floor is taken over random partitions of the kept pairs into bs float32 partials: the largest distance of such a
    result from the one of the fp64 sums of fp64 terms.  Returns dict(R, T, n_corr, floor_R, floor_T) + the pair margins."""
    P = first_iteration_pairs(ref, mod)
    keep, j = P["keep"], P["j"]
    m, r, nn = P["mod"][keep], np.asarray(ref, np.float32)[j[keep]], np.asarray(nrm, np.float32)[j[keep]]
    R64, T64 = _plane_solve(_plane_terms64(m, r, nn).sum(0))
    t32 = _plane_terms32(m, r, nn)
    k = len(t32)
    per = -(-k // bs)
    rng = np.random.default_rng(seed)
    floor_R = floor_T = 0.0
    for _ in range(n_partitions):
        cells = np.zeros((per * bs, 27), np.float32)
        cells[:k] = t32[rng.permutation(k)]
        cells = cells.reshape(per, bs, 27)
        acc = np.zeros((bs, 27), np.float32)
        for row in cells:                            # each partial in float32, in its own order
            acc = acc + row
        Rp, Tp = _plane_solve(acc.astype(np.float64).sum(0))
        floor_R = max(floor_R, float(np.abs(Rp.astype(np.float64) - R64).max()))
        floor_T = max(floor_T, float(np.abs(Tp.astype(np.float64) - T64).max()))
    return dict(R=R64, T=T64, n_corr=int(keep.sum()), floor_R=floor_R, floor_T=floor_T, gate_gap=P["gate_gap"],
                tie_gap=P["tie_gap"])


def normal_cases():
    """Depth images and pixel lists for scene_normal's tests: [(depth u16 (h, w), K, xs, ys, label)].  Pixels 2, 3, w - 4, w - 3
    (and the same rows) around the border rule, a missing return in the window and at the centre, a neighbour exactly at the
    depth-step gate and one past it on either side, depth 65535, slants up to the gate, fx != fy and a non-integer (cx, cy)."""
    cases = []
    w, h = 61, 47
    K = (571.3, 603.9, 30.37, 22.81)
    ys_, xs_ = np.mgrid[0:h, 0:w].astype(np.float64)
    edge_x, edge_y = [2, 3, 4, w // 2, w - 5, w - 4, w - 3], [2, 3, 4, h // 2, h - 5, h - 4, h - 3]
    gx, gy = np.meshgrid(edge_x, edge_y)
    for a, b, z0 in ((0.0, 0.0, 650.0), (2.1, -1.6, 600.0), (3.3, 0.0, 420.0), (0.2, 2.7, 455.0), (6.5, 0.0, 1200.0),
                     (0.0, -9.0, 1800.0), (-3.1, 0.4, 420.0)):
        # a plane, and a slight bowl on top of it; the slants reach the gate (2 % + 2 mm over three pixels), the last one
        # crosses it in places
        for curv in (0.0, 0.08):
            z = z0 + a * (xs_ - w / 2) + b * (ys_ - h / 2) + curv * ((xs_ - w / 2) ** 2 + (ys_ - h / 2) ** 2) / 8
            cases.append((np.rint(z).astype(np.uint16), K, gx.ravel(), gy.ravel(), "slant %g %g curv %g" % (a, b, curv)))
    # the gate: a flat window whose centre depth makes 0.02f * zc + 2.0f an integer, one neighbour at +-gate and +-(gate + 1)
    zc = next(v for v in range(400, 3000) if float(np.float32(np.float32(0.02) * np.float32(v)) + np.float32(2)).is_integer())
    g = int(np.float32(np.float32(0.02) * np.float32(zc)) + np.float32(2))
    xs, ys, ims = [], [], np.full((h, w), zc, np.uint16)
    for i, (dz, du, dv) in enumerate(((g, 3, 3), (-g, -3, 2), (g + 1, -3, -3), (-g - 1, 1, -3), (g, 0, 0))):
        cx, cy = 6 + 8 * i, 10
        ims[cy + dv, cx + du] = zc + dz
        xs.append(cx); ys.append(cy)
    # a missing return at a window corner, and at the centre
    ims[30 + 3, 10 - 3] = 0
    ims[30, 30] = 0
    xs += [10, 30, 31]; ys += [30, 30, 30]
    cases.append((ims, K, np.array(xs), np.array(ys), "gate %d at zc %d, missing returns" % (g, zc)))
    # the largest depth: flat, and slanted within its gate (about 1313 mm)
    big = np.full((h, w), 65535, np.uint16)
    big[:, :w // 2] = np.clip(np.rint(65535 - 300.0 * (w // 2 - xs_[:, :w // 2]) - 100.0 * ys_[:, :w // 2]), 0, 65535).astype(np.uint16)
    cases.append((big, (611.0, 587.5, 29.5, 24.25), np.array([10, 14, 28, 40, 50, w - 4, w - 3]), np.array([20, 5, 30, 20, 40, 20, 20]),
                  "depth 65535"))
    return cases
