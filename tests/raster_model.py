"""float32 restatement of the fl_render_views contract (the comment at the top of fealess_amd/csrc/fl_render.hip), written
from the contract and not by calling the library: the GPU must equal it bit for bit.

Every operation is one numpy float32 ufunc on float32 operands, in the contract's order (numpy fuses nothing), so each
intermediate is the correctly rounded float32 result, as on the GPU.  Coverage is evaluated for every (triangle, pixel
of its bounding box) pair at once; the depth test is the same 64-bit key (float bits of z, triangle index) reduced with
np.minimum.at, so the winner does not depend on an order either.
"""
import numpy as np

f32 = np.float32
GREY = 180            # FL_RENDER_GREY
AMBIENT = f32(0.2)    # FL_RENDER_AMBIENT
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _xform(p, V, with_t):
    out = np.stack([(p[4 * j] * V[:, 0] + p[4 * j + 1] * V[:, 1]) + p[4 * j + 2] * V[:, 2] for j in range(3)], -1)
    if with_t:
        out = out + np.array([p[3], p[7], p[11]], f32)
    return out


def _setup(P, tri):
    """Edge coefficients c (n_t, 3, 3), normal n (n_t, 3), D (n_t,) after the orientation flip; ok (n_t,): neither
    edge-on nor entirely at z <= 0."""
    P0, P1, P2 = P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]
    c = np.stack([_cross(P1, P2), _cross(P2, P0), _cross(P0, P1)], 1)
    n = _cross(P1 - P0, P2 - P0)
    D = _dot(P0, n)
    ok = ((D > 0) | (D < 0)) & ((P0[:, 2] > 0) | (P1[:, 2] > 0) | (P2[:, 2] > 0))
    neg = D < 0
    c = np.where(neg[:, None, None], -c, c)
    n = np.where(neg[:, None], -n, n)
    D = np.where(neg, -D, D)
    return (P0, P1, P2), c, n, D, ok


def _edges(c, dx, dy):
    return [(c[:, k, 0] * dx + c[:, k, 1] * dy) + c[:, k, 2] for k in range(3)]


def _edge_in(c, e):
    return (e > 0) | ((e == 0) & ((c[:, 0] > 0) | ((c[:, 0] == 0) & (c[:, 1] > 0))))


def render_view(vertices, triangles, pose13, K, w, h, normals=None, colors=None, light=None, ambient=None):
    """One view: returns bgr (h, w, 3) u8, depth (h, w) u16, mask (h, w) u8, tri (h, w) int32."""
    V = np.ascontiguousarray(vertices, f32).reshape(-1, 3)
    T = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    p = np.ascontiguousarray(pose13, f32).ravel()
    fx, fy, cx, cy = (f32(k) for k in K)
    ifx, ify = f32(1) / fx, f32(1) / fy
    lv = np.array([0, 0, 1] if light is None else light, f32)
    ll = np.sqrt((lv[0] * lv[0] + lv[1] * lv[1]) + lv[2] * lv[2])
    lv = np.array([lv[0] / ll, lv[1] / ll, lv[2] / ll], f32)
    amb = AMBIENT if ambient is None else f32(ambient)

    P = _xform(p, V, True)
    (P0, P1, P2), c, n, D, ok = _setup(P, T)
    # bounding boxes
    x0 = np.zeros(len(T), np.int64)
    x1 = np.full(len(T), w - 1, np.int64)
    y0 = np.zeros(len(T), np.int64)
    y1 = np.full(len(T), h - 1, np.int64)
    front = (P0[:, 2] > 0) & (P1[:, 2] > 0) & (P2[:, 2] > 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pu = [fx * (Q[:, 0] / Q[:, 2]) + cx for Q in (P0, P1, P2)]
        pv = [fy * (Q[:, 1] / Q[:, 2]) + cy for Q in (P0, P1, P2)]
        u0, u1 = np.fmin(np.fmin(pu[0], pu[1]), pu[2]), np.fmax(np.fmax(pu[0], pu[1]), pu[2])
        v0, v1 = np.fmin(np.fmin(pv[0], pv[1]), pv[2]), np.fmax(np.fmax(pv[0], pv[1]), pv[2])
        wm, hm = f32(w - 1), f32(h - 1)
        bx0 = np.fmin(np.fmax(np.floor(u0) - f32(1), f32(0)), wm)
        bx1 = np.fmin(np.fmax(np.ceil(u1) + f32(1), f32(0)), wm)
        by0 = np.fmin(np.fmax(np.floor(v0) - f32(1), f32(0)), hm)
        by1 = np.fmin(np.fmax(np.ceil(v1) + f32(1), f32(0)), hm)
    x0 = np.where(front, bx0.astype(np.int64), x0)
    x1 = np.where(front, bx1.astype(np.int64), x1)
    y0 = np.where(front, by0.astype(np.int64), y0)
    y1 = np.where(front, by1.astype(np.int64), y1)
    bw = np.maximum(x1 - x0 + 1, 0)
    nb = np.where(ok, bw * np.maximum(y1 - y0 + 1, 0), 0)
    # every (triangle, bounding-box pixel) pair
    t = np.repeat(np.arange(len(T)), nb)
    start = np.repeat(np.cumsum(nb) - nb, nb)
    q = np.arange(int(nb.sum())) - start
    py = q // bw[t]
    x = x0[t] + q - py * bw[t]
    y = y0[t] + py
    dx = (x.astype(f32) - cx) * ifx
    dy = (y.astype(f32) - cy) * ify
    ct, nt = c[t], n[t]
    E = _edges(ct, dx, dy)
    inside = _edge_in(ct[:, 0], E[0]) & _edge_in(ct[:, 1], E[1]) & _edge_in(ct[:, 2], E[2])
    S = (nt[:, 0] * dx + nt[:, 1] * dy) + nt[:, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z = D[t] / S
        hit = inside & (S > 0) & (z > 0) & (z < np.inf)
    keys = np.full(w * h, EMPTY, np.uint64)
    kz = (z[hit].view(np.uint32).astype(np.uint64) << np.uint64(32)) | t[hit].astype(np.uint64)
    np.minimum.at(keys, (y[hit] * w + x[hit]), kz)

    # resolve
    full = keys != EMPTY
    tri = np.full(w * h, -1, np.int32)
    depth = np.zeros(w * h, np.uint16)
    mask = np.zeros(w * h, np.uint8)
    bgr = np.zeros((w * h, 3), np.uint8)
    k = keys[full]
    tw = (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
    zw = (k >> np.uint64(32)).astype(np.uint32).view(f32)
    tri[full] = tw
    depth[full] = np.fmin(np.rint(zw), f32(65535)).astype(np.uint16)
    mask[full] = 255
    idx = np.nonzero(full)[0]
    xs, ys = (idx % w).astype(f32), (idx // w).astype(f32)
    dx, dy = (xs - cx) * ifx, (ys - cy) * ify
    E = _edges(c[tw], dx, dy)
    Es = (E[0] + E[1]) + E[2]
    pos = Es > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        b = [np.where(pos, E[j] / Es, f32(1 if j == 0 else 0)).astype(f32) for j in range(3)]
    i0, i1, i2 = T[tw, 0], T[tw, 1], T[tw, 2]
    if normals is not None:
        Nv = _xform(p, np.ascontiguousarray(normals, f32).reshape(-1, 3), False)
        N = np.stack([(b[0] * Nv[i0, j] + b[1] * Nv[i1, j]) + b[2] * Nv[i2, j] for j in range(3)], -1)
    else:
        N = n[tw]
    L2 = _dot(N, N)
    good = L2 > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        sl = np.sqrt(L2)
        U = N / sl[:, None]
        f = np.fmin(np.fmax(np.abs(_dot(U, lv)), amb), f32(1))
    f = np.where(good, f, amb).astype(f32)
    for ch in range(3):
        if colors is not None:
            col = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)[:, ch].astype(f32)
            alb = (b[0] * col[i0] + b[1] * col[i1]) + b[2] * col[i2]
        else:
            alb = np.full(len(idx), GREY, f32)
        bgr[full, ch] = np.fmin(np.fmax(np.rint(alb * f), f32(0)), f32(255)).astype(np.uint8)
    return bgr.reshape(h, w, 3), depth.reshape(h, w), mask.reshape(h, w), tri.reshape(h, w)


def render(vertices, triangles, poses13, K, w, h, normals=None, colors=None, light=None, ambient=None):
    """Every view of poses13 (n, 13): bgr (n, h, w, 3), depth (n, h, w), mask (n, h, w), tri (n, h, w)."""
    outs = [render_view(vertices, triangles, p, K, w, h, normals, colors, light, ambient)
            for p in np.asarray(poses13, f32).reshape(-1, 13)]
    return tuple(np.stack([o[i] for o in outs]) for i in range(4))
