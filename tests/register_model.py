"""numpy statement of depth registration (fl_register_depth_batch, include/fealess_hip.h), test infrastructure only.

Written from the header's text, not by calling the library: the GPU must equal it bit for bit.  Every operation is one
numpy float32 ufunc on float32 operands in the contract's order (numpy fuses nothing), so each intermediate is the correctly
rounded float32 result, as on the GPU.  The splat is a plain loop over the FL_REGISTER_MAX_SPLAT x FL_REGISTER_MAX_SPLAT
places of a footprint, each place a minimum into the image; the crack fill is written from the rule, on the unfilled image.
"""
import numpy as np

f32 = np.float32
MAX_SPLAT = 8         # FL_REGISTER_MAX_SPLAT


def footprints(depth, K_depth, K_color, R, t):
    """Per depth pixel, flattened row-major: live (it lands somewhere), val (u16) and the inclusive ranges x0, x1, y0, y1 (int64;
    meaningless where live is False).  K = (w, h, fx, fy, cx, cy)."""
    d = np.ascontiguousarray(depth, np.uint16)
    wd, hd = int(K_depth[0]), int(K_depth[1])
    wc, hc = int(K_color[0]), int(K_color[1])
    assert d.shape == (hd, wd)
    fx_d, fy_d, cx_d, cy_d = (f32(k) for k in K_depth[2:])
    fx_c, fy_c, cx_c, cy_c = (f32(k) for k in K_color[2:])
    ifx, ify = f32(1) / fx_d, f32(1) / fy_d
    R = np.asarray(R, f32).reshape(9)
    t = np.asarray(t, f32).reshape(3)
    v, u = np.divmod(np.arange(wd * hd), wd)
    z = d.ravel().astype(f32)
    uf, vf = u.astype(f32), v.astype(f32)

    def point(o):
        x = ((uf + f32(o)) - cx_d) * ifx * z
        y = ((vf + f32(o)) - cy_d) * ify * z
        return [((R[3 * j] * x + R[3 * j + 1] * y) + R[3 * j + 2] * z) + t[j] for j in range(3)]

    with np.errstate(all="ignore"):
        (XA, YA, ZA), (XB, YB, ZB), (_, _, ZC) = point(-0.5), point(0.5), point(0.0)
        live = (d.ravel() != 0) & (ZA > 0) & (ZB > 0) & (ZC >= f32(0.5))
        val = np.where(live, np.fmin(np.rint(ZC), f32(65535)), f32(0)).astype(np.uint16)
        pA, qA = XA / ZA * fx_c + cx_c, YA / ZA * fy_c + cy_c
        pB, qB = XB / ZB * fx_c + cx_c, YB / ZB * fy_c + cy_c
        live &= np.isfinite(pA) & np.isfinite(qA) & np.isfinite(pB) & np.isfinite(qB)

        def span(a, b, n):
            a, b = np.where(live, a, f32(0)), np.where(live, b, f32(0))
            lo = np.fmin(np.fmax(np.ceil(np.fmin(a, b)), f32(-1)), f32(n)).astype(np.int64)
            hi = np.fmin(np.fmax(np.floor(np.fmax(a, b)), f32(-1)), f32(n)).astype(np.int64)
            lo = np.maximum(lo, 0)
            hi = np.minimum(np.minimum(hi, n - 1), lo + MAX_SPLAT - 1)
            return lo, hi

        x0, x1 = span(pA, pB, wc)
        y0, y1 = span(qA, qB, hc)
    live &= (x1 >= x0) & (y1 >= y0)
    return live, val, x0, x1, y0, y1


def splat(depth, K_depth, K_color, R, t):
    """The unfilled image E (hc, wc) u16: the minimum of the values that land on a pixel, 0 where nothing lands."""
    wc, hc = int(K_color[0]), int(K_color[1])
    live, val, x0, x1, y0, y1 = footprints(depth, K_depth, K_color, R, t)
    big = np.full(wc * hc, 0xFFFFFFFF, np.uint32)
    for dy in range(MAX_SPLAT):
        for dx in range(MAX_SPLAT):
            m = live & (x0 + dx <= x1) & (y0 + dy <= y1)
            if m.any():
                np.minimum.at(big, (y0[m] + dy) * wc + (x0[m] + dx), val[m].astype(np.uint32))
    return np.where(big == 0xFFFFFFFF, 0, big).astype(np.uint16).reshape(hc, wc)


def fill(E):
    """The crack rule on the unfilled image E: a zero pixel takes min(left, right) where both exist and are non-zero, otherwise
    min(up, down) where both exist and are non-zero, otherwise stays 0."""
    E = np.asarray(E, np.uint16)
    out = E.copy()
    h, w = E.shape
    lr = np.zeros((h, w), bool)
    if w >= 3:
        l, r = E[:, :-2], E[:, 2:]
        ok = (E[:, 1:-1] == 0) & (l != 0) & (r != 0)
        out[:, 1:-1][ok] = np.minimum(l, r)[ok]
        lr[:, 1:-1] = ok
    if h >= 3:
        up, dn = E[:-2, :], E[2:, :]
        ok = (E[1:-1, :] == 0) & ~lr[1:-1, :] & (up != 0) & (dn != 0)
        out[1:-1, :][ok] = np.minimum(up, dn)[ok]
    return out


def register(depth, K_depth, K_color, R, t, fill_cracks=1):
    """One frame of fl_register_depth_batch: (hc, wc) u16."""
    E = splat(depth, K_depth, K_color, R, t)
    return fill(E) if fill_cracks else E


def rodrigues(rvec):
    """The rotation matrix of a rotation vector (rad), fp64: for the tests' extrinsics."""
    r = np.asarray(rvec, np.float64)
    th = float(np.linalg.norm(r))
    if th == 0:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
