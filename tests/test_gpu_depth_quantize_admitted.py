"""GPU parity of the depth quantiser's closed-form normal (k_depth_quantize, dq_normal_pattern).  A wavefront walks a strip
of 60 columns row by row, its 64 lanes on the columns 60 s - 2 .. 60 s + 61; a lane is active where its pixel is interior
(5 <= x < w - 6, 5 <= y < h - 6) and nearer than distance_threshold.  Where, in one row of one strip (a wave-step), every active
lane has all eight neighbours at +-5 within difference_threshold, the wave takes a branch on which the accumulated sums are
constants (A0 = A3 = 150, A1 = 0, det = 22500) and the normal comes from the neighbours directly; one active lane that
rejects a neighbour sends the whole wave-step down the general path.  Thresholds above 400 always take the general path.

A test cannot see from outside which branch ran, so every case proves on the CPU, with a numpy model of that decomposition
(`wave_steps`), that its input holds the kinds of wave-steps it is meant for: all-admitted ones, mixed ones (an active lane that
rejects a neighbour), or both.  Every image is compared byte for byte with the oracle's."""
import numpy as np
import pytest

from util import options

pytestmark = pytest.mark.gpu

# the ring neighbours n0 .. n7 of dq_normal_pattern as (dx, dy)
_RING = [(-5, -5), (0, -5), (5, -5), (-5, 0), (5, 0), (-5, 5), (0, 5), (5, 5)]


def lanes(d, dist=2000, diff=50):
    """(active, admitted): bool images.  Active: interior and below dist; admitted: all eight ring neighbours within diff."""
    h, w = d.shape
    D = d.astype(np.int64)
    active, adm = np.zeros((h, w), bool), np.zeros((h, w), bool)
    if h >= 12 and w >= 12:
        c = D[5:h - 6, 5:w - 6]
        a = np.ones(c.shape, bool)
        for dx, dy in _RING:
            a &= np.abs(D[5 + dy:h - 6 + dy, 5 + dx:w - 6 + dx] - c) < diff
        active[5:h - 6, 5:w - 6] = c < dist
        adm[5:h - 6, 5:w - 6] = a
    return active, adm


def wave_steps(d, dist=2000, diff=50):
    """(working, all_admitted, mixed): bool arrays [row, strip].  A working wave-step has an active lane; it is all-admitted when
    every active lane admits its eight neighbours and mixed when one does not.  Lanes beside the image, and pixels that are not
    interior or not below dist, are not active and count for nothing."""
    h, w = d.shape
    active, adm = lanes(d, dist, diff)
    ns = (w + 59) // 60
    working, mixed = np.zeros((h, ns), bool), np.zeros((h, ns), bool)
    for s in range(ns):
        x0, x1 = max(0, 60 * s - 2), min(w - 1, 60 * s + 61)
        act = active[:, x0:x1 + 1]
        working[:, s] = act.any(1)
        mixed[:, s] = (act & ~adm[:, x0:x1 + 1]).any(1)
    return working, working & ~mixed, mixed


def _strips_of(x, w):
    return [s for s in range((w + 59) // 60) if 60 * s - 2 <= x <= 60 * s + 61]


def _plane(w, h, base=800, ax=2, ay=3):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray((base + ax * xs + ay * ys).astype(np.uint16))


def _check(ctx, oracle, d, dist=2000, diff=50, what=""):
    e = oracle.quantized_normals(d, dist, diff)
    got = ctx.quantized_normals(d, dist, diff)
    bad = int((got != e).sum())
    if bad or what:
        print("%s %dx%d thresholds %d %d: %d bytes differ, %d labelled" % (what, d.shape[1], d.shape[0], dist, diff, bad,
                                                                              int((e != 0).sum())))
    assert np.array_equal(got, e), (what, d.shape, dist, diff, bad)
    return e


# Every working wave-step is all-admitted.  At the widths 61, 65, 70 and 122 the last strip has lanes beside the image; at 65
# and 70 it has active lanes too (one and six), so the decision may count active lanes only, and at 61 and 122 none.
@pytest.mark.parametrize("base,ax,ay", [(800, 2, 3), (1500, -4, 1)])
@pytest.mark.parametrize("w,h", [(136, 40), (61, 30), (65, 30), (70, 30), (122, 30)])
def test_tilted_planes(ctx, oracle, w, h, base, ax, ay):
    d = _plane(w, h, base, ax, ay)
    working, alladm, mixed = wave_steps(d)
    assert alladm.any() and not mixed.any() and np.array_equal(working, alladm)
    assert alladm[5:h - 6, 0].all()
    if w in (65, 70):
        assert alladm[5:h - 6, -1].all() and 60 * (alladm.shape[1] - 1) + 61 > w - 1
    if w in (61, 122):
        assert not working[:, -1].any()
    e = _check(ctx, oracle, d, what="plane")
    assert (e[8:h - 9, 8:w - 9] != 0).all()               # not vacuous: labels wherever the median's window is interior


# One lane of the plane 800 + x + y rejects exactly neighbour k (that pixel is lifted by 60, so it differs by 50 .. 70): its
# wave-step is mixed, the rows beside it are not.  The lane sits on both sides of the strip seams (x = 58 .. 62 are lanes 60 .. 63 of strip 0 and lanes 0 .. 4 of strip 1,
# x = 118 .. 122 the same of strips 1 and 2) and in the first and last interior rows.
@pytest.mark.parametrize("k", range(8))
def test_one_rejected_neighbour(ctx, oracle, k):
    w, h = 136, 40
    dx, dy = _RING[k]
    base = _plane(w, h, 800, 1, 1)
    n = 0
    for y in (5, 6, 20, h - 8, h - 7):
        for x in list(range(58, 63)) + list(range(118, 123)):
            d = base.copy()
            d[y + dy, x + dx] += 60
            working, alladm, mixed = wave_steps(d)
            strips = _strips_of(x, w)
            for s in strips:
                assert mixed[y, s], (x, y, s)
                for yy in (y - 1, y + 1):
                    if 5 <= yy < h - 6:
                        assert alladm[yy, s], (x, yy, s)
            n += bool({x - (60 * s - 2) for s in strips} & {0, 2, 61, 63})
            _check(ctx, oracle, d)
    assert n == 5 * 8                                      # x = 58, 60 (lanes 0, 2 of the right strip), 59, 61 (lanes 61, 63 of the left)


# A step edge through a wave: the lanes within five columns (rows) of it reject a neighbour, the lanes on both sides admit all.
@pytest.mark.parametrize("kind,at", [("x", 30), ("x", 59), ("x", 60), ("x", 63), ("x", 90), ("y", 12), ("y", 20), ("diag", 70)])
def test_step_edge(ctx, oracle, kind, at):
    w, h = 136, 40
    d = _plane(w, h).astype(np.int64)
    ys, xs = np.mgrid[0:h, 0:w]
    far = {"x": xs >= at, "y": ys >= at, "diag": xs + 2 * ys >= at}[kind]
    d[far] += 200
    d = np.ascontiguousarray(d.astype(np.uint16))
    working, alladm, mixed = wave_steps(d)
    assert alladm.any() and mixed.any()
    if kind == "x":                                        # the strips with the edge are mixed in every row, with admitted lanes on both sides
        for s in _strips_of(at, w):
            assert mixed[5:h - 6, s].all()
        adm = lanes(d)[1]
        assert adm[20, at - 6] and adm[20, at + 5] and not adm[20, at - 5:at + 5].any()
    _check(ctx, oracle, d, what="edge %s %d" % (kind, at))


# distance_threshold cuts through a wave: the far lanes are inactive, and what they would reject does not count.
@pytest.mark.parametrize("dist", [900, 1000, 1100])
def test_distance_threshold_through_a_wave(ctx, oracle, dist):
    w, h = 136, 40
    d = _plane(w, h)
    working, alladm, mixed = wave_steps(d, dist)
    assert alladm.any() and not mixed.any()
    active = lanes(d, dist)[0]
    cut = [(r, s) for r in range(5, h - 6) for s in range(2)
           if 0 < int(active[r, max(5, 60 * s - 2):60 * s + 62].sum()) < 60 * s + 62 - max(5, 60 * s - 2)]
    assert cut and all(alladm[r, s] for r, s in cut)      # wave-steps whose interior lanes are of both kinds
    # and far lanes that WOULD reject, were they looked at: the plane's neighbours differ by at most 25, so no active lane sees
    # the far side's hole
    d2 = d.copy()
    d2[d2 >= dist + 30] = 9000
    w2, a2, m2 = wave_steps(d2, dist)
    act2, adm2 = lanes(d2, dist)
    assert np.array_equal(a2, alladm) and not m2.any()
    assert any((~act2[r, max(5, 60 * s - 2):min(w - 6, 60 * s + 62)] & ~adm2[r, max(5, 60 * s - 2):min(w - 6, 60 * s + 62)]).any()
               for r, s in cut)                            # an inactive interior lane that rejects, in a wave-step that works
    _check(ctx, oracle, d, dist, 50, what="cut")
    _check(ctx, oracle, d2, dist, 50, what="cut, far side rejecting")


def _steps_frame():
    """130 x 66: a flat band (all-admitted at any positive threshold), a tilted band, and blocks of 13 x 11 at random heights
    whose differences include 399, 400 and 401."""
    w, h = 130, 66
    rng = np.random.default_rng(42)
    d = np.full((h, w), 1000, np.int64)
    ys, xs = np.mgrid[0:h, 0:w]
    d[22:44] = 1200 + 3 * xs[22:44] + 2 * ys[22:44]
    heights = np.array([0, 0, 0, 30, 49, 50, 120, 399, 400, 401, 900])
    blocks = rng.choice(heights, ((h - 44 + 10) // 11, (w + 12) // 13))
    d[44:] = 1300 + np.kron(blocks, np.ones((11, 13), np.int64))[:h - 44, :w]
    d[30:36, 70:76] += 400
    d[8:10, 100:103] += 1
    return np.ascontiguousarray(d.astype(np.uint16))


# 400 is the largest threshold of the closed form, 401 takes the 64-bit path; 0 and a negative threshold admit nothing.
@pytest.mark.parametrize("diff", [1, 50, 400, 401, 0, -3])
def test_thresholds(ctx, oracle, diff):
    d = _steps_frame()
    working, alladm, mixed = wave_steps(d, 2000, diff)
    assert working.any() and mixed.any()
    if diff > 0:
        assert alladm.any()
    else:
        assert not alladm.any() and np.array_equal(working, mixed)
    if diff == 400:                                        # 399, 400 and 401 tell the thresholds apart
        assert not np.array_equal(wave_steps(d, 2000, 401)[2], mixed) or not np.array_equal(
            oracle.quantized_normals(d, 2000, 401), oracle.quantized_normals(d, 2000, 400))
    _check(ctx, oracle, d, 2000, diff, what="steps")


def _stairs(w, h, along_x, top=None):
    """Depth that changes by exactly 399 every five pixels along one axis, up to the middle and down again: every lane's
    neighbours on that axis are at +-399, the bracket of b0 (b1) is +-6 * 399."""
    n = w if along_x else h
    j = np.arange(n) // 5
    J = j.max() // 2
    f = 399 * (J - np.abs(j - J))
    d = (1000 + f) if top is None else (top - f.max() + f)
    d = np.broadcast_to(d[None, :] if along_x else d[:, None], (h, w))
    return np.ascontiguousarray(d.astype(np.uint16))


@pytest.mark.parametrize("top", [None, 65535])
@pytest.mark.parametrize("along_x", [True, False])
def test_range_of_b(ctx, oracle, along_x, top):
    w, h = 136, 60
    d = _stairs(w, h, along_x, top)
    assert top is None or int(d.max()) == 65535
    working, alladm, mixed = wave_steps(d, 65536, 400)
    assert alladm.any() and not mixed.any()
    D = d.astype(np.int64)
    n = [D[5 + dy:h - 6 + dy, 5 + dx:w - 6 + dx] for dx, dy in _RING]
    b0, b1 = (n[2] + n[4] + n[7]) - (n[0] + n[3] + n[5]), (n[5] + n[6] + n[7]) - (n[0] + n[1] + n[2])
    b = b0 if along_x else b1
    assert int(b.max()) == 6 * 399 and int(b.min()) == -6 * 399, (int(b.min()), int(b.max()))
    e = _check(ctx, oracle, d, 65536, 400, what="stairs")
    assert len(np.unique(e[5:h - 6, 5:w - 6])) >= 2


def test_depth_near_65535(ctx, oracle):
    w, h = 136, 40
    d = _plane(w, h, 65535, -2, -3)
    d[0, 0] = 65535
    working, alladm, mixed = wave_steps(d, 65536, 400)
    assert alladm.any() and not mixed.any() and int(d[5:h - 6, 5:w - 6].max()) > 65500
    e = _check(ctx, oracle, d, 65536, 400, what="near 65535")
    assert (e[8:h - 9, 8:w - 9] != 0).all()


def _random_frame(w, h, seed):
    """Piecewise planar with noise +-1: horizontal bands of their own planes, more than 60 apart, some of them cut once."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    d = np.zeros((h, w), np.int64)
    y, k = 0, 0
    while y < h:
        bh = int(rng.integers(16, 40))
        rows = slice(y, min(h, y + bh))
        d[rows] = 700 + 130 * (k % 7) + int(rng.integers(-3, 4)) * xs[rows] // 2 + int(rng.integers(-3, 4)) * ys[rows]
        if rng.random() < 0.4:
            cut = int(rng.integers(10, w - 10))
            d[rows, cut:] += 90
        y += bh
        k += int(rng.integers(1, 4))
    d += rng.integers(-1, 2, (h, w))
    return np.ascontiguousarray(np.clip(d, 1, 65535).astype(np.uint16))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_frames(ctx, oracle, seed):
    d = _random_frame(200, 90, seed)
    working, alladm, mixed = wave_steps(d)
    share = alladm.sum() / working.sum()
    print("seed %d: %d working wave-steps, %.3f all-admitted" % (seed, int(working.sum()), share))
    assert 0.25 <= share <= 0.75, share
    _check(ctx, oracle, d, what="random")


# The batched launch, which writes level 1's image beside level 0's, with chunks of 60 rows (a seam at row 60) and of 120.
@pytest.mark.parametrize("rows", [60, 120])
def test_two_levels(ctx, oracle, rows):
    w, h = 184, 90
    rng = np.random.default_rng(5)
    depths = [_random_frame(w, h, 10 + i) for i in range(3)]
    for d in depths:
        working, alladm, mixed = wave_steps(d)
        assert alladm.any() and mixed.any()
    bgrs = [np.ascontiguousarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(3)]
    exps = [oracle.quantize_pyramid(b, d, 2) for b, d in zip(bgrs, depths)]
    assert not np.array_equal(exps[0][1], exps[1][1]) and not np.array_equal(exps[1][1], exps[2][1])
    with options(ctx, {"frontend_chunk_rows": rows}):
        got = ctx.dev_front_images(bgrs, depths, 2)
    for i, e in enumerate(exps):
        for l in range(2):
            g = got[i][l]["q1"]
            print("rows %d frame %d level %d: %d bytes differ" % (rows, i, l, int((g != e[2 * l + 1]).sum())))
            assert np.array_equal(g, e[2 * l + 1]), (rows, i, l)
