"""GPU parity of the depth quantiser (k_depth_quantize) where its register ring can go wrong.  A lane keeps the depth at the
columns x - 5, x, x + 5 (clamped into the row) for the rows c - 5 .. c + 5 of its current row of normals, loads one row ahead
(three loads a step) and trades the ring's slots over an unrolled loop of twelve steps; a chunk starts with a prologue that
loads the rows ahead of its first row, clamped into the image; virtual rows above row 0 and below row h - 1 leave the ring
alone.  Every image is compared byte for byte with the oracle's.

The depth image is a curved surface with steps, holes and far pixels, so that many labels occur and the gates go both ways;
for every size of at least 24 x 24 the oracle's own image has at least 6 distinct bytes, labels on at least 0.8 of the interior
and at least 0.05 of the vertically adjacent pairs differing (a ring that repeats or skips a row cannot pass)."""
import numpy as np
import pytest

from util import options

pytestmark = pytest.mark.gpu


def _depth(w, h, seed=None):
    seed = 1000 * w + h if seed is None else seed
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.default_rng(seed)
    d = 900 + 40 * np.sin(xs / 6 + seed % 7) + 40 * np.cos(ys / 5) + 25 * np.sin((xs + 2 * ys) / 9) + rng.integers(0, 3, (h, w))
    d += 120 * (((xs // 37).astype(int) + (ys // 29).astype(int)) % 2)
    d = d.astype(np.uint16)
    d[rng.random((h, w)) < 0.01] = 0
    if w > 20 and h > 20:
        d[h // 2:h // 2 + 3, w // 3:w // 3 + 6] = 2500
    return np.ascontiguousarray(d)


_CASES = {}


def _case(oracle, w, h, dist=2000, diff=50):
    """The depth image of a size and the oracle's image of it, computed once per size and thresholds and never modified."""
    key = (w, h, dist, diff)
    if key not in _CASES:
        d = _depth(w, h)
        e = oracle.quantized_normals(d, dist, diff)
        if w >= 24 and h >= 24 and (dist, diff) == (2000, 50):             # not vacuous
            inner = e[5:h - 6, 5:w - 6]
            values, share = len(np.unique(e)), float((inner != 0).mean())
            pairs = float((e[1:] != e[:-1]).mean())
            print("oracle image %dx%d: %d values, interior share %.3f, differing vertical pairs %.3f" % (w, h, values, share, pairs))
            assert inner.size == (w - 11) * (h - 11)
            assert values >= 6 and share >= 0.8 and pairs >= 0.05, (w, h, values, share, pairs)
        _CASES[key] = (d, e)
    return _CASES[key]


def _check(ctx, oracle, w, h, dist=2000, diff=50):
    d, e = _case(oracle, w, h, dist, diff)
    got = ctx.quantized_normals(d, dist, diff)
    print("%dx%d thresholds %d %d: %d bytes differ" % (w, h, dist, diff, int((got != e).sum())))
    assert np.array_equal(got, e)


# No interior below 12 rows; the prologue's rows clamp at the top and at the bottom at once.
@pytest.mark.parametrize("h", [1, 5, 11, 12, 13, 16, 23, 24, 25])
def test_interior_appears_and_rows_clamp(ctx, oracle, h):
    _check(ctx, oracle, 70, h)


# The clamped tap columns, the strip seams (60 columns a strip, two halo lanes a side) and the w - 6 bound.
@pytest.mark.parametrize("w", [1, 5, 11, 12, 13, 24, 59, 60, 61, 64, 65, 66, 67, 119, 120, 121, 125, 126, 127])
def test_columns_strip_seams_and_right_bound(ctx, oracle, w):
    _check(ctx, oracle, w, 30)


# Rows whose taps y +- 5 and median rows y +- 2 lie in the neighbouring chunk; last chunks of 1 to 12 rows, shorter than one
# unrolled period.
@pytest.mark.parametrize("rows", [60, 120])
@pytest.mark.parametrize("h", [59, 60, 61, 65, 66, 67, 71, 72, 119, 120, 121, 126, 127, 132, 250])
def test_chunk_seams(ctx, oracle, h, rows):
    with options(ctx, {"frontend_chunk_rows": rows}):
        _check(ctx, oracle, 70, h)


# Both accumulation paths (difference_threshold <= 400 in 32 bits, above in 64) at a seam, and a distance_threshold that
# cuts through the surface.
@pytest.mark.parametrize("dist,diff", [(2000, 50), (2000, 400), (2000, 401), (900, 50)])
def test_thresholds_at_a_seam(ctx, oracle, dist, diff):
    with options(ctx, {"frontend_chunk_rows": 60}):
        d, e = _case(oracle, 70, 127, dist, diff)
        if dist == 900:
            assert 0.2 < float((d < 900).mean()) < 0.8                     # the gate goes both ways
        _check(ctx, oracle, 70, 127, dist, diff)


# The batched launch, which also writes level 1's image (dst1) beside level 0's: three different frames, two levels.
@pytest.mark.parametrize("w,h", [(124, 66), (64, 48)])
def test_batched_launch_with_level_1(ctx, oracle, w, h):
    rng = np.random.default_rng(7 * w + h)
    depths = [_depth(w, h, seed=1000 * w + h + 17 * i) for i in range(3)]
    bgrs = [np.ascontiguousarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(3)]
    exps = [oracle.quantize_pyramid(b, d, 2) for b, d in zip(bgrs, depths)]
    for i in range(3):
        for j in range(i):
            assert not np.array_equal(exps[i][1], exps[j][1]) and not np.array_equal(exps[i][3], exps[j][3]), (i, j)
    with options(ctx, {"frontend_chunk_rows": 60}):
        got = ctx.dev_front_images(bgrs, depths, 2)
    for i, e in enumerate(exps):
        for l in range(2):
            g = got[i][l]["q1"]
            print("frame %d level %d: %d bytes differ" % (i, l, int((g != e[2 * l + 1]).sum())))
            assert np.array_equal(g, e[2 * l + 1]), (w, h, i, l)
