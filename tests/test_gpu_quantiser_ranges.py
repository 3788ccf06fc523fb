"""GPU: the quantisers against the oracle on images that drive their arithmetic to its ends (the depth quantiser's products,
square root, reciprocal and LUT index; the colour quantiser's arctangent quotient), bit for bit, as tests/test_gpu_frontend.py
compares ordinary images.  Sizes 70 x 23 and 131 x 17: a strip boundary at column 60, a last strip of 10 or 11 columns, and
interior pixels (y in 5 .. h - 7, x in 5 .. w - 7) in both.

The depth images are staircases over 5 x 5 blocks: depth(x, y) = base + CLASS * (5 * (y % 5) + x % 5) + step pattern of the block
(x // 5, y // 5).  A pixel's eight neighbours at +-5 share its (x % 5, y % 5) class, so their differences are those of the block
pattern alone, whatever the class offset: every interior pixel of an image meets the same neighbour steps at its own depth, and
the 25 classes times the blocks of a row spread the centre depths over the whole 16-bit range."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(70, 23), (131, 17)]
THRESHOLDS = [1, 50, 400, 401]          # the int32 path (<= 400), its boundary, the 64-bit path
FAR = 65536                             # distance_threshold: every depth passes
CLASS = 2622                            # 25 classes * 2622 >= 65536


def _grid(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return 5 * (y % 5) + x % 5, x // 5, y // 5


def _interior(w, h):
    m = np.zeros((h, w), bool)
    m[5:h - 6, 5:w - 6] = True
    return m


def _well_formed(raw):
    """interior pixels whose own depth and whose eight neighbours' were not clipped into 0 .. 65535"""
    h, w = raw.shape
    ok = (raw >= 0) & (raw <= 65535)
    m = _interior(w, h)
    out = m.copy()
    for dy in (-5, 0, 5):
        for dx in (-5, 0, 5):
            out[5:h - 6, 5:w - 6] &= ok[5 + dy:h - 6 + dy, 5 + dx:w - 6 + dx]
    return out


def _check(ctx, oracle, raw, t, covered=None):
    depth = np.clip(raw, 0, 65535).astype(np.uint16)
    got, exp = ctx.quantized_normals(depth, FAR, t), oracle.quantized_normals(depth, FAR, t)
    assert np.array_equal(got, exp), (t, int((got != exp).sum()), np.argwhere(got != exp)[:4].tolist())
    if covered is not None:
        covered[depth[_well_formed(raw)]] = True
    return exp


def _staircase_bases(step, blocks):
    """Bases under which the centre depths base + CLASS * k + step * b (k in 0 .. 24, b in 1 .. blocks) take every value from
    `step` on: a depth d = step + CLASS * k + q, q < CLASS, is met at base = q % step + span * (q // span), span = step * blocks,
    in block b = 1 + (q % span) // step.  Step 0: one class per depth."""
    if step == 0:
        return range(CLASS)
    span = step * blocks
    return [a + span * m for m in range((CLASS - 1) // span + 1) for a in range(step)]


@pytest.mark.parametrize("t", THRESHOLDS)
def test_normals_steps_around_every_depth(ctx, oracle, t):
    """Neighbour steps of +-(t - 1) (gates open: the largest |nx| the threshold admits, 617 * 150 * 30 * (t - 1)) and of +-t (those
    gates closed) around EVERY depth 1 .. 65535 that has both neighbours: rising and falling staircases along x on 131 x 17
    (24 interior blocks).  The same along y (the largest |ny|) on 70 x 23, whose 3 interior block rows would take eight times
    the images: there every 7th base.  A flat image (step 0: t = 1) has every gate open and ddx = ddy = 0."""
    n_images = 0
    for step in (t - 1, t):
        for rising in ((True, False) if step else (True,)):
            for axis, (w, h) in (("x", SIZES[1]), ("y", SIZES[0])):
                k, bx, by = _grid(w, h)
                b = bx if axis == "x" else by
                blocks = int(b[_interior(w, h)].max())
                stairs = step * (b if rising else blocks + 1 - b)
                covered = np.zeros(65536, bool)
                bases = _staircase_bases(step, blocks)
                for base in bases if axis == "x" else bases[::7]:
                    _check(ctx, oracle, base + CLASS * k + stairs, t, covered)
                    n_images += 1
                if axis == "x":
                    lo, hi = max(1, step), 65535 - step
                    missing = np.flatnonzero(~covered[lo:hi + 1])
                    assert missing.size == 0, (t, step, rising, (missing[:5] + lo).tolist(), missing.size)
    print(f"t {t}: {n_images} images")


@pytest.mark.parametrize("t", THRESHOLDS)
@pytest.mark.parametrize("w,h", SIZES)
def test_normals_equal_steps_all_gates_open(ctx, oracle, w, h, t):
    """Blocks (even, even) stand e = +-(t - 1) above all their eight neighbour blocks: all gates open with equal steps, so
    ddx = ddy = 0, det = 22500 and s is exactly |nz| = 22500 * d -- the largest det * d at d = 65535."""
    k, bx, by = _grid(w, h)
    dots = ((bx % 2 == 0) & (by % 2 == 0)).astype(np.int64)
    some = False
    for e in (t - 1, 1 - t):
        for base in list(range(0, CLASS, 131)) + [65535 - 24 * CLASS - max(e, 0)]:
            raw = base + max(-e, 0) + CLASS * k + e * dots
            exp = _check(ctx, oracle, raw, t)
            some |= bool(exp[_interior(w, h) & (dots == 1)].any())
    assert some


@pytest.mark.parametrize("t", THRESHOLDS)
@pytest.mark.parametrize("w,h", SIZES)
def test_normals_all_gates_closed(ctx, oracle, w, h, t):
    """Steps of t along x and 2 t along y: the eight differences are +-t, +-2 t, +-t +- 2 t, none below t, so s == 0 and
    every code is 0."""
    k, bx, by = _grid(w, h)
    for base in range(0, CLASS, 437):
        raw = base + CLASS * k + t * bx + 2 * t * by
        exp = _check(ctx, oracle, raw, t)
        assert not exp[_well_formed(raw)].any()


@pytest.mark.parametrize("t", THRESHOLDS)
@pytest.mark.parametrize("w,h", SIZES)
def test_normals_random_full_range(ctx, oracle, w, h, t):
    rng = np.random.default_rng(1000 * t + w)
    for _ in range(8):
        _check(ctx, oracle, rng.integers(0, 65536, (h, w)).astype(np.int64), t)
    # full-range noise passes almost no gate at these thresholds: a slope under noise, both of the threshold's size, does
    y, x = np.mgrid[0:h, 0:w]
    for _ in range(8):
        raw = 30000 + (t // 10) * x - (t // 16) * y + rng.integers(-(t // 4), t // 4 + 1, (h, w))
        assert _check(ctx, oracle, raw, t).any()


# ---- colour ---------------------------------------------------------------------------------------------------------------

def _check_color(ctx, oracle, bgr):
    got, exp = ctx.quantized_orientations(bgr, 10.0), oracle.quantized_orientations(bgr, 10.0)
    assert np.array_equal(got, exp), (int((got != exp).sum()), np.argwhere(got != exp)[:4].tolist())
    return exp


@pytest.mark.parametrize("period", [1, 2, 3, 5, 8])
def test_orientations_checkerboards(ctx, oracle, period):
    """0 / 255 checkerboards, per channel and in all three: the largest differences the blurred image can carry into the Sobel
    sums, at several block sizes (the 7 x 7 blur flattens the finest)."""
    w, h = SIZES[0]
    y, x = np.mgrid[0:h, 0:w]
    board = ((((x // period) + (y // period)) & 1) * 255).astype(np.uint8)
    hit = False
    for channels in ([0], [1], [2], [0, 1, 2]):
        for img in (board, 255 - board):
            bgr = np.zeros((h, w, 3), np.uint8)
            bgr[..., channels] = img[..., None]
            hit |= bool(_check_color(ctx, oracle, bgr).any())
    assert hit or period == 1


def test_orientations_edges_and_impulses(ctx, oracle):
    """Straight 0 / 255 edges in every direction of the 16 bins (the largest |dx|, |dy| and their ratios) and single-pixel
    impulses, in the image, on its border and beside the strip boundary at column 60."""
    w, h = SIZES[0]
    y, x = np.mgrid[0:h, 0:w]
    for a in np.arange(0, 360, 11.25):
        side = (np.cos(np.deg2rad(a)) * (x - 34.5) + np.sin(np.deg2rad(a)) * (y - 11.5)) > 0
        bgr = np.repeat((side * 255).astype(np.uint8)[..., None], 3, axis=2)
        assert _check_color(ctx, oracle, bgr).any()
    for value, ground in ((255, 0), (0, 255), (1, 0)):
        for ch in range(3):
            bgr = np.full((h, w, 3), ground, np.uint8)
            for px, py in ((0, 0), (69, 22), (34, 11), (59, 5), (60, 17), (61, 11), (3, 20), (66, 2)):
                bgr[py, px, ch] = value
            _check_color(ctx, oracle, bgr)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_orientations_random(ctx, oracle, seed):
    w, h = SIZES[0]
    rng = np.random.default_rng(seed)
    bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    _check_color(ctx, oracle, bgr)
    # two-valued noise: Sobel sums at and near their ends
    assert _check_color(ctx, oracle, (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)) is not None
