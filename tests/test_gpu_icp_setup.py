"""GPU parity of the 256-thread parity ICP kernel's set-up (fl_icp.hip): the crop's tile order (crop_clouds, build_tile_order)
and the fused first pass (first_pass: pre-translation, copyPoints, the initial distances and iteration 1's sums in one
producer / chain pass of 192-row tiles).

As in test_gpu_icp_idx16.py every case goes through fl_detection with icp_wide 0, so that the single job runs the 256-thread
kernel, in FL_ICP_PARITY, under icp_occ 4 and 5 and under icp_idx16 0 and 1; each result is compared with the float32 oracle
field by field and bit for bit.  The shapes are the smallest at which the new code can go wrong:
  rows per tile   crops of 1 .. 64, 191, 192, 193 and 2 * 192 + 1 kept points (one tile, the exact boundary, one row into the
                  next tile, an odd number of tiles for the two register sets); fewer than three points give "none"
  tile counts     ragged tiles (37 x 29), one tile (16 x 4), an even and an odd number of tile rows (the serpentine), holes at
                  crop pixel 0, at the last pixel and over one whole 16 x 4 tile, and the 2 x 23524 crop of more tiles than the
                  scratch holds (index order, nothing counted)
  loop control    it_thr 0 (the first pass's sums are dropped), 1 (only the index-pair iteration, fed by them), 3, and a
                  dist_mean_thr above the initial dist_mean (the loop stops before iteration 1)
  copyPoints      model points whose z passes 900 mm under the pre-translation become (0, 0, 0)
"""
import functools

import numpy as np
import pytest

from fealess_amd import _lib as L

import util
from test_gpu_icp_idx16 import DIST_MEAN_THR, FORCE_ALL_ITERS, K, RM, TM, _flat, _frames

pytestmark = pytest.mark.gpu

TQ = 192                     # rows per LDS tile of the 256-thread kernel (three producer waves)
BUILDS = [(occ, idx16) for occ in (4, 5) for idx16 in (0, 1)]


def _holes_with_an_empty_tile(cw, ch):
    """The idx16 test's holes (zeros and depths beyond 900 mm in both images, crop pixel 0 and the last one among them) and, on
    top, one whole 16 x 4 tile of the scene crop cleared: tile column 2 of tile row 3."""
    model, scene, rect_model, rect_ref = _frames(cw, ch, "holes")
    x0, y0 = rect_ref[0], rect_ref[1]
    scene[y0 + 12:y0 + 16, x0 + 32:x0 + 48] = 0
    return model, scene, rect_model, rect_ref


def _deep_model(cw, ch):
    """A model crop with depths up to 899 mm under a scene about 6 mm behind it: the pre-translation t_tmp = mean(ref) - mean(mod)
    lifts the deepest model points beyond 900 mm, where copyPoints zeroes them."""
    w, h = cw + 16, ch + 10
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    model = np.round(850.0 + 0.10 * x + 0.06 * y + 2.0 * np.sin(0.11 * x) * np.cos(0.07 * y)).astype(np.uint16)
    scene = np.round(856.0 + 0.11 * x + 0.05 * y + 2.0 * np.sin(0.11 * x + 0.4) * np.cos(0.07 * y)).astype(np.uint16)
    rect_model, rect_ref = (3, 2, cw, ch), (9, 5, cw, ch)
    crop = model[rect_model[1]:rect_model[1] + ch, rect_model[0]:rect_model[0] + cw]
    crop[5:8, 7:11] = 899                                      # a patch, the first point of a tile row and the last point
    crop[8, 0] = 898
    crop[ch - 1, cw - 1] = 899
    assert model.max() <= 899 and scene.max() < 900 and min(model.min(), scene.min()) > 1
    return model, scene, rect_model, rect_ref


def _crossing_points(model, scene, rect_model, rect_ref):
    """How many model points the pre-translation lifts beyond 900 mm, from the inputs alone (every pixel of these crops is valid,
    so t_tmp.z is the difference of the crops' mean depths; the count asks for a margin of half a millimetre)."""
    (mx, my, cw, ch), (rx, ry, _, _) = rect_model, rect_ref
    zm = model[my:my + ch, mx:mx + cw].astype(np.float64)
    zs = scene[ry:ry + ch, rx:rx + cw].astype(np.float64)
    assert zm.max() <= 900 and zs.max() <= 900 and zm.min() > 0 and zs.min() > 0
    return int((zm + (zs.mean() - zm.mean()) > 900.5).sum())


# name -> (frames, it_thr, what the loop must have done: iterations, or None where fewer than three points leave "none")
def _plain(cw, ch):
    return lambda: _frames(cw, ch, "plain")


CASES = {}
for _n in (191, 192, 193):
    CASES["rows_%d" % _n] = (_plain(_n, 1) if _n != 192 else _plain(16, 12), 3)
CASES["rows_385_35x11"] = (_plain(35, 11), 3)
CASES["ragged_tiles_37x29"] = (_plain(37, 29), 3)
CASES["one_tile_16x4"] = (_plain(16, 4), 3)
CASES["even_tile_rows_40x8"] = (_plain(40, 8), 3)
CASES["odd_tile_rows_40x12"] = (_plain(40, 12), 3)
CASES["holes_empty_tile_97x61"] = (lambda: _holes_with_an_empty_tile(97, 61), 3)
CASES["tile_order_fallback_2x23524"] = (lambda: _frames(2, 23524, "tall"), 3)
CASES["no_iteration_37x29"] = (_plain(37, 29), 0)
CASES["index_pairs_only_37x29"] = (_plain(37, 29), 1)
CASES["deep_model_45x23"] = (lambda: _deep_model(45, 23), 3)


def _oracle(frames, it_thr, dist_mean_thr=DIST_MEAN_THR):
    import oracle_py
    model, scene, rect_model, rect_ref = frames
    args = (model, scene, K, rect_model, rect_ref, it_thr, dist_mean_thr, FORCE_ALL_ITERS, RM, TM)
    return args, oracle_py.detection(*args, accum64=False)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's frames and the oracle's result, computed once and shared by its parametrisations."""
    make, it_thr = CASES[name]
    frames = make()
    args, exp = _oracle(frames, it_thr)
    for a in frames[:2]:
        a.setflags(write=False)
    return args, exp


def _run(ctx, args, occ, idx16):
    with util.options(ctx, {"icp_wide": 0, "icp_occ": occ, "icp_idx16": idx16}):
        got = ctx.detection(*args, L.FL_ICP_PARITY)
    assert got["status"] == 0
    return got


@pytest.mark.parametrize("occ,idx16", BUILDS)
@pytest.mark.parametrize("name", list(CASES))
def test_detection_equals_the_oracle(ctx, oracle, name, occ, idx16):
    args, exp = _case(name)
    it_thr = CASES[name][1]
    model, scene, rect_model, rect_ref = args[0], args[1], args[3], args[4]
    assert exp["rc"] == 0 and exp["icp"]["iters"] == it_thr
    if name.startswith("rows_"):
        assert exp["n_points"] == int(name.split("_")[1])       # every pixel is a point
    if name.startswith("holes"):
        assert 3 <= exp["n_points"] < rect_ref[2] * rect_ref[3] - 64
    if name.startswith("deep_model"):
        assert exp["n_points"] == rect_ref[2] * rect_ref[3]
        assert _crossing_points(model, scene, rect_model, rect_ref) >= 1
    assert _flat(_run(ctx, args, occ, idx16)) == _flat(exp), (name, occ, idx16)


@functools.lru_cache(maxsize=None)
def _small_crops():
    """Crops of 1 .. 64 points (n x 1 pixels, all valid) and the oracle's results."""
    return [_oracle(_frames(n, 1, "plain"), 3) for n in range(1, 65)]


@pytest.mark.parametrize("occ,idx16", BUILDS)
def test_crops_of_1_to_64_points(ctx, oracle, occ, idx16):
    """One tile, partly filled; one and two points are fewer than icpCloudToCloud_Ex takes: the result is "none"."""
    for n, (args, exp) in enumerate(_small_crops(), start=1):
        assert exp["rc"] == 0 and exp["n_points"] == n
        if n < 3:
            assert exp["icp"]["iters"] == 0 and float(exp["icp"]["dist_mean"]) == -1.0 and not exp["icp"]["R"].any()
        else:
            assert exp["icp"]["iters"] == 3
        assert _flat(_run(ctx, args, occ, idx16)) == _flat(exp), (n, occ, idx16)


@functools.lru_cache(maxsize=None)
def _stopped_before_iteration_1():
    """A dist_mean_thr above the initial dist_mean, taken from the oracle's own run without iterations."""
    frames = _frames(37, 29, "plain")
    _, first = _oracle(frames, 0)
    d0 = float(first["icp"]["dist_mean"])
    assert first["icp"]["iters"] == 0 and np.isfinite(d0) and d0 > 0
    return _oracle(frames, 3, dist_mean_thr=2.0 * d0) + (d0,)


@pytest.mark.parametrize("occ,idx16", BUILDS)
def test_loop_stops_before_iteration_1(ctx, oracle, occ, idx16):
    """dist_mean <= dist_mean_thr at the loop head: no iteration although it_thr allows three; the first pass's sums are dropped and
    dist_mean / px_ratio are the initial ones."""
    args, exp, d0 = _stopped_before_iteration_1()
    assert exp["rc"] == 0 and exp["icp"]["iters"] == 0 and float(exp["icp"]["dist_mean"]) == d0
    assert _flat(_run(ctx, args, occ, idx16)) == _flat(exp), (occ, idx16)
