"""GPU parity of the 256-thread parity ICP kernel's 16-bit builds (option icp_idx16, fl_icp.hip): nn[] and perm[] held as 16-bit
values, "no partner" as 0xFFFF, and the distance phase's reference point rebuilt from a 16-bit crop pixel and its depth factor.

Every case goes through fl_detection with icp_wide 0, so that the single job runs the 256-thread kernel, in FL_ICP_PARITY with
three forced iterations (index pairs, then two searched ones), under icp_occ 4 and 5 and under icp_idx16 0 and 1.  Each result
is compared with the float32 oracle field by field and bit for bit, and the two builds' results with each other.  The crops are
the smallest at which the index width can go wrong: fewer points than a search step, ragged tiles, indices above 2^15, the
largest capacity of the 16-bit build (65535), the first one beyond it (the 32-bit build must run), pixel != index (holes),
stored "none" entries (dropped pairs) and a crop of more tiles than the tile order's scratch holds (perm[] in index order).
"""
import functools

import numpy as np
import pytest

from fealess_amd import api
from fealess_amd import _lib as L

import util

pytestmark = pytest.mark.gpu

IT = 3                       # iteration 1 pairs by index; 2 and 3 search, store nn[] and read it back
DIST_MEAN_THR = -1.0         # with these two thresholds the loop never stops early: exactly IT iterations
FORCE_ALL_ITERS = -3.0e38
K = (601.5, 604.25, 131.75, 127.5)


def _surface(w, h, z0, gx, gy, amp, phase):
    """A depth image in mm: a tilted plane with a ripple, everywhere inside (0, 900]."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    z = z0 + gx * x + gy * y + amp * np.sin(0.11 * x + phase) * np.cos(0.07 * y)
    assert z.min() > 1 and z.max() < 890
    return np.round(z).astype(np.uint16)


def _frames(cw, ch, kind="plain"):
    """(model, scene, rect_model, rect_ref): both crops cw x ch, at different places of their images."""
    w, h = cw + 16, ch + 10
    gy = 0.004 if kind == "tall" else 0.13                    # (a crop of 23 k rows stays below 900 mm)
    scene = _surface(w, h, 610.0, 0.22, gy, 3.0, 0.0)
    model = _surface(w, h, 614.0, 0.20, gy + 0.02 * gy / 0.13, 3.0, 0.4)
    rect_model, rect_ref = (3, 2, cw, ch), (9, 5, cw, ch)
    if kind == "holes":
        # zeros and depths beyond 900 mm in both images; crop pixel 0 and the last crop pixel among them
        rng = np.random.default_rng(16)
        for img, (x0, y0, _, _), first, last in ((scene, rect_ref, 0, 901), (model, rect_model, 950, 0)):
            crop = img[y0:y0 + ch, x0:x0 + cw]
            r = rng.random((ch, cw))
            crop[r < 0.06] = 0
            crop[(r >= 0.06) & (r < 0.12)] = 901 + (rng.integers(0, 3000, (ch, cw)))[(r >= 0.06) & (r < 0.12)]
            crop[0, 0] = first
            crop[ch - 1, cw - 1] = last
    if kind == "dropped":
        # the right eighth of the model crop stands 40 mm behind its surface: no reference point within sqrt(3 dist_mean) of it
        x0, y0 = rect_model[0], rect_model[1]
        model[y0:y0 + ch, x0 + cw - cw // 8:x0 + cw] += 40
    return model, scene, rect_model, rect_ref


CASES = {
    "partial_step_20x3": (20, 3, "plain"),
    "ragged_tiles_37x29": (37, 29, "plain"),
    "above_2p15_224x147": (224, 147, "plain"),
    "limit_257x255": (257, 255, "plain"),
    "beyond_256x256": (256, 256, "plain"),
    "holes_97x61": (97, 61, "holes"),
    "dropped_pairs_97x61": (97, 61, "dropped"),
    # beyond the issue's table: more 16x4 tiles (5881) than build_tile_order's LDS scratch counts (5880), so perm[] is written in
    # index order by its fallback loop, which the 16-bit builds address differently
    "tile_order_fallback_2x23524": (2, 23524, "tall"),
}
RM = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], np.float32)
TM = np.array([1.5, -2.25, 3.0], np.float32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's frames and the oracle's result, computed once and shared by its parametrisations."""
    import oracle_py
    cw, ch, kind = CASES[name]
    model, scene, rect_model, rect_ref = _frames(cw, ch, kind)
    args = (model, scene, K, rect_model, rect_ref, IT, DIST_MEAN_THR, FORCE_ALL_ITERS, RM, TM)
    exp = oracle_py.detection(*args, accum64=False)
    for a in (model, scene):
        a.setflags(write=False)
    return args, exp


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flat(d):
    """Every field of a detection result as one list of (name, bit pattern or integer)."""
    ic = d["icp"]
    return [("n_points", d["n_points"]), ("iters", ic["iters"]), ("n_corr_last", ic["n_corr_last"]),
            ("R_final", _bits(d["R_final"]).tolist()), ("T_final", _bits(d["T_final"]).tolist()),
            ("icp.R", _bits(ic["R"]).tolist()), ("icp.T", _bits(ic["T"]).tolist()),
            ("dist_mean", int(_bits(ic["dist_mean"]).ravel()[0])), ("px_ratio", int(_bits(ic["px_ratio"]).ravel()[0]))]


@pytest.mark.parametrize("occ", [4, 5])
@pytest.mark.parametrize("name", list(CASES))
def test_detection_16_bit_and_32_bit_builds_equal_the_oracle(ctx, oracle, name, occ):
    args, exp = _case(name)
    cw, ch, kind = CASES[name]
    assert exp["rc"] == 0 and exp["icp"]["iters"] == IT
    if kind in ("plain", "tall"):
        assert exp["n_points"] == cw * ch                      # all pixels valid: the highest pixel is a point
    if kind == "holes":
        assert 3 <= exp["n_points"] < cw * ch
    if kind == "dropped":
        assert 3 <= exp["icp"]["n_corr_last"] < exp["n_points"]   # some points have no partner: "none" is stored and read
    got = {}
    for idx16 in (0, 1):
        with util.options(ctx, {"icp_wide": 0, "icp_occ": occ, "icp_idx16": idx16}):
            got[idx16] = ctx.detection(*args, L.FL_ICP_PARITY)
        assert got[idx16]["status"] == 0
        assert _flat(got[idx16]) == _flat(exp), (name, occ, idx16)
    assert _flat(got[0]) == _flat(got[1])


def test_icp_idx16_option_range_and_environment(ctx, monkeypatch):
    """icp_idx16 takes -1, 0 and 1, refuses -2 and 2 with FL_ERR_INVALID and keeps its value then; FL_ICP_IDX16 is read when a
    context is created and at no other time."""
    assert ctx.get_option("icp_idx16") == -1
    for v in (-1, 0, 1):
        with util.options(ctx, {"icp_idx16": v}):
            assert ctx.get_option("icp_idx16") == v
    for bad in (-2, 2):
        with pytest.raises(api.FealessError) as e:
            ctx.set_option("icp_idx16", bad)
        assert e.value.code == L.FL_ERR_INVALID and ctx.get_option("icp_idx16") == -1
    monkeypatch.setenv("FL_ICP_IDX16", "0")
    assert ctx.get_option("icp_idx16") == -1                  # a variable that appears later changes nothing
    c2 = api.Context(0)
    try:
        assert c2.get_option("icp_idx16") == 0                # a context created now starts from it
        monkeypatch.setenv("FL_ICP_IDX16", "1")
        assert c2.get_option("icp_idx16") == 0
    finally:
        c2.close()
    monkeypatch.setenv("FL_ICP_IDX16", "2")                   # out of range in the environment: the built-in default
    c3 = api.Context(0)
    try:
        assert c3.get_option("icp_idx16") == -1
    finally:
        c3.close()
