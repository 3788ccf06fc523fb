"""GPU parity of k_refine_lds: a frame's candidates are ordered by location, cut into groups whose united window fits the LDS
budget, and refined on spread bytes staged in LDS.  Whatever the kernel (option refine_lds = 1: k_refine, 2: k_refine_lds
wherever the level's windows fit) and the budget (refine_lds_bytes: smaller budgets move the group boundaries), the match
list is the oracle's, bit for bit.  Every case asserts through fl_dev_refine_kernel that the kernel it is meant for ran.

Shapes are the smallest that still reach each path.  The edge case uses 200 x 120 at T = [5, 4]: finalize refuses a level whose
size is no multiple of its T or whose pixel count is no multiple of 16, and this is a small pyramid with a width that is no
multiple of 16, so that the image rows are misaligned against the 16-byte staging loads."""
import numpy as np
import pytest

import clutter
from fealess_amd import api, synth
from fealess_amd import _lib as L
from fealess_amd.bank import TemplateBank
from util import options

pytestmark = pytest.mark.gpu

BUDGET = 65536                       # FL_REFINE_LDS_BYTES


def _assert_matches_equal(got, exp, tag=None):
    assert len(got) == len(exp), (tag, len(got), len(exp))
    for k in ("x", "y", "class_idx", "template_id"):
        assert np.array_equal(got[k], exp[k]), (tag, k)
    assert np.array_equal(got["similarity"].view(np.uint32), exp["similarity"].view(np.uint32)), tag


def _quant_pyramid(rng, w0, h0, levels, M, density=0.35):
    return [synth.random_quantized(rng, w0 >> l, h0 >> l, density) for l in range(levels) for _ in range(M)]


def _planted_at(rng, qs, levels, M, ox, oy, bbox, nf0=63):
    """synth.planted_pyramid at a chosen place: the features are read off the frame's own pyramid inside the window at (ox, oy)."""
    tl = []
    for l in range(levels):
        s, x0, y0 = bbox >> l, ox >> l, oy >> l
        for m in range(M):
            q = qs[l * M + m][y0:y0 + s + 1, x0:x0 + s + 1]
            f = synth.features_from_quantized(q, np.ones_like(q, bool), nf0 >> l, rng, min_dist=3.0)
            assert f is not None
            tl.append(dict(width=s, height=s, offset_x=x0, offset_y=y0, pyramid_level=l, features=f))
    return tl


def _window_max(det, level):
    return int(L.dev(det.lib, "fl_dev_refine_window_max")(det.h, level))


def _ran(det, level):
    return int(L.dev(det.lib, "fl_dev_refine_kernel")(det.h, level))


def _modes(det, levels, extra=()):
    """(refine_lds, refine_lds_bytes) pairs: the old kernel, the new one with the whole budget, with the smallest budget every
    fine level still fits, with one between, and the case's own."""
    lo = max(_window_max(det, l) for l in range(levels - 1))
    assert 0 < lo <= BUDGET, lo
    return [(1, 0), (2, 0), (2, lo), (2, (lo + BUDGET) // 2)] + [(2, b) for b in extra if lo <= b <= BUDGET]


def _check(ctx, det, levels, run, exp, n_exp, extra=()):
    for mode, nbytes in _modes(det, levels, extra):
        with options(ctx, {"refine_lds": mode, "refine_lds_bytes": nbytes}):
            got, n_got = run()
        assert n_got == n_exp, (mode, nbytes, n_got, n_exp)
        _assert_matches_equal(got, exp, (mode, nbytes))
        assert [_ran(det, l) for l in range(levels - 1)] == [mode] * (levels - 1), (mode, nbytes)


# ---- the cases: quantised pyramid, bank, threshold (also used on the CPU with the oracle alone) ------------------------------
def case_group_splits(T=(5, 8), w0=160, h0=160, far=(100, 100), n=40):
    """Two levels at 160 x 160 (the reference asserts that 8 divides the coarse level's 80 rows), 40 templates, half planted
    around (8, 8) and half around (100, 100).  With another fine T (and a size it divides) the fine level takes the paths of
    "every other T": k_refine's byte loads and k_refine_lds<0>."""
    T = list(T)
    rng = np.random.default_rng(21)
    qs = _quant_pyramid(rng, w0, h0, 2, 2)
    bank = TemplateBank("obj", 2, 2)
    for i in range(n):
        ox, oy = ((8, 8), far)[i % 2]
        bank.add_pyramid(_planted_at(rng, qs, 2, 2, ox + 2 * (i % 5), oy + 2 * (i % 3), 32))
    return w0, h0, T, qs, bank, 70.0


def case_edges(T=(5, 4)):
    """200 x 120 at T = [5, 4]: templates planted at the four image edges and in the corners, and one as large as the image with
    features outside it, whose patches leave the linear memory (test_quirks_overread_oob_and_big_template).  At T = [2, 4] the
    same clamping and slow path run under the instantiation for every other T."""
    w0, h0, T = 200, 120, list(T)
    rng = np.random.default_rng(22)
    qs = _quant_pyramid(rng, w0, h0, 2, 2, density=0.5)
    bank = TemplateBank("obj", 2, 2)
    for ox, oy in ((0, 40), (w0 - 34, 40), (80, 0), (80, h0 - 34), (0, 0), (w0 - 34, h0 - 34)):
        bank.add_pyramid(_planted_at(rng, qs, 2, 2, ox, oy, 32))
    big0 = np.array([[0, 0, 0], [180, 100, 4], [100, 60, 2], [400, 3, 2], [5, 300, 2], [-3, 4, 1]], np.int32)
    big1 = np.array([[0, 0, 0], [90, 50, 4], [50, 30, 2], [9, 56, 0]], np.int32)
    bank.add_pyramid([dict(width=190, height=112, offset_x=0, offset_y=0, pyramid_level=0, features=big0),
                      dict(width=190, height=112, offset_x=0, offset_y=0, pyramid_level=0, features=big0[::-1].copy()),
                      dict(width=95, height=56, offset_x=0, offset_y=0, pyramid_level=1, features=big1),
                      dict(width=95, height=56, offset_x=0, offset_y=0, pyramid_level=1, features=big1)])
    return w0, h0, T, qs, bank, 10.0


def case_three_levels():
    """640 x 480: at 320 x 240 the middle level (160 x 120, T = 8) clamps every candidate to one place and nothing matches."""
    w0, h0, T = 640, 480, [5, 8, 4]
    rng = np.random.default_rng(23)
    qs = _quant_pyramid(rng, w0, h0, 3, 2)
    bank = synth.make_bank("obj", 30, 3, 2, w0, h0, seed=5, qs=qs, planted_frac=0.4, bbox=64)
    return w0, h0, T, qs, bank, 60.0


def case_one_modality():
    w0, h0, T = 320, 240, [4, 8]
    rng = np.random.default_rng(24)
    qs = _quant_pyramid(rng, w0, h0, 2, 1)
    bank = synth.make_bank("obj", 30, 2, 1, w0, h0, seed=6, qs=qs, planted_frac=0.3, bbox=96)
    return w0, h0, T, qs, bank, 65.0


def case_long_list():
    """Threshold -100 on a dense image: every non-zero coarse cell of every template is a candidate, far more than the
    FL_REFINE_BLOCK = 256 the kernel orders at a time."""
    w0, h0, T = 320, 240, [4, 8]
    rng = np.random.default_rng(25)
    qs = _quant_pyramid(rng, w0, h0, 2, 1, density=0.9)
    bank = synth.make_bank("obj", 12, 2, 1, w0, h0, seed=9, bbox=64)
    return w0, h0, T, qs, bank, -100.0


CASES = dict(group_splits=case_group_splits, edges=case_edges, three_levels=case_three_levels, one_modality=case_one_modality,
             group_splits_T2=lambda: case_group_splits(T=(2, 8), n=12),
             group_splits_T6=lambda: case_group_splits(T=(6, 8), w0=192, h0=144, far=(120, 80), n=15),
             edges_T2=lambda: case_edges(T=(2, 4)))


def _detector(ctx, T, M, bank, w0, h0, **kw):
    det = api.Detector(ctx, M, T)
    det.add_class(bank)
    det.finalize(w0, h0, **kw)
    return det


@pytest.mark.parametrize("name", sorted(CASES))
def test_match_list_equals_oracle_under_every_kernel_and_budget(ctx, oracle, name):
    w0, h0, T, qs, bank, thr = CASES[name]()
    M = len(qs) // len(T)
    exp, n_exp = oracle.match_quantized(qs, w0, h0, T, [bank], thr)
    assert n_exp > 0, "test is vacuous: no matches"
    if name.startswith("group_splits"):              # matches at both places
        assert (exp["x"] < 60).any() and (exp["x"] > 90).any()
    if name.startswith("edges"):                     # matches whose candidates were clamped on every side, and the big template's
        assert (exp["x"] < 40).any() and (exp["x"] > w0 - 74).any() and (exp["y"] < 40).any() and (exp["y"] > h0 - 74).any()
        assert (exp["template_id"] == 6).any()
    det = _detector(ctx, T, M, bank, w0, h0)
    try:
        extra = ()
        if name.startswith("group_splits"):          # one group per frame, several, and the tightest budget the level allows
            extra = (_window_max(det, 0) + 16 * 108, _window_max(det, 0) * 2)
        _check(ctx, det, len(T), lambda: det.match_quantized(qs, thr), exp, n_exp, extra)
        if name == "three_levels":                   # level 0 meets candidates that level 1 erased
            assert det.frame_counters(0)[0] > n_exp
    finally:
        det.close()


def test_frame_without_a_candidate(ctx, oracle):
    w0, h0, T, qs, bank, _ = case_group_splits()
    rng = np.random.default_rng(3)
    other = _quant_pyramid(rng, w0, h0, 2, 2, density=0.02)
    exp, n_exp = oracle.match_quantized(other, w0, h0, T, [bank], 95.0)
    assert n_exp == 0
    det = _detector(ctx, T, 2, bank, w0, h0)
    try:
        _check(ctx, det, 2, lambda: det.match_quantized(other, 95.0), exp, 0)
        assert det.frame_counters(0)[0] == 0
    finally:
        det.close()


@pytest.mark.parametrize("max_candidates", [0, 64])
def test_lists_longer_than_the_ordering_block(ctx, oracle, max_candidates):
    w0, h0, T, qs, bank, thr = case_long_list()
    exp, n_exp = oracle.match_quantized(qs, w0, h0, T, [bank], thr)
    assert n_exp > 100
    det = _detector(ctx, T, 1, bank, w0, h0, max_batch=1, max_candidates=max_candidates)
    try:
        for mode in (2, 1):
            with options(ctx, {"refine_lds": mode}):
                got, n_got = det.match_quantized(qs, thr, cap=1 << 17)
            assert n_got == n_exp, mode
            _assert_matches_equal(got, exp, mode)
            assert _ran(det, 0) == mode
        assert det.frame_counters(0)[0] > 256
    finally:
        det.close()


def test_batch_of_nine_frames(ctx, oracle):
    """Nine different frames in one batch against the same frames one at a time under the old kernel: nothing a group or a
    frame left in LDS may reach the next."""
    w0, h0, T = 320, 240, [5, 8]
    rng = np.random.default_rng(90)
    frames = []
    for i in range(9):
        bgr = (rng.integers(0, 256, (h0 // 8, w0 // 8, 3)) // 32 * 32).astype(np.uint8).repeat(8, 0).repeat(8, 1)
        bgr = np.roll(bgr, 3 * i, axis=1)
        depth = (600 + 40 * rng.integers(0, 4, (h0 // 16, w0 // 16))).astype(np.uint16).repeat(16, 0).repeat(16, 1)
        frames.append((np.ascontiguousarray(bgr), np.ascontiguousarray(np.roll(depth, 5 * i, axis=0))))
    qs0 = oracle.quantize_pyramid(frames[0][0], frames[0][1], 2)
    bank = synth.make_bank("obj", 21, 2, 2, w0, h0, seed=3, qs=qs0, planted_frac=0.4, bbox=96)
    thr = 60.0
    exp0, n0 = oracle.match_images(frames[0][0], frames[0][1], T, [bank], thr)
    assert n0 > 0
    det = _detector(ctx, T, 2, bank, w0, h0, max_batch=9)
    try:
        with options(ctx, {"refine_lds": 1}):
            single = [det.match(b, d, thr) for b, d in frames]
        assert _ran(det, 0) == 1
        assert single[0][1] == n0
        _assert_matches_equal(single[0][0], exp0)
        assert len({s[0].tobytes() for s in single}) > 1 and sum(s[1] > 0 for s in single) > 1
        for nbytes in (0, _window_max(det, 0)):
            with options(ctx, {"refine_lds": 2, "refine_lds_bytes": nbytes}):
                both = det.match_batch([f[0] for f in frames], [f[1] for f in frames], thr)
            assert _ran(det, 0) == 2
            for (got, n_got), (exp, n_exp) in zip(both, single):
                assert n_got == n_exp, nbytes
                _assert_matches_equal(got, exp, nbytes)
    finally:
        det.close()


def test_lazy_fine_levels_of_recognition(ctx, oracle):
    """The recognition entry point computes the fine level only in the tiles the candidates can touch, the rest of the workspace
    poisoned (tests/conftest.py).  Cluttered frames with three instances each: the staged windows hold poisoned bytes, which no
    feature may read."""
    sc = clutter.build(oracle)
    bgrs = [sc["frames"][f][0] for f in clutter.FRAMES]
    depths = [sc["frames"][f][1] for f in clutter.FRAMES]
    p = (75.0, 10, 0.5, 0.01)
    exp = [oracle.recognition(b, d, sc["K"], clutter.T, sc["bank"], *p) for b, d in zip(bgrs, depths)]
    assert sum(e["found"] for e in exp) >= 2 and all(e["n_matches"] > 0 for e in exp[:3])
    det = _detector(ctx, clutter.T, 2, sc["bank"], clutter.W, clutter.H, max_batch=len(clutter.FRAMES))
    try:
        assert ctx.get_option("dev_poison") == 1
        for mode, nbytes in ((1, 0), (2, 0), (2, _window_max(det, 0))):
            with options(ctx, {"refine_lds": mode, "refine_lds_bytes": nbytes}):
                got = det.recognize_batch(bgrs, depths, sc["K"], *p)
            assert _ran(det, 0) == mode, (mode, nbytes)
            for i, (g, e) in enumerate(zip(got, exp)):
                tag = (mode, nbytes, i)
                assert g["status"] == 0 and g["found"] == e["found"] and g["n_matches"] == e["n_matches"], tag
                if e["found"]:
                    assert (g["best"]["x"], g["best"]["y"], g["best"]["template_id"]) == (e["best"]["x"], e["best"]["y"], e["best"]["template_id"]), tag
                    assert np.float32(g["best"]["similarity"]).view(np.uint32) == np.float32(e["best"]["similarity"]).view(np.uint32), tag
                    assert np.array_equal(np.ascontiguousarray(g["pose"], np.float32).view(np.uint32),
                                          np.ascontiguousarray(e["pose"], np.float32).view(np.uint32)), tag
            assert det.frame_counters(0)[0] >= 100
    finally:
        det.close()


def test_option_ranges(ctx):
    for name, bad, good in (("refine_lds", (-1, 3), (0, 1, 2)), ("refine_lds_bytes", (-1, BUDGET + 1), (0, 4096, BUDGET))):
        before = ctx.get_option(name)
        for v in bad:
            with pytest.raises(api.FealessError):
                ctx.set_option(name, v)
            assert ctx.get_option(name) == before
        for v in good:
            ctx.set_option(name, v)
            assert ctx.get_option(name) == v
        ctx.set_option(name, before)
