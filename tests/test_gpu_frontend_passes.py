"""GPU parity of the front-end passes that share launches: the pyrDown pair kernel that makes its own border pairs, the
depth quantiser that writes level 1's normals beside level 0's, and the chunk height of the whole-image quantiser launches
(option frontend_chunk_rows).  Every image is compared byte for byte with the oracle's, in batches of 3 frames whose contents
differ, so that reading a neighbour's frame cannot pass.

Two routes read the images back.  Detector.dev_frame_image reads a detector's workspaces, but LINEMOD's own asserts (T divides
every level, rows * cols % 16 == 0 at every level) keep a detector from being finalized at most of the small sizes that put
the kernels' edges close together (20x18, 136x132, 260x70, 72x190, ...).  Context.dev_front_images queues the very launches
of an eager batch's front-end (launch_front_images, shared with fl_launch_frontend) on frames of any size.  The lazy (tiled)
colour launches exist only inside a detector: they run at 144x132 and 160x190, which keep what 136x132 and 72x190 are
for (the last 60-row boundary 12 rows above the bottom; a height that is no multiple of 60) and can be finalized."""
import ctypes as C

import numpy as np
import pytest

import util
from fealess_amd import api, synth
from fealess_amd import _lib as L
from fealess_amd.bank import TemplateBank
from util import options

pytestmark = pytest.mark.gpu

QUANT, BGR = 0, 1                            # fl_dev_frame_image kinds
POISON = 0xFF                                # what a lazy batch leaves in the pixels it did not compute (never a quantised byte)
THR = 60.0
HOLES, BAND = 1, 2


@pytest.fixture(scope="module")
def c():
    """A context of its own: the options these tests set cannot leak into other tests."""
    ctx = api.Context(0)
    yield ctx
    ctx.close()


def _frame(w, h, rng, kind):
    """A (bgr, depth) frame with gradients and normals all over it: colour gratings, a tilted and rippled depth surface
    (neighbours 5 pixels apart differ by less than difference_threshold = 50), both with a little noise.  HOLES: sensor
    holes (depth 0); BAND: a band of rows beyond distance_threshold = 2000."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    bgr = np.zeros((h, w, 3))
    for ch in range(3):
        for _ in range(3):
            a, f, p = rng.uniform(0, np.pi), rng.uniform(0.15, 0.6), rng.uniform(0, 6)
            bgr[..., ch] += rng.uniform(20, 45) * np.sin(f * (np.cos(a) * xx + np.sin(a) * yy) + p)
    bgr = np.clip(128 + bgr + rng.integers(-3, 4, bgr.shape), 0, 255).astype(np.uint8)
    d = (800 + rng.uniform(-3, 3) * xx + rng.uniform(-3, 3) * yy +
         rng.uniform(15, 30) * np.sin(xx / rng.uniform(4, 9) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(4, 9)))
    d = (d + rng.integers(0, 3, d.shape)).astype(np.uint16)
    if kind == HOLES:
        for _ in range(6):
            y, x = int(rng.integers(0, h - 3)), int(rng.integers(0, w - 3))
            d[y:y + int(rng.integers(2, 12)), x:x + int(rng.integers(2, 12))] = 0
    elif kind == BAND:
        y0 = int(rng.integers(0, h // 2))
        n = len(d[y0:y0 + h // 3])
        d[y0:y0 + h // 3] = (2001 + rng.integers(0, 1500, (n, w))).astype(np.uint16)
    return np.ascontiguousarray(bgr), np.ascontiguousarray(d)


def _frames(w, h, seed):
    rng = np.random.default_rng(seed)
    return [_frame(w, h, rng, kind) for kind in (0, HOLES, BAND)]


def _expected(oracle, bgr, depth, levels):
    """The oracle's images of one frame: q[2 l + m] and the colour image per level."""
    q = oracle.quantize_pyramid(bgr, depth, levels)
    bgrs = [bgr]
    for _ in range(1, levels):
        bgrs.append(oracle.pyrdown_bgr(bgrs[-1]))
    return dict(q=q, bgr=bgrs)


_SCENES = {}


def _scene(oracle, w, h, levels):
    """Frames and oracle images of a size, computed once and shared (never modified)."""
    key = (w, h, levels)
    if key not in _SCENES:
        frames = _frames(w, h, seed=1000 * w + h)
        exps = [_expected(oracle, b, d, levels) for b, d in frames]
        for i in range(3):
            for j in range(i):
                assert not np.array_equal(exps[i]["q"][0], exps[j]["q"][0]), (i, j)      # no two frames share an image
                assert not np.array_equal(exps[i]["bgr"][-1], exps[j]["bgr"][-1]), (i, j)
                assert h < 32 or not np.array_equal(exps[i]["q"][1], exps[j]["q"][1]), (i, j)   # (tiny: no normals at all)
        _SCENES[key] = (frames, exps)
    return _SCENES[key]


def _diff(got, exp):
    return int((got != exp).sum())


def _assert_front_images(c, frames, exps, levels, tag):
    """The eager front-end launches on the batch (any size) against the oracle, every frame, every level, every image."""
    got = c.dev_front_images([f[0] for f in frames], [f[1] for f in frames], levels)
    for i, e in enumerate(exps):
        for l in range(levels):
            for m in range(2):
                g = got[i][l]["q%d" % m]
                assert np.array_equal(g, e["q"][2 * l + m]), (tag, "quant", i, l, m, _diff(g, e["q"][2 * l + m]))
            if l:
                assert np.array_equal(got[i][l]["bgr"], e["bgr"][l]), (tag, "bgr", i, l, _diff(got[i][l]["bgr"], e["bgr"][l]))


def _assert_detector_frame(det, i, exp, tag, lazy=False):
    """Frame i's QUANT and BGR workspace images, every level, against the oracle's.  lazy: a fine level's colour quantisation
    exists only in the marked tiles; every other byte holds POISON."""
    for l in range(det.L):
        for m in range(2):
            got, e = det.dev_frame_image(i, QUANT, l, m), exp["q"][2 * l + m]
            if lazy and m == 0 and l < det.L - 1:
                assert np.all((got == POISON) | (got == e)), (tag, i, l, m, int(((got != POISON) & (got != e)).sum()))
            else:
                assert np.array_equal(got, e), (tag, i, l, m, _diff(got, e))
        if l > 0:
            got = det.dev_frame_image(i, BGR, l)
            assert np.array_equal(got, exp["bgr"][l]), (tag, "bgr", i, l, _diff(got, exp["bgr"][l]))


def _trained_bank(oracle, frames, levels):
    """A template per frame, trained by the oracle on a window of that frame: every frame has candidates of its own, so a
    lazy batch marks tiles in every frame."""
    h, w = frames[0][1].shape
    bank = TemplateBank("obj", levels, 2)
    n = 0
    for b, d in frames:
        mask = np.zeros((h, w), np.uint8)
        mask[h // 4:h // 4 + h // 2, w // 4:w // 4 + w // 2] = 255
        ex = oracle.add_template(b, d, mask, levels)
        if ex is None:
            continue
        t, feats, _ = ex
        bank.add_pyramid([dict(width=int(hd["width"]), height=int(hd["height"]), offset_x=int(hd["offset_x"]),
                               offset_y=int(hd["offset_y"]), pyramid_level=int(hd["pyramid_level"]),
                               features=np.stack([f["x"], f["y"], f["label"]], 1).astype(np.int32)) for hd, f in zip(t, feats)],
                         None, None)
        n += 1
    assert n >= 2, n                                             # not vacuous
    return bank


def _planted_bank(exps, levels, w, h, bbox, nf0):
    """For sizes too small to train on: a template per frame whose features are read off that frame's own quantised pyramid."""
    rng = np.random.default_rng(w + h)
    bank = TemplateBank("obj", levels, 2)
    for e in exps:
        tl = synth.planted_pyramid(rng, e["q"], levels, 2, w, h, bbox=bbox, nf0=nf0)
        assert tl is not None
        bank.add_pyramid(tl, None, None)
    return bank


def _detector(c, w, h, T, bank, eager):
    det = api.Detector(c, 2, T)
    det.add_class(bank)
    with options(c, {"eager_frontend": int(eager)}):             # sampled by fl_detector_finalize
        det.finalize(w, h, max_batch=3)
    return det


# ---- pyrDown: the pair kernel makes the border pairs of every row itself ------------------------------------------------------
# 16x12: dw = 8, the smallest the pair kernel takes (two border pairs, two interior ones); 20x18: three interior pairs (dw =
# 10) and dh = 9; 136x132: dh = 66 is no multiple of PD_ROWS = 8 (nor of the 32 rows of a block); 260x70: 65 pairs, i.e. two
# waves per row, and dh = 35.  Reflection at all four edges in each.  18x14 (dw odd) and 14x10 (dw < 8) take the general kernel.
@pytest.mark.parametrize("w,h", [(16, 12), (20, 18), (136, 132), (260, 70), (18, 14), (14, 10)])
def test_pyrdown_border_pairs(c, oracle, w, h):
    frames, exps = _scene(oracle, w, h, 2)
    assert all(e["bgr"][1].std() > 5 for e in exps)
    _assert_front_images(c, frames, exps, 2, ("pyrdown", w, h))
    for (b, _), e in zip(frames, exps):                          # the single-image entry point takes the same launch
        got = c.pyrdown_bgr(b)
        assert np.array_equal(got, e["bgr"][1]), (w, h, _diff(got, e["bgr"][1]))


def test_pyrdown_border_pairs_in_a_detector(c, oracle):
    """16x12, the one border size a detector can be finalized for, read back from the workspaces."""
    frames, exps = _scene(oracle, 16, 12, 2)
    bank = TemplateBank("obj", 2, 2)
    bank.add_pyramid(synth.random_pyramid(np.random.default_rng(3), 2, 2, 16, 12, bbox=4, nf0=8), None, None)
    det = _detector(c, 16, 12, [2, 2], bank, eager=True)
    try:
        det.match_batch([f[0] for f in frames], [f[1] for f in frames], THR)
        for i, e in enumerate(exps):
            _assert_detector_frame(det, i, e, "16x12")
    finally:
        det.close()


# ---- level 1's normals come out of the depth quantiser ------------------------------------------------------------------------
# 136x132 and 72x64: even sizes, w % 8 == 0: level 1 from the quantiser, level 2 (3 levels) from the resize kernel reading
# level 1.  134x131: not the fast rule, every level from the resize kernels as before.
@pytest.mark.parametrize("levels", [2, 3])
@pytest.mark.parametrize("w,h", [(136, 132), (72, 64), (134, 131)])
def test_fused_level1_normals(c, oracle, w, h, levels):
    frames, exps = _scene(oracle, w, h, levels)
    for e in exps:                                               # normals of several labels at every level: not vacuous
        for l in range(levels):
            assert len(np.unique(e["q"][2 * l + 1])) >= 4, (w, h, l)
    assert (frames[1][1] == 0).any() and (frames[2][1] > 2000).any()      # the holes and the band are there
    _assert_front_images(c, frames, exps, levels, ("fused", w, h, levels))


@pytest.mark.parametrize("T", [[4, 2], [4, 2, 2]], ids=["2levels", "3levels"])
def test_fused_level1_normals_in_a_detector(c, oracle, T):
    """72x64 in a detector's workspaces (136x132 and 134x131 cannot be finalized), eager and through the lazy entry."""
    frames, exps = _scene(oracle, 72, 64, len(T))
    bank = _planted_bank(exps, len(T), 72, 64, bbox=24, nf0=16)
    for eager in (True, False):
        det = _detector(c, 72, 64, T, bank, eager)
        try:
            det.match_batch([f[0] for f in frames], [f[1] for f in frames], THR)
            for i, e in enumerate(exps):
                _assert_detector_frame(det, i, e, ("72x64", len(T), eager), lazy=not eager)
        finally:
            det.close()


# ---- chunk height of the whole-image launches ---------------------------------------------------------------------------------
CHUNKS = (60, 120, 240, 0)


@pytest.mark.parametrize("w,h", [(136, 132), (72, 190)])
def test_chunk_rows_eager_launches(c, oracle, w, h):
    """132 rows: the last 60-row boundary is 12 rows above the bottom; 190 is no multiple of 60.  Every height gives the
    oracle's images, so they equal each other."""
    frames, exps = _scene(oracle, w, h, 1)
    for rows in CHUNKS:
        with options(c, {"frontend_chunk_rows": rows}):
            _assert_front_images(c, frames, exps, 1, ("chunk", w, h, rows))


@pytest.mark.parametrize("w,h,T", [(144, 132, [4, 2]), (160, 190, [5, 5])], ids=["144x132", "160x190"])
def test_chunk_rows_eager_and_lazy_detector(c, oracle, w, h, T):
    """The same batch at every chunk height, eager and lazy, with a trained template per frame so that the lazy batches mark
    tiles: the tiled colour launch keeps its 60-row chunks whatever the option holds."""
    frames, exps = _scene(oracle, w, h, 2)
    bank = _trained_bank(oracle, frames, 2)
    assert c.get_option("dev_poison") == 1
    for eager in (True, False):
        det = _detector(c, w, h, T, bank, eager)
        try:
            for rows in CHUNKS:
                with options(c, {"frontend_chunk_rows": rows}):
                    det.match_batch([f[0] for f in frames], [f[1] for f in frames], THR)
                    computed = 0
                    for i, e in enumerate(exps):
                        _assert_detector_frame(det, i, e, (w, h, rows, eager), lazy=not eager)
                        computed += int((det.dev_frame_image(i, QUANT, 0, 0) != POISON).any())
                    assert computed >= 2, (w, h, rows, eager, computed)          # the lazy batches did compute tiles
        finally:
            det.close()


def test_chunk_rows_must_be_a_multiple_of_60(c):
    before = c.get_option("frontend_chunk_rows")
    for bad in (61, 30, 100, -60, 60 * 1024 + 60):
        with pytest.raises(api.FealessError) as e:
            c.set_option("frontend_chunk_rows", bad)
        assert e.value.code == L.FL_ERR_INVALID and c.get_option("frontend_chunk_rows") == before, bad
    for good in (0, 60, 120, 240, 480):
        c.set_option("frontend_chunk_rows", good)
        assert c.get_option("frontend_chunk_rows") == good
    c.set_option("frontend_chunk_rows", before)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_recognition_bytes_do_not_depend_on_the_chunk_height(c):
    """The VGA recognition golden with the option at 60, at auto and at 240 and 480 (a batch of one stays at 60 under auto, so
    the taller chunks are forced too): the fl_recognition_result bytes are identical, and they are the golden's."""
    g = util.golden("recognition_vga.npz")
    bank = util.bank_from_arrays(g["templates"], g["features"], g["poses"], 2, 2, model_depths=g["model_depths"])
    det = api.Detector(c, 2, [5, 8])
    det.add_class(bank)
    det.finalize(640, 480, max_batch=1)
    try:
        b, d = np.ascontiguousarray(g["bgr"], np.uint8), np.ascontiguousarray(g["depth"], np.uint16)
        bp, dp = (C.c_void_p * 1)(b.ctypes.data), (C.c_void_p * 1)(d.ctypes.data)
        k = L.Intrinsics(640, 480, *(float(v) for v in g["K"]))
        p = det._params(75.0, 10, 0.5, 0.01, L.FL_ICP_PARITY)
        raw = {}
        for rows in (60, 0, 240, 480):
            with options(c, {"frontend_chunk_rows": rows}):
                res = (L.RecognitionResult * 1)()
                c.check(det.lib.fl_recognize_batch(det.h, 1, bp, dp, L.FL_MEM_HOST, C.byref(k), C.byref(p), res))
                raw[rows] = bytes(memoryview(res).cast("B"))
                r = api.recognition_result_to_dict(res[0])
                assert r["found"] == 1 and np.array_equal(r["pose"], g["pose"]), rows
        assert raw[0] == raw[60] and raw[240] == raw[60] and raw[480] == raw[60]
    finally:
        det.close()
