"""The linear memories (k_build_lm) and the spread images (k_spread) byte for byte against the oracle, at the smallest shapes
on which the fast kernels of fl_linmem.hip can go wrong: every edge of their launch rules, runs that are no multiples of
16 bytes, one grid row, several bands with a short last one, batches whose frames and modalities differ, stale memory, and
the lazy fine level's marked tiles (everything outside them is poisoned under the test suite, tests/conftest.py).

Detector.finalize keeps LINEMOD's own asserts (T divides every level, rows * cols % 16 == 0 at every level), so a batch cannot
have a 40 x 20 level 0 (its level 1 would be 20 x 10) or T = 5 at 64 x 48: the batches below use 80 x 40 with T = {5, 5}
(level 1 is the 40 x 20, T = 5 case) and 64 x 48 with T = {4, 8} (level 1: 32 x 24, T = 8) in their place."""
import numpy as np
import pytest

from fealess_amd import _lib as L
from fealess_amd import api, synth
from fealess_amd.bank import TemplateBank
from util import options

QUANT, SPREAD, LM = 0, 2, 3                  # fl_dev_frame_image kinds
POISON = 0xFF                                # what a lazy batch leaves in the bytes it did not compute (a spread byte may be 0xFF
                                             # too: such a byte passes as either)
THR = 60.0

# fl_launch_build_lm (build_lm_band in fl_linmem.hip), for n_frames * n_mod = 1 as Context.build_linear_memories launches it:
#   generic kernel unless w % 4 == 0, W = w / T >= 4, W % 4 == 0, H = h / T >= 1 and 2 <= T <= 8;
#   HB = the most rows yt whose LDS, max(align16(HB * (w + 16)), 2048) + T * HB * W, stays within 20 KiB (at least 1; generic
#        if one row needs more than 64 KiB);
#   fewer than 1024 workgroups (here always: there are T per band): HB = min(HB, max(H // ceil(1024 / T), ceil(256 / W), 1));
#   HB < H is rounded down to a multiple of step = 16 / gcd(W, 16) where HB >= step.
# Instances: T = 4, 5, 8 compiled in, the others through the run-time form; rows staged in 16-byte pieces iff w % 16 == 0;
# labels stored in 16-byte pieces iff W * H % 16 == 0 (and, with several bands, HB * W % 16 == 0), else in dwords.
# (w, h, T, expected band height HB, 0 = generic kernel)
LM_EDGES = [(150, 80, 5, 0),       # w % 4 != 0                                                  -> generic
            (80, 48, 8, 0),        # W = 10: W % 4 != 0                                          -> generic
            (64, 48, 16, 0),       # T > 8                                                       -> generic
            (64, 48, 2, 8),        # T = 2, the lower bound; run-time T; W = 32: min run 256 B = 8 rows, three bands
            (96, 48, 6, 8),        # T = 6, run-time form, one band
            (112, 56, 7, 8),       # T = 7, run-time form, one band
            (64, 200, 4, 16),      # H = 50 in bands of 16, 16, 16, 2: a short last band; 16-byte pieces everywhere
            (16, 260, 4, 64),      # W = 4 (step 4), H = 65: bands of 64 and 1; W * H = 260: dword stores
            (32736, 8, 8, 1),      # one row needs 65 488 B of LDS: the last width that fits 64 KiB
            (32768, 8, 8, 0)]      # one row needs 65 552 B                                      -> generic although W % 4 == 0
LM_SHAPES = [(32, 16, 8, 2),       # W = 4, H = 2; W * H = 8: dword stores
             (40, 20, 5, 4),       # w % 16 != 0: rows staged as dwords; W * H = 32: 16-byte stores
             (16, 16, 4, 4),       # W * H = 16: one 16-byte piece per grid
             (64, 8, 8, 1),        # H = 1: one grid row
             (96, 40, 8, 5),       # H = 5, W = 12: W * H = 60, dword stores
             (320, 240, 8, 6)]     # the workload's shape, alone: min run 256 B = 7 rows, step 2 -> five bands of 6 rows


def _band(lib, n_frames, n_mod, w, h, T):
    return int(L.dev(lib, "fl_dev_build_lm_band")(n_frames, n_mod, w, h, T))


def test_band_rule_for_batches():
    """The launch rule is host code: what it decides for the workload's batches, and where the LDS bound cuts a band."""
    lib = L.load()
    assert _band(lib, 4096, 2, 320, 240, 8) == 30               # whole grid rows: 9600 contiguous bytes per label and workgroup
    assert _band(lib, 64, 2, 320, 240, 8) == 30                 # 1024 workgroups: still whole
    assert _band(lib, 8, 2, 320, 240, 8) == 6                   # 128 per band: 8 bands wanted, H // 8 = 3 < the 7 rows of a 256-byte run
    assert _band(lib, 1, 2, 320, 240, 8) == 6
    assert _band(lib, 64, 2, 320, 248, 8) == 31                 # H = 31: 31 * 656 = 20 336 <= 20 480: still one band
    assert _band(lib, 64, 2, 320, 256, 8) == 30                 # H = 32: 32 * 656 = 20 992 > 20 480: bands of 30 and 2
    assert _band(lib, 64, 2, 640, 480, 8) == 15                 # 1296 B per row: 15 rows; W = 80, step 1
    for w, h, T, hb in LM_EDGES + LM_SHAPES:
        assert _band(lib, 1, 1, w, h, T) == hb, (w, h, T)


@pytest.mark.gpu
@pytest.mark.parametrize("density", [0.05, 0.9])
@pytest.mark.parametrize("w,h,T,hb", LM_EDGES + LM_SHAPES)
def test_linear_memories_equal_oracle(ctx, oracle, w, h, T, hb, density):
    """The whole (8, fl_lm_label_stride) array, pads included."""
    assert _band(ctx.lib, 1, 1, w, h, T) == hb
    q = synth.random_quantized(np.random.default_rng(w * 31 + h * 7 + T), w, h, density)
    got = ctx.build_linear_memories(q, T)
    exp = oracle.build_linear_memories(q, T)
    assert got.shape == exp.shape
    assert np.array_equal(got, exp), int((got != exp).sum())
    W, H = w // T, h // T
    assert not got[:, T * T * W * H:].any()                      # the pads


# ---- batches ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c():
    """A context of its own: the options these tests set cannot leak into other tests."""
    ctx = api.Context(0)
    yield ctx
    ctx.close()


def _frame(w, h, rng):
    """A (bgr, depth) frame with gradients and normals all over it: colour gratings and a tilted, rippled depth surface."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    bgr = np.zeros((h, w, 3))
    for ch in range(3):
        for _ in range(3):
            a, f, p = rng.uniform(0, np.pi), rng.uniform(0.15, 0.6), rng.uniform(0, 6)
            bgr[..., ch] += rng.uniform(20, 45) * np.sin(f * (np.cos(a) * xx + np.sin(a) * yy) + p)
    bgr = np.clip(128 + bgr + rng.integers(-3, 4, bgr.shape), 0, 255).astype(np.uint8)
    d = (800 + rng.uniform(-3, 3) * xx + rng.uniform(-3, 3) * yy +
         rng.uniform(15, 30) * np.sin(xx / rng.uniform(4, 9) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(4, 9)))
    return bgr, (d + rng.integers(0, 3, d.shape)).astype(np.uint16)


def _random_bank(levels, w, h, seed, n=6):
    rng = np.random.default_rng(seed)
    bank = TemplateBank("obj", levels, 2)
    bbox = max(8, min(160, (min(w, h) // 2) >> levels << levels))
    for _ in range(n):
        bank.add_pyramid(synth.random_pyramid(rng, levels, 2, w, h, bbox=bbox), None, None)
    return bank


def _detector(c, w, h, T, bank, max_batch, eager):
    det = api.Detector(c, 2, T)
    det.add_class(bank)
    with options(c, {"eager_frontend": int(eager)}):             # sampled by fl_detector_finalize
        det.finalize(w, h, max_batch=max_batch)
    return det


def _assert_batch(det, oracle, n, T, tag):
    """Every frame's and modality's spread images and linear memories against the oracle's of the quantised images in the
    same workspace, pads zero; no two (frame, modality) planes alike, so a neighbour's stream cannot pass."""
    Lv = len(T)
    seen = []
    for f in range(n):
        for m in range(2):
            for l in range(Lv - 1):
                q = det.dev_frame_image(f, QUANT, l, m)
                got, exp = det.dev_frame_image(f, SPREAD, l, m), oracle.spread(q, T[l])
                assert np.array_equal(got, exp), (tag, "spread", f, l, m, int((got != exp).sum()))
            q = det.dev_frame_image(f, QUANT, Lv - 1, m)
            assert q.any() and not any(np.array_equal(q, s) for s in seen), (tag, f, m)
            seen.append(q)
            got, exp = det.dev_frame_image(f, LM, Lv - 1, m), oracle.build_linear_memories(q, T[-1])
            assert got.shape == exp.shape
            assert np.array_equal(got, exp), (tag, "lm", f, m, int((got != exp).sum()))
            h, w = q.shape
            assert not got[:, w * h:].any(), (tag, "pad", f, m)


# (w, h, T per level): what the level-0 spread and the level-1 linear memories run as
BATCH_GEOMS = [(64, 48, [4, 8]),      # spread T = 4 in 16-byte pieces; linear memories of 32 x 24, T = 8: W = 4, H = 3, dword stores
               (80, 40, [5, 5]),      # spread T = 5; linear memories of 40 x 20, T = 5: rows staged as dwords
               (72, 48, [4, 4]),      # w % 16 != 0: the spread's 4-byte form on whole images; 36 x 24, T = 4: W = 9 -> generic build
               (1280, 40, [5, 5]),    # the widest row of the workload's configurations: strips of 3 * T rows; 640 x 20: H = 4
               (150, 160, [5, 5])]    # w % 4 != 0: both generic kernels, frames and modalities in blockIdx.z


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,T", BATCH_GEOMS, ids=["%dx%d" % g[:2] for g in BATCH_GEOMS])
def test_batch_spreads_and_linear_memories(c, oracle, w, h, T):
    """match_batch of 3 frames x 2 modalities, eager.  The batch is checked twice: fresh, and again after the same workspaces
    held other content -- the frames in another order, then (frame 0) a pyramid whose quantised images are all 0xFF, whose
    linear memories are 4 everywhere outside the pads: a stale byte in a pad or in a neighbour's stream shows."""
    rng = np.random.default_rng(w * 13 + h)
    frames = [_frame(w, h, rng) for _ in range(3)]
    bs, ds = [f[0] for f in frames], [f[1] for f in frames]
    det = _detector(c, w, h, T, _random_bank(len(T), w, h, seed=w + h), 3, eager=True)
    try:
        det.match_batch(bs, ds, THR)
        _assert_batch(det, oracle, 3, T, "fresh")
        det.match_batch(bs[::-1], ds[::-1], THR)
        det.match_quantized([np.full((h >> l, w >> l), 0xFF, np.uint8) for l in range(len(T)) for _ in range(2)], 101.0)
        lm = det.dev_frame_image(0, LM, len(T) - 1, 1)
        assert (lm[:, :(w >> 1) * (h >> 1)] == 4).all() and not lm[:, (w >> 1) * (h >> 1):].any()
        det.match_batch(bs, ds, THR)
        _assert_batch(det, oracle, 3, T, "after other content")
    finally:
        det.close()


@pytest.mark.gpu
def test_batch_bands_cut_by_the_lds_bound(c, oracle):
    """64 frames x 2 modalities x T = 8 are 1024 workgroups per band, so the bands are as high as the LDS bound allows: at
    320 x 256 (one level) 30 rows and a last band of 2, stored in 16-byte pieces at offsets that are no multiples of a line."""
    w, h, T, n = 320, 256, [8], 64
    assert _band(c.lib, n, 2, w, h, 8) == 30
    rng = np.random.default_rng(5)
    base = [_frame(w, h, rng) for _ in range(4)]
    frames = [(np.roll(base[i % 4][0], 3 * i, axis=1), np.roll(base[i % 4][1], 3 * i, axis=1)) for i in range(n)]
    det = _detector(c, w, h, T, _random_bank(1, w, h, seed=9), n, eager=True)
    try:
        det.match_batch([f[0] for f in frames], [f[1] for f in frames], THR)
        _assert_batch(det, oracle, n, T, "64 frames")
    finally:
        det.close()


# ---- the lazy fine level -------------------------------------------------------------------------------------------------------
LAZY_W, LAZY_H, LAZY_T = 320, 240, [5, 8]
# object poses (tx, ty, tz, yaw, tilt, roll) under synth's intrinsics, of which a 320 x 240 frame is the upper left quarter
LAZY_POSES = {0: (-168.0, -178.0, 760.0, 0.3, 0.35, 0.1),      # right-most feature + 7 * T in [300, 320): the clipped tile column
              2: (-126.0, -95.0, 480.0, -0.2, 0.3, 0.0)}        # a template wider than w - 16 * T: its patches leave the image


def lazy_scene(oracle):
    """Frame 0: the object so that its candidate's patches end in the last, 20 pixel wide tile column.  Frame 1: nothing.
    Frame 2: the object so close that its template is wider than w - 16 * T: the reference's clamp of the refined position to
    [8 * T, w - width - 8 * T] then puts patches outside the image, which marks the whole frame.  The bank: the oracle's
    template of frames 0 and 2 (each matches its frame with 100 %), and random pyramids.  Also, per frame with the object,
    (x reach, y reach, template width, template height) at level 0."""
    frames, masks = [], []
    for i in range(3):
        if i == 1:
            frames.append((np.full((LAZY_H, LAZY_W, 3), 90, np.uint8), np.full((LAZY_H, LAZY_W), 1200, np.uint16)))
            masks.append(None)
            continue
        R, t = synth.object_pose(*LAZY_POSES[i])
        d, b, mk = synth.render(LAZY_W, LAZY_H, R, t, seed=40 + i)
        frames.append((np.ascontiguousarray(b, np.uint8), np.ascontiguousarray(d, np.uint16)))
        masks.append(mk)
    bank = TemplateBank("obj", 2, 2)
    reach = {}
    for i in (0, 2):
        t, feats, _ = oracle.add_template(frames[i][0], frames[i][1], (masks[i] * 255).astype(np.uint8), 2)
        bank.add_pyramid([dict(width=int(hd["width"]), height=int(hd["height"]), offset_x=int(hd["offset_x"]),
                               offset_y=int(hd["offset_y"]), pyramid_level=int(hd["pyramid_level"]),
                               features=np.stack([f["x"], f["y"], f["label"]], 1).astype(np.int32)) for hd, f in zip(t, feats)],
                         None, None)
        # level 0 (templates 0 and 1): the refinement's 16 x 16 patch of steps of T starts 8 * T before a feature and ends 7 * T after it
        reach[i] = (max(int(f["x"].max()) + int(hd["offset_x"]) for hd, f in zip(t[:2], feats[:2])) + 7 * LAZY_T[0],
                    max(int(f["y"].max()) + int(hd["offset_y"]) for hd, f in zip(t[:2], feats[:2])) + 7 * LAZY_T[0],
                    max(int(hd["width"]) for hd in t[:2]), max(int(hd["height"]) for hd in t[:2]))
    rng = np.random.default_rng(3)
    for _ in range(4):
        bank.add_pyramid(synth.random_pyramid(rng, 2, 2, LAZY_W, LAZY_H, bbox=56), None, None)
    return frames, bank, reach


def test_lazy_scene_is_what_the_gpu_test_needs(oracle):
    """No GPU: frame 0's patches reach into the clipped tile column and stay inside the image, its template leaves the clamp
    room; frame 2's template does not."""
    _, _, reach = lazy_scene(oracle)
    room_w, room_h = LAZY_W - 16 * LAZY_T[0], LAZY_H - 16 * LAZY_T[0]
    assert 300 <= reach[0][0] < LAZY_W and reach[0][1] < LAZY_H and reach[0][2] <= room_w and reach[0][3] <= room_h, reach
    assert reach[2][2] > room_w, reach


@pytest.mark.gpu
def test_lazy_tiles_spread_equals_oracle_and_poison_stays(c, oracle):
    """A lazy batch: inside the marked tiles the level-0 spread bytes are the oracle's, outside them the poison is intact; the
    matches equal those of an eager detector.  At this threshold the oracle finds one match in frame 0 and one in frame 2."""
    assert c.get_option("dev_poison") == 1
    frames, bank, _ = lazy_scene(oracle)
    bs, ds = [f[0] for f in frames], [f[1] for f in frames]
    thr = 80.0
    got = {}
    for eager in (False, True):
        det = _detector(c, LAZY_W, LAZY_H, LAZY_T, bank, 3, eager=eager)
        try:
            got[eager] = det.match_batch(bs, ds, thr)
            if eager:
                continue
            for i, (b, d) in enumerate(frames):
                cnt = det.frame_counters(i)
                q = oracle.quantize_pyramid(b, d, 2)
                for m in range(2):
                    sp, exp = det.dev_frame_image(i, SPREAD, 0, m), oracle.spread(q[m], LAZY_T[0])
                    done = sp != POISON
                    assert np.all(~done | (sp == exp)), (i, m, int((done & (sp != exp)).sum()))
                    ty, tx = -(-LAZY_H // 60), -(-LAZY_W // 60)
                    pad = np.zeros((ty * 60, tx * 60), bool)
                    pad[:LAZY_H, :LAZY_W] = done
                    tiles = int(pad.reshape(ty, 60, tx, 60).any(axis=(1, 3)).sum())
                    assert tiles <= cnt[3], (i, m, tiles, cnt)
                    if i == 0:                                   # some tiles, the clipped column among them, not the frame
                        assert cnt[0] > 0 and 0 < cnt[3] < ty * tx, cnt
                        assert done[:, 300:].any() and not done.all(), (m, cnt)
                        rows = np.flatnonzero(done[:, 300:].any(axis=1))
                        assert np.array_equal(sp[rows[0]:rows[-1] + 1, 300:], exp[rows[0]:rows[-1] + 1, 300:]), m
                    elif i == 1:                                 # every strip returned
                        assert cnt[0] == 0 and not done.any(), cnt
                    else:                                        # the whole frame
                        assert cnt[3] == ty * tx, cnt
                        assert np.array_equal(sp, exp), (m, int((sp != exp).sum()))
        finally:
            det.close()
    for i in range(3):
        (ml, nl), (me, ne) = got[False][i], got[True][i]
        assert nl == ne and np.array_equal(ml, me), i
    assert got[True][0][1] > 0 and got[True][1][1] == 0 and got[True][2][1] > 0
