"""GPU parity of the batched front-end, frame by frame: every frame of a batch, read back from its workspace
(Detector.dev_frame_image), equals the oracle's quantised pyramid, pyrDown images, spreads and coarsest linear memories,
whatever route the frames took in (host array, host frames, device frames read in place or gathered), at odd pitches,
past 2^31 and 2^32 bytes of input and of workspace, at geometries that take the general kernels, in lazy batches and
after the device zoom.  Every frame of a batch has content of its own, so that reading a neighbour's frame cannot pass."""
import numpy as np
import pytest
import torch

from fealess_amd import api, synth
from fealess_amd import _lib as L
from fealess_amd.bank import TemplateBank
from util import options

pytestmark = pytest.mark.gpu

QUANT, BGR, SPREAD, LM = 0, 1, 2, 3          # fl_dev_frame_image kinds
POISON = 0xFF                                # what a lazy batch leaves in the pixels it did not compute (never a quantised byte)
THR = 60.0


def _K(w, h):
    s = w / 640.0
    return (synth.FX * s, synth.FY * s, w / 2.0, h / 2.0)


def _pose(rng, s):
    return synth.object_pose(tx=float(rng.uniform(-90, 90)) * s, ty=float(rng.uniform(-50, 50)) * s, tz=float(rng.uniform(600, 760)),
                             yaw=float(rng.uniform(-0.8, 0.8)), tilt=float(rng.uniform(0.1, 0.6)), roll=float(rng.uniform(-0.3, 0.3)))


def _frames(w, h, n, seed):
    """n (bgr, depth) frames of w x h, each one different: the object at a pose of its own, a rolled copy of the previous frame
    with noise of its own, sensor holes, depth beyond distance_threshold (2000), random noise, two objects in front of the
    textured clutter background -- in turn.  Also the object masks (rectangles for the noise frames)."""
    rng = np.random.default_rng(seed)
    K = _K(w, h)
    kw = dict(fx=K[0], fy=K[1], cx=K[2], cy=K[3])
    out, masks = [], []
    for i in range(n):
        kind = i % 6
        if kind == 1 and out:
            (b, d), mk = out[-1], masks[-1]
            dy, dx = int(rng.integers(3, h // 3)), int(rng.integers(5, w // 3))
            b = np.clip(np.roll(b, (dy, dx), axis=(0, 1)).astype(np.int16) + rng.integers(-3, 4, b.shape), 0, 255).astype(np.uint8)
            d = np.roll(d, (dy, dx), axis=(0, 1)) + rng.integers(0, 3, d.shape).astype(np.uint16)
            mk = np.roll(mk, (dy, dx), axis=(0, 1))
        elif kind == 4:
            b = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            d = (650 + rng.integers(0, 90, (h, w))).astype(np.uint16)
            mk = np.zeros((h, w), bool)
            mk[h // 3:h // 2, w // 3:w // 2] = True
        elif kind == 5:
            d, b, ms = synth.render_clutter(w, h, [_pose(rng, w / 640.0), _pose(rng, w / 640.0)], seed=seed * 10 + i, **kw)
            mk = ms[0]
        else:
            R, t = _pose(rng, w / 640.0)
            d, b, mk = synth.render(w, h, R, t, seed=seed * 10 + i, **kw)
            if kind == 2:                                        # sensor holes
                for _ in range(12):
                    y, x = int(rng.integers(0, h - 4)), int(rng.integers(0, w - 4))
                    d[y:y + int(rng.integers(2, 30)), x:x + int(rng.integers(2, 30))] = 0
            elif kind == 3:                                      # a band beyond distance_threshold
                y0 = int(rng.integers(0, h // 2))
                d[y0:y0 + h // 3] = (2001 + rng.integers(0, 1500, (len(d[y0:y0 + h // 3]), w))).astype(np.uint16)
        out.append((np.ascontiguousarray(b, np.uint8), np.ascontiguousarray(d, np.uint16)))
        masks.append(mk)
    return out, masks


def _bank(oracle, frames, masks, levels, seed, n_random=16):
    """Templates trained by the oracle on a window of every frame (so that every frame has candidates of its own, and the lazy
    batches compute fine-level tiles in every frame), padded with random pyramids.  No depth renders: match only."""
    rng = np.random.default_rng(seed)
    h, w = frames[0][1].shape
    bank = TemplateBank("obj", levels, 2)
    for (b, d), mk in zip(frames, masks):
        ex = oracle.add_template(b, d, (mk * 255).astype(np.uint8), levels)
        if ex is not None:
            t, feats, _ = ex
            bank.add_pyramid([dict(width=int(hd["width"]), height=int(hd["height"]), offset_x=int(hd["offset_x"]),
                                   offset_y=int(hd["offset_y"]), pyramid_level=int(hd["pyramid_level"]),
                                   features=np.stack([f["x"], f["y"], f["label"]], 1).astype(np.int32)) for hd, f in zip(t, feats)],
                             None, None)
    bbox = min(160, (min(w, h) // 2) >> levels << levels)
    for _ in range(n_random):
        bank.add_pyramid(synth.random_pyramid(rng, levels, 2, w, h, bbox=bbox), None, None)
    return bank


def _expected(oracle, bgr, depth, T):
    """The oracle's images of one frame."""
    Lv = len(T)
    q = oracle.quantize_pyramid(bgr, depth, Lv)
    bgrs = [bgr]
    for _ in range(1, Lv):
        bgrs.append(oracle.pyrdown_bgr(bgrs[-1]))
    spread = {(l, m): oracle.spread(q[2 * l + m], T[l]) for l in range(Lv - 1) for m in range(2)}
    lm = [oracle.build_linear_memories(q[2 * (Lv - 1) + m], T[-1]) for m in range(2)]
    return dict(q=q, bgr=bgrs, spread=spread, lm=lm)


def _distinct(exps):
    """No two frames have the same level-0 images (so a frame read from a neighbour's memory cannot pass)."""
    for i in range(len(exps)):
        for j in range(i):
            for m in range(2):
                assert not np.array_equal(exps[i]["q"][m], exps[j]["q"][m]), (i, j, m)


def _diff(got, exp):
    return int((got != exp).sum())


def _assert_frame(det, i, exp, tag, lazy=False):
    """Frame i's workspace images against the oracle's.  lazy: the finer levels' colour quantisation and spreads exist only
    where the candidates look, every other byte holds POISON; those images must be POISON or the oracle's value there."""
    Lv = det.L
    for l in range(Lv):
        for m in range(2):
            got, e = det.dev_frame_image(i, QUANT, l, m), exp["q"][2 * l + m]
            if lazy and m == 0 and l < Lv - 1:
                assert np.all((got == POISON) | (got == e)), (tag, i, l, m, int(((got != POISON) & (got != e)).sum()))
            else:
                assert np.array_equal(got, e), (tag, i, l, m, _diff(got, e))
            if l < Lv - 1:
                got, e = det.dev_frame_image(i, SPREAD, l, m), exp["spread"][(l, m)]
                if lazy:
                    assert np.all((got == POISON) | (got == e)), (tag, "spread", i, l, m)
                else:
                    assert np.array_equal(got, e), (tag, "spread", i, l, m, _diff(got, e))
        if l > 0:
            got = det.dev_frame_image(i, BGR, l)
            assert np.array_equal(got, exp["bgr"][l]), (tag, "bgr", i, l, _diff(got, exp["bgr"][l]))
    for m in range(2):
        got = det.dev_frame_image(i, LM, Lv - 1, m)
        assert np.array_equal(got, exp["lm"][m]), (tag, "lm", i, m, _diff(got, exp["lm"][m]))


def _detector(c, w, h, T, bank, max_batch, eager, extra=None):
    opts = {"eager_frontend": int(eager)}
    opts.update(extra or {})
    det = api.Detector(c, 2, T)
    det.add_class(bank)
    with options(c, opts):                                       # sampled by fl_detector_finalize
        det.finalize(w, h, max_batch=max_batch)
    return det


def _place(frames, bgr_offsets, depth_offsets, device=True):
    """One allocation per modality (device, or host memory), frame k's bytes at the given offsets: (buffers, bgr ptrs, depth
    ptrs).  Regular offsets make the frames one strided array; irregular ones make them separate frames."""
    fb, fd = frames[0][0].nbytes, frames[0][1].nbytes
    if device:
        tb = torch.zeros(max(bgr_offsets) + fb, dtype=torch.uint8, device="cuda")
        td = torch.zeros(max(depth_offsets) + fd, dtype=torch.uint8, device="cuda")
        for (b, d), ob, od in zip(frames, bgr_offsets, depth_offsets):
            tb[ob:ob + fb].copy_(torch.from_numpy(b.reshape(-1)))
            td[od:od + fd].copy_(torch.from_numpy(d.view(np.uint8).reshape(-1)))
        torch.cuda.synchronize()                                 # the library's stream does not wait for torch's
        pb, pd = tb.data_ptr(), td.data_ptr()
    else:
        tb, td = np.zeros(max(bgr_offsets) + fb, np.uint8), np.zeros(max(depth_offsets) + fd, np.uint8)
        for (b, d), ob, od in zip(frames, bgr_offsets, depth_offsets):
            tb[ob:ob + fb] = b.reshape(-1)
            td[od:od + fd] = d.view(np.uint8).reshape(-1)
        pb, pd = tb.ctypes.data, td.ctypes.data
    return (tb, td), [pb + o for o in bgr_offsets], [pd + o for o in depth_offsets]


def _submit(det, bp, dp, mem=L.FL_MEM_DEVICE):
    det.match_batch_submit(bp, dp, THR, mem)
    det.match_batch_collect(0, 0)                                # waits for the batch


@pytest.fixture(scope="module")
def c():
    """A context of its own: the options these tests set cannot leak into other tests."""
    ctx = api.Context(0)
    yield ctx
    ctx.close()


def _scene(oracle, w, h, T, n, seed):
    frames, masks = _frames(w, h, n, seed)
    exps = [_expected(oracle, b, d, T) for b, d in frames]
    _distinct(exps)
    return dict(frames=frames, exps=exps, bank=_bank(oracle, frames, masks, len(T), seed + 1), T=T, w=w, h=h)


@pytest.fixture(scope="module")
def vga(oracle):
    return _scene(oracle, 640, 480, [5, 8], 6, seed=1)


# ---- A. eager batch, every frame, every image --------------------------------------------------------------------------------
def test_eager_batch_every_frame_equals_oracle(c, vga):
    det = _detector(c, 640, 480, [5, 8], vga["bank"], 8, eager=True)
    try:
        det.match_batch([f[0] for f in vga["frames"]], [f[1] for f in vga["frames"]], THR)
        for i, e in enumerate(vga["exps"]):
            _assert_frame(det, i, e, "eager")
            assert det.frame_counters(i)[3] == -1                # not a lazy batch
    finally:
        det.close()


def test_dev_frame_image_refuses_what_the_workspace_does_not_hold(c, vga):
    import ctypes as C
    det = _detector(c, 640, 480, [5, 8], vga["bank"], 2, eager=True)
    try:
        with pytest.raises(api.FealessError) as e:
            det.dev_frame_image(0, QUANT, 0, 0)                  # nothing matched yet
        assert e.value.code == L.FL_ERR_STATE
        det.match_batch([vga["frames"][0][0]], [vga["frames"][0][1]], THR)
        # frame >= last batch, level 0's colour image, a spread of the coarsest level, linear memories of a fine level, level
        # and modality out of range, no such kind
        for frame, kind, level, m in ((1, QUANT, 0, 0), (0, BGR, 0, 0), (0, SPREAD, 1, 0), (0, LM, 0, 0), (0, QUANT, 2, 0),
                                      (0, QUANT, 0, 2), (0, 7, 0, 0)):
            with pytest.raises(api.FealessError) as e:
                det.dev_frame_image(frame, kind, level, m)
            assert e.value.code == L.FL_ERR_INVALID, (frame, kind, level, m)
        n, buf = C.c_size_t(0), np.zeros(16, np.uint8)
        for kind, level, m, need in ((QUANT, 0, 0, 640 * 480), (LM, 1, 1, 8 * det.lib.fl_lm_label_stride(320, 240, 8))):
            rc = det.lib.fl_dev_frame_image(det.h, 0, kind, level, m, buf.ctypes.data, buf.nbytes, C.byref(n))
            assert rc == L.FL_ERR_INVALID and n.value == need   # too small a buffer: the size still comes back
    finally:
        det.close()


# ---- B. the four input routes, and both upload buffers ------------------------------------------------------------------------
def test_input_routes_give_the_oracle_images(c, vga):
    """Host frames in one array (one strided copy per modality), host frames apart (one copy per frame), device frames at a
    regular pitch (read in place) and at irregular addresses (gathered).  The three host batches run back to back, so that
    both upload buffers serve."""
    frames, exps = vga["frames"], vga["exps"]
    n = len(frames)
    fb, fd = frames[0][0].nbytes, frames[0][1].nbytes
    regular = ([k * fb for k in range(n)], [k * fd for k in range(n)])
    irregular = ([k * fb + 256 * k * k for k in range(n)], [k * fd + 512 * k * (k + 1) for k in range(n)])
    det = _detector(c, 640, 480, [5, 8], vga["bank"], n, eager=True)
    try:
        for route, offs, shift, mem in (("host array", regular, 1, L.FL_MEM_HOST), ("host frames", irregular, 2, L.FL_MEM_HOST),
                                        ("host array again", regular, 3, L.FL_MEM_HOST), ("device in place", regular, 4, L.FL_MEM_DEVICE),
                                        ("device gathered", irregular, 5, L.FL_MEM_DEVICE)):
            order = [(k + shift) % n for k in range(n)]
            bufs, bp, dp = _place([frames[j] for j in order], *offs, device=mem == L.FL_MEM_DEVICE)
            _submit(det, bp, dp, mem)
            for k, j in enumerate(order):
                _assert_frame(det, k, exps[j], route)
            del bufs
    finally:
        det.close()
        torch.cuda.empty_cache()


# ---- C. unusual pitches read in place --------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra_b,extra_d", [(13, 10), (1, 2), (13, 7)])
def test_odd_pitches(c, vga, extra_b, extra_d):
    """Colour pitch = frame bytes + an odd number (odd frame bases), depth pitch = frame bytes + 2 mod 8, read in place; an odd
    depth pitch cannot be read in place (the frames are gathered instead).  The images are the oracle's in every case."""
    frames, exps = vga["frames"][:4], vga["exps"][:4]
    pb, pd = frames[0][0].nbytes + extra_b, frames[0][1].nbytes + extra_d
    det = _detector(c, 640, 480, [5, 8], vga["bank"], len(frames), eager=True)
    try:
        bufs, bp, dp = _place(frames, [k * pb for k in range(4)], [k * pd for k in range(4)])
        _submit(det, bp, dp)
        for k in range(4):
            _assert_frame(det, k, exps[k], (extra_b, extra_d))
        del bufs
    finally:
        det.close()
        torch.cuda.empty_cache()


# ---- D. offsets past 2^31 and 2^32 ---------------------------------------------------------------------------------------
def test_input_frames_past_4gib(c, vga):
    """Six frames at a pitch just above 1 GiB, read in place from one allocation per modality (5 GiB + a frame each): frames 2
    and 3 start between 2^31 and 2^32 bytes after the first, frames 4 and 5 above 2^32."""
    frames = vga["frames"]
    pb, pd = (1 << 30) + 4096 + 3 * 256, (1 << 30) + 2048
    assert 2 * pb > 1 << 31 and 3 * pb < 1 << 32 < 4 * pb and 2 * pd > 1 << 31 and 3 * pd < 1 << 32 < 4 * pd
    det = _detector(c, 640, 480, [5, 8], vga["bank"], len(frames), eager=True)
    bufs = None
    try:
        bufs, bp, dp = _place(frames, [k * pb for k in range(len(frames))], [k * pd for k in range(len(frames))])
        _submit(det, bp, dp)
        for k in range(len(frames)):
            _assert_frame(det, k, vga["exps"][k], "input offset %d" % (k * pb))
    finally:
        del bufs
        det.close()
        torch.cuda.empty_cache()


def test_workspaces_past_4gib(c, vga):
    """260 frames with ws_pad at its 16 MiB maximum: the workspace stride is above 16 MiB, so the last frames' workspaces
    start more than 2^32 bytes after the first.  The six contents, at irregular device addresses, are gathered into the
    workspaces and read from there; every frame equals the oracle's images of its content."""
    frames, exps = vga["frames"], vga["exps"]
    n = 260
    assert (n - 1) * (16 << 20) > 1 << 32
    order = [(5 * i + i // 7) % len(frames) for i in range(n)]
    det = _detector(c, 640, 480, [5, 8], vga["bank"], n, eager=True, extra={"ws_pad": 16 << 20})
    bufs = None
    try:
        fb, fd = frames[0][0].nbytes, frames[0][1].nbytes
        bufs, bp, dp = _place(frames, [k * (fb + 256) for k in range(len(frames))], [k * (fd + 512) for k in range(len(frames))])
        _submit(det, [bp[j] for j in order], [dp[j] for j in order])
        for i, j in enumerate(order):
            _assert_frame(det, i, exps[j], "workspace %d" % i)
    finally:
        del bufs
        det.close()
        torch.cuda.empty_cache()


# ---- E / F. geometries that take the general kernels; lazy batches ---------------------------------------------------------
# 150x160: level 1 is 75 wide (k_pyrdown_general) and 150 is no multiple of 8 (k_resize_nn_half).  180x192 with T = {4, 6, 3}:
# its coarsest level is 45x48, an odd width (any 3-level geometry with an odd coarsest width w2 needs 16 | h2, and T2 | w2, h2).
GEOMS = [(150, 160, [5, 5]), (1280, 720, [5, 8, 4]), (180, 192, [4, 6, 3]), (640, 480, [5, 8])]


@pytest.mark.parametrize("w,h,T", GEOMS, ids=["150x160", "1280x720", "180x192", "640x480"])
def test_eager_and_lazy_batches_per_geometry(c, oracle, vga, w, h, T):
    """An eager and a lazy batch of several frames.  Lazy (dev_poison is on under the test suite): the coarsest level and the
    depth quantisation equal the oracle's; a fine level's colour quantisation is POISON or the oracle's value; every frame with
    candidates computed some level-0 pixels, in at most as many 60x60 tiles as fl_frame_counters reports."""
    sc = vga if (w, h) == (640, 480) else _scene(oracle, w, h, T, 4 if w < 1280 else 3, seed=w + h)
    assert c.get_option("dev_poison") == 1
    n = len(sc["frames"])
    bs, ds = [f[0] for f in sc["frames"]], [f[1] for f in sc["frames"]]
    for eager in (True, False):
        det = _detector(c, w, h, T, sc["bank"], n, eager=eager)
        try:
            det.match_batch(bs, ds, THR)
            with_cands = 0
            for i, e in enumerate(sc["exps"]):
                _assert_frame(det, i, e, ("eager" if eager else "lazy", w, h), lazy=not eager)
                cnt = det.frame_counters(i)
                if eager:
                    assert cnt[3] == -1
                    continue
                q0 = det.dev_frame_image(i, QUANT, 0, 0)
                done = q0 != POISON
                if cnt[0] > 0:
                    with_cands += 1
                    assert done.any(), (w, h, i, cnt)
                ty, tx = -(-h // 60), -(-w // 60)
                pad = np.zeros((ty * 60, tx * 60), bool)
                pad[:h, :w] = done
                tiles = int(pad.reshape(ty, 60, tx, 60).any(axis=(1, 3)).sum())
                assert 0 <= tiles <= cnt[3], (w, h, i, tiles, cnt)
            if not eager and (w, h) != (180, 192):                 # no template of this bank fits 180x192's 45x48 level
                assert with_cands >= 2, (w, h, with_cands)         # not vacuous
        finally:
            det.close()


# ---- G. the device zoom --------------------------------------------------------------------------------------------------------
def _same_reco(g, e, tag):
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert (g["status"], g["found"], g["n_matches"]) == (e["status"], e["found"], e["n_matches"]), tag
    assert (g["best"]["x"], g["best"]["y"], g["best"]["template_id"]) == (e["best"]["x"], e["best"]["y"], e["best"]["template_id"]), tag
    assert bits(g["best"]["similarity"]) == bits(e["best"]["similarity"]), tag
    assert np.array_equal(bits(g["pose"]), bits(e["pose"])), tag
    assert g["det"]["n_points"] == e["det"]["n_points"] and g["det"]["icp"]["iters"] == e["det"]["icp"]["iters"], tag


@pytest.mark.parametrize("dw,dh,T,sources", [(640, 480, [5, 8], [(800, 600), (1024, 768)]), (640, 360, [5, 4], [(1280, 720)])],
                         ids=["to640x480", "to640x360"])
def test_device_zoom_equals_oracle_zoom(c, oracle, dw, dh, T, sources):
    """fl_recognize_batch_zoom from host and from device sources; the second source size is larger, so the upload buffer
    grows.  Every frame's images equal the oracle's of the oracle's INTER_LINEAR zoom, and the recognition results equal
    fl_recognize_batch's on the oracle-zoomed frames."""
    sc = synth.recognition_scene(lambda b, d, l: oracle.quantize_pyramid(b, d, l), levels=2, w=dw, h=dh, seed=9, n_views=3, n_random=8)
    K = sc["K"]
    n = 3
    det = _detector(c, dw, dh, T, sc["bank"], n, eager=True)
    found = 0
    try:
        for sw, sh in sources:
            s = sw / dw
            srcs = []
            for k in range(n):
                R = synth.rot_z(0.03 * k) @ sc["R_true"]
                d, b, _ = synth.render(sw, sh, R, sc["t_true"] + np.array([15.0 * k, -5.0 * k, 0.0]), seed=70 + k,
                                       fx=K[0] * s, fy=K[1] * s, cx=K[2] * s, cy=K[3] * s)
                srcs.append((b, d))
            zoomed = [(oracle.resize_linear_u8(b, dw, dh), oracle.resize_linear_u16(d, dw, dh)) for b, d in srcs]
            exps = [_expected(oracle, b, d, T) for b, d in zoomed]
            _distinct(exps)
            ref = det.recognize_batch([z[0] for z in zoomed], [z[1] for z in zoomed], K)
            for mem in (L.FL_MEM_HOST, L.FL_MEM_DEVICE):
                tag = (sw, sh, "host" if mem == L.FL_MEM_HOST else "device")
                if mem == L.FL_MEM_HOST:
                    got = det.recognize_batch_zoom([f[0] for f in srcs], [f[1] for f in srcs], K)
                else:
                    fb, fd = srcs[0][0].nbytes, srcs[0][1].nbytes
                    bufs, bp, dp = _place(srcs, [k * fb + 64 * k for k in range(n)], [k * fd for k in range(n)])
                    got = det.recognize_batch_zoom(bp, dp, K, mem=L.FL_MEM_DEVICE, src_size=(sw, sh))
                    del bufs
                for i in range(n):
                    _assert_frame(det, i, exps[i], tag)
                    _same_reco(got[i], ref[i], tag + (i,))
                found += sum(r["found"] for r in got)
        if dh == 480:
            assert found > 0                                     # the refinement ran too
    finally:
        det.close()
        torch.cuda.empty_cache()
