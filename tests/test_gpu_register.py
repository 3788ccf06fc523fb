"""GPU: depth registration (fl_register_depth_batch, include/fealess_hip.h) against tests/register_model.py, the numpy statement of
its contract.  Every comparison is GPU == model bit for bit unless it says otherwise."""
import ctypes as C

import numpy as np
import pytest

import cadreco_depth_py as CD
import cadreco_py as CR
import register_cases as RC
import register_model as GM
import verify_model as VM
from fealess_amd import _lib as L
from fealess_amd import api, synth

pytestmark = pytest.mark.gpu

EYE, ZERO = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)


def _K(w, h, f=0.95, dx=-0.3, dy=0.2):
    """A camera for a w x h image: focal length f * w, the principal point a fraction of a pixel off the centre."""
    return (w, h, f * w, f * w * 1.01, w / 2 + dx, h / 2 + dy)


def _frame(w, h, seed, lo=650, hi=1300, holes=0.1):
    """A depth frame with everything registration meets: a sloping surface from lo to hi mm, nearer blocks with sharp edges,
    single-pixel noise and pixels without a measurement."""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    z = lo + (hi - lo) * (0.7 * u / max(w - 1, 1) + 0.3 * v / max(h - 1, 1))
    for _ in range(4):
        x0, y0 = int(rng.integers(0, max(w - 2, 1))), int(rng.integers(0, max(h - 2, 1)))
        z[y0:y0 + int(rng.integers(1, max(h // 2, 2))), x0:x0 + int(rng.integers(1, max(w // 2, 2)))] -= float(rng.integers(60, 250))
    z = np.clip(np.rint(z + rng.integers(-2, 3, size=z.shape)), 1, 65535).astype(np.uint16)
    z[rng.random((h, w)) < holes] = 0
    return z


def _model(frames, Kd, Kc, R, t, fill):
    return np.stack([GM.register(f, Kd, Kc, R, t, fill) for f in frames])


def _device(ctx, frames, Kd, Kc, R, t, fill):
    """The frames registered with mem=FL_MEM_DEVICE: device tensors in, the output tensor's content back on the host."""
    import torch
    d_in = torch.from_numpy(np.stack(frames).view(np.int16)).to(f"cuda:{ctx.device}")
    d_out = torch.full((len(frames), Kc[1], Kc[0]), -23131, dtype=torch.int16, device=d_in.device)     # 0xA5A5: every pixel is written
    torch.cuda.synchronize()
    px_in, px_out = Kd[0] * Kd[1] * 2, Kc[0] * Kc[1] * 2
    ctx.register_depth([d_in.data_ptr() + i * px_in for i in range(len(frames))], Kd, Kc, R, t, fill, mem=L.FL_MEM_DEVICE,
                       out=[d_out.data_ptr() + i * px_out for i in range(len(frames))])
    ctx.synchronize()
    return d_out.cpu().numpy().view(np.uint16)


def _check(ctx, frames, Kd, Kc, R, t, fills=(0, 1)):
    """Host frames and device frames against the model, for each fill; returns the model's output of the last fill."""
    for fill in fills:
        want = _model(frames, Kd, Kc, R, t, fill)
        got = ctx.register_depth(frames, Kd, Kc, R, t, fill)
        assert got.dtype == np.uint16 and got.shape == want.shape
        assert np.array_equal(got, want), (fill, int((got != want).sum()))
        assert np.array_equal(_device(ctx, frames, Kd, Kc, R, t, fill), want), fill
    return want


# ---- (a) shapes -------------------------------------------------------------------------------------------------------------------
def test_two_camera_scene(ctx):
    """The scene of tests/test_register_cpu.py at 640 x 480, with and without the fill, and the 320 x 240 depth camera."""
    s = RC.scene()
    R, t = RC.extrinsics()
    F = _check(ctx, [s["depth_cam"]], RC.K_DEPTH, RC.K_COLOR, R, t)[0]
    c = RC.compare(F, s["color_cam"])
    assert c["within2"] / c["both"] > 0.99 and c["empty"] < 0.01 * F.size            # it is the registration the CPU test measures
    _check(ctx, [s["depth_cam_half"]], RC.K_DEPTH_HALF, RC.K_COLOR, R, t)


SHAPES = {
    "64x48 to 64x48": ((64, 48), (64, 48), 1.0),
    "322x250 to 322x250: a pixel tail, rows at odd addresses": ((322, 250), (322, 250), 1.0),
    "17x9 to 23x11": ((17, 9), (23, 11), 23 / 17),
    "32x24 to 64x48: footprints of several pixels": ((32, 24), (64, 48), 2.0),
    "8x6 to 128x96: every footprint hits the cap": ((8, 6), (128, 96), 16.0),
}


@pytest.mark.parametrize("case", sorted(SHAPES))
def test_shapes(ctx, case):
    (wd, hd), (wc, hc), zoom = SHAPES[case]
    Kd = _K(wd, hd)
    Kc = (wc, hc, Kd[2] * zoom * 1.03, Kd[3] * zoom * 0.98, wc / 2 + 0.4, hc / 2 - 0.1)
    R, t = GM.rodrigues((0.01, -0.02, 0.015)).astype(np.float32), np.array([12.0, -7.0, 3.0], np.float32)
    frames = [_frame(wd, hd, 3), _frame(wd, hd, 4, holes=0.4)]
    out = _check(ctx, frames, Kd, Kc, R, t)
    assert (out != 0).any()
    if zoom == 16.0:
        live, _, x0, x1, y0, y1 = GM.footprints(frames[0], Kd, Kc, R, t)
        assert live.any() and ((x1 - x0)[live] <= GM.MAX_SPLAT - 1).all() and ((x1 - x0)[live] == GM.MAX_SPLAT - 1).any()


def test_many_source_pixels_per_target(ctx):
    """640 x 480 of a plane onto 160 x 120: footprints a quarter of a pixel wide land only where they hold a pixel centre, and where
    several do -- a camera offset of a whole number of pixels puts centres on shared footprint edges -- the minimum decides."""
    u, v = np.meshgrid(np.arange(640.0), np.arange(480.0))
    plane = np.rint(800.0 + 0.5 * u + 0.25 * v).astype(np.uint16)
    Kd, Kc = (640, 480, 512.0, 512.0, 320.0, 240.0), (160, 120, 128.0, 128.0, 80.125, 60.125)
    out = _check(ctx, [plane], Kd, Kc, EYE, ZERO)[0]
    live = GM.footprints(plane, Kd, Kc, EYE, ZERO)[0]
    assert (out != 0).all() and live.sum() > out.size                       # more source pixels land than there are targets
    tilted = GM.rodrigues((0.02, 0.03, -0.01)).astype(np.float32)
    _check(ctx, [plane, _frame(640, 480, 9)], Kd, _K(160, 120), tilted, np.array([30.0, 5.0, -4.0], np.float32))


# ---- (b) data extremes ------------------------------------------------------------------------------------------------------------
def test_data_extremes(ctx):
    Kd, Kc = _K(64, 48), _K(72, 40, f=1.1)
    R = GM.rodrigues((0.0, 0.01, 0.0)).astype(np.float32)
    scene = _frame(64, 48, 5, holes=0.0)
    assert scene.min() >= 400 and scene.max() <= 1300
    # a frame of all 0
    assert not _check(ctx, [np.zeros((48, 64), np.uint16)], Kd, Kc, R, np.array([5.0, 0.0, 0.0], np.float32)).any()
    # all 65535 with t_z = +10: saturation
    out = _check(ctx, [np.full((48, 64), 65535, np.uint16)], Kd, Kd, EYE, np.array([0.0, 0.0, 10.0], np.float32), fills=(0,))
    assert (out[out != 0] == 65535).all() and (out != 0).sum() > 0.9 * out.size
    # t_z = -700 on a scene around it: Z <= 0 and the 0.5 rule
    near = np.clip(scene, 650, 1300)
    near[::3, ::5] = 700                                                     # Z_C = 0 exactly
    near[1::3, ::5] = 701                                                    # Z_C = 1
    out = _check(ctx, [near], Kd, Kc, EYE, np.array([0.0, 0.0, -700.0], np.float32))
    assert (out != 0).any()
    assert not _check(ctx, [np.full((48, 64), 650, np.uint16)], Kd, Kc, EYE, np.array([0.0, 0.0, -700.0], np.float32)).any()
    # 180 degrees about y: everything behind the camera
    assert not _check(ctx, [scene], Kd, Kc, GM.rodrigues((0.0, np.pi, 0.0)).astype(np.float32), ZERO).any()
    # t_x = 5000: everything out of view
    assert not _check(ctx, [scene], Kd, Kc, EYE, np.array([5000.0, 0.0, 0.0], np.float32)).any()
    # footprints straddling each border: the projection is twice the output's size around it, footprints about two pixels wide
    Kc = (40, 30, Kd[2] * 2.1, Kd[3] * 2.1, 20.3, 14.6)
    out = _check(ctx, [scene], Kd, Kc, EYE, ZERO, fills=(0,))[0]
    live, _, x0, x1, y0, y1 = GM.footprints(scene, Kd, Kc, EYE, ZERO)
    assert out[0].all() and out[-1].all() and out[:, 0].all() and out[:, -1].all()
    # the footprints tile the projection, 2.1 pixels each at no whole-pixel phase, so the ones that cover a border pixel cross the border
    for axis_lo, axis_hi, n in ((x0, x1, 40), (y0, y1, 30)):
        assert (live & (axis_lo == 0)).any() and (live & (axis_hi == n - 1)).any()
    assert (~live).any()                                                     # and pixels that fall outside altogether


# ---- (c) batching -----------------------------------------------------------------------------------------------------------------
def test_batching_across_the_chunk(ctx):
    """70 different frames of 64 x 48 cross the 64-frame chunk; a batch equals the single calls in either order; host frames equal
    device frames; two runs of one call are byte-equal."""
    assert L.FL_REGISTER_CHUNK_FRAMES == 64
    Kd, Kc = _K(64, 48), _K(64, 48, f=1.02, dx=0.1)
    R, t = GM.rodrigues((0.004, -0.006, 0.003)).astype(np.float32), np.array([25.0, -1.0, 2.0], np.float32)
    frames = [_frame(64, 48, 100 + i) for i in range(70)]
    want = _model(frames, Kd, Kc, R, t, 1)
    assert len({w.tobytes() for w in want}) == 70
    batch = ctx.register_depth(frames, Kd, Kc, R, t, 1)
    assert np.array_equal(batch, want)
    assert ctx.register_depth(frames, Kd, Kc, R, t, 1).tobytes() == batch.tobytes()
    for order in (range(70), reversed(range(70))):
        for i in order:
            assert np.array_equal(ctx.register_depth([frames[i]], Kd, Kc, R, t, 1)[0], want[i]), i
    dev = _device(ctx, frames, Kd, Kc, R, t, 1)
    assert np.array_equal(dev, want) and _device(ctx, frames, Kd, Kc, R, t, 1).tobytes() == dev.tobytes()
    out = np.zeros((70, 48, 64), np.uint16)
    assert ctx.register_depth(frames, Kd, Kc, R, t, 1, out=out) is out and np.array_equal(out, want)


def test_refusals_raise(ctx):
    frames = [_frame(64, 48, 1)]
    Kd = _K(64, 48)
    for bad in (dict(R=np.eye(3) * 1.1), dict(fill=2), dict(Kc=(64, 0) + Kd[2:]), dict(Kc=(64, 48, -1.0, 60.0, 32.0, 24.0)), dict(t=(np.nan, 0, 0))):
        with pytest.raises(api.FealessError) as e:
            ctx.register_depth(frames, Kd, bad.get("Kc", Kd), bad.get("R", EYE), bad.get("t", ZERO), bad.get("fill", 1))
        assert e.value.code == L.FL_ERR_INVALID


# ---- (d) composition in HBM -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_detector(ctx, oracle):
    sc = synth.recognition_scene(lambda b, d, l: oracle.quantize_pyramid(b, d, l), levels=2, seed=7, n_views=3)
    det = api.Detector(ctx, 2, [5, 8])
    det.add_class(sc["bank"])
    det.finalize(640, 480, max_batch=2)
    yield sc, det
    det.close()


def _to_depth_camera(depth):
    """A colour-aligned frame as the depth camera of tests/register_cases.py would have seen it: the model, the other way round."""
    R, t = RC.extrinsics()
    Ri = R.astype(np.float64).T
    return GM.register(depth, RC.K_COLOR, RC.K_DEPTH, Ri.astype(np.float32), (-Ri @ t.astype(np.float64)).astype(np.float32), 1)


def test_registered_frames_feed_verify_and_recognition_by_device_pointer(ctx, small_detector):
    import torch
    sc, det = small_detector
    s = RC.scene()
    R, t = RC.extrinsics()
    dev = f"cuda:{ctx.device}"
    raw = [s["depth_cam"].copy(), _to_depth_camera(sc["depth"])]             # the scene's arrays are read-only: torch wants writable ones
    d_raw = [torch.from_numpy(r.view(np.int16)).to(dev) for r in raw]
    d_reg = [torch.empty((RC.H, RC.W), dtype=torch.int16, device=dev) for _ in raw]
    d_bgr = torch.from_numpy(sc["bgr"]).to(dev)
    torch.cuda.synchronize()
    trk = api.Tracker(ctx, s["mesh"]["vertices"], s["mesh"]["triangles"], w=RC.W, h=RC.H, max_frames=2, max_tracks=2, max_crop_px=320 * 240)
    params, k = L.RecognitionParams(75.0, 10, 0.5, 0.01, L.FL_ICP_PARITY), L.Intrinsics(640, 480, *sc["K"])

    def recognize(bgr_ptr, depth_ptr, mem):
        """fl_recognize_batch on one frame, by pointer: the record as the library wrote it."""
        res = (L.RecognitionResult * 1)()
        ctx.check(ctx.lib.fl_recognize_batch(det.h, 1, (C.c_void_p * 1)(bgr_ptr), (C.c_void_p * 1)(depth_ptr), mem, C.byref(k), C.byref(params), res))
        return res

    try:
        # before: verification and recognition on host frames the model registered
        want = _model(raw, RC.K_DEPTH, RC.K_COLOR, R, t, 1)
        poses = np.stack([s["pose13_color"]] * 2)
        v_before = trk.verify([want[0]], [0, 0], poses, RC.K_COLOR[2:])
        r_before = bytes(recognize(sc["bgr"].ctypes.data, want[1].ctypes.data, L.FL_MEM_HOST))
        # registration in HBM, results handed on by pointer
        ctx.register_depth(d_raw, RC.K_DEPTH, RC.K_COLOR, R, t, 1, mem=L.FL_MEM_DEVICE, out=d_reg)
        v_dev = trk.verify([d_reg[0]], [0, 0], poses, RC.K_COLOR[2:])
        r_dev = recognize(d_bgr.data_ptr(), d_reg[1].data_ptr(), L.FL_MEM_DEVICE)
        ctx.synchronize()
        reg_host = [d.cpu().numpy().view(np.uint16) for d in d_reg]
        assert np.array_equal(np.stack(reg_host), want)
        # verification equals the model on the model's registered frame
        model = VM.verify(s["mesh"], [want[0]], [0, 0], poses, RC.K_COLOR[2:])
        assert v_dev.tobytes() == model.tobytes() and v_dev["n_inlier"][0] > 0.98 * v_dev["n_model"][0] > 0
        # recognition on the device pointers equals the same call on host copies of them, byte for byte
        res = recognize(sc["bgr"].ctypes.data, reg_host[1].ctypes.data, L.FL_MEM_HOST)
        assert bytes(res) == bytes(r_dev) and res[0].found == 1 and res[0].status == 0
        # after: the calls around the registration are unchanged (the scratch is shared)
        assert trk.verify([want[0]], [0, 0], poses, RC.K_COLOR[2:]).tobytes() == v_before.tobytes() == v_dev.tobytes()
        r_after = bytes(recognize(sc["bgr"].ctypes.data, want[1].ctypes.data, L.FL_MEM_HOST))
        assert r_after == r_before == bytes(res)                              # the whole record, and it is the registered frame's
    finally:
        trk.close()


# ---- (e) the facade ---------------------------------------------------------------------------------------------------------------
def test_facade_depth_camera(ctx, tmp_path):
    """On a frame the facade recognises: with the depth camera set and the depth sensor's frame passed in, Recognition equals
    Recognition on the host-registered frame bit for bit; on = 0 equals the result without a depth camera."""
    K0, W, H = (608.0, 608.0, 320.0, 240.0), 640, 480
    mesh = synth.object_mesh(2)
    obj = str(tmp_path / "object.obj")
    synth.write_obj(obj, mesh)
    R, t = RC.extrinsics()
    with CR.handle() as h:
        P = api.view_sphere(0, [700.0], n_inplane=1, inplane_deg=0.0, upper_hemisphere=True)
        rc, tov = CR.train_mesh(h, tmp_path / "bank", obj, len(P), dict(subdivisions=0, upper=1, distances=[700.0], n_inplane=1, inplane_deg=0.0))
        assert rc == 0 and (tov >= 0).any() and CR.lib().cadreco_add_obj(h, str(tmp_path / "bank").encode()) == 0
        V, N, T = CR.read_obj(obj)
        view = P[int(np.flatnonzero(tov >= 0)[0])]
        bgr, dep, msk, _ = ctx.render_views(V, T, view[None], K0, W, H, normals=N)
        u, v = np.meshgrid(np.arange(float(W)), np.arange(float(H)))
        m = msk[0] > 0
        depth = np.ascontiguousarray(np.where(m, dep[0], np.rint(950.0 + 0.06 * u + 0.04 * v)).astype(np.uint16))
        cell = (np.floor(u / 23.0) + 2 * np.floor(v / 17.0)) % 5
        col = np.where(m[..., None], bgr[0].astype(np.float64), (70 + 30 * cell)[..., None] * np.array([1.0, 0.9, 0.75]))
        col = np.ascontiguousarray(np.clip(np.rint(col), 0, 255).astype(np.uint8))
        today = CR.recognition(h, col, depth, K0)
        assert today[0] == 0 and today[1] == 1 and today[2] == b"mesh"

        def same(a, b):
            return a[:3] == b[:3] and a[3].tobytes() == b[3].tobytes()

        raw = np.ascontiguousarray(_to_depth_camera(depth))                  # what the depth sensor delivers, 640 x 480
        host = ctx.register_depth([raw], RC.K_DEPTH, RC.K_COLOR, R, t, 1)[0]
        assert CD.set_depth_camera(h, 1, RC.K_DEPTH, R, t, 1) == 0
        on = CR.recognition(h, col, raw, K0)
        bad = CR.recognition(h, col, np.zeros((240, 320), np.uint16), K0, camera_size=(W, H))   # not K_depth's size (nor the colour image's)
        assert CD.set_depth_camera(h, 0, RC.K_DEPTH, None, None, 1) == 0
        assert same(on, CR.recognition(h, col, host, K0)) and on[0] == 0 and on[1] == 1 and on[2] == b"mesh"
        assert bad[0] == CR.INVALID and bad[1] == 0
        # a depth camera of another size, through the shim that takes it
        half = np.ascontiguousarray(GM.register(depth, RC.K_COLOR, RC.K_DEPTH_HALF, EYE, ZERO, 1))
        host = ctx.register_depth([half], RC.K_DEPTH_HALF, RC.K_COLOR, EYE, ZERO, 0)[0]
        assert CD.set_depth_camera(h, 1, RC.K_DEPTH_HALF, EYE, ZERO, 0) == 0
        on = CD.recognition_depth(h, col, half, K0)
        assert CR.recognition(h, col, depth, K0)[0] == CR.INVALID               # a colour-sized depth image is refused while it is on
        assert CD.set_depth_camera(h, 0, RC.K_DEPTH_HALF, EYE, ZERO, 0) == 0
        assert same(on, CR.recognition(h, col, host, K0)) and on[0] == 0
        # on = 0: today's result
        assert same(today, CR.recognition(h, col, depth, K0))
        # the frame helper CadRecoTrack, CadRecoVerify and CadRecoArbitrate share: each with the camera set on the sensor's frame
        # equals the call without it on the host-registered frame
        host = ctx.register_depth([raw], RC.K_DEPTH, RC.K_COLOR, R, t, 1)[0]
        assert CR.lib().cadreco_set_tracking_mesh(h, obj.encode(), 1.0) == 0
        moved = today[3].copy()
        moved[3] += 3.0
        poses = np.stack([today[3], moved])
        tags = (C.c_char_p * 2)(b"mesh", b"mesh")

        def mesh_calls(frame):
            ver, arb, trk, p = np.zeros(2 * 8, np.int32), np.zeros(2 * 11, np.int32), np.zeros(2, np.int32), poses.copy()
            f = CR.frame_args(frame, 1.0, K0)
            codes = (CR.lib().cadreco_verify(h, *f, 2, poses.ctypes.data, 10.0, ver.ctypes.data),
                     CR.lib().cadreco_arbitrate(h, *f, 2, poses.ctypes.data, tags, 10.0, 0.5, arb.ctypes.data),
                     CR.lib().cadreco_track(h, *f, 2, p.ctypes.data, trk.ctypes.data))
            return codes, ver.tobytes(), arb.tobytes(), trk.tobytes(), p.tobytes()

        off = mesh_calls(host)
        assert off[0] == (0, 0, 0) and np.frombuffer(off[1], np.int32)[1] > 5000 and np.frombuffer(off[3], np.int32).all()
        assert CD.set_depth_camera(h, 1, RC.K_DEPTH, R, t, 1) == 0
        assert mesh_calls(raw) == off
        small = np.zeros((240, 320), np.uint16)                                 # not K_depth's size: refused, nothing written
        assert mesh_calls(small)[0] == (CR.INVALID,) * 3 and not np.frombuffer(mesh_calls(small)[1], np.int32).any()
        assert CD.set_depth_camera(h, 0, RC.K_DEPTH, R, t, 1) == 0
        assert mesh_calls(host) == off
