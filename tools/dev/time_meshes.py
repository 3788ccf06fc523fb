"""Dev aid: what one tracker of several meshes buys over one tracker per mesh.  Three meshes (the box of synth.object_mesh alone,
12 triangles; icosphere(3) * 60, 1280; synth.object_mesh(2), 332), --per poses each (1, 8, 21) on shared frames of
tests/test_gpu_track.py's sequence (640 x 480, frames by device pointer), warm, median of --reps calls of the host wall time:
  three   what a caller does without fl_tracker_create_meshes: three one-mesh trackers and three calls, each staging the frames
  multi   one three-mesh tracker, one call with mesh_of
for fl_verify_batch (verify_fused 0 and 1) and fl_track_batch_verified (point-to-plane, one pass, keep_input 0), with the median
device time by stage (of the last of the three calls for `three`: fl_dev_tracker_*_ms are per tracker).
Then the render stage (verify_fused 0) of --grid-views views: the 1280-triangle mesh alone on a one-mesh tracker (k_raster<false>),
the same through mesh_of (k_raster<true>), and 12- and 1280-triangle meshes mixed -- k_raster<true> launches the largest mesh's
waves for every view.  And the device memory of one three-mesh tracker against three one-mesh trackers at the facade's sizes
(one frame, 16 tracks, crops of 320 x 240).
FEALESS_HIP_LIB may name an older build of the library: only `three` is printed."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (runtime load order, see tests/conftest.py)
from fealess_amd import _lib as L  # noqa: E402

_probe = C.CDLL(L.LIB_PATH)
for _name in [n for n in L.SIGNATURES if not hasattr(_probe, n)]:      # an older build: bind what it has
    del L.SIGNATURES[_name]
from fealess_amd import api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--per", type=int, nargs="+", default=[1, 8, 21])
ap.add_argument("--grid-views", type=int, default=42)
args = ap.parse_args()
HAVE = "fl_tracker_create_meshes" in L.SIGNATURES

W, H, K0 = 640, 480, (608.0, 608.0, 320.0, 240.0)
MOTION_T, MOTION_A = (4.0, -2.0, 3.0), (0.02, -0.01, 0.015)


def gt(k):
    return synth.object_pose(10 + MOTION_T[0] * k, -5 + MOTION_T[1] * k, 720.0 + MOTION_T[2] * k, 0.3 + MOTION_A[0] * k, 0.35 + MOTION_A[1] * k,
                             0.1 + MOTION_A[2] * k)


def median_ms(fn, stages):
    for _ in range(args.warmup):
        fn()
    t, st = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
        st.append(stages())
    return statistics.median(t), min(t), max(t), {k: round(statistics.median(s[k] for s in st), 4) for k in st[0]}


def line(med, **fields):
    print(json.dumps(dict(fields, reps=args.reps, median_ms=round(med[0], 3), min_ms=round(med[1], 3), max_ms=round(med[2], 3), stage_ms=med[3])),
          flush=True)


def f32i32(v, t):
    return np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(t, np.int32).reshape(-1, 3)


bv, _, bt = synth.box_mesh(np.array([45.0, 0.0, 10.0]), np.array([55.0, 35.0, 25.0]))
sv, sf = synth.icosphere(3)
obj = synth.object_mesh(2)
MESHES = [f32i32(np.array(bv), np.array(bt)), f32i32(sv * 60.0, sf), f32i32(obj["vertices"], obj["triangles"])]     # 12, 1280, 332 triangles

NF = 6
frames = [synth.render(W, H, *gt(k), seed=100 + k)[0] for k in range(1, NF + 1)]
poses_in = np.stack([synth.pose13(*gt(k - 1)) for k in range(1, NF + 1)])
d_d = torch.from_numpy(np.stack(frames).view(np.int16)).cuda()
torch.cuda.synchronize()
dptr = [d_d.data_ptr() + i * W * H * 2 for i in range(NF)]

ctx = api.Context(0)
K = L.Intrinsics(W, H, *K0)
prm = L.TrackParams(12, 1, 10, 0.5, 0.01, L.FL_ICP_POINT_TO_PLANE, 0.0, 0.0)
vp = L.TrackVerifyParams(L.VerifyParams(10, 1, 0.0, 0.0), 0, 0)
n_max = 3 * max(max(args.per), (args.grid_views + 2) // 3)


def free_mb():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0] / 2 ** 20


# ---- device memory at the facade's sizes --------------------------------------------------------------------------------------
m0 = free_mb()
small = [api.Tracker(ctx, v, t, W, H, 1, 16, 320 * 240) for v, t in MESHES]
m1 = free_mb()
for t in small:
    t.close()
mem = dict(what="memory_mb", three_one_mesh_trackers=round(m0 - m1, 2))
if HAVE:
    m2 = free_mb()
    t = api.Tracker(ctx, meshes=MESHES, w=W, h=H, max_frames=1, max_tracks=16, max_crop_px=320 * 240)
    mem["one_three_mesh_tracker"] = round(m2 - free_mb(), 2)
    t.close()
print(json.dumps(mem), flush=True)

ones = [api.Tracker(ctx, v, t, W, H, NF, n_max, 40000) for v, t in MESHES]
multi = api.Tracker(ctx, meshes=MESHES, w=W, h=H, max_frames=NF, max_tracks=n_max, max_crop_px=40000) if HAVE else None
for per in args.per:
    nf = min(per, NF)
    dp = (C.c_void_p * nf)(*dptr[:nf])
    fof1 = np.ascontiguousarray(np.arange(per) % nf, np.int32)
    p1 = np.ascontiguousarray(poses_in[fof1], np.float32)
    fof3, p3 = np.ascontiguousarray(np.tile(fof1, 3)), np.ascontiguousarray(np.tile(p1, (3, 1)))
    mof = np.ascontiguousarray(np.repeat(np.arange(3), per), np.int32)
    v1, v3 = np.zeros((3, per), api.VERIFY_DTYPE), np.zeros(3 * per, api.VERIFY_DTYPE)
    t1, t3 = np.zeros((3, per), api.VERIFIED_TRACK_DTYPE), np.zeros(3 * per, api.VERIFIED_TRACK_DTYPE)

    def verify_three():
        for m, trk in enumerate(ones):
            ctx.check(trk.lib.fl_verify_batch(trk.handle, nf, dp, L.FL_MEM_DEVICE, per, fof1.ctypes.data, p1.ctypes.data, 0, None, C.byref(K), None,
                                              v1[m].ctypes.data))

    def verify_multi():
        ctx.check(multi.lib.fl_verify_batch_meshes(multi.handle, nf, dp, L.FL_MEM_DEVICE, 3 * per, fof3.ctypes.data, mof.ctypes.data, p3.ctypes.data, 0, None,
                                                   C.byref(K), None, v3.ctypes.data))

    def track_three():
        for m, trk in enumerate(ones):
            ctx.check(trk.lib.fl_track_batch_verified(trk.handle, nf, dp, L.FL_MEM_DEVICE, per, fof1.ctypes.data, p1.ctypes.data, 0, None, C.byref(K),
                                                      C.byref(prm), C.byref(vp), t1[m].ctypes.data))

    def track_multi():
        ctx.check(multi.lib.fl_track_batch_verified_meshes(multi.handle, nf, dp, L.FL_MEM_DEVICE, 3 * per, fof3.ctypes.data, mof.ctypes.data, p3.ctypes.data,
                                                           0, None, C.byref(K), C.byref(prm), C.byref(vp), t3.ctypes.data))

    for fused in (0, 1):
        ctx.set_option("verify_fused", fused)
        line(median_ms(verify_three, ones[-1].verify_ms), what="verify", how="three", verify_fused=fused, meshes=3, per_mesh=per, frames=nf)
        if HAVE:
            line(median_ms(verify_multi, multi.verify_ms), what="verify", how="multi", verify_fused=fused, meshes=3, per_mesh=per, frames=nf)
            assert v3.tobytes() == v1.tobytes()
    ctx.set_option("verify_fused", 0)
    line(median_ms(track_three, lambda: dict(ones[-1].stage_ms(), **ones[-1].track_verified_ms())), what="track_verified", how="three", meshes=3,
         per_mesh=per, frames=nf)
    if HAVE:
        line(median_ms(track_multi, lambda: dict(multi.stage_ms(), **multi.track_verified_ms())), what="track_verified", how="multi", meshes=3,
             per_mesh=per, frames=nf)
        assert t3.tobytes() == t1.tobytes()

# ---- the largest mesh sizes the grid: the render stage of --grid-views views ---------------------------------------------------
n = args.grid_views
dp = (C.c_void_p * NF)(*dptr)
fof = np.ascontiguousarray(np.arange(n) % NF, np.int32)
p = np.ascontiguousarray(poses_in[fof], np.float32)
out = np.zeros(n, api.VERIFY_DTYPE)
ctx.set_option("verify_fused", 0)


def render_of(trk, mesh_of):
    mo = None if mesh_of is None else np.ascontiguousarray(mesh_of, np.int32)

    def fn():
        if mo is None:
            ctx.check(trk.lib.fl_verify_batch(trk.handle, NF, dp, L.FL_MEM_DEVICE, n, fof.ctypes.data, p.ctypes.data, 0, None, C.byref(K), None, out.ctypes.data))
        else:
            ctx.check(trk.lib.fl_verify_batch_meshes(trk.handle, NF, dp, L.FL_MEM_DEVICE, n, fof.ctypes.data, mo.ctypes.data, p.ctypes.data, 0, None, C.byref(K),
                                                     None, out.ctypes.data))
    return median_ms(fn, trk.verify_ms)


line(render_of(ones[1], None), what="grid", how="one-mesh tracker, 1280 triangles", views=n)
line(render_of(ones[0], None), what="grid", how="one-mesh tracker, 12 triangles", views=n)
if HAVE:
    line(render_of(multi, np.full(n, 1)), what="grid", how="mesh_of: 1280 triangles for every view", views=n)
    line(render_of(multi, np.arange(n) % 2), what="grid", how="mesh_of: 12 and 1280 triangles in turn", views=n)
    line(render_of(multi, np.zeros(n)), what="grid", how="mesh_of: 12 triangles for every view, grid of 1280", views=n)
for t in ones + ([multi] if HAVE else []):
    t.close()
ctx.close()
