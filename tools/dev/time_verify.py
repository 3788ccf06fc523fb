"""Dev aid: what a fit figure per pose costs -- verified (fl_verify_batch), or tracked one pass (fl_track_batch, which is what a
caller without verification runs to get icp.dist_mean / px_ratio).  Frames of the object of tests/test_gpu_track.py's sequence
(640 x 480, noise and background on), one pose per frame, each coming in with the previous frame's true pose, frames by device
pointer, warm, median of --reps calls of the host wall time, for 1, 8 and 64 poses:
  verify  fl_verify_batch with the default parameters, every pose its own group, and once more with groups of up to eight (the
          pick kernel), with the median device time by stage (copy, render, score, finish; fl_dev_tracker_verify_ms); where the
          library has the option, with verify_fused 0 and 1 (then `score` is k_verify_fused and `render` is empty), the latter at
          every band budget of --fused-px (0 = the compiled one);
  track   fl_track_batch, one pass, FL_ICP_POINT_TO_PLANE (the default) and FL_ICP_PARITY, with its median device time by stage.
FEALESS_HIP_LIB may name an older build of the library: the entry points it lacks are skipped (only `track` is printed)."""
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
ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64])
ap.add_argument("--fused-px", type=int, nargs="+", default=[0])
args = ap.parse_args()

W, H, K0 = 640, 480, (608.0, 608.0, 320.0, 240.0)
MOTION_T, MOTION_A = (4.0, -2.0, 3.0), (0.02, -0.01, 0.015)


def gt(k):
    return synth.object_pose(10 + MOTION_T[0] * k, -5 + MOTION_T[1] * k, 720.0 + MOTION_T[2] * k, 0.3 + MOTION_A[0] * k, 0.35 + MOTION_A[1] * k,
                             0.1 + MOTION_A[2] * k)


def median_ms(fn, stages):
    """(median, min, max) of the host wall time of fn() over --reps calls, and the median of every entry of stages(), the device
    time by stage of the call just made, read outside the timed region."""
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


n_max = max(args.sizes)
frames = [synth.render(W, H, *gt(k), seed=100 + k)[0] for k in range(1, 7)]
poses_in = np.stack([synth.pose13(*gt(k - 1)) for k in range(1, 7)])
idx = np.arange(n_max) % 6
d_d = torch.from_numpy(np.stack([frames[i] for i in idx]).view(np.int16)).cuda()
torch.cuda.synchronize()
dptr = [d_d.data_ptr() + i * W * H * 2 for i in range(n_max)]

ctx = api.Context(0)
mesh = synth.object_mesh(2)
trk = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], W, H, n_max, n_max, 40000)
K = L.Intrinsics(W, H, *K0)
try:
    ctx.get_option("verify_fused")
    variants = [(0, 0)] + [(1, px) for px in args.fused_px]
except api.FealessError:
    variants = [(None, None)]
for n in args.sizes:
    dp = (C.c_void_p * n)(*dptr[:n])
    fof = np.arange(n, dtype=np.int32)
    p13 = np.ascontiguousarray(poses_in[idx[:n]], np.float32)
    if "fl_verify_batch" in L.SIGNATURES:
        out = np.zeros(n, api.VERIFY_DTYPE)
        gf = np.ascontiguousarray(list(range(0, n, 8)) + [n], np.int32)
        for groups, (fused, px) in ((g, v) for g in (None, gf) for v in variants):
            if fused is not None:
                ctx.set_option("verify_fused", fused)
                ctx.set_option("verify_fused_px", px)

            def fn():           # raw ctypes: the same host work as the track call below
                ctx.check(trk.lib.fl_verify_batch(trk.handle, n, dp, L.FL_MEM_DEVICE, n, fof.ctypes.data, p13.ctypes.data,
                                                  0 if groups is None else len(groups) - 1, None if groups is None else groups.ctypes.data,
                                                  C.byref(K), None, out.ctypes.data))
            fn()
            assert (out["n_model"] > 5000).all() and (out["inlier_ratio"] > 0.8).all()
            med = median_ms(fn, trk.verify_ms)
            line(med, what="verify", fused=fused, fused_px=px, groups=0 if groups is None else len(groups) - 1, poses=n,
                 per_pose_ms=round(med[0] / n, 4), n_model=int(out["n_model"][0]))
        if variants[0][0] is not None:
            ctx.set_option("verify_fused", 0)
            ctx.set_option("verify_fused_px", 0)
    out = np.zeros(n, api.TRACK_DTYPE)
    for mode, name in ((L.FL_ICP_POINT_TO_PLANE, "point_to_plane"), (L.FL_ICP_PARITY, "parity")):
        prm = L.TrackParams(12, 1, 10, 0.5, 0.01, mode, 0.0, 0.0)

        def fn():
            ctx.check(trk.lib.fl_track_batch(trk.handle, n, dp, L.FL_MEM_DEVICE, n, fof.ctypes.data, p13.ctypes.data, C.byref(K), C.byref(prm),
                                             out.ctypes.data))
        fn()
        assert out["tracked"].all()
        med = median_ms(fn, trk.stage_ms)
        line(med, what="track", mode=name, passes=1, poses=n, per_pose_ms=round(med[0] / n, 4))
trk.close()
ctx.close()
