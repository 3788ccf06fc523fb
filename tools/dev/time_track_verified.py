"""Dev aid: what a trustworthy `tracked` costs -- fl_track_batch_verified against what a caller did before it, fl_track_batch
followed by fl_verify_batch of the poses it returned.  Frames of the object of tests/test_gpu_track.py's sequence (640 x 480,
noise and background on), one track per frame, each coming in with the previous frame's true pose, frames by device pointer,
point-to-plane, one pass, warm, median of --reps calls of the host wall time, for 1, 8 and 64 tracks:
  sequence        fl_track_batch, the poses of its records copied into a poses13 array, fl_verify_batch; with verify_fused 1 (the
                  kernel the new call runs) and 0 (render + score)
  track_verified  fl_track_batch_verified with keep_input 0 and 1, with the median device time of its stages: the passes'
                  (fl_dev_tracker_stage_ms) and fused / finish (fl_dev_tracker_track_verified_ms)
FEALESS_HIP_LIB may name an older build of the library: the entry points it lacks are skipped (only `sequence` is printed)."""
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
prm = L.TrackParams(12, 1, 10, 0.5, 0.01, L.FL_ICP_POINT_TO_PLANE, 0.0, 0.0)
for n in args.sizes:
    dp = (C.c_void_p * n)(*dptr[:n])
    fof = np.arange(n, dtype=np.int32)
    p13 = np.ascontiguousarray(poses_in[idx[:n]], np.float32)
    tout, vout, p_out = np.zeros(n, api.TRACK_DTYPE), np.zeros(n, api.VERIFY_DTYPE), np.zeros((n, 13), np.float32)

    def sequence():             # raw ctypes on both sides: the same host work per call
        ctx.check(trk.lib.fl_track_batch(trk.handle, n, dp, L.FL_MEM_DEVICE, n, fof.ctypes.data, p13.ctypes.data, C.byref(K), C.byref(prm),
                                         tout.ctypes.data))
        p_out[:, :12] = tout["pose"][:, :12]
        ctx.check(trk.lib.fl_verify_batch(trk.handle, n, dp, L.FL_MEM_DEVICE, n, fof.ctypes.data, p_out.ctypes.data, 0, None, C.byref(K), None,
                                          vout.ctypes.data))
    for fused in (1, 0):
        ctx.set_option("verify_fused", fused)
        sequence()
        assert tout["tracked"].all() and (vout["inlier_ratio"] > 0.9).all()
        med = median_ms(sequence, lambda: dict(trk.stage_ms(), **{"verify_" + k: v for k, v in trk.verify_ms().items()}))
        line(med, what="sequence", verify_fused=fused, tracks=n, per_track_ms=round(med[0] / n, 4))
    ctx.set_option("verify_fused", 0)
    if "fl_track_batch_verified" not in L.SIGNATURES:
        continue
    out = np.zeros(n, api.VERIFIED_TRACK_DTYPE)
    for keep in (0, 1):
        vp = L.TrackVerifyParams(L.VerifyParams(10, 1, 0.0, 0.0), keep, 0)

        def fn():
            ctx.check(trk.lib.fl_track_batch_verified(trk.handle, n, dp, L.FL_MEM_DEVICE, n, fof.ctypes.data, p13.ctypes.data, 0, None, C.byref(K),
                                                      C.byref(prm), C.byref(vp), out.ctypes.data))
        fn()
        assert out["track"]["tracked"].all() and out["verify"].tobytes() == vout.tobytes() and not out["kept_input"].any()
        med = median_ms(fn, lambda: dict(trk.stage_ms(), **trk.track_verified_ms()))
        line(med, what="track_verified", keep_input=keep, tracks=n, per_track_ms=round(med[0] / n, 4))
trk.close()
ctx.close()
