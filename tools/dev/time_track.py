"""Dev aid: what a pose per frame costs -- recognised from scratch, or tracked.  Frames of the object of tests/test_gpu_track.py's
sequence (640 x 480, noise and background on), one object per frame, frames by device pointer, warm, median of --reps calls
of the host wall time, for 1, 8 and 64 frames:
  recognize  fl_recognize_batch on a 2000-template bank (views of the object around the sequence's poses + random templates):
             front-end, scan, refinement and ICP per frame -- what a caller does without the tracker;
  track      fl_track_batch, one track per frame, in FL_ICP_PARITY and FL_ICP_POINT_TO_PLANE with passes 1 and 2, with the
             device time of the last call by stage (copy, render, rects, ICP, finish; fl_dev_tracker_stage_ms).
FEALESS_HIP_LIB may name an older build of the library: the entry points it lacks are skipped (only `recognize` is printed)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (runtime load order, see tests/conftest.py)
from fealess_amd import _lib as L  # noqa: E402

_probe = C.CDLL(L.LIB_PATH)
for _name in [n for n in L.SIGNATURES if not hasattr(_probe, n)]:      # an older build: bind what it has
    del L.SIGNATURES[_name]
from fealess_amd import api, synth  # noqa: E402
from fealess_amd.bank import TemplateBank  # noqa: E402
import oracle_py as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--templates", type=int, default=2000)
ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64])
args = ap.parse_args()

W, H, K0 = 640, 480, (608.0, 608.0, 320.0, 240.0)
MOTION_T, MOTION_A = (4.0, -2.0, 3.0), (0.02, -0.01, 0.015)


def gt(k):
    return synth.object_pose(10 + MOTION_T[0] * k, -5 + MOTION_T[1] * k, 720.0 + MOTION_T[2] * k, 0.3 + MOTION_A[0] * k, 0.35 + MOTION_A[1] * k,
                             0.1 + MOTION_A[2] * k)


def median_ms(fn):
    for _ in range(args.warmup):
        fn()
    t = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def line(name, n, fn, **extra):
    med, lo, hi = median_ms(fn)
    print(json.dumps(dict(what=name, frames=n, reps=args.reps, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
                          per_frame_ms=round(med / n, 4), **extra)), flush=True)


n_max = max(args.sizes)
# frames 1 .. 6 of the sequence, repeated; a track comes in with the previous frame's true pose
frames = [synth.render(W, H, *gt(k), seed=100 + k) for k in range(1, 7)]
poses_in = np.stack([synth.pose13(*gt(k - 1)) for k in range(1, 7)])
idx = np.arange(n_max) % 6
d_d = torch.from_numpy(np.stack([frames[i][0] for i in idx]).view(np.int16)).cuda()
d_b = torch.from_numpy(np.stack([frames[i][1] for i in idx])).cuda()
torch.cuda.synchronize()
dptr = [d_d.data_ptr() + i * W * H * 2 for i in range(n_max)]
bptr = [d_b.data_ptr() + i * W * H * 3 for i in range(n_max)]

ctx = api.Context(0)
# the bank: a view of the object near every frame of the sequence, padded with random templates
bank = TemplateBank("obj", 2, 2)
for k in range(1, 7):
    R, t = gt(k)
    out = synth.rendered_template(lambda b, d, l: O.quantize_pyramid(b, d, l), synth.rot_z(0.02) @ R, t + np.array([6.0, -4.0, 3.0]), 2, W, H, seed=k)
    assert out is not None
    bank.add_pyramid(*out)
rng = np.random.default_rng(1)
for _ in range(args.templates - bank.n_pyramids):
    bank.add_pyramid(synth.random_pyramid(rng, 2, 2, W, H), None, None)
det = api.Detector(ctx, 2, [5, 8])
det.add_class(bank)
det.finalize(W, H, max_batch=n_max)
K = L.Intrinsics(W, H, *K0)
P = L.RecognitionParams(75.0, 10, 0.5, 0.01, L.FL_ICP_PARITY)
for n in args.sizes:
    bp, dp = (C.c_void_p * n)(*bptr[:n]), (C.c_void_p * n)(*dptr[:n])
    res = (L.RecognitionResult * n)()

    def reco():
        ctx.check(det.lib.fl_recognize_batch(det.h, n, bp, dp, L.FL_MEM_DEVICE, C.byref(K), C.byref(P), res))
    reco()
    found = sum(res[i].found for i in range(n))
    line("recognize", n, reco, templates=bank.n_pyramids, found=found,
         stage_ms={k: round(float(v), 4) for k, v in det.stage_times().items() if k.endswith("_ms")})
det.close()

if "fl_track_batch" in L.SIGNATURES:
    mesh = synth.object_mesh(2)
    trk = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], W, H, n_max, n_max, 40000)
    for n in args.sizes:
        dp = (C.c_void_p * n)(*dptr[:n])
        fof = np.arange(n, dtype=np.int32)
        p13 = np.ascontiguousarray(poses_in[idx[:n]], np.float32)
        out = np.zeros(n, api.TRACK_DTYPE)
        for mode, name in ((L.FL_ICP_PARITY, "parity"), (L.FL_ICP_POINT_TO_PLANE, "point_to_plane")):
            for passes in (1, 2):
                prm = L.TrackParams(12, passes, 10, 0.5, 0.01, mode, 0.0, 0.0)

                def fn():           # raw ctypes like reco: the same host work on both sides
                    ctx.check(trk.lib.fl_track_batch(trk.handle, n, dp, L.FL_MEM_DEVICE, n, fof.ctypes.data, p13.ctypes.data, C.byref(K), C.byref(prm),
                                                     out.ctypes.data))
                fn()
                assert out["tracked"].all()
                med = median_ms(fn)
                st = trk.stage_ms()
                print(json.dumps(dict(what="track", mode=name, passes=passes, frames=n, reps=args.reps, median_ms=round(med[0], 3), min_ms=round(med[1], 3),
                                      max_ms=round(med[2], 3), per_frame_ms=round(med[0] / n, 4), crop_px=int(out["rect_model"][0][2] * out["rect_model"][0][3]),
                                      icp_iters=int(out["det"]["icp"]["iters"].sum()), stage_ms={k: round(v, 4) for k, v in st.items()})), flush=True)
    trk.close()
ctx.close()
