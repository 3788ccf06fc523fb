"""Dev aid: what depth registration costs per frame (fl_register_depth_batch).  Frames of the object of tests/test_gpu_track.py's
sequence (640 x 480, noise and background on) taken as the depth camera's (K = 580 / 580 / 318 / 242), registered to the colour
camera 608 / 608 / 320 / 240 at rotation vector (0.004, -0.006, 0.003) rad and t = (25, -1, 2) mm, 640 x 480 -> 640 x 480.  Frames
by device pointer, every frame and every output a buffer of its own, warm, median of --reps calls of the DEVICE time of one call
(events on the context's stream around it), for --sizes frames, with fill_cracks 0 and 1.  Per line: the time per frame, the bytes
a frame needs (2 wd hd + 2 wc hc), the bytes the clear and the two kernels move (the depth frame read, the 4-byte z-buffer cleared,
updated by one atomic per landed pixel and read back, the output written), and the needed bytes per second against the 8 TB/s
HBM peak."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (runtime load order, see tests/conftest.py)
from fealess_amd import _lib as L  # noqa: E402
from fealess_amd import api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--sizes", type=int, nargs="+", default=[1, 64, 4096])
args = ap.parse_args()

W, H = 640, 480
K_DEPTH, K_COLOR = (W, H, 580.0, 580.0, 318.0, 242.0), (W, H, 608.0, 608.0, 320.0, 240.0)
RVEC, T = np.array([0.004, -0.006, 0.003]), np.array([25.0, -1.0, 2.0], np.float32)
HBM_PEAK = 8.0e12
MOTION_T, MOTION_A = (4.0, -2.0, 3.0), (0.02, -0.01, 0.015)


def rodrigues(r):
    th = float(np.linalg.norm(r))
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)).astype(np.float32)


def gt(k):
    return synth.object_pose(10 + MOTION_T[0] * k, -5 + MOTION_T[1] * k, 720.0 + MOTION_T[2] * k, 0.3 + MOTION_A[0] * k, 0.35 + MOTION_A[1] * k,
                             0.1 + MOTION_A[2] * k)


n_max = max(args.sizes)
frames = np.stack([synth.render(W, H, *gt(k), seed=100 + k)[0] for k in range(1, 7)])
ctx = api.Context(0)
dev = f"cuda:{ctx.device}"
d_in = torch.from_numpy(frames.view(np.int16)).to(dev)[torch.arange(n_max, device=dev) % 6].contiguous()      # n_max frames, each its own memory
d_out = torch.empty((n_max, H, W), dtype=torch.int16, device=dev)
torch.cuda.synchronize()
stream = torch.cuda.Stream(device=dev)        # the context queues on a torch stream, so that torch events bound a call (as fealess_amd/bench_sharded.py does)
ctx.set_stream(stream.cuda_stream)
kd, kc = L.Intrinsics(*K_DEPTH), L.Intrinsics(*K_COLOR)
ext = L.Extrinsics((C.c_float * 9)(*rodrigues(RVEC).ravel()), (C.c_float * 3)(*T))
px = W * H
for n in args.sizes:
    ip = (C.c_void_p * n)(*[d_in.data_ptr() + i * px * 2 for i in range(n)])
    op = (C.c_void_p * n)(*[d_out.data_ptr() + i * px * 2 for i in range(n)])
    for fill in (0, 1):
        prm = L.RegisterParams(fill)

        def call():
            ctx.check(ctx.lib.fl_register_depth_batch(ctx.h, n, ip, L.FL_MEM_DEVICE, C.byref(kd), C.byref(kc), C.byref(ext), C.byref(prm), op))

        for _ in range(args.warmup):
            call()
        ctx.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        out = d_out[:min(n, 6)].cpu().numpy().view(np.uint16)
        landed = int((frames[:min(n, 6)] != 0).sum()) / min(n, 6)          # source pixels with a measurement: about one atomic each
        assert (out != 0).mean() > 0.9                                        # it registered something
        med = statistics.median(ms)
        needed = 2 * px + 2 * px
        moved = 2 * px + 4 * px + 4 * landed + 4 * px + 2 * px
        per_frame_us = med * 1e3 / n
        print(json.dumps(dict(what="register", frames=n, fill_cracks=fill, reps=args.reps, median_ms=round(med, 4), min_ms=round(min(ms), 4),
                              max_ms=round(max(ms), 4), per_frame_us=round(per_frame_us, 3), frames_per_s=round(n / (med * 1e-3)),
                              needed_bytes=needed, moved_bytes=int(moved), needed_gb_s=round(needed / (per_frame_us * 1e-6) / 1e9, 1),
                              hbm_peak_fraction=round(needed / (per_frame_us * 1e-6) / HBM_PEAK, 4))), flush=True)
ctx.close()
