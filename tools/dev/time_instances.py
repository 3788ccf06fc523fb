"""Dev aid: wall time of getting every instance out of a batch of 64 copies of the cluttered frame a (tests/clutter.py: 41
matches, three instances), frames by device pointer, warm, median of --reps calls:
  topk+nms   fl_recognize_batch_topk(k = 41, every match refined) + fl_nms per frame: the way without the grouping;
  instances  fl_recognize_batch_instances {8, 48, 4} and {8, 48, 1}, with the stage times of the last call
             (group_ms: the grouping and the pick kernel).
On a tree without fl_recognize_batch_instances only the first line is printed."""
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
from fealess_amd import api  # noqa: E402
from fealess_amd import _lib as L  # noqa: E402
import clutter  # noqa: E402
import oracle_py as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

sc = clutter.build(O)
bgr, depth = sc["frames"]["a"]
n = args.frames
ctx = api.Context(0)
det = api.Detector(ctx, 2, clutter.T)
det.add_class(sc["bank"])
det.finalize(clutter.W, clutter.H, max_batch=n)
d_b = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(bgr, (n,) + bgr.shape))).cuda()
d_d = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(depth, (n,) + depth.shape)).view(np.int16)).cuda()
torch.cuda.synchronize()
bptr = [d_b.data_ptr() + i * bgr.nbytes for i in range(n)]
dptr = [d_d.data_ptr() + i * depth.nbytes for i in range(n)]
bp, dp = (C.c_void_p * n)(*bptr), (C.c_void_p * n)(*dptr)
K = L.Intrinsics(clutter.W, clutter.H, *sc["K"])
P = L.RecognitionParams(75.0, 10, 0.5, 0.01, L.FL_ICP_PARITY)
TOPK = 41


def topk_nms():
    res = (L.RecognitionResult * (n * TOPK))()
    cnt = (C.c_int * n)()
    ctx.check(det.lib.fl_recognize_batch_topk(det.h, n, bp, dp, L.FL_MEM_DEVICE, C.byref(K), C.byref(P), TOPK, res, cnt))
    win, nw, out = (C.c_int * TOPK)(), C.c_int(0), []
    for f in range(n):
        ctx.check(det.lib.fl_nms(C.byref(res, f * TOPK * C.sizeof(L.RecognitionResult)), cnt[f], 60.0, win, C.byref(nw)))
        out.append([int(win[i]) for i in range(nw.value)])
    return out


def median_ms(fn):
    for _ in range(args.warmup):
        fn()
    t = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def line(name, fn, **extra):
    med, lo, hi = median_ms(fn)
    print(json.dumps(dict(what=name, frames=n, reps=args.reps, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), **extra)), flush=True)


w = topk_nms()
assert all(len(x) == 3 for x in w), w[0]
line("topk41+nms", topk_nms, icp_jobs_per_frame=TOPK, winners=w[0])
if hasattr(det.lib, "fl_recognize_batch_instances"):
    G = 8
    for hyp in (4, 1):
        ip = L.InstanceParams(G, 48, hyp)
        res, cnt, drop = (L.InstanceResult * (n * G))(), (C.c_int32 * n)(), (C.c_int32 * n)()

        def fn():               # raw ctypes like topk_nms: the same host work on both sides
            ctx.check(det.lib.fl_recognize_batch_instances(det.h, n, bp, dp, L.FL_MEM_DEVICE, C.byref(K), C.byref(P), C.byref(ip), res, cnt, drop))
        fn()
        assert all(cnt[f] == 3 for f in range(n))
        med = median_ms(fn)
        st = det.stage_times()
        print(json.dumps(dict(what="instances{8,48,%d}" % hyp, frames=n, reps=args.reps, median_ms=round(med[0], 3), min_ms=round(med[1], 3),
                              max_ms=round(med[2], 3), icp_jobs_per_frame=sum(res[g].n_refined for g in range(3)), ranks=[res[g].rank for g in range(3)],
                              stage_ms={k: round(float(v), 4) for k, v in st.items() if k.endswith("_ms")})), flush=True)
det.close()
ctx.close()
