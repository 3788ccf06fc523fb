"""Dev aid: what a verified answer for every instance costs, on a batch of 64 copies of the cluttered frame a (tests/clutter.py:
41 matches, three instances), frames by device pointer, warm, median of --reps calls of the host wall time, at {8, 48, 4} and
{8, 48, 1}:
  instances           fl_recognize_batch_instances, with its stage times (icp_ms includes group_ms);
  instances+verify    what a caller does today for a verified answer: that call, then fl_verify_batch on the picked poses;
  instances_verified  fl_recognize_batch_instances_verified, with its stage times and the device time of its verification
                      stage (fl_dev_instances_verify_ms: the fused render + score, then finish + pick).
The mesh is synth.object_mesh(2).  FEALESS_HIP_LIB may name an older build: only the lines it can run are printed."""
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
mesh = synth.object_mesh(2)
trk = api.Tracker(ctx, mesh["vertices"], mesh["triangles"], clutter.W, clutter.H, n, 8 * n, 1000)
d_b = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(bgr, (n,) + bgr.shape))).cuda()
d_d = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(depth, (n,) + depth.shape)).view(np.int16)).cuda()
torch.cuda.synchronize()
bptr = [d_b.data_ptr() + i * bgr.nbytes for i in range(n)]
dptr = [d_d.data_ptr() + i * depth.nbytes for i in range(n)]


def median_ms(fn):
    for _ in range(args.warmup):
        fn()
    t = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(statistics.median(t), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3), reps=args.reps)


def stages():
    t = det.stage_times()
    return {k: round(float(t[k]), 4) for k in ("total_ms", "icp_ms", "group_ms")}


for G, dist, h in ((8, 48, 4), (8, 48, 1)):
    def plain():
        return det.recognize_batch_instances(bptr, dptr, sc["K"], G, dist, h, mem=L.FL_MEM_DEVICE)

    def then_verify():
        got = plain()
        poses = np.stack([np.asarray(i["pose"], np.float32).reshape(4, 4) for f in got for i in f])
        fof = np.concatenate([np.full(len(f), k, np.int32) for k, f in enumerate(got)])
        return trk.verify(dptr_t, fof, poses, sc["K"])

    dptr_t = [d_d[i] for i in range(n)]
    shape = dict(frames=n, max_instances=G, min_dist_px=dist, hyp_per_instance=h)
    print(json.dumps(dict(shape, what="instances", **median_ms(plain), stage_ms=stages())), flush=True)
    if "fl_verify_batch" in L.SIGNATURES:
        v = then_verify()
        print(json.dumps(dict(shape, what="instances+verify", poses=len(v), **median_ms(then_verify), verify_stage_ms=trk.verify_ms())), flush=True)
    if "fl_recognize_batch_instances_verified" in L.SIGNATURES:
        def verified():
            return det.recognize_batch_instances_verified(trk, bptr, dptr, sc["K"], G, dist, h, mem=L.FL_MEM_DEVICE)
        got = verified()
        assert all(len(f) == 3 and all(i["verify"]["accepted"] for i in f) for f in got)
        med = median_ms(verified)
        print(json.dumps(dict(shape, what="instances_verified", **med, stage_ms=stages(), verify_ms=det.instances_verify_ms())), flush=True)
trk.close()
det.close()
ctx.close()
