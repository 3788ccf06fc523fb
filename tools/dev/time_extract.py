"""Dev aid: wall time per training view of template extraction (Detector::addTemplate) at 640x480, two levels, with masks:
fl_extract_template_pyramid one view at a time, fl_extract_template_batch at 1 / 16 / 64 / 256 views, and the CPU oracle.
--batch N [--reps R]: only R calls of one N-view batch (for a rocprofv3 --kernel-trace run)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401,E402  (runtime load order, see tests/conftest.py)
from fealess_amd import api, synth  # noqa: E402
import oracle_py as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=0)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

ctx = api.Context(0)
N_DISTINCT = 32
views = []
rng = np.random.default_rng(5)
for s in range(N_DISTINCT):
    R, t = synth.object_pose(tx=float(rng.uniform(-60, 60)), ty=float(rng.uniform(-40, 40)), tz=float(rng.uniform(520, 700)),
                             yaw=float(rng.uniform(-1, 1)), tilt=float(rng.uniform(0.1, 0.6)))
    d, b, m = synth.render(640, 480, R, t, seed=s, noise=False)
    views.append((np.ascontiguousarray(b), np.ascontiguousarray(d), (m * 255).astype(np.uint8)))


def batch(n):
    vs = [views[k % N_DISTINCT] for k in range(n)]
    return ctx.extract_template_batch([v[0] for v in vs], [v[1] for v in vs], [v[2] for v in vs], 2)


def per_view_ms(fn, n_views, reps):
    fn()                                                                       # warm-up: code objects, scratch, pinned memory
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / (reps * n_views) * 1e3


if args.batch:
    batch(args.batch)
    for _ in range(args.reps):
        batch(args.batch)
    sys.exit(0)

single = [ctx.extract_template_pyramid(v[0], v[1], v[2], 2) for v in views]
got = batch(N_DISTINCT)
assert all((a is None) == (b is None) for a, b in zip(single, got))
rows = [("single-view loop (64 calls)", per_view_ms(lambda: [ctx.extract_template_pyramid(*views[k % N_DISTINCT], 2) for k in range(64)], 64, 3))]
for n in (1, 16, 64, 256):
    rows.append((f"batch of {n}", per_view_ms(lambda: batch(n), n, max(3, 256 // n))))
rows.append(("CPU oracle (8 views)", per_view_ms(lambda: [O.add_template(*views[k], 2) for k in range(8)], 8, 1)))
for name, ms in rows:
    print(f"{name:32s} {ms:8.3f} ms per view", flush=True)
