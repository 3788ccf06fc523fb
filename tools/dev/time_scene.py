"""Dev aid: what the arbitration adds to a verification.  70 poses at 640 x 480 in 7 scenes of 10 -- per frame one object and ten
hypotheses on it: the four meshes of tests/meshes.py at and near the true pose, one 150 mm off -- through Tracker.verify_scene
and, in the same process and alternating with it, through Tracker.verify with verify_fused = 0.  Frames by host pointer, warm,
the median (and min, max) over --reps calls of the device time by stage: fl_dev_tracker_scene_ms {copy, render, score, finish,
overlap, pick} and fl_dev_tracker_verify_ms {copy, render, score, finish}.  One JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (runtime load order, see tests/conftest.py)
from fealess_amd import api, synth  # noqa: E402
import meshes as MS  # noqa: E402
from util import p13, pose  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()

W, H, K = 640, 480, (608.0, 608.0, 320.0, 240.0)
OBJECTS = [(10, -5, 720, .30, .35, .10), (-60, 30, 690, -.5, .2, .3), (80, -40, 750, .9, .5, -.2), (-150, 60, 700, .1, .4, 0), (120, 70, 680, -.3, .3, .2),
           (0, 0, 760, .6, .25, .1), (-90, -70, 710, -.8, .45, -.1)]
NAMES = "AABCAABCDA"
OFFSETS = [((0, 0, 0), (0, 0, 0)), ((3, -2, 2), (.01, 0, 0)), ((0, 0, 0), (0, 0, 0)), ((0, 0, 0), (0, 0, 0)), ((-4, 3, -2), (0, .01, 0)),
           ((8, 0, 3), (0, 0, .02)), ((2, 2, 0), (0, 0, 0)), ((1, 0, 1), (0, 0, 0)), ((0, 0, 0), (0, 0, 0)), ((150, 0, 0), (0, 0, 0))]

ctx = api.Context(0)
ctx.set_option("verify_fused", 0)
trk = api.Tracker(ctx, meshes=MS.in_order(MS.all_meshes()), w=W, h=H, max_frames=7, max_tracks=70, max_crop_px=40000)
scenes = [synth.render(W, H, *pose(p), seed=30 + i)[0] for i, p in enumerate(OBJECTS)]
frame_of = np.repeat(np.arange(7), 10).astype(np.int32)
poses = np.stack([p13(OBJECTS[f], OFFSETS[k % 10]) for k, f in enumerate(frame_of)])
mesh_of = np.array([MS.INDEX[NAMES[k % 10]] for k in range(70)], np.int32)
scene_first = np.arange(0, 71, 10, dtype=np.int32)
scene, verify = [], []
for it in range(args.warmup + args.reps):
    got = trk.verify_scene(scenes, frame_of, poses, K, scene_first, mesh_of=mesh_of)
    s = trk.scene_ms()
    rec = trk.verify(scenes, frame_of, poses, K, mesh_of=mesh_of)
    v = trk.verify_ms()
    assert got["verify"].tobytes() == rec.tobytes()
    if it >= args.warmup:
        scene.append(s)
        verify.append(v)


def stats(rows):
    return {k: [round(f([r[k] for r in rows]), 4) for f in (statistics.median, min, max)] for k in rows[0]}


shared = trk.dev_scene_shared()
out = dict(what="scene", poses=70, scenes=7, reps=args.reps, pairs=len(shared), pairs_sharing=int((shared > 0).sum()),
           accepted=int(got["verify"]["accepted"].sum()), kept=int(got["kept"].sum()), scene_stage_ms=stats(scene), verify_stage_ms=stats(verify))
out["scene_total_ms"] = round(sum(v[0] for v in out["scene_stage_ms"].values()), 4)
out["verify_total_ms"] = round(sum(v[0] for v in out["verify_stage_ms"].values()), 4)
print(json.dumps(out), flush=True)
trk.close()
ctx.close()
