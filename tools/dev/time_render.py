"""Dev aid: time per view of fl_render_views at 640x480 (device outputs: kernel work only, no read-back) for 64 / 256 /
1024 views on three meshes -- synth.object_mesh() (5132 triangles), a subdivision-7 icosphere (327 680 small triangles)
and a 12-triangle box that fills most of the image -- and of render -> fl_extract_template_batch from device memory
against the same extraction from host images.  --mesh NAME --views N [--reps R]: only R renders of one batch (for a
rocprofv3 --kernel-trace run)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (runtime load order, see tests/conftest.py)
from fealess_amd import _lib as L  # noqa: E402
from fealess_amd import api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mesh", default="")
ap.add_argument("--views", type=int, default=0)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

K = (synth.FX, synth.FY, synth.CX, synth.CY)
W, H = 640, 480


def meshes():
    m = synth.object_mesh()
    sv, sf = synth.icosphere(7)
    box = synth.object_mesh(0)                                      # its last 12 triangles are the box; scale it up
    bt = box["triangles"][-12:]
    bv = (box["vertices"] - np.array([45.0, 0.0, 10.0], np.float32)) * 4.0
    return {"object": (m["vertices"], m["triangles"], m["normals"], m["colors"]),
            "icosphere7": ((sv * 90.0).astype(np.float32), sf, sv.astype(np.float32), None),
            "box12": (bv.astype(np.float32), bt, box["normals"], None)}


ctx = api.Context(0)
M = meshes()
P_all = api.view_sphere(3, [600.0, 700.0], n_inplane=3, inplane_deg=10.0)           # 642 points x 2 x 3 = 3852 views


def render(name, n, out):
    V, T, N, Cc = M[name]
    ctx.render_views(V, T, P_all[:n], K, W, H, normals=N, colors=Cc, mem=L.FL_MEM_DEVICE, out=out)


def bufs(n):
    return dict(bgr=torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda"), depth=torch.empty((n, H, W), dtype=torch.int16, device="cuda"),
                mask=torch.empty((n, H, W), dtype=torch.uint8, device="cuda"))


if args.mesh:
    out = bufs(args.views)
    torch.cuda.synchronize()
    for _ in range(args.reps + 1):
        render(args.mesh, args.views, out)
    ctx.synchronize()
    sys.exit(0)

for name in M:
    for n in (64, 256, 1024):
        out = bufs(n)
        torch.cuda.synchronize()
        render(name, n, out)
        ctx.synchronize()
        reps = max(2, 1024 // n)
        t0 = time.perf_counter()
        for _ in range(reps):
            render(name, n, out)
        ctx.synchronize()
        print(f"render {name:11s} {n:5d} views {(time.perf_counter() - t0) / (reps * n) * 1e3:8.4f} ms per view", flush=True)
        del out

# render -> extract, 64 views of the object: from device memory, and from host copies of the same images
n = 64
out = bufs(n)
torch.cuda.synchronize()
render("object", n, out)
ctx.synchronize()
hb, hd, hm = out["bgr"].cpu().numpy(), out["depth"].cpu().numpy().view(np.uint16), out["mask"].cpu().numpy()


def dev():
    render("object", n, out)
    return ctx.extract_template_batch([out["bgr"][v] for v in range(n)], [out["depth"][v] for v in range(n)],
                                      [out["mask"][v] for v in range(n)], 2, mem=L.FL_MEM_DEVICE)


def host():
    return ctx.extract_template_batch(list(hb), list(hd), list(hm), 2)


a, b = dev(), host()
assert all((x is None) == (y is None) for x, y in zip(a, b))
for label, fn in (("render + extract, device", dev), ("extract from host images", host)):
    t0 = time.perf_counter()
    for _ in range(4):
        fn()
    print(f"{label:28s} {n} views {(time.perf_counter() - t0) / (4 * n) * 1e3:8.4f} ms per view", flush=True)
