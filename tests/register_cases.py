"""The two-camera scene the registration tests share (tests/test_register_cpu.py, tests/test_gpu_register.py), rendered with
tests/raster_model.py; computed once per process and read only."""
import functools

import numpy as np

import raster_model as RM
import register_model as GM
from fealess_amd import synth

W, H = 640, 480
K_DEPTH = (W, H, 580.0, 580.0, 318.0, 242.0)
K_COLOR = (W, H, 608.0, 608.0, 320.0, 240.0)
K_DEPTH_HALF = (320, 240, 290.0, 290.0, 159.0, 121.0)
RVEC, T = (0.004, -0.006, 0.003), (25.0, -1.0, 2.0)          # depth camera -> colour camera: rad, mm


@functools.lru_cache(maxsize=None)
def extrinsics():
    """(R (3, 3) f32, t (3,) f32): X_colour = R X_depth + t."""
    return GM.rodrigues(RVEC).astype(np.float32), np.array(T, np.float32)


@functools.lru_cache(maxsize=None)
def scene():
    """synth.object_mesh(3) at synth.object_pose() in the DEPTH camera's frame, in front of a slanted backdrop quad from z = 1000
    to 1300 mm.  Returns dict(mesh: the object alone; pose13_color: its pose in the colour camera; depth_cam, depth_cam_half:
    the depth camera's renders at 640 x 480 and 320 x 240; color_cam: the colour camera's render, what registration aims at)."""
    mesh = synth.object_mesh(3)
    Ro, to = synth.object_pose()
    Vo = (mesh["vertices"].astype(np.float64) @ Ro.T + to).astype(np.float32)
    quad = np.array([[-1400, -1000, 1000], [1400, -1000, 1300], [1400, 1000, 1300], [-1400, 1000, 1000]], np.float32)
    n = len(Vo)
    V = np.concatenate([Vo, quad])
    Tr = np.concatenate([mesh["triangles"], np.array([[n, n + 1, n + 2], [n, n + 2, n + 3]], np.int32)])
    R, t = extrinsics()
    eye = synth.pose13(np.eye(3), np.zeros(3))
    to_color = synth.pose13(R.astype(np.float64), t.astype(np.float64))
    Rd, td = R.astype(np.float64), t.astype(np.float64)
    out = dict(mesh=dict(vertices=mesh["vertices"], triangles=mesh["triangles"]), pose13_color=synth.pose13(Rd @ Ro, Rd @ to + td),
               depth_cam=RM.render_view(V, Tr, eye, K_DEPTH[2:], W, H)[1], depth_cam_half=RM.render_view(V, Tr, eye, K_DEPTH_HALF[2:], 320, 240)[1],
               color_cam=RM.render_view(V, Tr, to_color, K_COLOR[2:], W, H)[1])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def compare(registered, direct):
    """The figures of a registered frame against the direct render of the colour camera: dict(both: pixels where both have depth,
    within2: those within 2 mm, empty: pixels empty where the direct render has depth, isolated: those of them whose four
    neighbours all have depth in the registered frame)."""
    r, d = registered.astype(np.int64), direct.astype(np.int64)
    both = (r != 0) & (d != 0)
    empty = (r == 0) & (d != 0)
    full = np.zeros_like(empty)
    full[1:-1, 1:-1] = (r[1:-1, :-2] != 0) & (r[1:-1, 2:] != 0) & (r[:-2, 1:-1] != 0) & (r[2:, 1:-1] != 0)
    return dict(both=int(both.sum()), within2=int((both & (np.abs(r - d) <= 2)).sum()), empty=int(empty.sum()), isolated=int((empty & full).sum()),
                direct=int((d != 0).sum()))
