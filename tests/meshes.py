"""The four meshes of the several-meshes-on-one-tracker tests (tests/test_meshes_cpu.py, tests/test_gpu_meshes.py), all from
fealess_amd/synth.py, and the order they go on a tracker in: B, D, C, A -- the largest is not mesh 0 and a small one sits
between large ones.

  A  synth.object_mesh(2)      332 triangles   the sphere-and-box object the scenes show
  B  its box alone             12 triangles    fewer triangles than a wave's share of a fused round
  C  icosphere(3) * 60         1280 triangles  more than the fused kernel's 1024 triangles per round
  D  one triangle              1 triangle      n_t = 1
"""
import numpy as np

from fealess_amd import synth


def _mesh(v, t):
    return dict(vertices=np.ascontiguousarray(v, np.float32).reshape(-1, 3), triangles=np.ascontiguousarray(t, np.int32).reshape(-1, 3))


def mesh_a():
    m = synth.object_mesh(2)
    return _mesh(m["vertices"], m["triangles"])


def mesh_b():
    bv, _, bt = synth.box_mesh(np.array([45.0, 0.0, 10.0]), np.array([55.0, 35.0, 25.0]))
    return _mesh(np.array(bv), np.array(bt))


def mesh_c():
    v, f = synth.icosphere(3)
    return _mesh(v * 60.0, f)


def mesh_d():
    return _mesh([[-40.0, -30.0, 0.0], [40.0, -30.0, 0.0], [0.0, 40.0, 0.0]], [[0, 1, 2]])


ORDER = "BDCA"                                   # the tracker's meshes 0..3
INDEX = {name: i for i, name in enumerate(ORDER)}
N_TRIANGLES = dict(A=332, B=12, C=1280, D=1)


def all_meshes():
    """name -> mesh dict (vertices f32 (n, 3), triangles i32 (m, 3))."""
    return dict(A=mesh_a(), B=mesh_b(), C=mesh_c(), D=mesh_d())


def in_order(meshes):
    """[(vertices, triangles), ...] as api.Tracker(meshes=...) takes them, in ORDER."""
    return [(meshes[n]["vertices"], meshes[n]["triangles"]) for n in ORDER]
