"""The argument refusals of the facade's mesh calls -- cadreco_track, cadreco_verify, cadreco_verify_tagged, cadreco_arbitrate --
through one table of cases on one handle: every refusal returns ERROR_INVALID_PARAM, leaves the caller's buffers alone and
leaves the handle usable.  Every case is an argument check on the host; the one kernel work is the good call at the end."""
import ctypes as C

import numpy as np
import pytest

import cadreco_py as CR
from fealess_amd import synth

pytestmark = pytest.mark.gpu

INVALID = CR.INVALID
K0, W, H = (608.0, 608.0, 320.0, 240.0), 640, 480
ENTRIES = ("cadreco_track", "cadreco_verify", "cadreco_verify_tagged", "cadreco_arbitrate")
SENTINEL, CAP, NAN = -7, 17, float("nan")


def _call(h, entry, depth, n=1, ts=0.0, tag=b"box", tau=10.0, ratio=0.5, frame=None):
    """One call of `entry` on n copies of the pose, the outputs filled with SENTINEL beforehand.  Returns the code, and checks
    what a call that is not SUCCESS must leave behind."""
    pose = np.eye(4, dtype=np.float32)
    pose[2, 3] = 700.0
    poses = np.tile(pose.reshape(16), (CAP, 1))
    before = poses.copy()
    out = np.full(CAP * 11, SENTINEL, np.int32)
    tags = (C.c_char_p * CAP)(*([tag] * CAP))
    f = frame if frame is not None else CR.frame_args(depth, ts, K0)
    rest = {"cadreco_track": (), "cadreco_verify": (tau,), "cadreco_verify_tagged": (tags, tau), "cadreco_arbitrate": (tags, tau, ratio)}[entry]
    rc = getattr(CR.lib(), entry)(h, *f, n, poses.ctypes.data, *rest, out.ctypes.data)
    if rc != 0 or n == 0:
        assert poses.tobytes() == before.tobytes(), entry
        written = n if entry == "cadreco_track" else 0                               # CadRecoTrack reports every entry as lost
        assert not out[:written].any() and (out[written:] == SENTINEL).all(), entry
    return rc


def test_refusals_leave_the_buffers_and_the_handle_alone(tmp_path):
    lib = CR.lib()
    bv, bn, bt = synth.box_mesh(np.zeros(3), np.array([55.0, 35.0, 25.0]))
    box = str(tmp_path / "box.obj")
    synth.write_obj(box, dict(vertices=np.array(bv, np.float32), normals=np.array(bn, np.float32), triangles=np.array(bt, np.int32)))
    depth = np.full((H, W), 675, np.uint16)                                          # the box's front face at 700 - 25 mm
    with CR.handle() as h:
        for e in ENTRIES:
            assert _call(h, e, depth) == INVALID, e                                  # no mesh set yet
        assert lib.cadreco_set_tracking_mesh(h, box.encode(), 1.0) == 0
        for e in ENTRIES:
            assert _call(h, e, np.zeros((240, 320), np.uint16)) == INVALID, e                                  # a 320 x 240 frame
            assert _call(h, e, None, frame=(None, W, H, 0.0, *K0)) == INVALID, e     # a null depth pointer
            assert _call(h, e, depth, ts=-1.0) == INVALID, e                         # a negative timestamp
            assert _call(h, e, depth, n=17) == INVALID, e                            # more than FEALESS_TRACK_MAX_OBJECTS
            assert _call(h, e, depth, n=0) == 0, e                                   # nothing to do, nothing written
            if e != "cadreco_track":
                for tau in (-1.0, 65536.0, NAN):
                    assert _call(h, e, depth, tau=tau) == INVALID, (e, tau)
        for ratio in (0.0, 1.5, NAN):
            assert _call(h, "cadreco_arbitrate", depth, ratio=ratio) == INVALID, ratio
        # a tag with no mesh: the untagged entries carry the empty tag
        assert lib.cadreco_set_tracking_meshes(h, 1, (C.c_char_p * 1)(b"box"), (C.c_char_p * 1)(box.encode()), 1.0) == 0
        for e in ENTRIES:
            assert _call(h, e, depth, tag=b"sphere") == INVALID, e
        # the handle is still good: one mesh for every tag again, and one call that works per entry point
        assert lib.cadreco_set_tracking_mesh(h, box.encode(), 1.0) == 0
        for e in ENTRIES:
            assert _call(h, e, depth) == 0, e
