"""CPU: the verified pick as the model states it (tests/verified_pick_model.py) on hand-made groups, and the argument lists
fl_recognize_batch_instances_verified refuses before its first device call, on a detector and a tracker without a device."""
import ctypes as C

import numpy as np
import pytest

import instances_model as M
import verified_pick_model as VP
import verify_model as VM
from fealess_amd import _lib as L
from fealess_amd import api


def _records(rows):
    """(accepted, n_inlier, n_model) per member."""
    r = np.zeros(len(rows), VM.DTYPE)
    for i, (acc, ni, nm) in enumerate(rows):
        r["accepted"][i], r["n_inlier"][i], r["n_model"][i] = acc, ni, nm
        if nm:
            r["inlier_ratio"][i] = np.float32(ni) / np.float32(nm)
    return r


# (found, records, nms, verified) -> (pick, best)
CASES = {
    "the best ratio wins, not the NMS pick": (([1, 1, 1], [(1, 50, 100), (1, 90, 100), (1, 70, 100)], 0, True), (1, 1)),
    "an exact tie goes to the earlier member": (([1, 1, 1], [(1, 30, 60), (1, 50, 100), (1, 1, 2)], 2, True), (0, 0)),
    "no accepted member: the NMS pick, no best": (([1, 1], [(0, 99, 100), (0, 98, 100)], 1, True), (1, -1)),
    "a member that was not found is passed over, whatever its record": (([0, 1], [(1, 100, 100), (1, 10, 100)], 1, True), (1, 1)),
    # both ratios are 0.33333334 as float32, where a tie would go to member 0; exactly, member 1's is larger
    "ratios equal as float32 but not exactly": (([1, 1], [(1, 5000002, 15000005), (1, 5000001, 15000002)], 0, True), (1, 1)),
    "products beyond 2^32": (([1, 1], [(1, 2 ** 31 - 2, 2 ** 31 - 1), (1, 2 ** 31 - 3, 2 ** 31 - 2)], 1, True), (0, 0)),
    "an empty group": (([], [], 0, True), (0, -1)),
    "a group of another class keeps the NMS pick": (([1, 1], [(1, 10, 100), (1, 90, 100)], 0, False), (0, -1)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_pick_model(name):
    (found, rows, nms, verified), exp = CASES[name]
    assert VP.pick(found, _records(rows), nms, verified) == exp


def test_float32_ratios_of_the_near_tie_are_equal():
    r = _records(CASES["ratios equal as float32 but not exactly"][0][1])
    assert r["inlier_ratio"][0] == r["inlier_ratio"][1] and 5000001 * 15000005 > 5000002 * 15000002


def test_nms_pick_model():
    assert VP.nms_pick([1, 1, 1], [1000, 900, 849], [0.5, 0.4, 0.1]) == 1         # 849 <= (int)(1000 * 0.85) = 850 is passed over
    assert VP.nms_pick([0, 0], [10, 10], [0.1, 0.1]) == 0 and VP.nms_pick([0, 1], [10, 10], [0.1, 0.2]) == 1


# ---- the refusals -------------------------------------------------------------------------------------------------------------
W, H = 640, 480


@pytest.fixture(scope="module")
def host():
    lib = L.load()
    det = api._host_only_detector(2, [5, 8])
    for b in M.small_banks():
        det.add_class(b)
    trk = C.c_void_p()
    assert L.dev(lib, "fl_dev_tracker_create_host")(W, H, 1, 4, 1000, C.byref(trk)) == 0 and trk.value
    yield lib, det, trk
    lib.fl_tracker_destroy(trk)
    det.close()


def _call(lib, det0, trk0, **over):
    a = dict(det=det0.h, trk=trk0, n_frames=1, K=(W, H, 608.0, 608.0, 320.0, 240.0), ip=(8, 48, 4), verify=(10, 1, 0.0, 0.0), class_idx=-1, vp=True,
             results=True)
    a.update(over)
    bgr, depth = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint16)
    bp, dp = (C.c_void_p * 1)(bgr.ctypes.data), (C.c_void_p * 1)(depth.ctypes.data)
    k = L.Intrinsics(*a["K"])
    p = L.RecognitionParams(75.0, 10, 0.5, 0.01, L.FL_ICP_PARITY)
    ip = L.InstanceParams(*a["ip"])
    vp = L.InstanceVerifyParams(L.VerifyParams(*a["verify"]), a["class_idx"], 0)
    out = np.full(8 * C.sizeof(L.VerifiedInstanceResult), 0xA5, np.uint8)
    cnt, drop = (C.c_int32 * 1)(-7), (C.c_int32 * 1)(-7)
    rc = lib.fl_recognize_batch_instances_verified(a["det"], a["trk"], a["n_frames"], bp, dp, L.FL_MEM_HOST, C.byref(k), C.byref(p), C.byref(ip),
                                                   C.byref(vp) if a["vp"] else None, out.ctypes.data if a["results"] else None, cnt, drop, None)
    return rc, bool((out == 0xA5).all()) and cnt[0] == -7 and drop[0] == -7, lib.fl_last_error(det0.ctx.h).decode()


NAN = float("nan")
REFUSED = {
    "tracker null": (dict(trk=None), "null tracker"), "vp null": (dict(vp=False), "null tracker"),
    "results null": (dict(results=False), None), "detector null": (dict(det=None), None), "n_frames 0": (dict(n_frames=0), None),
    "max_instances 0": (dict(ip=(0, 48, 4)), "fl_instance_params"), "hyp_per_instance 65": (dict(ip=(8, 48, 65)), "fl_instance_params"),
    "tau_mm -1": (dict(verify=(-1, 1, 0.0, 0.0)), "fl_verify_params"), "tau_mm 65536": (dict(verify=(65536, 1, 0.0, 0.0)), "fl_verify_params"),
    "min_model_px 0": (dict(verify=(10, 0, 0.0, 0.0)), "fl_verify_params"), "min_inlier_ratio nan": (dict(verify=(10, 1, NAN, 0.0)), "fl_verify_params"),
    "max_behind_ratio inf": (dict(verify=(10, 1, 0.0, float("inf"))), "fl_verify_params"),
    "fx 0 as a float": (dict(K=(W, H, 1e-60, 608.0, 320.0, 240.0)), "as floats"), "cy inf as a float": (dict(K=(W, H, 608.0, 608.0, 320.0, 1e300)), "as floats"),
    "fy nan": (dict(K=(W, H, 608.0, NAN, 320.0, 240.0)), "as floats"),
    "class_idx -2": (dict(class_idx=-2), "class_idx"), "class_idx = classes": (dict(class_idx=2), "class_idx"),
    "a tracker on another context": (dict(), "another context"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_before_any_device_call(host, name):
    """A detector and a tracker without a device: a call that reached HIP would not come back with FL_ERR_INVALID.  The tracker
    made by fl_dev_tracker_create_host owns a context of its own, so the otherwise valid call is itself refused, as a tracker
    on another context; the error text tells the refusals apart.  That each refusal is its own -- on a call that is accepted
    without it -- and the refusals of a tracker of another size or context are shown on the GPU
    (tests/test_gpu_instances_verified.py::test_each_refusal_is_its_own), where a tracker can share the detector's context."""
    lib, det, trk = host
    over, text = REFUSED[name]
    rc, untouched, err = _call(lib, det, trk, **over)
    assert rc == L.FL_ERR_INVALID and untouched, (name, rc, err)
    if text:
        assert text in err, (name, err)
