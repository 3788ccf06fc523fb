"""fl_recognize_submit with two batches in flight (option pipeline_icp): the ICP stage of batch i runs on the context's ICP
stream beside the LINEMOD stages of batch i+1.  What ICP(i) reads of a frame workspace -- the counters and the sorted match
list -- exists twice, so batch i+1 must not disturb it; fl_recognize_collect_previous hands batch i over while batch i+1 is
still running.  Frames a - d of tests/clutter.py; every result is compared with the ORACLE's Recognition() bit for bit
(test_gpu_clutter.py's checks), never with the serial path alone.

Batches X, Y and Z are cyclic shifts of (a, b, c, d), tiled over the batch: every slot holds a different frame, with a
different found / not-found pattern, in consecutive batches.  A result that leaked from a neighbouring batch cannot pass."""
import numpy as np
import pytest

import clutter
from fealess_amd import api
from fealess_amd import _lib as L
from test_gpu_clutter import PARAMS, _assert_matches_equal, _assert_reco_equal, _bits, _detector
from util import options as _options

pytestmark = pytest.mark.gpu

NF = len(clutter.FRAMES)
SHIFTS = (0, 1, 2)                       # X, Y, Z: slot i holds frame (i + shift) % 4
PIPELINE_VALUES = (0, 1, 2, 3)
PX = clutter.W * clutter.H


@pytest.fixture(scope="module")
def scene(oracle):
    sc = clutter.build(oracle)
    sc["bgrs"] = [np.ascontiguousarray(sc["frames"][f][0], np.uint8) for f in clutter.FRAMES]
    sc["depths"] = [np.ascontiguousarray(sc["frames"][f][1], np.uint16) for f in clutter.FRAMES]
    return sc


@pytest.fixture(scope="module")
def expected(oracle, scene):
    """The oracle's Recognition() per parameter set and frame, and its match list per frame: computed once, never changed."""
    reco = {p: [oracle.recognition(b, d, scene["K"], clutter.T, scene["bank"], *p) for b, d in zip(scene["bgrs"], scene["depths"])]
            for p in PARAMS}
    matches = [oracle.match_images(b, d, clutter.T, [scene["bank"]], 75.0) for b, d in zip(scene["bgrs"], scene["depths"])]
    assert [e["found"] for e in reco[PARAMS[0]]] == [1, 1, 1, 0]          # the pattern that differs from slot to slot
    return dict(reco=reco, matches=matches)


@pytest.fixture(scope="module")
def own_ctx():
    c = api.Context(0)                   # a context of its own: an option left set cannot leak into other tests
    yield c
    c.close()


class _DeviceBatches:
    """X, Y, Z of n frames each as device arrays at a regular pitch (read in place: irregular addresses would be gathered
    into the workspaces, which takes the one-stream path), built on the device from one upload of a - d."""

    def __init__(self, scene, n):
        import torch
        self.n = n
        d_b = torch.from_numpy(np.stack(scene["bgrs"])).cuda()
        d_d = torch.from_numpy(np.stack(scene["depths"]).view(np.int16)).cuda()
        self.order, self.keep, self.bp, self.dp = [], [], [], []
        for s in SHIFTS:
            order = [(i + s) % NF for i in range(n)]
            idx = torch.tensor(order, device="cuda")
            b, d = d_b[idx].contiguous(), d_d[idx].contiguous()
            self.keep.append((b, d))
            self.order.append(order)
            self.bp.append([b.data_ptr() + i * PX * 3 for i in range(n)])
            self.dp.append([d.data_ptr() + i * PX * 2 for i in range(n)])
        torch.cuda.synchronize()


def _check(res, order, exp, tag):
    for i, r in enumerate(res):
        _assert_reco_equal(api.recognition_result_to_dict(r), exp[order[i]], tag + (i,))


def _xyz(det, submit, n, orders, exp, tag):
    """submit X; submit Y with no host synchronisation; collect_previous = X; submit Z; collect_previous = Y; collect = Z"""
    submit(0)
    submit(1)
    _check(det.recognize_collect_previous(n), orders[0], exp, tag + ("X",))
    submit(2)
    _check(det.recognize_collect_previous(n), orders[1], exp, tag + ("Y",))
    _check(det.recognize_collect(n), orders[2], exp, tag + ("Z",))


def _state_error(call):
    with pytest.raises(api.FealessError) as e:
        call()
    assert e.value.code == L.FL_ERR_STATE


# ---- 1. the hazard itself -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(own_ctx, scene):
    """More ICP jobs than ICP slots: one 256-thread workgroup per CU (icp_wide 0, icp_wg_per_cu 1) and CU count + 64 frames,
    so the last 64 workgroups start one workgroup lifetime after the first -- after the next batch's whole LINEMOD has run.
    One detector per fine-level mode (sampled at finalize), shared by the cases below."""
    import torch
    n = torch.cuda.get_device_properties(0).multi_processor_count + 64
    dets = {}
    for mode in ("lazy", "eager"):
        with _options(own_ctx, {"eager_frontend": 1 if mode == "eager" else 0}):
            dets[mode] = _detector(own_ctx, scene, max_batch=n, max_candidates=4096)
    yield dict(n=n, dets=dets, frames=_DeviceBatches(scene, n))
    for d in dets.values():
        d.close()


@pytest.mark.parametrize("mode", ("lazy", "eager"))
@pytest.mark.parametrize("p", PARAMS)
@pytest.mark.parametrize("pipeline_icp", PIPELINE_VALUES)
def test_next_batch_does_not_disturb_the_icp_stage_in_flight(own_ctx, scene, expected, big, pipeline_icp, p, mode):
    det, fr, n = big["dets"][mode], big["frames"], big["n"]
    params = L.RecognitionParams(*p, L.FL_ICP_PARITY)
    with _options(own_ctx, {"icp_wide": 0, "icp_wg_per_cu": 1, "pipeline_icp": pipeline_icp}):
        _xyz(det, lambda k: det.recognize_submit_device(fr.bp[k], fr.dp[k], scene["K"], params), n, fr.order, expected["reco"][p],
             (pipeline_icp, p, mode))


# ---- 2. small batches on the default kernel choice ------------------------------------------------------------------
@pytest.mark.parametrize("source", ("device", "host"))
@pytest.mark.parametrize("pipeline_icp", PIPELINE_VALUES)
def test_small_batches_device_and_host_frames(own_ctx, scene, expected, pipeline_icp, source):
    """Batch 4 takes the 1024-thread ICP kernel; host frames go through the two input buffers, whose read event is now
    recorded on the ICP stream."""
    det = _detector(own_ctx, scene)
    orders = [[(i + s) % NF for i in range(NF)] for s in SHIFTS]
    try:
        with _options(own_ctx, {"pipeline_icp": pipeline_icp}):
            for p in PARAMS:
                params = L.RecognitionParams(*p, L.FL_ICP_PARITY)
                if source == "device":
                    fr = _DeviceBatches(scene, NF)
                    submit = lambda k: det.recognize_submit_device(fr.bp[k], fr.dp[k], scene["K"], params)   # noqa: E731
                else:
                    submit = lambda k: det.recognize_submit_host([scene["bgrs"][o].ctypes.data for o in orders[k]],   # noqa: E731
                                                                 [scene["depths"][o].ctypes.data for o in orders[k]], scene["K"], params)
                _xyz(det, submit, NF, orders, expected["reco"][p], (pipeline_icp, p, source))
    finally:
        det.close()


# ---- 3. fallbacks and joins -----------------------------------------------------------------------------------------
def test_caller_stream_takes_the_one_stream_path(scene, expected):
    """With a stream of the caller's on the context, synchronising THAT stream finishes the batch: everything was queued on it."""
    import torch
    c = api.Context(0)
    s = torch.cuda.Stream()
    p = PARAMS[0]
    params = L.RecognitionParams(*p, L.FL_ICP_PARITY)
    try:
        assert c.get_option("pipeline_icp") != 0
        c.set_stream(s.cuda_stream)
        det = _detector(c, scene)
        fr = _DeviceBatches(scene, NF)
        det.recognize_submit_device(fr.bp[0], fr.dp[0], scene["K"], params)
        det.recognize_submit_device(fr.bp[1], fr.dp[1], scene["K"], params)
        s.synchronize()                  # a plain hipStreamSynchronize of the caller's stream
        assert s.query()
        _check(det.recognize_collect_previous(NF), fr.order[0], expected["reco"][p], ("stream", "X"))
        _check(det.recognize_collect(NF), fr.order[1], expected["reco"][p], ("stream", "Y"))
        det.close()
        c.set_stream(0)
    finally:
        c.close()


def test_other_entry_points_join_the_icp_stream(own_ctx, scene, expected):
    """Right after a pipelined submit, match_batch, recognize_batch_topk and export_topk give what they give on a fresh
    detector (the match lists: what the oracle gives), and the batch before is no longer there to collect."""
    import torch
    p = PARAMS[1]
    params = L.RecognitionParams(*p, L.FL_ICP_PARITY)
    fr = _DeviceBatches(scene, NF)
    k = 12
    fresh = _detector(own_ctx, scene)
    topk_fresh = fresh.recognize_batch_topk(scene["bgrs"], scene["depths"], scene["K"], k, *p)
    exp_fresh = torch.zeros(NF * k * 5, dtype=torch.int32, device="cuda")
    fresh.recognize_submit_device(fr.bp[0], fr.dp[0], scene["K"], params)
    fresh.recognize_collect(NF)
    fresh.export_topk_batch(NF, k, 0, exp_fresh.data_ptr())
    own_ctx.synchronize()
    fresh.close()

    det = _detector(own_ctx, scene)
    with _options(own_ctx, {"pipeline_icp": 1}):
        _state_error(lambda: det.recognize_collect_previous(NF))          # nothing submitted
        det.recognize_submit_device(fr.bp[1], fr.dp[1], scene["K"], params)
        _state_error(lambda: det.recognize_collect_previous(NF))          # one batch only
        det.recognize_submit_device(fr.bp[0], fr.dp[0], scene["K"], params)
        lists = det.match_batch(scene["bgrs"], scene["depths"], 75.0)
        _state_error(lambda: det.recognize_collect_previous(NF))
        for i in range(NF):
            assert lists[i][1] == expected["matches"][i][1]
            _assert_matches_equal(lists[i][0], expected["matches"][i][0], ("match_batch", i))

        det.recognize_submit_device(fr.bp[1], fr.dp[1], scene["K"], params)
        det.recognize_submit_device(fr.bp[0], fr.dp[0], scene["K"], params)
        got = det.recognize_batch_topk(scene["bgrs"], scene["depths"], scene["K"], k, *p)
        _state_error(lambda: det.recognize_collect_previous(NF))
        for i in range(NF):
            assert len(got[i]) == len(topk_fresh[i]), i
            for r, (g, e) in enumerate(zip(got[i], topk_fresh[i])):
                assert g["status"] == 0 and g["found"] == e["found"] and g["det"]["n_points"] == e["det"]["n_points"], (i, r)
                assert np.array_equal(_bits(g["pose"]), _bits(e["pose"])), (i, r)

        det.recognize_submit_device(fr.bp[1], fr.dp[1], scene["K"], params)
        det.recognize_submit_device(fr.bp[0], fr.dp[0], scene["K"], params)
        exp_got = torch.zeros_like(exp_fresh)
        det.export_topk_batch(NF, k, 0, exp_got.data_ptr())
        _state_error(lambda: det.recognize_collect_previous(NF))
        _check(det.recognize_collect(NF), fr.order[0], expected["reco"][p], ("after export",))
        own_ctx.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(exp_got, exp_fresh)
        # collected once: not again
        det.recognize_submit_device(fr.bp[1], fr.dp[1], scene["K"], params)
        det.recognize_submit_device(fr.bp[2], fr.dp[2], scene["K"], params)
        _check(det.recognize_collect_previous(NF), fr.order[1], expected["reco"][p], ("once",))
        _state_error(lambda: det.recognize_collect_previous(NF))
        _check(det.recognize_collect(NF), fr.order[2], expected["reco"][p], ("latest",))
    det.close()


# ---- 4. overflow with two batches in flight -------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline_icp", PIPELINE_VALUES)
def test_overflow_with_two_batches_in_flight(own_ctx, scene, expected, pipeline_icp):
    p = PARAMS[0]
    params = L.RecognitionParams(*p, L.FL_ICP_PARITY)
    cap = 64
    # which frames have more coarse candidates than the buffers hold (the count the scan leaves with room for all of them)
    roomy = _detector(own_ctx, scene)
    roomy.recognize_batch(scene["bgrs"], scene["depths"], scene["K"], *p)
    over = [roomy.frame_counters(i)[0] > cap for i in range(NF)]
    roomy.close()
    assert over[0] and not all(over), over
    fr = _DeviceBatches(scene, NF)
    det = _detector(own_ctx, scene, max_candidates=cap)
    with _options(own_ctx, {"pipeline_icp": pipeline_icp}):
        det.recognize_submit_device(fr.bp[0], fr.dp[0], scene["K"], params)
        det.recognize_submit_device(fr.bp[1], fr.dp[1], scene["K"], params)
        for k, res in ((0, det.recognize_collect_previous(NF)), (1, det.recognize_collect(NF))):
            for i, r in enumerate(res):
                o = fr.order[k][i]
                if over[o]:
                    assert r.status == L.FL_ERR_OVERFLOW and r.found == 0, (k, i)
                else:
                    _assert_reco_equal(api.recognition_result_to_dict(r), expected["reco"][p][o], ("small", k, i))
        assert det.grow_candidates(NF) > cap
        det.recognize_submit_device(fr.bp[0], fr.dp[0], scene["K"], params)
        det.recognize_submit_device(fr.bp[1], fr.dp[1], scene["K"], params)
        _check(det.recognize_collect_previous(NF), fr.order[0], expected["reco"][p], ("grown", "X"))
        _check(det.recognize_collect(NF), fr.order[1], expected["reco"][p], ("grown", "Y"))
    det.close()


# ---- 5. option plumbing ---------------------------------------------------------------------------------------------
def test_pipeline_icp_option(monkeypatch):
    c = api.Context(0)
    default = c.get_option("pipeline_icp")
    for v in PIPELINE_VALUES:
        c.set_option("pipeline_icp", v)
        assert c.get_option("pipeline_icp") == v
    for bad in (4, -1):
        with pytest.raises(api.FealessError) as e:
            c.set_option("pipeline_icp", bad)
        assert e.value.code == L.FL_ERR_INVALID and c.get_option("pipeline_icp") == PIPELINE_VALUES[-1]
    c.set_option("pipeline_icp", default)
    other = 0 if default else 2
    monkeypatch.setenv("FL_PIPELINE_ICP", str(other))         # after the context exists: changes nothing
    assert c.get_option("pipeline_icp") == default
    c2 = api.Context(0)                                        # read at context creation
    assert c2.get_option("pipeline_icp") == other
    monkeypatch.setenv("FL_PIPELINE_ICP", "4")                 # out of range: the built-in default
    c3 = api.Context(0)
    assert c3.get_option("pipeline_icp") == default
    for x in (c, c2, c3):
        x.close()
