"""The stage of template extraction between quantisation and the sort, on its own: k_local_mask, k_color_candidates,
k_depth_candidates with ex_chessboard and k_depth_keys (fl_extract.hip) through Context.dev_extract_quantized, which runs the
launch functions extract_chunk runs for one pyramid level on quantized images given by the caller; and the magnitude image of
k_color_quantize<true, *>, the build only extraction launches, through Context.dev_quantized_orientations_mag.

Every intermediate product is compared bit for bit: the local mask with oracle.erode_rect, the candidate set and its scores
with extract_model.color_candidates / depth_candidates, the distances also with scipy's chessboard transform, the counts and
the area, the sorted segment with extract_model.sorted_keys, the features and the refusals with oracle.extract_template_color /
_depth, and all of them with the numpy model of tests/extract_candidate_cases.py, whose mutants tests/test_extract_candidates_cpu.py
shows these cases to catch.  Candidates arrive in the order the atomics gave: the list before the sort is compared as a set
ordered by raster, the sorted segment as it is."""
import functools

import numpy as np
import pytest

import extract_candidate_cases as XC
from fealess_amd import _lib as L
from fealess_amd import api
from test_gpu_color_quantize_edges import _plain_scene
from test_gpu_frontend_passes import c  # noqa: F401  (a context of its own for the tests that set options)
from util import options

pytestmark = pytest.mark.gpu
FILL = -7
CASES = XC.by_name()


@functools.lru_cache(maxsize=None)
def _refs(name):
    """The model's and the oracle's products of a case, computed once and never modified."""
    return XC.expected(CASES[name]), XC.oracle_products(CASES[name])


def _call(ctx, views):
    v0 = views[0]
    assert all((v["modality"], v["thr"], v["nf"], v["q"].shape) == (v0["modality"], v0["thr"], v0["nf"], v0["q"].shape) for v in views)
    masks = [v["mask"] for v in views]
    return ctx.dev_extract_quantized(v0["modality"], [v["q"] for v in views], [v["mag"] for v in views],
                                     None if all(m is None for m in masks) else masks, v0["thr"], v0["nf"], fill=FILL)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(got, case):
    name, nf = case["name"], case["nf"]
    exp, orc = _refs(name)
    h, w = case["q"].shape
    # the local mask
    if case["mask"] is None:
        assert got["local"] is None
    else:
        assert np.array_equal(got["local"], orc["local"]) and np.array_equal(got["local"], exp["local"]), name
    # counts and area
    assert got["n_cand"] == exp["n_cand"] == int(orc["cand"].sum()), (name, got["n_cand"], exp["n_cand"])
    assert got["area"] == exp["area"] == orc["area"], (name, got["area"], exp["area"])
    assert np.array_equal(got["label_counts"], exp["label_counts"]), (name, got["label_counts"], exp["label_counts"])
    # the candidates before the sort, as a set ordered by raster, with the scores the candidate kernel produced
    o = np.argsort(got["raster"], kind="stable")
    raster = got["raster"][o]
    assert np.array_equal(raster, np.flatnonzero(orc["cand"])) and np.array_equal(raster, np.flatnonzero(exp["cand"])), name
    for ref in (orc["score"], exp["score"]):
        assert np.array_equal(_bits(got["score"][o]), _bits(ref.ravel()[raster])), name
    if case["modality"] == 1:
        inside = np.ones((h, w), bool) if case["mask"] is None else orc["local"] != 0
        assert np.array_equal(_bits(got["score"][o]), _bits(XC.scipy_distances(case["q"], inside).ravel()[raster])), name
    assert got["tails_unwritten"], name
    # the sorted segment, the features, the refusal
    if exp["n_cand"] < nf:
        assert exp["features"] is None and orc["features"] is None
        assert got["keys"] is None and got["n_out"] == -1 and (got["features"] == FILL).all(), name
    else:
        assert got["keys"] is not None and np.array_equal(got["keys"], exp["keys"]), name
        assert got["n_out"] == nf and (got["features"][nf:] == FILL).all(), name
        assert np.array_equal(got["features"][:nf], orc["features"]) and np.array_equal(got["features"][:nf], exp["features"]), name


def _same_view(a, b):
    """Two results of one view: everything equal, the lists before the sort as sets."""
    oa, ob = np.argsort(a["raster"], kind="stable"), np.argsort(b["raster"], kind="stable")
    same = np.array_equal(a["raster"][oa], b["raster"][ob]) and np.array_equal(_bits(a["score"][oa]), _bits(b["score"][ob]))
    for k in ("local", "keys"):
        same = same and (a[k] is None) == (b[k] is None) and (a[k] is None or np.array_equal(a[k], b[k]))
    return same and all(np.array_equal(a[k], b[k]) for k in ("n_cand", "label_counts", "area", "n_out", "features"))


@pytest.mark.parametrize("name", [k["name"] for k in XC.shape_cases()])
def test_sizes_that_are_no_multiple_of_the_launch_tile(ctx, name):
    """8 x 8, 9 x 8, 65 x 9, 97 x 61, both modalities, with and without a mask; magnitudes from {3000, 3025, 3026, 4000}."""
    _check(_call(ctx, [CASES[name]])[0], CASES[name])


@pytest.mark.parametrize("name", [k["name"] for k in XC.launch_shape_cases()])
def test_launch_shapes_no_small_view_reaches(ctx, name):
    """One label everywhere (every distance the 8192 cap; with one far pixel, rmax rings), more than 16384 candidates (the second
    trip of k_depth_keys' grid-stride loop, a 32768-key sort), exactly 8192 candidates (k_pad_keys has nothing to pad) and 8191,
    a mask of all 255 (an empty colour border mask, a whole eroded mask)."""
    exp, _ = _refs(name)
    if name == "depth_blocks_192x128_thr1":
        assert exp["n_cand"] > 16384
    if "_of_128x64" in name:
        assert exp["n_cand"] == int(name.split("_")[1])
    _check(_call(ctx, [CASES[name]])[0], CASES[name])


@pytest.mark.parametrize("name", [k["name"] for k in XC.rule_cases()])
def test_num_features_at_the_candidate_count_and_one_below_it(ctx, name):
    """num_features 63, 31, 15, 7 with exactly that many candidates (all taken) and with one fewer (refused)."""
    _check(_call(ctx, [CASES[name]])[0], CASES[name])


@pytest.mark.parametrize("modality", ["color", "depth"])
def test_several_views_in_one_call_and_an_unmasked_call_after_a_masked_one(ctx, modality):
    """Three views of differing content with masks on views 0 and 2, then the same images without masks on the same context:
    the local-mask buffer the first call filled is stale in the second.  Every view equals the references and its own
    single-view call."""
    mv = XC.multi_view_cases()
    masked, plain = mv[f"{modality}_masks_0_2"], mv[f"{modality}_no_masks"]
    got_masked = _call(ctx, masked)
    got_plain = _call(ctx, plain)
    for views, got in ((masked, got_masked), (plain, got_plain)):
        assert len(got) == 3
        for v, g in zip(views, got):
            _check(g, v)
    # single-view calls, a masked view right before the unmasked view of the same slot
    for views, got in ((masked, got_masked), (plain, got_plain)):
        for v, g in zip(views, got):
            assert _same_view(_call(ctx, [v])[0], g), v["name"]


def test_refusals_write_nothing(ctx):
    case = CASES["color_8x8_nomask"]
    q, mag = case["q"], case["mag"]

    def refused(**kw):
        args = dict(modality=0, quantized=[q], magnitudes=[mag], masks=None, threshold=55.0, num_features=7, fill=FILL)
        args.update(kw)
        with pytest.raises(api.FealessError) as e:
            ctx.dev_extract_quantized(**args)
        assert e.value.code == L.FL_ERR_INVALID
        for b in e.value.buffers:
            assert (b["local"] == FILL & 0xFF).all() and all((b[k] == FILL).all() for k in ("counters", "raster", "score", "features"))
            assert (b["keys"] == np.int64(FILL).astype(np.uint64)).all()

    for nf in (0, -1, 64):
        refused(num_features=nf)
    for w, h in ((0, 8), (8, 0), (-8, 8), (65537, 1), (1, 65537)):
        refused(w=w, h=h)
    refused(modality=2)
    refused(modality=-1)
    fn = L.dev(ctx.lib, "fl_dev_extract_quantized")
    views = (L.DevExtractView * 1)()                              # every pointer null
    assert fn(ctx.h, 1, views, 8, 8, 0, 55.0, 2, 7) == L.FL_ERR_INVALID
    assert fn(ctx.h, 0, views, 8, 8, 0, 55.0, 2, 7) == L.FL_ERR_INVALID
    assert fn(ctx.h, 1, None, 8, 8, 0, 55.0, 2, 7) == L.FL_ERR_INVALID
    assert fn(None, 1, views, 8, 8, 0, 55.0, 2, 7) == L.FL_ERR_INVALID
    # a colour view without a magnitude image, a masked view without room for the local mask
    keep = [np.zeros(64, np.uint8), np.zeros(64, np.float32), np.full(64, 255, np.uint8), np.zeros(64, np.uint8), np.zeros(11, np.int32),
            np.zeros(64, np.int32), np.zeros(64, np.float32), np.zeros(64, np.uint64), np.zeros((64, 3), np.int32)]
    for null in range(9):
        if null == 2:                                            # no mask is no refusal
            continue
        ptrs = [a.ctypes.data for a in keep]
        ptrs[null] = None
        views[0] = L.DevExtractView(*ptrs)
        assert fn(ctx.h, 1, views, 8, 8, 0, 55.0, 2, 7) == L.FL_ERR_INVALID, null
    _check(_call(ctx, [case])[0], case)                         # and the context still works


# ---- the magnitude image of k_color_quantize<true, *> -------------------------------------------------------------------------
_MAG = {}


def _mag_scene(oracle, w, h):
    """test_gpu_color_quantize_edges' three frames of a size with the oracle's labels and magnitudes, computed once."""
    if (w, h) not in _MAG:
        frames, exps = _plain_scene(oracle, w, h)
        ref = [oracle.quantized_orientations_mag(b) for b, _ in frames]
        for (q, _), e in zip(ref, exps):
            assert np.array_equal(q, e["q"][0])
        _MAG[(w, h)] = ([b for b, _ in frames], ref)
    return _MAG[(w, h)]


def _check_mag(ctx, oracle, w, h, busy=True):
    bgrs, ref = _mag_scene(oracle, w, h)
    q, mag = ctx.dev_quantized_orientations_mag(bgrs, 10.0)
    assert q.shape == (3, h, w) and mag.shape == (3, h, w)
    for i, (eq, em) in enumerate(ref):
        assert not busy or (em > 100).any() and len(np.unique(eq)) >= 3
        assert np.array_equal(q[i], eq), (w, h, i, int((q[i] != eq).sum()))
        assert np.array_equal(_bits(mag[i]), _bits(em)), (w, h, i, int((_bits(mag[i]) != _bits(em)).sum()))
        assert np.array_equal(q[i], ctx.quantized_orientations(bgrs[i], 10.0)), (w, h, i)      # the <false> build


@pytest.mark.parametrize("w", [7, 8, 9, 10, 11])
def test_magnitude_at_narrow_widths(c, oracle, w):
    """Width 7 takes the byte path (k_color_quantize<true, true>); 8 .. 11: every row misalignment, every lane an edge lane."""
    _check_mag(c, oracle, w, 16)


@pytest.mark.parametrize("w", [59, 60, 61, 62, 63, 64, 65, 66, 119, 120, 121, 125])
def test_magnitude_in_a_last_strip_of_a_few_columns(c, oracle, w):
    _check_mag(c, oracle, w, 20)


@pytest.mark.parametrize("h", [3, 4, 5, 6, 7, 8, 9, 13, 14, 15])
def test_magnitude_at_heights_around_the_ring_period(c, oracle, h):
    _check_mag(c, oracle, 70, h, busy=h >= 4)


@pytest.mark.parametrize("h,rows", [(61, 60), (121, 60), (121, 120), (61, 120)])
def test_magnitude_in_a_one_row_chunk_after_a_full_one(c, oracle, h, rows):
    with options(c, {"frontend_chunk_rows": rows}):
        _check_mag(c, oracle, 70, h)
