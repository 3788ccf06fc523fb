"""GPU: fl_extract_template_pyramid / fl_extract_template_batch against the oracle's add_template on views built for the
edges of extraction: one job of a view exactly at, one below and one above its feature count while its siblings pass, such
views between good ones in a batch, masks that touch the image border, have a hole, are one pixel wide or hold values
other than 255, and the smallest geometries.  The views are block-noise colour over tilted depth patches
(tests/extract_model.py); every case first asserts, with the oracle's own stage functions, the candidate counts it was
built for."""
import numpy as np
import pytest

import extract_model as M
from test_gpu_extract_batch import _same, _same_as_oracle

pytestmark = pytest.mark.gpu
W, H, LEVELS = M.W, M.H, M.LEVELS
TH = M.thresholds(LEVELS)


def _case(job, target):
    case = M.threshold_case(job, target)
    assert case is not None, f"no view with {target} candidates in job {job}"
    counts = M.candidate_counts(case["bgr"], case["depth"], case["mask"], LEVELS)
    print("job", job, "target", target, "seed", case["seed"], case["what"], "counts", counts)
    assert counts[job] == target and all(counts[k] >= TH[k] + M.MARGIN for k in range(4) if k != job)
    return case


@pytest.mark.parametrize("job,target", M.THRESHOLD_CASES)
def test_one_job_at_its_threshold(ctx, oracle, job, target):
    case = _case(job, target)
    exp = oracle.add_template(case["bgr"], case["depth"], case["mask"], LEVELS)
    assert (exp is None) == (target < TH[job])
    _same_as_oracle(ctx.extract_template_pyramid(case["bgr"], case["depth"], case["mask"], LEVELS), exp)


def test_one_failing_job_in_a_batch(ctx, oracle):
    """Views in which a single job is one candidate short, between views that succeed: the failing views' jobs are
    handed to the sort and the selection as n_pow2 = 0 beside live jobs."""
    good = [_case(job, TH[job] + d) for job in range(4) for d in (0, 1)]
    failing = [_case(job, TH[job] - 1) for job in range(4)]
    views = [good[0], failing[0], good[1], good[2], failing[1], failing[2], good[3], good[4], failing[3], good[5], good[6], good[7]]
    fails = [any(v is f for f in failing) for v in views]
    got = ctx.extract_template_batch([v["bgr"] for v in views], [v["depth"] for v in views], [v["mask"] for v in views], LEVELS)
    for v, g, f in zip(views, got, fails):
        exp = oracle.add_template(v["bgr"], v["depth"], v["mask"], LEVELS)
        assert (exp is None) == f and (g is None) == f
        _same_as_oracle(g, exp)
        _same(g, ctx.extract_template_pyramid(v["bgr"], v["depth"], v["mask"], LEVELS))


def _masks():
    dots = M.dotted_mask(W, H)
    hole = M.rect_mask(W, H, 4, 4, 88, 72)
    hole[25:49, 30:60] = 0
    return dict(full=np.full((H, W), 255, np.uint8),
                corner=np.maximum(dots, M.rect_mask(W, H, 0, 0, 70, 60)),
                corner_far=np.maximum(dots, M.rect_mask(W, H, 30, 24, 66, 56)),
                hole=hole,
                line=np.maximum(dots, M.rect_mask(W, H, 3, 41, 90, 1)))


@pytest.mark.parametrize("name", ["full", "corner", "corner_far", "hole", "line"])
def test_mask_shapes(ctx, oracle, name):
    sc = M.edge_scene(0)
    mask = _masks()[name]
    counts = sc.counts(mask)
    print(name, "counts", counts)
    exp = oracle.add_template(sc.bgr, sc.depth, mask, LEVELS)
    if name == "full":                                       # BORDER_REPLICATE: a full mask has no border, the colour jobs are empty
        assert counts[0] == 0 and counts[2] == 0 and counts[1] >= 63 and counts[3] >= 31 and exp is None
    elif name == "line":                                     # nothing survives the 5x5 erosion: the depth jobs alone fail
        assert counts[1] == 0 and counts[3] == 0 and counts[0] >= 63 and counts[2] >= 31 and exp is None
    else:
        assert M.predicts_template(counts) and exp is not None
    if name.startswith("corner"):                            # the rectangle touches two image edges
        assert (mask[0, 0] and mask[0, 5] and mask[5, 0]) or (mask[H - 1, W - 1] and mask[H - 1, W - 6] and mask[H - 6, W - 1])
    _same_as_oracle(ctx.extract_template_pyramid(sc.bgr, sc.depth, mask, LEVELS), exp)


def test_mask_values_other_than_255(ctx, oracle):
    sc = M.edge_scene(0)
    base = _masks()["hole"]
    exp = oracle.add_template(sc.bgr, sc.depth, base, LEVELS)
    assert exp is not None
    masks = [np.where(base > 0, v, 0).astype(np.uint8) for v in (255, 128, 1)]
    got = ctx.extract_template_batch([sc.bgr] * 3, [sc.depth] * 3, masks, LEVELS)
    for m, g in zip(masks, got):
        assert sc.counts(m) == sc.counts(base)
        _same_as_oracle(g, oracle.add_template(sc.bgr, sc.depth, m, LEVELS))
        _same_as_oracle(g, exp)
        _same(g, ctx.extract_template_pyramid(sc.bgr, sc.depth, m, LEVELS))


def _view(w, h, seed=0):
    return M.block_noise_bgr(seed, w, h), M.tilted_patch_depth(seed, w, h)


def test_sizes_that_are_no_multiple_of_the_tiles(ctx, oracle):
    """150 x 90, three levels: 150, 75, 37 are no multiples of 64 and 90, 45, 22 none of 4; without and with a mask."""
    w, h, levels = 150, 90, 3
    assert all((w >> l) % 64 and (h >> l) % 4 for l in range(levels))
    bgr, depth = _view(w, h)
    mask = np.maximum(M.dotted_mask(w, h, 8), M.rect_mask(w, h, 37, 21, 113, 69))      # to the right and lower edges
    exps = [oracle.add_template(bgr, depth, m, levels) for m in (None, mask)]
    assert exps[0] is not None and exps[1] is not None
    got = ctx.extract_template_batch([bgr, bgr], [depth, depth], [None, mask], levels)
    for g, e in zip(got, exps):
        _same_as_oracle(g, e)


def test_four_levels_at_the_smallest_size(ctx, oracle):
    """levels = 4: 64 x 64 is the smallest size the entry accepts (8 x 8 at the coarsest level), and the oracle returns a
    template for it: candidate counts [1191, 650, 292, 676, 51, 169, 14, 49] against 63, 63, 31, 31, 15, 15, 7, 7."""
    bgr, depth = _view(64, 64)
    counts = M.candidate_counts(bgr, depth, None, 4)
    print("counts", counts)
    assert M.predicts_template(counts)
    exp = oracle.add_template(bgr, depth, None, 4)
    assert exp is not None
    _same_as_oracle(ctx.extract_template_pyramid(bgr, depth, None, 4), exp)


def test_one_level_at_the_smallest_size_that_succeeds(ctx, oracle):
    """levels = 1, square views from 16 x 16 (the smallest the entry accepts): the oracle refuses every size below 28 x 28
    for want of depth candidates (62 at 27 x 27) and returns a template at 28 x 28, where the depth job has exactly 63."""
    smallest = None
    for s in range(16, 33):
        bgr, depth = _view(s, s)
        counts = M.candidate_counts(bgr, depth, None, 1)
        exp = oracle.add_template(bgr, depth, None, 1)
        assert (exp is not None) == M.predicts_template(counts)
        if exp is not None and smallest is None:
            smallest = s
            print("smallest", s, "counts", counts)
            assert counts[1] == 63
        _same_as_oracle(ctx.extract_template_pyramid(bgr, depth, None, 1), exp)
    assert smallest == 28
