"""CPU check of the cluttered-scene fixture (tests/clutter.py) with the oracle alone: the frames must stay in the cluttered
regime that test_gpu_clutter.py relies on -- many matches per frame, several instances found, a real occlusion, a real
border crossing, and a background that matches nothing."""
import numpy as np
import pytest

import clutter


@pytest.fixture(scope="module")
def scene(oracle):
    return clutter.build(oracle)


def _instances_hit(winners, masks, K, r=15):
    """Indices of the instances whose visible mask lies within r pixels of a winner's refined translation, projected."""
    fx, fy, cx, cy = K
    hit = set()
    for w in winners:
        X, Y, Z = (float(v) for v in w["det"]["T_final"])
        u, v = int(round(fx * X / Z + cx)), int(round(fy * Y / Z + cy))
        for j, m in enumerate(masks):
            if m[max(v - r, 0):v + r + 1, max(u - r, 0):u + r + 1].any():
                hit.add(j)
    return hit


def test_clutter_fixture_stays_cluttered(oracle, scene):
    bank, K = scene["bank"], scene["K"]
    assert scene["n_trained"] == 3 * 8
    need = {"a": 3, "b": 2, "c": 2}
    for name in clutter.FRAMES:
        bgr, depth = scene["frames"][name]
        m, n = oracle.match_images(bgr, depth, clutter.T, [bank], 75.0)
        top, win = oracle.recognition_topk(bgr, depth, K, clutter.T, bank, 12, 75.0, 10, 0.5, 0.01, nms_dist=60.0)
        if name == "d":
            assert n == 0 and top == [] and win == []
            continue
        assert n >= 20, (name, n)
        assert len(top) == 12 and all(t["found"] for t in top), name
        hit = _instances_hit([top[i] for i in win], scene["masks"][name], K)
        assert len(win) >= need[name] and len(hit) >= need[name], (name, win, hit)
        if name == "a":
            assert len(win) == 3
    # b: the nearer instance hides a fifth of the farther one, which stays mostly visible
    vis, full = scene["masks"]["b"][1], scene["full_masks_b"][1]
    assert 0.6 * full.sum() < vis.sum() < 0.9 * full.sum()
    # c: one instance of a straddles the column where frame c wraps round
    seam = clutter.W - clutter.SHIFT_C
    cols = [np.nonzero(m.any(axis=0))[0] for m in scene["masks"]["a"]]
    assert any(c.min() < seam <= c.max() for c in cols)
