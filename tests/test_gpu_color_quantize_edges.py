"""GPU parity of the colour quantiser (k_color_quantize) where its window fetch, its edge lanes and its unrolled row ring can
go wrong.  Every lane fetches its 7-pixel window as six 4-byte aligned dwords and moves it into place by a per-lane byte
shift; lanes within 3 columns of an image edge rebuild BORDER_REPLICATE from a window clamped into the row; the 7-row ring of
horizontal sums trades roles over an unrolled loop of seven steps, and the virtual rows outside the image repeat the row before.

Every image is compared byte for byte with the oracle's, in batches of 3 frames whose contents differ, through
Context.dev_front_images(levels=1): the frames are packed, so at odd sizes they start at misaligned addresses (3 w h mod 4),
and at widths that are no multiple of 4 the misalignment changes from row to row."""
import numpy as np
import pytest

from test_gpu_frontend_passes import (POISON, QUANT, THR, _assert_detector_frame, _assert_front_images, _detector, _expected,
                                      _frame, _scene, _trained_bank, c)  # noqa: F401  (c: the module's context fixture)
from util import options

pytestmark = pytest.mark.gpu


_PLAIN = {}


def _plain_scene(oracle, w, h):
    """Three frames of differing colour content and the oracle's level-0 images, computed once per size and never modified
    (_scene's frames carry depth holes and bands whose placement needs h > 3; depth is not what these tests are about)."""
    if (w, h) not in _PLAIN:
        rng = np.random.default_rng(1000 * w + h)
        frames = [_frame(w, h, rng, 0) for _ in range(3)]
        _PLAIN[(w, h)] = (frames, [_expected(oracle, b, d, 1) for b, d in frames])
    return _PLAIN[(w, h)]


def _check(c, oracle, w, h, tag, busy=True):
    frames, exps = _plain_scene(oracle, w, h)
    for i in range(3):
        for j in range(i):
            assert not np.array_equal(frames[i][0], frames[j][0])
            assert not busy or not np.array_equal(exps[i]["q"][0], exps[j]["q"][0]), (w, h, i, j)
    if busy:                                                     # not vacuous: labels come out, several of them
        assert all(len(np.unique(e["q"][0])) >= 3 for e in exps), (w, h)
    _assert_front_images(c, frames, exps, 1, (tag, w, h))


# 3 w mod 4 = 0, 3, 2, 1: every misalignment, changing from row to row.  At these widths every lane is an edge lane or the
# neighbour of one, and the image's only wave rebuilds both borders.
@pytest.mark.parametrize("w", [8, 9, 10, 11])
def test_narrow_widths_every_row_misalignment(c, oracle, w):
    assert sorted((3 * v) % 4 for v in (8, 9, 10, 11)) == [0, 1, 2, 3]
    _check(c, oracle, w, 16, "narrow")


# The last strip (60 columns a strip) holds 1..6 columns or a whole strip; with 1..3 columns the right edge lanes sit in the
# strip before it as well (lanes 60..63 are its halo).
@pytest.mark.parametrize("w", [59, 60, 61, 62, 63, 64, 65, 66, 119, 120, 121, 125])
def test_last_strip_of_a_few_columns(c, oracle, w):
    _check(c, oracle, w, 20, "last-strip")


def test_width_7_takes_the_byte_path(c, oracle):
    _check(c, oracle, 7, 16, "w7")


# Every phase of the seven-step ring is an exit phase; at the smallest heights the window is stuck at the top and at the
# bottom image row at once (rows -3.. and ..h+2 clamp into the image in the first window already).
@pytest.mark.parametrize("h", [3, 4, 5, 6, 7, 8, 9, 13, 14, 15])
def test_heights_around_the_ring_period(c, oracle, h):
    _check(c, oracle, 70, h, "ring", busy=h >= 4)               # (3 rows: one row of labels, the same in every frame)


# A chunk of one row follows a full one.
@pytest.mark.parametrize("h,rows", [(61, 60), (121, 60), (121, 120), (61, 120)])
def test_one_row_chunk_after_a_full_one(c, oracle, h, rows):
    with options(c, {"frontend_chunk_rows": rows}):
        _check(c, oracle, 70, h, ("chunk", rows))


@pytest.mark.parametrize("w,h,T", [(144, 132, [4, 2]), (160, 190, [5, 5])], ids=["144x132", "160x190"])
def test_tiled_launch_at_the_image_edges(c, oracle, w, h, T):
    """The lazy (tiled) colour launch of level 0 inside a detector, a trained template per frame: the marked tiles reach the
    left and the right image edge (the edge lanes' border rebuild in a tiled launch) and some have trimmed row ranges (computed
    rows that are no whole tile rows).  What a lazy batch did not compute holds POISON."""
    frames, exps = _scene(oracle, w, h, 2)
    bank = _trained_bank(oracle, frames, 2)
    assert c.get_option("dev_poison") == 1
    det = _detector(c, w, h, T, bank, eager=False)
    try:
        det.match_batch([f[0] for f in frames], [f[1] for f in frames], THR)
        left = right = trimmed = 0
        for i, e in enumerate(exps):
            _assert_detector_frame(det, i, e, (w, h, "lazy"), lazy=True)
            done = det.dev_frame_image(i, QUANT, 0, 0) != POISON
            left += int(done[:, 0].any())
            right += int(done[:, w - 1].any())
            rows = np.flatnonzero(done.any(axis=1))
            trimmed += int(len(rows) > 0 and (rows[0] % 60 != 0 or (rows[-1] + 1) % 60 not in (0, h % 60)))
        assert left >= 1 and right >= 1 and trimmed >= 1, (w, h, left, right, trimmed)
    finally:
        det.close()
