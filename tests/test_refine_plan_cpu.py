"""CPU test of k_refine_lds's planner (fl_internal.h: fl_refine_plan, fl_refine_pitch and fl_refine_qmask are host + device
code, exported as fl_dev_refine_plan / fl_dev_refine_pitch for this check; no GPU).  The planner takes the candidates'
rectangles in processing order and returns the longest prefix whose united window fits the LDS budget.  It is compared with
a restatement written from the rule's description: the window starts at x0 rounded down to a multiple of 4, a row's pitch is
the smallest multiple of 16 that holds the row and whose quarter lies on one of the residues mod 32 at which the 8 rows x 4
column groups of one LDS cycle share the fewest banks."""
import ctypes as C

import numpy as np
import pytest

from fealess_amd import _lib as L

TS = (4, 5, 8, 3, 7)
W, H = 150, 110                     # a width that is no multiple of 16


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _residues(T):
    worst = {}
    for q in range(0, 32, 4):
        banks = [(T * (row * q + cg)) % 32 for row in range(8) for cg in range(4)]
        worst[q] = max(banks.count(b) for b in set(banks))
    best = min(worst.values())
    return best, {q for q, v in worst.items() if v == best}


def _pitch(width, T):
    _, res = _residues(T)
    p = (width + 15) // 16 * 16
    while (p // 4) % 32 not in res:
        p += 16
    return p


def _bytes(r, T):
    if r[2] < r[0]:
        return 0
    return _pitch(r[2] - r[0] // 4 * 4 + 1, T) * (r[3] - r[1] + 1)


def _union(rects):
    live = [r for r in rects if r[2] >= r[0]]
    if not live:
        return rects[0]
    a = np.array(live)
    return (a[:, 0].min(), a[:, 1].min(), a[:, 2].max(), a[:, 3].max())


def _plan(lib, rects, max_len, budget, T):
    fn = L.dev(lib, "fl_dev_refine_plan")
    arr = np.ascontiguousarray(rects, np.int32)
    uni = np.zeros(4, np.int32)
    n = fn(arr.ctypes.data, len(arr), max_len, budget, T, uni.ctypes.data)
    return n, tuple(int(v) for v in uni)


def test_pitch_rule(lib):
    fn = L.dev(lib, "fl_dev_refine_pitch")
    for T in TS:
        best, res = _residues(T)
        assert res, T
        if T % 2:
            assert best == 1, T      # an odd T has a pitch without any bank conflict
        for width in range(1, 700):
            p = fn(width, T)
            assert p == _pitch(width, T), (T, width)
            assert p >= width and p % 16 == 0 and p - width < 16 * 8


def _random_rects(rng, n):
    """Rectangles inside the W x H image, some touching each edge, a few empty, widths of every residue mod 16."""
    out = []
    for i in range(n):
        w = int(rng.integers(1, 70))
        h = int(rng.integers(1, 50))
        x0 = int(rng.integers(0, W - w + 1))
        y0 = int(rng.integers(0, H - h + 1))
        kind = i % 8
        if kind == 0:
            x0 = 0
        elif kind == 1:
            x0 = W - w
        elif kind == 2:
            y0 = 0
        elif kind == 3:
            y0 = H - h
        if kind == 4 and i % 3 == 0:
            out.append((0, 0, -1, -1))
            continue
        out.append((x0, y0, x0 + w - 1, y0 + h - 1))
    return out


@pytest.mark.parametrize("T", TS)
def test_longest_prefix_that_fits(lib, T):
    rng = np.random.default_rng(T)
    seen_edges = set()
    lengths = set()
    for trial in range(60):
        rects = _random_rects(rng, int(rng.integers(1, 24)))
        for r in rects:
            seen_edges |= {k for k, hit in zip("lrtb", (r[0] == 0, r[2] == W - 1, r[1] == 0, r[3] == H - 1)) if hit and r[2] >= r[0]}
        largest = max(_bytes(r, T) for r in rects)
        whole = _bytes(_union(rects), T)
        for budget in sorted({largest, largest + 1, largest + 16, (largest + whole) // 2, whole - 1, whole, whole + 1, 1 << 16}):
            if budget < largest:
                continue
            for max_len in (1, 3, 8, 1000):
                n, uni = _plan(lib, rects, max_len, budget, T)
                assert 1 <= n <= min(len(rects), max_len)
                assert _bytes(rects[0], T) <= budget          # a prefix of length 1 always fits
                u = _union(rects[:n])
                assert tuple(int(v) for v in u) == uni or all(r[2] < r[0] for r in rects[:n])
                assert _bytes(u, T) <= budget, (rects, budget, n)
                if n < min(len(rects), max_len):
                    assert _bytes(_union(rects[:n + 1]), T) > budget, (rects, budget, n)
                lengths.add(n)
    assert seen_edges == set("lrtb")
    assert 1 in lengths and max(lengths) > 8


def test_a_single_rectangle_and_an_exact_budget(lib):
    for T in TS:
        r = (13, 7, 13 + 36, 7 + 20)
        b = _bytes(r, T)
        assert _plan(lib, [r], 8, b, T) == (1, r)
        two = [r, (14, 7, 14 + 36, 7 + 20)]
        assert _plan(lib, two, 8, b, T)[0] == (2 if _bytes(_union(two), T) <= b else 1)
        far = [r, (100, 80, 149, 109)]
        assert _plan(lib, far, 8, b, T)[0] == 1
        assert _plan(lib, far, 8, _bytes(_union(far), T), T)[0] == 2
