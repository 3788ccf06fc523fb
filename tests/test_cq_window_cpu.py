"""CPU tests of the colour quantiser's window fetch (fl_frontend.hip: cq_window_addr and cq_window are host + device code,
exported as fl_dev_cq_window_addr / fl_dev_cq_window_taps for this check; no GPU).  A lane fetches its 7-pixel window as six
4-byte aligned dwords and moves it into place with a byte-align step; lanes at an image edge rebuild BORDER_REPLICATE from the
window clamped into the row.  Every row-address misalignment 0..3, every width 8..70 and every column of the row."""
import ctypes as C

import numpy as np
import pytest

from fealess_amd import _lib as L

WIDTHS = range(8, 71)


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_window_addressing_reads_only_dwords_of_the_window(lib):
    addr = L.dev(lib, "fl_dev_cq_window_addr")
    off, shift, first = C.c_uint(), C.c_uint(), C.c_int()
    n = 0
    for mis in range(4):
        for w in WIDTHS:
            for xc in range(w):
                addr(mis, w, xc, C.byref(off), C.byref(shift), C.byref(first))
                f = first.value
                assert f == min(max(xc - 3, 0), w - 7)
                lo = mis + 3 * f                                 # the window's bytes, counted from the aligned row address
                need = set(range(lo, lo + 21))                   # 7 pixels
                assert off.value % 4 == 0 and shift.value == lo - off.value and 0 <= shift.value <= 3
                dwords = [range(off.value + 4 * k, off.value + 4 * k + 4) for k in range(6)]      # a 16-byte and an 8-byte load
                assert need <= {b for d in dwords for b in d}, (mis, w, xc)
                for d in dwords:                                 # no dword without a byte of the 24-byte window -- nor of its 21
                    assert set(d) & set(range(lo, lo + 24)) and set(d) & need, (mis, w, xc, d)
                # the window stays inside the row: [mis, mis + 3 w)
                assert lo >= mis and lo + 21 <= mis + 3 * w
                n += 1
    assert n == 4 * sum(WIDTHS)


@pytest.mark.parametrize("edges", [(0, 0), (1, 1)], ids=["own-edges", "both-forced"])
def test_window_taps_are_the_replicated_border_taps(lib, edges):
    """The 21 bytes cq_window makes of a row are the taps clamp(xc + t - 3, 0, w - 1) of the three channels.  The row lies in a
    buffer whose other bytes hold a guard value that is no pixel's.  own-edges: the edge steps run only where the lane needs
    them (as in a wave without such lanes the steps are skipped); both-forced: every lane runs both steps, as the lanes of a
    narrow image's only wave do, and the ones that need neither keep their window."""
    taps = L.dev(lib, "fl_dev_cq_window_taps")
    rng = np.random.default_rng(11)
    out = np.zeros(21, np.uint8)
    for mis in range(4):
        for w in WIDTHS:
            buf = np.full(3 * w + 16, 0xEE, np.uint8)            # 8-byte aligned by numpy; the row starts at byte 4 + mis
            assert buf.ctypes.data % 4 == 0
            row = rng.integers(0, 0xE0, (w, 3)).astype(np.uint8)
            buf[4 + mis:4 + mis + 3 * w] = row.reshape(-1)
            for xc in range(w):
                left = edges[0] or xc < 3
                right = edges[1] or xc > w - 4
                taps(buf.ctypes.data + 4, mis, w, xc, int(left), int(right), out.ctypes.data)
                exp = row[np.clip(np.arange(xc - 3, xc + 4), 0, w - 1)].reshape(-1)
                assert np.array_equal(out, exp), (mis, w, xc, out, exp)
