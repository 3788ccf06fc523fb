"""CPU test of k_scan's work list (fl_context.hip: fl_build_scan_items is host code, exported as fl_dev_scan_items for this
check; no GPU).  One 64-byte record per (pyramid, chunk) of the list the scan has always walked -- chunk 0 of every pyramid,
and every later 1024-position chunk some modality's template_positions reach -- each exactly once, pyramid major; its fields
are the FlScanHdr entries' and its first eight words modality 0's first offset group; the offset table is padded."""
import ctypes as C

import numpy as np
import pytest

from fealess_amd import _lib as L

PAD = 8            # FL_SCAN_OFF_PAD
ZERO = 0xABCD00


@pytest.fixture(scope="module")
def build():
    fn = L.dev(L.load(), "fl_dev_scan_items")

    def run(hdr, M, WH, offs):
        hdr = np.ascontiguousarray(hdr, np.int32).reshape(-1, 4)
        offs = np.ascontiguousarray(offs, np.uint32)
        n_pyr = len(hdr) // M
        cap = n_pyr * ((WH + 1023) // 1024) + 1
        items = np.full((cap, 16), 0xEEEEEEEE, np.uint32)
        out = np.full(len(offs) + PAD + 4, 0xEEEEEEEE, np.uint32)
        n = fn(hdr.ctypes.data, n_pyr, M, WH, ZERO, offs.ctypes.data, len(offs), items.ctypes.data, cap, out.ctypes.data)
        assert 0 <= n < cap
        assert np.all(items[n:] == 0xEEEEEEEE) and np.all(out[len(offs) + PAD:] == 0xEEEEEEEE)
        return items[:n], out[:len(offs) + PAD]
    return run


def _random_bank(rng, n_pyr, M, WH):
    hdr, offs = [], []
    for _ in range(n_pyr * M):
        nf = int(rng.integers(0, 64))
        kept = int(rng.integers(0, nf + 1))                        # features inside the image
        n_pad = (kept + 7) // 8 * 8
        P = int(rng.choice([-5, 0, 1, 17, 1023, 1024, 1025, WH // 2, WH - 1, WH]))
        hdr.append((P, len(offs), n_pad, nf))
        offs += [int(v) for v in rng.integers(0, 1 << 20, kept)] + [ZERO] * (n_pad - kept)
    return np.array(hdr, np.int32), np.array(offs, np.uint32)


@pytest.mark.parametrize("M,WH,n_pyr", [(2, 1200, 41), (1, 1200, 9), (2, 48, 5), (2, 3600, 23), (2, 1024, 7), (2, 1200, 0)])
def test_records_are_the_old_work_list_with_the_headers_fields(build, M, WH, n_pyr):
    rng = np.random.default_rng(1000 * M + WH + n_pyr)
    hdr, offs = _random_bank(rng, n_pyr, M, WH)
    items, offs_out = build(hdr, M, WH, offs)
    # the padded table: unchanged entries, then PAD zero offsets
    assert np.array_equal(offs_out[:len(offs)], offs) and np.all(offs_out[len(offs):] == ZERO)
    # the list as it was built before: (g, c) for c == 0 or c * 1024 < the largest P of the pyramid's modalities
    nchunks = (WH + 1023) // 1024
    old = [(g, c) for g in range(n_pyr) for c in range(nchunks)
           if c == 0 or c * 1024 < max(int(hdr[g * M + m][0]) for m in range(M))]
    assert [(int(r[8]), int(r[9] & 0xFFFF)) for r in items] == old
    assert len(set(old)) == len(old)
    for r in items:
        g = int(r[8])
        h = [hdr[g * M + m] if m < M else (0, 0, 0, 0) for m in range(2)]
        assert int(r[9] >> 16) == sum(int(x[3]) for x in h[:M])                  # features of all modalities
        for m in range(2):
            P, off_begin, npad_nf = int(r[10 + 3 * m].astype(np.int32)), int(r[11 + 3 * m]), int(r[12 + 3 * m])
            assert (P, off_begin, npad_nf & 0xFFFF, npad_nf >> 16) == tuple(int(v) for v in h[m]), (g, m)
        first = offs[h[0][1]:h[0][1] + 8] if h[0][2] > 0 else np.full(8, ZERO, np.uint32)
        assert np.array_equal(r[:8], first), g
    # whatever group a record or a header names, the eight entries behind it lie inside the padded table
    for P, off_begin, n_pad, nf in hdr:
        assert off_begin + n_pad + PAD <= len(offs_out)


def test_bad_arguments_are_refused(build):
    fn = L.dev(L.load(), "fl_dev_scan_items")
    hdr = np.array([[10, 0, 16, 9]], np.int32)                       # 16 entries from 0 on, but the table holds 8
    offs = np.zeros(8, np.uint32)
    items = np.zeros((4, 16), np.uint32)
    out = np.zeros(32, np.uint32)
    assert fn(hdr.ctypes.data, 1, 1, 1200, ZERO, offs.ctypes.data, 8, items.ctypes.data, 4, out.ctypes.data) == L.FL_ERR_INVALID
    assert fn(hdr.ctypes.data, 1, 3, 1200, ZERO, offs.ctypes.data, 8, items.ctypes.data, 4, out.ctypes.data) == L.FL_ERR_INVALID
