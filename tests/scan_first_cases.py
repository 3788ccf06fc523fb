"""Banks for the tests of k_scan's streamed first piece (tests/test_gpu_scan_first.py, tests/test_scan_first_model_cpu.py).

The scene is tests/scan_lane_cases.py's: 8x8 blocks of a 320x240 image at T = 8, a feature reads exactly the labels of one block,
and planting a template at a position gives it a full score there.  The modalities here have COUNTS features, so that a first
piece of 12, 14 or 16 ends at the modality's end (12, 14, 16), at a pad (9, 11, 13, 15: the group is padded to 16), inside the
second group of eight (17, 31) or is the modality's only group (1, 7, 8).  Feature k sits on block (k % 12, k // 12) of the
template, so a template is twelve blocks wide and one to three tall.

Kinds, per count n (both modalities have n features):
  S  planted at one position: that lane survives every check and yields the candidate
  E  nothing planted: the item ends at a check, most of them at the first one (counted from seven features on; a single feature
     meets its label somewhere in the background)
and once, for n = 31:
  L  the first 16 colour features planted and nothing else: the lane passes the check behind the first piece whatever its length
     and dies ten lost features later, at a check behind a piece of `step` features
The single-modality bank has S and E for 1, 9, 16 and 31 features."""
import numpy as np

from fealess_amd.bank import TemplateBank
from scan_lane_cases import H0, T, W0, WB, Scene, lane_of

COUNTS = (1, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17, 31)
SINGLE_COUNTS = (1, 9, 16, 31)
THR = 70.0
# S positions with a meaning: lane 63 of chunk 0 under a three-row template (the tail dword, streamed), lane 63's last
# position under a two-row one, and chunk 1
SPECIAL = {31: 1010, 16: 1023, 12: 1144}


def features(rng, n):
    k = np.arange(n)
    return np.stack([T * (k % 12), T * (k // 12), rng.integers(0, 8, n)], 1).astype(np.int32)


def template(f):
    n = len(f)
    return dict(width=T * min(n, 12), height=T * ((n + 11) // 12), offset_x=0, offset_y=0, pyramid_level=0, features=f)


def _slots():
    """Positions whose 12 x 3 blocks are disjoint from one another and from SPECIAL's (rows 25 and up)."""
    return [r * WB + c for r in range(0, 24, 3) for c in (0, 14, 28)]


def first_bank(seed=21, modalities=2):
    """(qs, bank, kinds, where, counts): kinds[g] in "SEL", where[g] the planted position or None, counts[g] the features per
    modality."""
    sc = Scene(seed, background=0.03)
    rng = sc.rng
    bank, kinds, where, counts = TemplateBank("obj", 1, modalities), [], [], []
    slots = _slots()
    plan = [(n, k) for n in (COUNTS if modalities == 2 else SINGLE_COUNTS) for k in "SE"]
    if modalities == 2:
        plan.insert(len(plan) // 2, (31, "L"))
    for n, kind in plan:
        fs = [features(rng, n) for _ in range(modalities)]
        at = None
        if kind == "S":
            at = SPECIAL[n] if modalities == 2 and n in SPECIAL else slots.pop(0)
            for m in range(modalities):
                sc.plant(m, at, fs[m])
        elif kind == "L":
            at = slots.pop(0)
            sc.plant(0, at, fs[0], keep=16)
        bank.add_pyramid([template(f) for f in fs])
        kinds.append(kind)
        where.append(at)
        counts.append(n)
    return sc.quantized()[:modalities], bank, kinds, where, counts


def check_cases(items, kinds, where, counts, mid, lanes, step, first):
    """The model's items (scan_first_model.scan) of first_bank under the very options: every kind is what it is meant to be.
    Raises AssertionError where one is not.  Returns how many items ended at a first piece's check, survived one to a
    candidate, and died at a later check behind a piece of `step` features."""
    by = {(it["g"], it["chunk"]): it for it in items}
    ended_first = survived = later = 0
    for g, (kind, at, n) in enumerate(zip(kinds, where, counts)):
        own = [by[g, c] for c in (0, 1) if (g, c) in by]
        cand = {(x // T) + (y // T) * WB for it in own for x, y, _, _ in it["candidates"]}
        n_pad = -(-n // 8) * 8
        piece = first if n_pad > 8 else 8                  # the first piece of a modality of n features
        bit = 1 if piece > 8 else 0
        if kind == "E":
            assert n < 7 or not cand, g
            if n >= 7 and (mid >> bit) & 1:
                # (a lane that meets another template's planted blocks can outlive the first check: counted, not demanded of all)
                assert all(it["ended"] is None or it["ended"] >= piece for it in own), (g, n, [it["ended"] for it in own])
                ended_first += sum(it["first_end"] and it["ended"] == piece for it in own)
            continue
        chunk, lane = lane_of(at)
        it = by[g, chunk]
        if kind == "S":
            assert at in cand, (g, n, at, cand)
            assert it["ended"] is None
            if (mid >> bit) & 1:
                assert it["checks"][0][0] == piece, (g, it["checks"][:2])      # the first check stands behind the first piece
                if lanes:
                    assert (it["checks"][0][1] >> lane) & 1
                survived += 1
            continue
        assert kind == "L" and not cand, g
        if (mid >> 3) & 1 and (mid >> 1) & 1:
            first_check = it["checks"][0]
            assert first_check[0] == first and (first_check[1] >> lane) & 1, (g, first_check)
            # lost features cost 4 each and the threshold leaves room for nine: dead once the 26th colour feature is in
            want = {8: 32, 4: 28, 2: 26}[step]
            assert it["ended"] == want and not it["first_end"], (g, it["ended"], want)
            later += 1
    return ended_first, survived, later
