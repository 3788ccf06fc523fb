"""Several classes on one detector: tests/clutter.py's scene with its bank split into three classes, added in an order that
is not the sorted one.

  added first   "zeta"   pyramids [0, 8)     the eight near views of instance 0
  added second  "alpha"  pyramids [8, 16)    the eight near views of instance 1
  added third   "mid"    pyramids [16, 124)  the eight near views of instance 2, then the 100 random pyramids without renders

A detector keeps its classes in the order of their ids (std::map order): alpha = class index 0, mid = 1, zeta = 2, so
class_first = {0, 8, 116}, every class's index differs from its place in the order of addition, and a wrong class offset
lands on another instance's view: a plausible pose of the wrong template.

build() asserts, from the oracle alone, what makes the scene worth testing with: the best match of frames a and c lies in
class index 2 and that of frame b in class index 0, the first 12 matches of frame a hold all three classes, and frame a's
list over three classes is longer than over one (Match::operator== includes the class, so std::unique keeps more).  Should
the scene ever change, build() fails instead of handing out frames on which every class index is the same."""
import numpy as np

import clutter

ADDED = (("zeta", 0, 8), ("alpha", 8, 8), ("mid", 16, 108))        # (class id, first pyramid, count) in the order of addition
SORTED_IDS = ("alpha", "mid", "zeta")
CLASS_FIRST = (0, 8, 116)
THRESHOLD = 75.0
BEST_CLASS = {"a": 2, "b": 0, "c": 2, "d": None}
N_RENDERS = {"alpha": 8, "mid": 8, "zeta": 8}                      # mid's renders are those of its first eight pyramids


def split(bank):
    """The three classes in the order of addition."""
    out = []
    for cid, first, count in ADDED:
        b = bank.subset(first, count)
        b.class_id = cid
        out.append(b)
    return out


def build(oracle):
    """dict(scene (clutter.build's), K, bgrs, depths (frames a - d in clutter.FRAMES order), added (the banks in the order of
    addition), banks (in class order), by_id, lists (per frame the oracle's match list over the three classes, class_idx in
    class order), n_single (the length of frame a's list with the whole bank as one class))."""
    sc = clutter.build(oracle)
    assert sc["n_trained"] == 24 and sc["bank"].n_pyramids == 124
    added = split(sc["bank"])
    banks = sorted(added, key=lambda b: b.class_id)
    assert tuple(b.class_id for b in banks) == SORTED_IDS and tuple(b.class_id for b in added) != SORTED_IDS
    assert tuple(int(v) for v in np.cumsum([0] + [b.n_pyramids for b in banks])[:-1]) == CLASS_FIRST
    for b in banks:
        assert sum(m is not None for m in b.model_depths) == N_RENDERS[b.class_id] == len(b.model_depths)
    bgrs = [sc["frames"][f][0] for f in clutter.FRAMES]
    depths = [sc["frames"][f][1] for f in clutter.FRAMES]
    lists = []
    for f, b, d in zip(clutter.FRAMES, bgrs, depths):
        m, n = oracle.match_images(b, d, clutter.T, banks, THRESHOLD)
        assert n == len(m)
        lists.append(m)
        # non-vacuity: the best match's class
        if BEST_CLASS[f] is None:
            assert n == 0, (f, n)
        else:
            assert n >= 16 and int(m["class_idx"][0]) == BEST_CLASS[f], (f, n, m[:1])
    a = lists[0]
    assert set(int(c) for c in a["class_idx"][:12]) == {0, 1, 2}, a["class_idx"][:12]
    n_single = oracle.match_images(bgrs[0], depths[0], clutter.T, [sc["bank"]], THRESHOLD)[1]
    assert len(a) > n_single, (len(a), n_single)
    return dict(scene=sc, K=sc["K"], bgrs=bgrs, depths=depths, added=added, banks=banks, by_id={b.class_id: b for b in banks},
                lists=lists, n_single=n_single)
