"""Scenes and banks for the tests of k_scan's per-lane pruning (tests/test_scan_prune_model_cpu.py, tests/test_gpu_scan_lanes.py).

Everything lives on the 8x8 blocks of a 320x240 image at T = 8: a feature (8 dx, 8 dy, label) reads, at position p, exactly the
labels of block p + (dx, dy) (grid cell 0 of the linear memories, no spill into a neighbouring block), and a block's labels sit on
separate pixels of its first row.  So a template's score map is sum_k LUT(label_k, block[p + d_k]), and planting a template at
position j -- putting label_k into block j + d_k -- gives it a full score there and next to nothing elsewhere: which lanes stay
alive, and where, is decided position by position.  Templates are one block tall and twelve wide (1189 template_positions:
64 lanes in chunk 0, lanes 0..10 in chunk 1) or six tall (989 positions: lanes 0..61)."""
import numpy as np

from fealess_amd.bank import TemplateBank

W0, H0, T = 320, 240, 8
WB, HB = W0 // T, H0 // T
NF = 12                  # features per modality: dx = 0 .. 11, i.e. every byte misalignment three times over
THR = 90.0               # raw threshold 91 of 96: after eight colour features a position needs seven full responses to go on


class Scene:
    def __init__(self, seed, background=0.05):
        self.rng = np.random.default_rng(seed)
        self.blocks = [np.zeros((HB, WB), np.uint8) for _ in range(2)]      # label bits per block, per modality
        for b in self.blocks:
            on = self.rng.random((HB, WB)) < background
            b[on] = (1 << self.rng.integers(0, 8, size=(HB, WB)))[on].astype(np.uint8)

    def plant(self, m, j, feats, keep=None):
        """Put the labels of modality m's features (the first `keep` of them) where a template at position j reads them."""
        for x, y, lab in feats[:keep]:
            self.blocks[m][j // WB + y // T, j % WB + x // T] |= np.uint8(1 << lab)

    def quantized(self):
        qs = []
        for b in self.blocks:
            q = np.zeros((H0, W0), np.uint8)
            for lab in range(8):
                ys, xs = np.nonzero(b & (1 << lab))
                q[ys * T, xs * T + lab] = 1 << lab
            qs.append(q)
        return qs


def feats(rng, tall=1):
    """NF features on block origins: dx = 0 .. 11 in row 0, or spread over `tall` rows."""
    dy = rng.integers(0, tall, NF) if tall > 1 else np.zeros(NF, np.int64)
    return np.stack([T * np.arange(NF), T * dy, rng.integers(0, 8, NF)], 1).astype(np.int32)


def pyramid(f0, f1, tall0=1, tall1=1):
    def tpl(f, tall):
        return dict(width=T * NF, height=T * tall, offset_x=0, offset_y=0, pyramid_level=0, features=f)
    return [tpl(f0, tall0), tpl(f1, tall1)]


# position -> (chunk, lane)
def lane_of(j):
    return j // 1024, (j % 1024) // 16


SINGLE = [5, 327, 1010, 1091, 1186, 175, 447, 687]   # lane 0; a middle lane; lane 63 of chunk 0; chunk 1: lane 4 and its last
                                                     # lane with positions (10); three with j % 16 == 15 (lanes 10, 27, 42)
PAIRS = [(210, 226), (50, 805), (612, 628), (93, 1108)]       # adjacent lanes (13, 14 and 38, 39), far apart, one per chunk


def lane_bank(seed=14):
    """(qs, bank, kinds, where): eight rounds of the kinds below in rotated orders, so that whatever way the items are dealt a
    wave meets a pruned item, a surviving one and (under fl_similarity_maps) a tapped one after another.
      S  planted at one position (SINGLE, in turn): one lane survives the first check and yields the candidate
      P  planted at two positions (PAIRS, in turn): two survivors
      C  colour planted, depth not: every lane left dies inside modality 1
      D  planted at j, and its first eight colour features at a second position: that lane passes the check after eight features and
         dies at the next one (at the modality boundary where the mask leaves group 1 out)
      E  nothing planted: the item ends at its first check
      F  colour six blocks tall (989 positions), depth one (1189): all planted at 980, the last lane of the colour template (61)
    kinds[g] is the letter, where[g] the planted positions (D: (j, the colour-only position))."""
    sc = Scene(seed)
    rng = sc.rng
    bank, kinds, where = TemplateBank("obj", 1, 2), [], []
    orders = ["SPCDEF", "PDSFEC", "CESPFD", "DSCPEF", "EPDCFS", "SCEFPD", "PESDCF", "DCPSFE"]
    used = set()

    def free_row_slot(avoid_lanes=()):
        """A position whose twelve blocks no earlier planting uses, away from the given lanes."""
        for _ in range(1000):
            j = int(rng.integers(0, 24)) * WB + int(rng.integers(0, WB - NF))
            if lane_of(j)[1] in avoid_lanes or any((j + d) in used for d in range(-1, NF + 1)):
                continue
            return j
        raise AssertionError("no free slot")

    def claim(j, tall=1):
        for r in range(tall):
            used.update(range(j + r * WB, j + r * WB + NF))

    for j in SINGLE + [p for pr in PAIRS for p in pr] + [980]:
        claim(j, 6 if j == 980 else 1)
    for rnd, order in enumerate(orders):
        for kind in order:
            f0, f1 = feats(rng, 6 if kind == "F" else 1), feats(rng)
            at = ()
            if kind == "S":
                at = (SINGLE[rnd],)
            elif kind == "P":
                at = PAIRS[rnd % len(PAIRS)]
            elif kind == "F":
                at = (980,)
            elif kind in "CD":
                at = (free_row_slot(),)
                claim(at[0])
            for j in at:
                sc.plant(0, j, f0)
                if kind != "C":
                    sc.plant(1, j, f1)
            if kind == "D":
                j2 = free_row_slot(avoid_lanes=(lane_of(at[0])[1] - 1, lane_of(at[0])[1], lane_of(at[0])[1] + 1))
                claim(j2)
                sc.plant(0, j2, f0, keep=8)
                at = (at[0], j2)
            bank.add_pyramid(pyramid(f0, f1, 6 if kind == "F" else 1, 1))
            kinds.append(kind)
            where.append(at)
    return sc.quantized(), bank, kinds, where


def check_cases(items, kinds, where, mid, lanes):
    """The model's items (scan_prune_model.scan) of lane_bank: what each kind shows under per-lane pruning (lanes = 1) and a mask `mid`; under lanes = 0 only
    what holds for whole waves.  Raises AssertionError where a case is not what it is meant to be."""
    by = {(it["g"], it["chunk"]): it for it in items}
    seen = dict.fromkeys("SPCDEF", 0)
    for g, (kind, at) in enumerate(zip(kinds, where)):
        own = [by[g, c] for c in (0, 1) if (g, c) in by]
        cand = {(x // 8) + (y // 8) * WB for it in own for x, y, _, _ in it["candidates"]}
        if kind == "E":
            assert not cand and all(it["ended"] is not None or not mid for it in own), g
            seen["E"] += 1
            continue
        if kind == "C":
            assert not cand, g
            it = by[g, lane_of(at[0])[0]]
            if mid & 1:                                    # ended inside the depth modality, past all 16 padded colour features
                assert it["ended"] is not None and it["ended"] > 16, (g, it["ended"])
            seen["C"] += 1
            continue
        wanted = set(at[:1]) if kind == "D" else set(at)
        assert wanted <= cand, (g, kind, at, cand)
        seen[kind] += 1
        if not lanes or not mid:
            continue
        for j in wanted:                                   # exactly the planted lanes survive the first check of their item
            chunk, lane = lane_of(j)
            first = by[g, chunk]["checks"][0][1]
            here = {lane_of(p)[1] for p in at if lane_of(p)[0] == chunk}
            assert {i for i in range(64) if (first >> i) & 1} == here, (g, kind, j, bin(first))
            if j % 16 == 15:
                assert lane + 1 not in here                # the upper neighbour, whose first dword is this lane's tail, is dead
        if kind == "D":                                    # the colour-only lane: alive after 8 features, gone once all 12 are in
            chunk, lane = lane_of(at[1])
            checks = by[g, chunk]["checks"]
            nxt = next(c for c in checks if c[0] >= 12)
            assert (checks[0][1] >> lane) & 1 and not (nxt[1] >> lane) & 1, (g, checks[:4])
            if not (mid >> 1) & 1:
                assert nxt[0] == 16 and checks[1] == nxt   # ... at the check between the modalities, the mask leaving group 1 out
    assert all(v == 8 for v in seen.values()), seen
