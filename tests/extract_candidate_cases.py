"""Cases and a plain numpy model for the stage of template extraction between quantisation and the sort (test infrastructure):
k_local_mask, k_color_candidates, k_depth_candidates with ex_chessboard, k_depth_keys (fealess_amd/csrc/fl_extract.hip), reached
through fl_dev_extract_quantized.

`expected(case)` restates ColorGradientPyramid::extractTemplate (linemod.cpp:461-513) and DepthNormalPyramid::extractTemplate
(:747-825) up to the candidate list in numpy alone -- erosion, border mask, chessboard distance, comparisons, counts, the
division -- and hands the list to the oracle's selection.  It exists to be MUTATED: `expected(case, mutant)` is the same text
with one operator changed, and tests/test_extract_candidates_cpu.py asserts that the unmutated model equals the oracle's stage
functions on every case and that every mutant changes the expected output of the cases named in CAUGHT_BY.  The GPU test
(tests/test_gpu_extract_candidates.py) compares the kernels with the oracle, scipy and this model.
"""
import functools

import numpy as np

import extract_model as EM
import oracle_py as O

F32 = np.float32
CAP = 8192                                                   # orc_distance_transform_c3: OpenCV's capped INIT_DIST0
STRONG = 55.0
MUTANTS = ("strong_ge", "threshold_gt", "erosion_radius", "border_no_subtraction", "labels_0_255", "outside_is_zero", "cap",
           "other_label_count", "area_pixel_count")


# ---- the model -------------------------------------------------------------------------------------------------------------
def erode(mask, r):
    """cv::erode by a (2r + 1)^2 rectangle, BORDER_REPLICATE."""
    h, w = mask.shape
    p = np.pad(mask, r, mode="edge")
    out = np.full(mask.shape, 255, np.uint8)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out = np.minimum(out, p[dy:dy + h, dx:dx + w])
    return out


def chessboard(nonzero, outside_is_zero=False, cap=CAP):
    """L-infinity distance of every non-zero pixel to the nearest zero pixel of the image, 0 on the zero pixels, `cap` where the
    image has no zero pixel.  Pixels outside the image are no zeros."""
    h, w = nonzero.shape
    d = np.zeros((h, w), F32)
    if not outside_is_zero and nonzero.all():
        d[:] = F32(cap)
        return d
    cur, r = nonzero.copy(), 0
    while cur.any():
        r += 1
        d[cur] = F32(r)                                      # alive after r - 1 erosions: at least r away
        p = np.pad(cur, 1, constant_values=not outside_is_zero)
        cur = np.logical_and.reduce([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])
    return d


def _label_of(q):
    return np.log2(np.where(q > 0, q, 1).astype(np.float64)).astype(np.int64)


def expected(case, mutant=None):
    """Every product of the stage for one view: local (the local mask image, None without a mask), cand (boolean image), score
    (float32 image: the magnitude / the undivided distance on the candidates, 0 elsewhere), n_cand, label_counts (8), area
    (the counter: pixels inside a depth view's eroded mask, else 0), keys (the sorted segment, None when the view is refused)
    and features ((num_features, 3), None when refused)."""
    assert mutant is None or mutant in MUTANTS
    q, mask, nf = case["q"], case["mask"], case["nf"]
    h, w = q.shape
    counts = np.zeros(8, np.int64)
    if case["modality"] == 0:
        mag = case["mag"]
        thr_sq = F32(F32(case["thr"]) * F32(case["thr"]))
        local = None
        if mask is not None:
            er = erode(mask, 2 if mutant == "erosion_radius" else 1)
            local = mask.copy() if mutant == "border_no_subtraction" else np.where(mask > er, mask - er, 0).astype(np.uint8)
        inside = np.ones(q.shape, bool) if local is None else local != 0
        cand = inside & (q > 0) & ((mag >= thr_sq) if mutant == "strong_ge" else (mag > thr_sq))
        score = np.where(cand, mag, F32(0)).astype(F32)
        final = score
        area = 0
        distance = EM.color_distance(int(cand.sum()), nf)
        lab = _label_of(q)
    else:
        local = None if mask is None else erode(mask, 1 if mutant == "erosion_radius" else 2)
        inside = np.ones(q.shape, bool) if local is None else local != 0
        cand = np.zeros(q.shape, bool)
        score = np.zeros(q.shape, F32)
        lab = np.where(q == 255, 7, _label_of(q))
        for k in range(8):
            bit = np.uint8(1 << k)
            d = chessboard(inside & ((q & bit) != 0), mutant == "outside_is_zero", 8191 if mutant == "cap" else CAP)
            sel = inside & (q == bit)
            if mutant == "labels_0_255":                     # background (no bit: label 0's image) and shadow (every bit: label 7's)
                sel |= inside & (((q == 0) & (k == 0)) | ((q == 255) & (k == 7)))
            ok = sel & ((d > F32(case["thr"])) if mutant == "threshold_gt" else (d >= F32(case["thr"])))
            cand |= ok
            score[ok] = d[ok]
            counts[k] = int(ok.sum())
        area = 0 if mask is None else int(inside.sum())
        used = q.size if mask is None or mutant == "area_pixel_count" else area
        if mutant == "area_pixel_count" and mask is not None:
            area = q.size
        distance = EM.depth_distance(used, nf)
        div = counts[(lab + 1) % 8] if mutant == "other_label_count" else counts[lab]
        with np.errstate(divide="ignore", invalid="ignore"):
            final = np.where(cand, score / div.astype(F32), F32(0)).astype(F32)
    raster = np.flatnonzero(cand)
    n = len(raster)
    keys = feats = None
    if n >= nf:
        keys = EM.sorted_keys(raster, final.ravel()[raster])
        f = O.select_scattered_list(raster % w, raster // w, lab.ravel()[raster], final.ravel()[raster], nf, distance)
        feats = np.stack([f["x"], f["y"], f["label"]], 1).astype(np.int32)
    return dict(local=local, cand=cand, score=score, n_cand=n, label_counts=counts, area=area, keys=keys, features=feats)


def differs(a, b):
    """The first product in which two expected outputs differ, or None."""
    for k in ("local", "cand", "score", "n_cand", "label_counts", "area", "keys", "features"):
        x, y = a[k], b[k]
        if (x is None) != (y is None) or (x is not None and not np.array_equal(np.asarray(x), np.asarray(y))):
            return k
    return None


# ---- the same products from the oracle's stage functions and scipy ---------------------------------------------------------
def scipy_distances(q, inside, cap=CAP):
    """The undivided distance of every one-hot pixel inside the mask: scipy's chessboard transform of its label's image, the
    cap where that image has no zero pixel (scipy has no such rule; it is orc_distance_transform_c3's)."""
    from scipy import ndimage
    dist = np.zeros(q.shape, F32)
    for k in range(8):
        bit = np.uint8(1 << k)
        img = inside & ((q & bit) != 0)
        d = np.full(q.shape, F32(cap)) if img.all() else ndimage.distance_transform_cdt(img, metric="chessboard").astype(F32)
        sel = inside & (q == bit)
        dist[sel] = d[sel]
    return dist


def oracle_products(case):
    """local, cand, score, area, features of `expected`, from oracle.erode_rect, extract_model.color_candidates /
    depth_candidates and oracle.extract_template_color / _depth."""
    q, mask, nf = case["q"], case["mask"], case["nf"]
    if case["modality"] == 0:
        er = None if mask is None else O.erode_rect(mask, 1)
        local = None if mask is None else np.where(mask > er, mask - er, 0).astype(np.uint8)
        cand = EM.color_candidates(q, case["mag"], mask)
        score = np.where(cand, case["mag"], F32(0)).astype(F32)
        area = 0
        f = O.extract_template_color(q, case["mag"], mask, case["thr"], nf)
    else:
        local = None if mask is None else O.erode_rect(mask, 2)
        cand, dist, a = EM.depth_candidates(q, mask, case["thr"])
        score = np.where(cand, dist, F32(0)).astype(F32)
        area = 0 if mask is None else a
        f = O.extract_template_depth(q, mask, case["thr"], nf)
    feats = None if f is None else np.stack([f["x"], f["y"], f["label"]], 1).astype(np.int32)
    return dict(local=local, cand=cand, score=score, area=area, features=feats)


# ---- images ----------------------------------------------------------------------------------------------------------------
def color_images(seed, w, h, mags=(3000.0, 3025.0, 3026.0, 4000.0)):
    rng = np.random.default_rng(seed)
    q = (1 << rng.integers(0, 8, (h, w))).astype(np.uint8)
    q[rng.random((h, w)) < 0.3] = 0
    return q, rng.choice(np.array(mags, F32), (h, w))


def depth_blocks(seed, w, h, bw, bh, lines=True):
    """Labels in bw x bh blocks; `lines`: a background column and a shadow row across them, where the image is large enough."""
    rng = np.random.default_rng(seed)
    n = (1 << rng.integers(0, 8, (h // bh + 1, w // bw + 1)).repeat(bh, 0).repeat(bw, 1)[:h, :w]).astype(np.uint8)
    if lines and w > 48 and h > 43:
        n[:, 45:48], n[40:43, :] = 0, 255
    elif lines and w > 20:
        n[:, 17:19] = 0
        n[h // 2, :] = 255
    return n


def inset_mask(w, h):
    """A rectangle a pixel or so inside the image, open towards the bottom edge where the image is low."""
    m = np.zeros((h, w), np.uint8)
    m[1:h if h < 12 else h - 2, 1 if w < 12 else 3:w - (1 if w < 12 else 5)] = 255
    return m


def _case(name, modality, q, mag, mask, thr, nf):
    return dict(name=name, modality=modality, q=np.ascontiguousarray(q, np.uint8), mag=None if mag is None else np.ascontiguousarray(mag, F32),
                mask=None if mask is None else np.ascontiguousarray(mask, np.uint8), thr=thr, nf=nf)


SHAPES = ((8, 8, 7), (9, 8, 7), (65, 9, 15), (97, 61, 63))   # (w, h, num_features): none a multiple of the 64 x 4 launch tile


@functools.lru_cache(maxsize=None)
def shape_cases():
    """Both modalities at every size of SHAPES, with and without a mask.  8 x 8 is the smallest level a public call can
    produce; 65 and 97 leave one and 33 columns to the second block of a row, 9 and 61 one row to the last block of a column."""
    out = []
    for (w, h, nf) in SHAPES:
        for masked in (False, True):
            mask = inset_mask(w, h) if masked else None
            tag = f"{w}x{h}_{'mask' if masked else 'nomask'}"
            q, mag = color_images(200 + w + h, w, h)
            out.append(_case(f"color_{tag}", 0, q, mag, mask, STRONG, nf))
            small = w < 20
            n = depth_blocks(300 + w + h, w, h, 4 if small else 8, 4 if small else 5)
            out.append(_case(f"depth_{tag}", 1, n, None, mask, 1 if small else 2, 7 if masked and h < 12 else nf))
    return out


MV_W, MV_H = 97, 61


@functools.lru_cache(maxsize=None)
def multi_view_cases():
    """name -> the views of one call: three views of differing content with masks on views 0 and 2, then the same images
    without any mask, per modality."""
    m0, m2 = inset_mask(MV_W, MV_H), np.zeros((MV_H, MV_W), np.uint8)
    m2[5:50, 20:90] = 200
    out = {}
    for masks, tag in (((m0, None, m2), "masks_0_2"), ((None, None, None), "no_masks")):
        cv, dv = [], []
        for v in range(3):
            q, mag = color_images(400 + v, MV_W, MV_H)
            cv.append(_case(f"mv_color_{tag}_view{v}", 0, q, mag, masks[v], STRONG, 63))
            dv.append(_case(f"mv_depth_{tag}_view{v}", 1, depth_blocks(410 + v, MV_W, MV_H, 9 + v, 7), None, masks[v], 2, 63))
        out[f"color_{tag}"], out[f"depth_{tag}"] = cv, dv
    return out


@functools.lru_cache(maxsize=None)
def launch_shape_cases():
    """The paths no 128 x 96 case with several labels reaches."""
    out = []
    one = np.full((96, 128), 1 << 3, np.uint8)
    out.append(_case("depth_one_label_128x96", 1, one, None, None, 2, 63))           # every distance is the cap
    other = one.copy()
    other[95, 127] = 1 << 5
    out.append(_case("depth_one_label_far_corner_128x96", 1, other, None, None, 2, 63))      # (0, 0): 127 = rmax rings
    rng = np.random.default_rng(51)
    blocks = (1 << rng.integers(0, 8, (128 // 12 + 1, 192 // 16 + 1)).repeat(12, 0).repeat(16, 1)[:128, :192]).astype(np.uint8)
    blocks[:, 45:48], blocks[40:43, :] = 0, 255
    out.append(_case("depth_blocks_192x128_thr1", 1, blocks, None, None, 1, 63))     # > 16384 candidates: k_depth_keys' second trip
    # exactly a power of two, and one below it: 128 x 64, every pixel a candidate
    q = (1 << np.random.default_rng(52).integers(0, 8, (64, 128))).astype(np.uint8)
    mag = np.full((64, 128), 4000.0, F32)
    out.append(_case("color_8192_of_128x64", 0, q, mag, None, STRONG, 63))
    q1 = q.copy()
    q1[33, 70] = 0
    out.append(_case("color_8191_of_128x64", 0, q1, mag, None, STRONG, 63))
    one = np.full((64, 128), 1 << 6, np.uint8)
    out.append(_case("depth_8192_of_128x64", 1, one, None, None, 1, 63))
    hole = one.copy()
    hole[33, 70] = 0                                         # its neighbours are at distance 1 >= 1: only the pixel itself drops out
    out.append(_case("depth_8191_of_128x64", 1, hole, None, None, 1, 63))
    # a mask of all 255: with the replicated border the erosion leaves it whole
    full = np.full((8, 8), 255, np.uint8)
    q8, mag8 = color_images(53, 8, 8, mags=(4000.0,))
    out.append(_case("color_full_mask_8x8", 0, q8, mag8, full, STRONG, 7))
    out.append(_case("depth_full_mask_8x8", 1, depth_blocks(54, 8, 8, 4, 4, lines=False), None, full, 1, 7))
    return out


@functools.lru_cache(maxsize=None)
def rule_cases():
    """n_cand == num_features and one below, colour, 97 x 61: 55^2 everywhere (no candidate), `exact` labelled pixels above it
    (the `exact` construction of reference_cases.extract_color_input)."""
    out = []
    for nf in (63, 31, 15, 7):
        for exact in (nf, nf - 1):
            rng = np.random.default_rng(600 + nf + exact)
            q, _ = color_images(700 + nf, 97, 61)
            mag = np.full((61, 97), 3025.0, F32)
            idx = rng.permutation(np.flatnonzero(q > 0))[:exact]
            mag.ravel()[idx] = rng.choice(np.array([3026.0, 4000.0, 9000.0], F32), exact)
            out.append(_case(f"color_{exact}_of_{nf}_97x61", 0, q, mag, None, STRONG, nf))
    return out


def all_cases():
    out = shape_cases() + launch_shape_cases() + rule_cases()
    for views in multi_view_cases().values():
        out += views
    return out


def by_name():
    return {c["name"]: c for c in all_cases()}


# Per mutant, cases whose expected output it must change (tests/test_extract_candidates_cpu.py asserts each one).
CAUGHT_BY = {
    "strong_ge": ["color_97x61_nomask", "color_65x9_mask", "color_8x8_nomask", "color_62_of_63_97x61", "color_6_of_7_97x61"],
    "threshold_gt": ["depth_97x61_nomask", "depth_8x8_nomask", "depth_8191_of_128x64", "depth_blocks_192x128_thr1"],
    "erosion_radius": ["color_97x61_mask", "depth_97x61_mask", "color_9x8_mask", "depth_65x9_mask"],
    "border_no_subtraction": ["color_97x61_mask", "color_8x8_mask", "color_full_mask_8x8", "mv_color_masks_0_2_view2"],
    "labels_0_255": ["depth_97x61_nomask", "depth_97x61_mask", "depth_blocks_192x128_thr1", "mv_depth_no_masks_view1"],
    "outside_is_zero": ["depth_one_label_128x96", "depth_one_label_far_corner_128x96", "depth_8x8_nomask", "depth_full_mask_8x8"],
    "cap": ["depth_one_label_128x96", "depth_8192_of_128x64"],
    "other_label_count": ["depth_97x61_nomask", "depth_blocks_192x128_thr1", "mv_depth_masks_0_2_view0"],
    "area_pixel_count": ["depth_97x61_mask", "mv_depth_masks_0_2_view2"],
}
