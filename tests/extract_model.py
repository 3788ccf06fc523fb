"""Plain models and case generators for template extraction's sort and scattered selection (test infrastructure).

select_model restates Candidate::operator< + std::stable_sort + QuantizedPyramid::selectScatteredFeatures
(linemod.hpp:98-101, linemod.cpp:135-164) candidate by candidate, with float32 arithmetic for distance and distance_sq.
select_walk gives the same features from per-pass numpy work; it exists to count relaxations on lists the plain loop is
too slow for, and tests/test_extract_model_cpu.py holds both to the oracle.  The generators build the candidate lists of
tests/test_gpu_extract_select.py; Scene / candidate_counts / the searches build the views of tests/test_gpu_extract_edges.py.
"""
import functools

import numpy as np

import oracle_py as O

F32 = np.float32


# ---- the two start distances -------------------------------------------------------------------------------------------
def color_distance(n, num_features):                       # linemod.cpp:503-505
    return F32(n // num_features + 1)


def depth_distance(area, num_features):                    # linemod.cpp:815-817
    return F32(np.sqrt(F32(area)) / np.sqrt(F32(num_features)) + F32(1.5))


def sort_order(score):
    """std::stable_sort with Candidate::operator< (score descending) of a list in the given arrival order."""
    return np.argsort(-np.asarray(score, F32), kind="stable")


# ---- the selection -----------------------------------------------------------------------------------------------------
def select_model(x, y, label, score, num_features, distance):
    """Returns (features (num_features, 3), stats) or (None, None) when the list is too short.  stats: relaxations = how
    often the distance was lowered, wraps_after_take = how often that happened right after the last sorted candidate
    was taken, full_passes = how often it happened after a candidate that was not taken, kept_at_equal = how many features
    were kept with a chosen feature at exactly the required distance."""
    n = len(x)
    if n < num_features:
        return None, None
    order = sort_order(score)
    cx = [int(v) for v in np.asarray(x)[order]]
    cy = [int(v) for v in np.asarray(y)[order]]
    cl = [int(v) for v in np.asarray(label)[order]]
    distance = F32(distance)
    dsq = float(F32(distance * distance))
    fx, fy, out = [], [], []
    i = 0
    stats = dict(relaxations=0, wraps_after_take=0, full_passes=0, kept_at_equal=0)
    while len(out) < num_features:
        px, py = cx[i], cy[i]
        keep = True
        equal = False
        for j in range(len(fx)):
            dx, dy = px - fx[j], py - fy[j]
            d2 = dx * dx + dy * dy
            d2 = d2 if d2 < (1 << 24) else float(F32(d2))
            if not (d2 >= dsq):                                              # (float)(int) >= float
                keep = False
                break
            equal |= d2 == dsq
        if keep:
            stats["kept_at_equal"] += equal                                  # `>=` decided: `>` would have refused
            fx.append(px)
            fy.append(py)
            out.append((px, py, cl[i]))
        i += 1
        if i == n:
            i = 0
            distance = F32(distance - F32(1.0))
            dsq = float(F32(distance * distance))
            stats["relaxations"] += 1
            stats["wraps_after_take" if keep else "full_passes"] += 1
    return np.array(out, np.int32), stats


def select_walk(x, y, label, score, num_features, distance):
    """select_model's result and relaxation count, one numpy pass per accepted feature and per relaxation."""
    n = len(x)
    if n < num_features:
        return None, None
    order = sort_order(score)
    cx, cy, cl = (np.asarray(a, np.int64)[order] for a in (x, y, label))
    distance = F32(distance)
    dsq = F32(distance * distance)
    mind2 = np.full(n, np.iinfo(np.int64).max, np.int64)
    out = []
    i = relax = 0
    while len(out) < num_features:
        ok = np.flatnonzero(mind2[i:].astype(F32) >= dsq)
        if len(ok) == 0:
            p = n - 1
        else:
            p = i + int(ok[0])
            out.append((cx[p], cy[p], cl[p]))
            mind2 = np.minimum(mind2, (cx - cx[p]) ** 2 + (cy - cy[p]) ** 2)
        i = p + 1
        if i == n:
            i = 0
            distance = F32(distance - F32(1.0))
            dsq = F32(distance * distance)
            relax += 1
    return np.array(out, np.int32), dict(relaxations=relax)


# ---- candidate lists ---------------------------------------------------------------------------------------------------
def pack_keys(raster, score):
    bits = np.asarray(score, F32).view(np.uint32)
    return ((~bits).astype(np.uint64) << np.uint64(32)) | np.asarray(raster, np.int64).astype(np.uint64)


def sorted_keys(raster, score):
    """The keys in (score descending, raster ascending) order."""
    raster, score = np.asarray(raster, np.int64), np.asarray(score, F32)
    o = np.lexsort((raster, -score.astype(np.float64)))
    return pack_keys(raster[o], score[o])


def label_image(w, h, seed=1):
    return (1 << np.random.default_rng(seed).integers(0, 8, (h, w))).astype(np.uint8)


def make_job(name, w, h, raster, score, num_features=63, depth_mode=0, area=0, seed=1):
    raster = np.asarray(raster, np.int32)
    return dict(name=name, w=w, h=h, num_features=num_features, depth_mode=depth_mode, area=area, raster=raster,
                score=np.asarray(score, F32), labels=label_image(w, h, seed))


def job_distance(job):
    if job["depth_mode"] == 0:
        return color_distance(len(job["raster"]), job["num_features"])
    return depth_distance(job["area"] if job["depth_mode"] == 2 else job["w"] * job["h"], job["num_features"])


def job_xyl(job):
    r = job["raster"].astype(np.int64)
    x, y = r % job["w"], r // job["w"]
    label = np.log2(job["labels"][y, x].astype(np.float64)).astype(np.int32) if len(r) else np.zeros(0, np.int32)
    return x.astype(np.int32), y.astype(np.int32), label


def job_expected(job):
    """(features or None, sorted keys).  The features are the oracle's (orc_select_scattered_list) for the list in raster
    order, the order in which the reference meets its candidates whatever order they arrive in here; the keys are the lexsort."""
    x, y, label = job_xyl(job)
    o = np.argsort(job["raster"], kind="stable")
    f = O.select_scattered_list(x[o], y[o], label[o], job["score"][o], job["num_features"], job_distance(job))
    exp = None if f is None else np.stack([f["x"], f["y"], f["label"]], 1).astype(np.int32)
    return exp, sorted_keys(job["raster"], job["score"])


def block_rasters(w, bw, bh, x0=3, y0=2):
    ys, xs = np.mgrid[y0:y0 + bh, x0:x0 + bw]
    return (ys * w + xs).ravel().astype(np.int32)


def scores(kind, n, rng):
    if kind == "distinct":
        return (rng.permutation(n).astype(F32) + F32(3026.0))            # above 55^2, all different
    if kind == "three":
        return np.array([3100.0, 4000.5, 9000.25], F32)[rng.integers(0, 3, n)]
    if kind == "five":
        return np.array([3100.0, 3500.0, 4000.5, 9000.25, 20000.0], F32)[rng.integers(0, 5, n)]
    if kind == "equal":
        return np.full(n, 5000.0, F32)
    raise ValueError(kind)


def arrival(kind, raster, score, rng):
    o = {"raster": np.argsort(raster, kind="stable"), "reversed": np.argsort(raster, kind="stable")[::-1],
         "shuffled": rng.permutation(len(raster))}[kind]
    return raster[o], score[o]


def rule_jobs(nf):
    """n = nf - 1, nf, nf + 1, 2 nf - 1, 2 nf candidates packed into the smallest square block that holds them."""
    out = []
    for n in (nf - 1, nf, nf + 1, 2 * nf - 1, 2 * nf):
        rng = np.random.default_rng(1000 * nf + n)
        side = int(np.ceil(np.sqrt(n)))
        r = block_rasters(40, side, side)[:n]
        r, s = arrival("shuffled", r, scores("three", n, rng), rng)
        out.append(make_job(f"rule-nf{nf}-n{n}", 40, 30, r, s, num_features=nf))
    return out


SORT_COUNTS = (2047, 2048, 2049, 4096, 4097, 8192, 8193)


def sort_job(n, dist, order, w=160, h=120):
    rng = np.random.default_rng(n * 31 + len(dist) * 7 + len(order))
    r = rng.permutation(w * h)[:n].astype(np.int32)
    r, s = arrival(order, r, scores(dist, n, rng), rng)
    return make_job(f"sort-{n}-{dist}-{order}", w, h, r, s)


MIXED_COUNTS = (0, 62, 63, 64, 2048, 2049, 8193, 20000)


def mixed_jobs(counts=MIXED_COUNTS, w=160, h=120):
    """One job per count; a count beyond the image's pixels repeats pixels (colour jobs may: their distance reaches 0)."""
    out = []
    for n in counts:
        rng = np.random.default_rng(77 + n)
        r = np.concatenate([rng.permutation(w * h), rng.integers(0, w * h, max(0, n - w * h))])[:n].astype(np.int32)
        r, s = arrival("shuffled", r, scores("five" if n % 2 else "distinct", n, rng), rng)
        out.append(make_job(f"mixed-{n}", w, h, r, s, seed=n + 1))
    return out


def deep_jobs():
    rng = np.random.default_rng(5)
    a = block_rasters(160, 80, 80, 40, 20)
    r1, s1 = arrival("shuffled", a[:6300], scores("equal", 6300, rng), rng)
    r2, s2 = arrival("shuffled", a, scores("five", 6400, rng), rng)
    b = block_rasters(160, 8, 8, 100, 50)[:63]
    r3, s3 = arrival("reversed", b, scores("three", 63, rng), rng)
    return [make_job("deep-6300-equal", 160, 120, r1, s1), make_job("deep-6400-five", 160, 120, r2, s2),
            make_job("deep-all-taken", 160, 120, r3, s3)]


def depth_scores(job_labels, raster, w, rng):
    """Scores as DepthNormalPyramid::extractTemplate makes them: a small integer distance over the label's count."""
    r = raster.astype(np.int64)
    lab = np.log2(job_labels[r // w, r % w].astype(np.float64)).astype(np.int64)
    counts = np.bincount(lab, minlength=8)
    return (rng.integers(1, 5, len(r)).astype(F32) / counts[lab].astype(F32)).astype(F32)


# 63 k^2 - 1, 63 k^2, 63 k^2 + 1: start distances around k + 1.5.  279 / 280: distance^2 = 12.992 / 13.019, either side of
# the squared distance 13 of the offset (2, 3), so the float-versus-int compare decides differently for the two.
DEPTH_AREAS = tuple(63 * k * k + d for k in (2, 5) for d in (-1, 0, 1)) + (279, 280)


def depth_jobs():
    out = []
    w, h = 96, 80
    lab = label_image(w, h, 9)

    def job(name, n, nf, mode, area, seed):
        rng = np.random.default_rng(seed)
        r = rng.permutation(block_rasters(w, 40, 40, 20, 10))[:n]
        j = make_job(name, w, h, r, depth_scores(lab, r, w, rng), num_features=nf, depth_mode=mode, area=area, seed=9)
        return j
    out.append(job("depth-mode1-total_px", 600, 63, 1, 0, 1))
    for a in DEPTH_AREAS:
        out.append(job(f"depth-mode2-area{a}", 600, 63, 2, a, a))
    for a in (31 * 9 - 1, 31 * 9, 31 * 9 + 1):
        out.append(job(f"depth-mode2-nf31-area{a}", 300, 31, 2, a, a))
    out.append(job("depth-mode2-area0", 200, 63, 2, 0, 3))
    out.append(job("depth-mode2-n63", 63, 63, 2, 400, 4))
    return out


def coordinate_jobs():
    rng = np.random.default_rng(11)
    w, h = 4096, 64
    corners = np.array([0, w - 1, (h - 1) * w, h * w - 1], np.int64)
    rest = np.setdiff1d(rng.permutation(w * h)[:320], corners)[:300]
    r = np.concatenate([corners, rest]).astype(np.int32)
    s = scores("three", len(r), rng)
    s[:4] = F32(30000.0)                                     # the corners sort first: the largest dx, dy come early
    r, s = arrival("shuffled", r, s, rng)
    wide = make_job("wide-4096x64-colour", w, h, r, s, seed=12)
    wide_d = make_job("wide-4096x64-depth", w, h, r, s, depth_mode=1, seed=12)
    r17 = rng.permutation(17 * 23)[:200].astype(np.int32)
    return [wide, wide_d, make_job("w17", 17, 23, r17, scores("five", 200, rng), seed=13)]


def all_select_jobs():
    out = [j for nf in (63, 31, 15, 7) for j in rule_jobs(nf)]
    out += [sort_job(n, d, o) for n in SORT_COUNTS for d in ("distinct", "three", "equal") for o in ("raster", "reversed", "shuffled")]
    return out + mixed_jobs() + deep_jobs() + depth_jobs() + coordinate_jobs()


# ---- candidate counts of a view, from the oracle's stage functions ------------------------------------------------------
def color_candidates(quantized, magnitude, mask):
    """ColorGradientPyramid::extractTemplate's candidates (:461-500): boolean image."""
    c = (quantized > 0) & (magnitude > F32(55.0 * 55.0))
    if mask is not None:
        c &= mask > O.erode_rect(mask, 1)                     # mask - erode(mask), saturating
    return c


def depth_candidates(normal, mask, threshold):
    """DepthNormalPyramid::extractTemplate's candidates (:752-800): (boolean image, distance image, area)."""
    local = None if mask is None else O.erode_rect(mask, 2)
    inside = np.ones(normal.shape, bool) if local is None else local != 0
    cand = np.zeros(normal.shape, bool)
    dist = np.zeros(normal.shape, F32)
    for k in range(8):
        bit = np.uint8(1 << k)
        d = O.distance_transform_c3(np.where(inside, normal & bit, 0).astype(np.uint8))
        sel = inside & (normal == bit)
        cand |= sel & (d >= F32(threshold))
        dist[sel] = d[sel]
    return cand, dist, int(inside.sum()) if local is not None else normal.size


class Scene:
    """The mask-independent stages of a view, computed once: per level the colour quantisation + magnitude and the normals."""

    def __init__(self, bgr, depth, levels):
        self.bgr, self.depth, self.levels = bgr, depth, levels
        self.color, self.normal = [], []
        src, qn = np.ascontiguousarray(bgr, np.uint8), O.quantized_normals(depth)
        for l in range(levels):
            if l > 0:
                src, qn = O.pyrdown_bgr(src), O.resize_nn_half(qn)
            self.color.append(O.quantized_orientations_mag(src))
            self.normal.append(qn)

    def mask_pyramid(self, mask):
        mk = [None if mask is None else np.ascontiguousarray(mask, np.uint8)]
        for l in range(1, self.levels):
            mk.append(None if mask is None else O.resize_nn_half(mk[-1]))
        return mk

    def job_count(self, masks, k):
        """Candidates of job k = l * 2 + m under the mask pyramid `masks`."""
        l, m = divmod(k, 2)
        if m == 0:
            return int(color_candidates(*self.color[l], masks[l]).sum())
        return int(depth_candidates(self.normal[l], masks[l], 2 >> l)[0].sum())

    def counts(self, mask):
        """Candidates per job, order [l * 2 + m]."""
        masks = self.mask_pyramid(mask)
        return [self.job_count(masks, k) for k in range(self.levels * 2)]


def candidate_counts(bgr, depth, mask, levels):
    return Scene(bgr, depth, levels).counts(mask)


def thresholds(levels):
    return [63 >> (k // 2) for k in range(levels * 2)]


def predicts_template(counts):
    return all(c >= t for c, t in zip(counts, thresholds(len(counts) // 2)))


# ---- the edge views ----------------------------------------------------------------------------------------------------
def block_noise_bgr(seed, w, h):
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, ((h + 3) // 4, (w + 3) // 4, 3), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(b, 4, 0), 4, 1)[:h, :w])


def tilted_patch_depth(seed, w, h, patch=12):
    rng = np.random.default_rng(seed + 10000)
    ny, nx = (h + patch - 1) // patch, (w + patch - 1) // patch
    ax, ay = rng.uniform(-6, 6, (ny, nx)), rng.uniform(-6, 6, (ny, nx))
    ys, xs = np.mgrid[0:h, 0:w]
    py, px = ys // patch, xs // patch
    z = 1000.0 + ax[py, px] * (xs % patch - patch / 2) + ay[py, px] * (ys % patch - patch / 2)
    return np.round(z).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def edge_scene(seed, w=96, h=80, levels=2):
    return Scene(block_noise_bgr(seed, w, h), tilted_patch_depth(seed, w, h), levels)


def rect_mask(w, h, x0, y0, rw, rh, value=255, extra=()):
    m = np.zeros((h, w), np.uint8)
    m[y0:y0 + rh, x0:x0 + rw] = value
    for (x, y) in extra:
        m[y, x] = value
    return m


def dotted_mask(w, h, step=4):
    """Isolated mask pixels on a grid that survives the nearest-neighbour halving: all border for the colour modality,
    nothing left for the depth modality once the mask is eroded."""
    m = np.zeros((h, w), np.uint8)
    m[::step, ::step] = 255
    return m


MARGIN = 8                                                   # "comfortably above": every other job has this many to spare
W, H, LEVELS = 96, 80, 2


def _search_masks(job):
    """The bounded, deterministic family a threshold view is searched in: (seed, mask, description).  Colour jobs: a
    rectangle with up to two isolated extra pixels.  Depth jobs: a low, long rectangle on top of a dotted mask, which keeps
    the colour jobs supplied while the depth jobs see the rectangle alone."""
    if job % 2 == 0:
        for seed in (0, 1):
            for rh in range(26, 57, 3):
                for rw in range(40, 88, 3):
                    for n_extra in range(3):
                        extra = tuple((W - 3 - 3 * e, H - 3) for e in range(n_extra))
                        yield seed, rect_mask(W, H, 4, 5, rw, rh, extra=extra), ("rect", 4, 5, rw, rh, extra)
    else:
        for seed in (0, 1, 2):
            for rh in (11, 12, 13):
                for rw in range(50, 74):
                    for (x0, y0) in ((4, 5), (5, 6)):
                        m = dotted_mask(W, H)
                        m[y0:y0 + rh, x0:x0 + rw] = 255
                        yield seed, m, ("dots+rect", x0, y0, rw, rh)


@functools.lru_cache(maxsize=None)
def threshold_case(job, target):
    """The first 96x80, two-level view of the job's search family in which job `job` has exactly `target` candidates while
    every other job has MARGIN to spare; None if the search ends without one."""
    th = thresholds(LEVELS)
    for seed, mask, what in _search_masks(job):
        sc = edge_scene(seed, W, H, LEVELS)
        masks = sc.mask_pyramid(mask)
        if sc.job_count(masks, job) != target:
            continue
        c = sc.counts(mask)
        if all(c[k] >= th[k] + MARGIN for k in range(len(c)) if k != job):
            return dict(seed=seed, bgr=sc.bgr, depth=sc.depth, mask=mask, counts=c, what=what)
    return None


THRESHOLD_CASES = [(job, (63 >> (job // 2)) + d) for job in range(4) for d in (-1, 0, 1)]
