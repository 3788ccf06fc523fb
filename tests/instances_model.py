"""numpy restatement of the multi-instance rules (include/fealess_hip.h, "multi-instance recognition"): the yardstick of
fl_group_matches and fl_recognize_batch_instances.

Grouping: greedy over the match list in its order.  Match i, of template pyramid g, has the doubled box centre
c2 = (2 x + width0(g), 2 y + height0(g)); it joins the first group in creation order whose leader has the same class_idx and
(dc2x)^2 + (dc2y)^2 < (2 min_dist_px)^2 (strict), else founds a group while fewer than max_instances exist, else is dropped
(-1).  Distances go to the leader only.
Pick: nonMaximumSuppression's choice (ICP/NMS.cpp:6-40) among the first hyp_per_instance members of a group that were
found, in list order."""
import numpy as np


def widths_heights(banks):
    """Per class (banks in class order): an (n_pyramids, 2) array of templates[0]'s width and height."""
    out = []
    for b in banks:
        t = b.arrays()[0]
        lm = b.levels * b.modalities
        out.append(np.stack([t["width"][::lm], t["height"][::lm]], axis=1).astype(np.int64))
    return out


def centres2(matches, wh):
    """The doubled box centres, int64."""
    cls, tid = np.asarray(matches["class_idx"], np.int64), np.asarray(matches["template_id"], np.int64)
    w, h = np.zeros(len(matches), np.int64), np.zeros(len(matches), np.int64)
    for c, a in enumerate(wh):
        sel = cls == c
        w[sel], h[sel] = a[tid[sel], 0], a[tid[sel], 1]
    return 2 * np.asarray(matches["x"], np.int64) + w, 2 * np.asarray(matches["y"], np.int64) + h


def _near(dx, dy, r):
    """dx^2 + dy^2 < r^2 without leaving int64: |d| >= r decides on its own, below that the squares are < 2^62 (r <= 2^31)."""
    box = (np.abs(dx) < r) & (np.abs(dy) < r)
    dx, dy = np.where(box, dx, 0), np.where(box, dy, 0)
    return box & (dx * dx + dy * dy < r * r)


def group(matches, wh, max_instances, min_dist_px):
    """The sequential walk.  Returns (group_of[n] int32, group_size[max_instances] int32, n_groups)."""
    n = len(matches)
    cx, cy = centres2(matches, wh)
    cls = np.asarray(matches["class_idx"], np.int64)
    r = np.int64(2 * min_dist_px)
    gof = np.full(n, -1, np.int32)
    size = np.zeros(max_instances, np.int32)
    lx, ly, lc = (np.zeros(max_instances, np.int64) for _ in range(3))
    G = 0
    for i in range(n):
        hit = np.nonzero((lc[:G] == cls[i]) & _near(lx[:G] - cx[i], ly[:G] - cy[i], r))[0]
        if len(hit):
            g = int(hit[0])
        elif G < max_instances:
            g = G
            lx[G], ly[G], lc[G] = cx[i], cy[i], cls[i]
            G += 1
        else:
            continue
        gof[i] = g
        size[g] += 1
    return gof, size, G


def group_rounds(matches, wh, max_instances, min_dist_px):
    """The same groups by rounds: in round r the lowest-index match without a group becomes leader r, and every match
    without a group within its radius joins it."""
    n = len(matches)
    cx, cy = centres2(matches, wh)
    cls = np.asarray(matches["class_idx"], np.int64)
    r = np.int64(2 * min_dist_px)
    gof = np.full(n, -2, np.int32)
    size = np.zeros(max_instances, np.int32)
    G = 0
    while G < max_instances and (gof == -2).any():
        l = int(np.nonzero(gof == -2)[0][0])
        join = (gof == -2) & (cls == cls[l]) & _near(cx - cx[l], cy - cy[l], r)
        gof[join] = G
        size[G] = join.sum()
        G += 1
    gof[gof == -2] = -1
    return gof, size, G


def pick(refined, members):
    """refined[i]: result dict of list index i (found, det.n_points, det.icp.dist_mean); members: the list indices of a
    group's refined members, in list order.  Returns the list index picked (the leader when none was found)."""
    o, size_th = None, 0
    for j in members:
        c = refined[j]
        if not c["found"]:
            continue
        if o is None:
            o, size_th = j, int(np.float64(np.float32(c["det"]["n_points"])) * 0.85)
        elif c["det"]["n_points"] > size_th and c["det"]["icp"]["dist_mean"] < refined[o]["det"]["icp"]["dist_mean"]:
            o = j
    return members[0] if o is None else o


def instances(matches, wh, refined, max_instances, min_dist_px, hyp_per_instance):
    """Per group, in creation order: dict(rank, n_members, n_refined); and the number of dropped matches."""
    gof, size, G = group(matches, wh, max_instances, min_dist_px)
    out = []
    for g in range(G):
        mem = [int(i) for i in np.nonzero(gof == g)[0][:hyp_per_instance]]
        out.append(dict(rank=pick(refined, mem), n_members=int(size[g]), n_refined=len(mem)))
    return out, int((gof == -1).sum())


# ---- lists both test files use ------------------------------------------------------------------------------------------
def small_banks(seed=11, n_pyramids=(7, 5)):
    """Two classes of random pyramids whose templates[0] have different (odd and even) widths and heights, so that the
    doubled centre is not a constant offset of the match position."""
    from fealess_amd import synth
    from fealess_amd.bank import TemplateBank
    rng = np.random.default_rng(seed)
    banks = []
    for ci, n in enumerate(n_pyramids):
        b = TemplateBank("cls%d" % ci, 2, 2)
        for _ in range(n):
            tl = synth.random_pyramid(rng, 2, 2, 640, 480, bbox=40)
            w, h = int(rng.integers(21, 120)), int(rng.integers(21, 120))
            for t in tl:
                t["width"], t["height"] = w >> t["pyramid_level"], h >> t["pyramid_level"]
            b.add_pyramid(tl)
        banks.append(b)
    return banks


def random_list(rng, n, banks, spread=600, clusters=0):
    """n matches: uniform over a spread x spread window, or (clusters > 0) scattered 30 px around that many centres."""
    from fealess_amd.bank import MATCH_DTYPE
    m = np.zeros(n, MATCH_DTYPE)
    if clusters:
        c = rng.integers(0, spread, (clusters, 2))
        k = rng.integers(0, clusters, n)
        m["x"], m["y"] = c[k, 0] + rng.integers(-30, 31, n), c[k, 1] + rng.integers(-30, 31, n)
    else:
        m["x"], m["y"] = rng.integers(0, spread, n), rng.integers(0, spread, n)
    m["class_idx"] = rng.integers(0, len(banks), n)
    m["template_id"] = [rng.integers(0, banks[c].n_pyramids) for c in m["class_idx"]]
    m["similarity"] = np.sort(rng.uniform(75, 100, n).astype(np.float32))[::-1]
    return m
