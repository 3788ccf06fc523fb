"""The fixed, seeded case list on which the oracle, the HIP kernels and the reference's compiled code (tests/reference_py.py)
are compared bit for bit, and the two back ends that compute a case: the oracle and a build of the compiled reference.

One list serves three users, so that they cannot drift apart: tests/golden/make_golden.py --reference records the reference's
outputs on it (tests/golden/reference_linemod.npz), tests/test_reference_cpu.py compares the oracle with the live libraries
and with that record, tests/test_gpu_reference.py does the same for the kernels.  Every input is regenerated from its seed;
the record holds a digest of every input, so a numpy whose generators drifted fails loudly instead of comparing other data.

Where an input could make the reference's behaviour UNDEFINED, the input is built so that it cannot, and check_* asserts
that property of the input (never of an output):
  * similarity / similarityLocal read `positions` / 15 * W + 16 bytes from a feature's address; that must stay inside the
    label's T*T x W*H Mat (in_mat).  Reads that leave it are quirk Q2: cases whose name starts with "q2_" are DEFINED BY THE
    STAND-IN'S ALLOCATOR (zeroed guard), UB IN THE REFERENCE, and kept in a group of their own;
  * quantizedNormals indexes NORMAL_LUT[20][20][20] with int(n * 10 + 10) / int(nz * 20 + 20): a unit normal with nz == 0
    (zero depth or a singular system with a non-zero gradient) or a component that rounds to 1.0f indexes past the table
    (normals_safe; unsafe pixels are pushed behind distance_threshold when the case is built);
  * the SSE2 spread stores 16 bytes aligned at every row start, so the SIMD build takes widths that are multiples of 16;
  * hysteresisGradient's one OpenCV call, convertTo(CV_8U, 16/360), agrees between a float and a double product on every
    float in [0, 360] except two, which the angle pools leave out (angles_unambiguous);
  * icpCloudToCloud_Ex walks the ref iterator past its end when the model has more points than the reference cloud
    (getL2distClouds, the covariance loop): no case has n_model > n_ref (check_icp_case);
  * which of two reference points at exactly the same float32 squared distance FLANN returns is unspecified: no case has
    such a tie at any search the loop performs (nn_ties, by exhaustion over the iterations actually run), except the cases
    whose name starts with "tie_", which are DEFINED BY THE STAND-IN'S RULE (lowest index), UNSPECIFIED IN FLANN, and kept
    in a group of their own like q2_;
  * detection()'s two crops must have one size and lie inside the frame (the second is the reference's own CV_Assert, Q10,
    and is recorded as a refusal); cv::norm(t_i, t_j) in nonMaximumSuppression is taken on small integers, where the order
    of the subtraction and the widening to double cannot matter.

The ICP half (icp_groups) follows the same pattern on tests/golden/reference_icp.npz: that record holds digests of the inputs
and RESULTS ONLY (float bit patterns as uint32, ints, digests of the clouds depthTo3d returns), no cloud and no image.

Template extraction (extract_groups) the same way on tests/golden/reference_extract.npz: digests of the inputs, the feature
lists, templates and bounding boxes in full, refusals as such, images as digests; its conditions are listed where it begins.
"""
import functools
import hashlib

import numpy as np

import extract_model as EM
import oracle_py as O
from fealess_amd import synth
from fealess_amd.bank import FEATURE_DTYPE, MATCH_DTYPE, TEMPLATE_DTYPE, TemplateBank


def digest(a):
    a = np.ascontiguousarray(a)
    hsh = hashlib.sha256(f"{a.dtype.str}{a.shape}".encode())
    hsh.update(a.tobytes())
    return np.frombuffer(hsh.digest(), np.uint8).copy()


def lm_stride(w, h, T):
    """orc_lm_label_stride / fl_lm_label_stride: bytes per label of the padded linear-memory layout."""
    W, H = w // T, h // T
    return (T * T * W * H + W * H + 16 * W + 64 + 63) & ~63


# ---- spread / response maps / linearize ------------------------------------------------------------------------------
DENSITIES = (0.0, 0.03, 0.9)


def spread_cases():
    """(name, w, h, T, density, seed): any size; w % T and h % T non-zero wherever the width allows it."""
    out = []
    sizes = [(64, 37), (80, 45), (150, 50), (320, 61), (640, 43), (67, 33)]
    for T in (2, 4, 5, 8, 16):
        for i, (w, h) in enumerate(sizes):
            for k, dens in enumerate(DENSITIES):
                if w >= 320 and k != (i + T) % 3:
                    continue                                # the large ones take one density each, all three over the list
                out.append((f"spread_{w}x{h}_T{T}_d{k}", w, h, T, dens, 1000 + 37 * T + 3 * i + k))
    return out


def spread_input(case):
    _, w, h, T, dens, seed = case
    return synth.random_quantized(np.random.default_rng(seed), w, h, dens)


def linearize_cases():
    """(name, w, h, T, density, seed); sizes divisible by T, and the refusal of 80x45 with T = 8 (CV_Assert :1062)."""
    sizes = {2: [(64, 48), (150, 50), (320, 240)], 4: [(64, 48), (80, 48), (320, 60)], 5: [(80, 45), (150, 50), (320, 240), (640, 480)],
             8: [(64, 48), (80, 48), (320, 240), (640, 480)], 16: [(64, 48), (80, 48), (320, 240), (640, 480)]}
    out = []
    for T, ss in sizes.items():
        for i, (w, h) in enumerate(ss):
            k = (i + T) % 3
            out.append((f"lm_{w}x{h}_T{T}_d{k}", w, h, T, DENSITIES[k], 2000 + 41 * T + i))
    out.append(("lm_refused_80x45_T8", 80, 45, 8, 0.9, 2999))
    return out


# ---- similarity / similarityLocal / addSimilarities ------------------------------------------------------------------
def _templ(width, height, feats, level=0):
    t = np.zeros(1, TEMPLATE_DTYPE)
    t["width"], t["height"], t["pyramid_level"], t["feat_count"] = width, height, level, len(feats)
    f = np.zeros(len(feats), FEATURE_DTYPE)
    if len(feats):
        a = np.asarray(feats, np.int32).reshape(-1, 3)
        f["x"], f["y"], f["label"] = a[:, 0], a[:, 1], a[:, 2]
    return t, f


def _rand_feats(rng, n, width, height):
    return np.stack([rng.integers(0, width, n), rng.integers(0, height, n), rng.integers(0, 8, n)], 1).astype(np.int32)


def in_mat(feats_xy, w, h, T, extent):
    """Per in-image feature: does a read of `extent` bytes from its linear-memory address stay inside the label's Mat?"""
    W, H = w // T, h // T
    ok = []
    for x, y in feats_xy:
        if x < 0 or y < 0 or x >= w or y >= h:
            continue
        start = ((y % T) * T + x % T) * W * H + (y // T) * W + x // T
        ok.append(start + max(extent, 0) <= T * T * W * H)
    return ok


def positions(w, h, T, width, height):
    """template_positions of similarity() (linemod.cpp:1141-1155), C division truncating toward zero."""
    W, H = w // T, h // T
    wf, hf = int((width - 1) / T) + 1, int((height - 1) / T) + 1
    return (H - hf) * W + (W - wf) + 1


def similarity_cases():
    """(name, w, h, T, density, seed, width, height, feats).  Names starting with q2_ read past the label's Mat."""
    out = []
    geo = [(320, 240, 8), (160, 120, 4), (160, 80, 5), (64, 48, 2), (640, 480, 5), (320, 240, 16)]
    for gi, (w, h, T) in enumerate(geo):
        for n in (1, 8, 63):
            rng = np.random.default_rng(3000 + 10 * gi + n)
            width, height = int(rng.integers(8, w // 3)), int(rng.integers(8, h // 3))
            out.append((f"sim_{w}x{h}_T{T}_n{n}", w, h, T, 0.5, 3100 + gi, width, height, _rand_feats(rng, n, width, height)))
    rng = np.random.default_rng(3500)
    f = _rand_feats(rng, 20, 40, 40)
    f[::4, 0] += 400                                        # outside the image: skipped (:1179)
    f[1::4, 1] += 300
    f[2::4, 0] -= 50
    out.append(("sim_features_outside", 320, 240, 8, 0.5, 3501, 40, 40, f))
    f = _rand_feats(rng, 12, 100, 100)
    out.append(("sim_template_wider_than_image", 160, 120, 8, 0.5, 3502, 400, 60, f))     # span_x < 0
    out.append(("sim_template_larger_than_image", 160, 120, 8, 0.5, 3503, 400, 300, f))   # positions < 0
    out.append(("sim_uncropped_template", 160, 120, 8, 0.5, 3504, -1, -1, f[:3] // 16))   # (-2) / 8 == 0 in C
    out.append(("sim_zero_size_template", 160, 120, 8, 0.5, 3505, 0, 0, np.array([[0, 0, 3]], np.int32)))
    # Q1: a feature in the last column of its template: the positions of one image row run on into the next row
    out.append(("sim_row_wrap", 160, 120, 8, 0.9, 3506, 64, 32, np.array([[63, 0, 1], [63, 31, 2], [0, 31, 5], [62, 17, 7]], np.int32)))
    out.append(("sim_empty_image", 160, 120, 8, 0.0, 3507, 40, 40, _rand_feats(rng, 8, 40, 40)))
    # Q2 (own group): features beyond the template's declared size in the LAST grid row (x % T == y % T == T - 1)
    out.append(("q2_sim_last_grid_row", 160, 120, 8, 0.9, 3508, 16, 16, np.array([[159, 119, 1], [151, 111, 6], [7, 7, 2], [3, 3, 0]], np.int32)))
    out.append(("q2_sim_y_equals_height", 160, 120, 8, 0.9, 3509, 16, 16, np.array([[15, 119, 1], [159, 16, 2], [9, 16, 0]], np.int32)))
    return out


def check_similarity_case(case):
    name, w, h, T, _, _, width, height, feats = case
    ok = in_mat(feats[:, :2].tolist(), w, h, T, positions(w, h, T, width, height))
    assert (not all(ok)) if name.startswith("q2_") else all(ok), name


def local_cases():
    """(name, w, h, T, density, seed, feats, cx, cy): similarityLocal windows at the four corners, at centres that the
    caller would have clamped, and inside.  Features that would read past the label's Mat are moved one row up unless the
    case is in the Q2 group."""
    out = []
    for gi, (w, h, T) in enumerate([(320, 240, 5), (160, 120, 8), (80, 60, 4)]):
        rng = np.random.default_rng(4000 + gi)
        centres = {"tl": (0, 0), "tr": (w - 1, 0), "bl": (0, h - 1), "br": (w - 1, h - 1), "mid": (w // 2 + 1, h // 2 - 2),
                   "clamp_lo": (8 * T, 8 * T), "clamp_hi": (w - 40 - 8 * T, h - 40 - 8 * T), "neg": (-37, -5)}
        for ci, (cn, (cx, cy)) in enumerate(centres.items()):
            n = (1, 8, 63)[(ci + gi) % 3]
            for q2 in (False, True):
                f = _rand_feats(np.random.default_rng(4100 + 10 * gi + ci), n, 40, 40)
                if cn not in ("bl", "br") and q2:
                    continue
                ox, oy = (int(cx / T) - 8) * T, (int(cy / T) - 8) * T
                if q2:
                    f[0] = (w - 1 - ox, h - 1 - oy, 3)      # lands on the image's last pixel: last grid row, last cell
                else:
                    for _ in range(h):                      # move offenders up until their 16 rows fit
                        bad = [i for i in range(n) if in_mat([(f[i, 0] + ox, f[i, 1] + oy)], w, h, T, 15 * (w // T) + 16) == [False]]
                        if not bad:
                            break
                        f[bad, 1] -= 1
                out.append((("q2_" if q2 else "") + f"loc_{w}x{h}_T{T}_{cn}_n{n}", w, h, T, 0.6, 4200 + gi, f, cx, cy))
        out.append((f"loc_{w}x{h}_T{T}_empty", w, h, T, 0.0, 4300 + gi, _rand_feats(rng, 8, 40, 40), w // 2, h // 2))   # Q4 input
    return out


def check_local_case(case):
    name, w, h, T, _, _, f, cx, cy = case
    ox, oy = (int(cx / T) - 8) * T, (int(cy / T) - 8) * T
    ok = in_mat([(int(x) + ox, int(y) + oy) for x, y in f[:, :2]], w, h, T, 15 * (w // T) + 16)
    assert (not all(ok)) if name.startswith("q2_") else all(ok), name


# ---- Detector::match on quantized images -----------------------------------------------------------------------------
def _pyramid(rng, w0, h0, levels, M, density):
    return [synth.random_quantized(rng, w0 >> l, h0 >> l, density) for l in range(levels) for _ in range(M)]


def _count_bank(class_id, levels, M, counts, w, h, seed, bbox=48):
    """One pyramid per entry of counts, every template of it with that many features (inside its declared size)."""
    rng = np.random.default_rng(seed)
    b = TemplateBank(class_id, levels, M)
    for n in counts:
        ox, oy = int(rng.integers(0, w - bbox)), int(rng.integers(0, h - bbox))
        tl = []
        for l in range(levels):
            for _ in range(M):
                s = max(bbox >> l, 2)
                tl.append(dict(width=s, height=s, offset_x=ox >> l, offset_y=oy >> l, pyramid_level=l, features=_rand_feats(rng, n, s, s)))
        b.add_pyramid(tl)
    return b


def match_cases():
    """name -> dict(qs, w0, h0, T, banks (insertion order), thresholds, class_ids, min_matches).  Built lazily: call it."""
    out = {}

    def add(name, w0, h0, T, M, seed, density, classes, n, thresholds, class_ids=(), planted=0.3, bbox=64, min_matches=1, qs=None):
        levels = len(T)
        if qs is None:
            qs = _pyramid(np.random.default_rng(seed), w0, h0, levels, M, density)
        banks = [synth.make_bank(c, n, levels, M, w0, h0, seed=seed + 7 * i + 1, qs=qs, planted_frac=planted, bbox=bbox)
                 for i, c in enumerate(classes)]
        out[name] = dict(qs=qs, w0=w0, h0=h0, T=T, M=M, banks=banks, thresholds=thresholds, class_ids=tuple(class_ids),
                         min_matches=min_matches)

    add("match_1level_2mod", 320, 240, [8], 2, 5001, 0.05, ["obj"], 24, [70.0])
    add("match_2level_2mod", 320, 240, [5, 8], 2, 5002, 0.05, ["obj"], 24, [60.0, 75.0])
    add("match_3level_2mod", 640, 480, [5, 8, 4], 2, 5003, 0.05, ["obj"], 24, [0.0, 60.0])
    add("match_2level_1mod_classes_out_of_order", 320, 240, [4, 8], 1, 5004, 0.3, ["zeta", "alpha", "mid"], 12, [65.0], bbox=96)
    add("match_class_filter_duplicate_and_unknown", 320, 240, [4, 8], 1, 5004, 0.3, ["zeta", "alpha", "mid"], 12, [65.0],
        class_ids=("mid", "nope", "mid"), bbox=96)
    add("match_class_filter_unknown_only", 320, 240, [4, 8], 1, 5004, 0.3, ["zeta", "alpha", "mid"], 12, [65.0], class_ids=("nope",),
        bbox=96, min_matches=0)
    add("match_thresholds", 320, 240, [5, 8], 2, 5005, 0.3, ["obj"], 6, [-100.0, -30.0, 0.0, 50.0, 75.0, 100.0], bbox=32, min_matches=0)
    add("match_more_than_2048", 320, 240, [8], 1, 5006, 0.9, ["obj"], 6, [-100.0], min_matches=2049)
    # Q4: nothing at the fine level, so every refinement window is all zero and the argmax stays (-1, -1)
    qs = _pyramid(np.random.default_rng(5007), 160, 120, 2, 1, 0.5)
    qs[0][:] = 0
    add("match_q4_empty_fine_level", 160, 120, [4, 5], 1, 5007, 0.5, ["obj"], 4, [-100.0, 0.0], bbox=32, qs=qs)
    # many ties in similarity and template id: one pyramid repeated, few features
    b = _count_bank("obj", 1, 1, [2, 2, 2, 2], 160, 120, 5008, bbox=16)
    qs = _pyramid(np.random.default_rng(5008), 160, 120, 1, 1, 0.7)
    out["match_many_ties"] = dict(qs=qs, w0=160, h0=120, T=[8], M=1, banks=[b], thresholds=[50.0, 99.0], class_ids=(), min_matches=1)
    return out


def sorted_banks(case):
    return sorted(case["banks"], key=lambda b: b.class_id)


def matched_banks(case):
    """The banks Detector::match visits, each once, in std::map order, and their indices in that order."""
    srt = sorted_banks(case)
    keep = [i for i, b in enumerate(srt) if not case["class_ids"] or b.class_id in case["class_ids"]]
    return [srt[i] for i in keep], keep


def canonical(raw):
    """The project's canonical order (similarity descending, template id ascending, then class, y, x) and then std::unique
    with Match::operator== (x, y, similarity, class; NOT template id): adjacent repeats only."""
    m = np.array(raw, MATCH_DTYPE)
    if len(m) == 0:
        return m
    m = m[np.lexsort((m["x"], m["y"], m["class_idx"], m["template_id"], -m["similarity"]))]
    keep = np.ones(len(m), bool)
    last = 0
    for i in range(1, len(m)):
        a, b = m[last], m[i]
        if a["x"] == b["x"] and a["y"] == b["y"] and a["similarity"] == b["similarity"] and a["class_idx"] == b["class_idx"]:
            keep[i] = False
        else:
            last = i
    return m[keep]


def matches_equal(a, b):
    return (len(a) == len(b) and all(np.array_equal(a[k], b[k]) for k in ("x", "y", "class_idx", "template_id"))
            and np.array_equal(a["similarity"].view(np.uint32), b["similarity"].view(np.uint32)))


# ---- quantizedNormals ------------------------------------------------------------------------------------------------
NORMAL_THRESHOLDS = [(2000, 50), (2000, 400), (2000, 401), (65535, 5000), (65535, 65535), (2000, 1), (2000, 0), (2000, -3)]


def normals_unsafe(depth, dist_thr, diff_thr):
    """Pixels where the reference would index NORMAL_LUT outside [0, 20)^3: |nz| of the unit normal below 1e-3 with a
    non-zero normal (then int(nz * 20 + 20) can be 20, and nx or ny can round to 1.0f).  Exact integer sums in int64, as the
    reference's `long`; the float part only as a margin, in double."""
    d = depth.astype(np.int64)
    h, w = d.shape
    r = 5
    if h <= 2 * r + 1 or w <= 2 * r + 1:
        return np.zeros((h, w), bool)
    c = d[r:h - r - 1, r:w - r - 1]
    A0 = np.zeros_like(c); A1 = np.zeros_like(c); A3 = np.zeros_like(c); b0 = np.zeros_like(c); b1 = np.zeros_like(c)
    for j in (-r, 0, r):
        for i in (-r, 0, r):
            if i == 0 and j == 0:
                continue
            delta = d[r + j:h - r - 1 + j, r + i:w - r - 1 + i] - c
            f = (np.abs(delta) < diff_thr).astype(np.int64)
            A0 += f * i * i; A1 += f * i * j; A3 += f * j * j; b0 += f * i * delta; b1 += f * j * delta
    det = A0 * A3 - A1 * A1
    nx, ny, nz = (617 * (A3 * b0 - A1 * b1)).astype(np.float64), (617 * (-A1 * b0 + A0 * b1)).astype(np.float64), (-det * c).astype(np.float64)
    norm = np.sqrt(nx * nx + ny * ny + nz * nz)
    bad = (c < dist_thr) & (norm > 0) & (np.abs(nz) < 1e-3 * norm)
    out = np.zeros((h, w), bool)
    out[r:h - r - 1, r:w - r - 1] = bad
    return out


def _normals_base(kind, w, h, rng, dist_thr):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "plane":
        d = 600 + 1.7 * xx + 0.9 * yy + rng.integers(0, 3, (h, w))
    elif kind == "steps":
        d = 500 + 300 * rng.integers(0, 4, (h // 8 + 1, w // 8 + 1)).repeat(8, 0).repeat(8, 1)[:h, :w] + rng.integers(0, 20, (h, w))
    elif kind == "zeros":
        d = 700 + 0.5 * xx + 2.0 * yy + rng.integers(0, 4, (h, w))
        d[rng.random((h, w)) < 0.03] = 0
        d[h // 3:h // 3 + 7, w // 4:w // 4 + 9] = 0
    elif kind == "around_threshold":
        d = min(dist_thr, 65534) + rng.integers(-2, 2, (h, w)) + (xx // 6) % 3 - 1
    elif kind == "rough":
        d = rng.integers(0, 65536, (h, w))
    elif kind == "deep":
        d = 65535 - 3 * xx - 2 * yy - rng.integers(0, 30, (h, w))
    return np.clip(d, 0, 65535).astype(np.uint16)


def normals_cases():
    """(name, kind, w, h, dist_thr, diff_thr, seed)."""
    out = []
    kinds = ["plane", "steps", "zeros", "around_threshold", "rough", "deep"]
    for si, (w, h) in enumerate([(23, 17), (64, 48), (97, 61)]):
        for ki, kind in enumerate(kinds):
            for ti, (dt, ft) in enumerate(NORMAL_THRESHOLDS):
                if kind == "deep" and dt < 65535:
                    continue
                if (si, ki) != (1, 2) and kind not in ("rough", "deep") and ti not in (0, (si + ki) % len(NORMAL_THRESHOLDS)):
                    continue                                # every pair on zeros at 64x48, on rough and on deep; two elsewhere
                out.append((f"normals_{kind}_{w}x{h}_{dt}_{ft}", kind, w, h, dt, ft, 6000 + 100 * si + 10 * ki + ti))
    out.append(("normals_steps_640x480_2000_50", "steps", 640, 480, 2000, 50, 6900))
    out.append(("normals_rough_640x480_65535_5000", "rough", 640, 480, 65535, 5000, 6901))
    return out


def normals_input(case):
    _, kind, w, h, dt, ft, seed = case
    d = _normals_base(kind, w, h, np.random.default_rng(seed), dt)
    for _ in range(64):                                     # push unsafe pixels behind distance_threshold (their neighbours change: repeat)
        bad = normals_unsafe(d, dt, ft)
        if not bad.any():
            return d
        d[bad] = 65535
    raise AssertionError(case[0])


# ---- hysteresisGradient ----------------------------------------------------------------------------------------------
AMBIGUOUS_ANGLES = np.array([123.749992, 213.749985], np.float32)     # float and double products round differently: left out


def angles_unambiguous(angle):
    a = np.asarray(angle, np.float32)
    return bool(np.array_equal(np.rint(a.astype(np.float64) * (16.0 / 360.0)), np.rint(a * np.float32(16.0 / 360.0)).astype(np.float64)))


def edge_angles():
    """The 16 bin edges 11.25 + 22.5 k, their float neighbours, 348.75 .. 360 and 0: without the two ambiguous floats."""
    e = (11.25 + 22.5 * np.arange(16)).astype(np.float32)
    pool = np.concatenate([e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(400)),
                           np.array([0.0, 348.75, 350.0, 355.5, 359.99997, 360.0], np.float32),
                           (22.5 * np.arange(17)).astype(np.float32)])
    return pool[~np.isin(pool, AMBIGUOUS_ANGLES)]


def hysteresis_cases():
    return [(f"hyst_{kind}_{w}x{h}", kind, w, h, 7000 + 10 * i + j) for i, (w, h) in enumerate([(23, 17), (64, 48), (97, 61), (3, 3), (640, 480)])
            for j, kind in enumerate(["random", "blocks", "edges"])]


def hysteresis_input(case):
    """(magnitude, angle, threshold): magnitudes are integers as the reference's (sums of two squares), many equal to the
    threshold; `blocks` and `edges` keep 4x4 blocks in one bin so that the 5-of-9 vote passes."""
    _, kind, w, h, seed = case
    rng = np.random.default_rng(seed)
    thr = 100.0
    mag = rng.choice(np.array([0, 99, 100, 101, 5000], np.float32), (h, w))
    if kind == "random":
        ang = rng.uniform(0, 360, (h, w)).astype(np.float32)
    else:
        pool = edge_angles() if kind == "edges" else (22.5 * rng.integers(0, 16, 64) + rng.uniform(-11, 11, 64)).astype(np.float32) % np.float32(360)
        blocks = rng.integers(0, len(pool), (h // 4 + 1, w // 4 + 1)).repeat(4, 0).repeat(4, 1)[:h, :w]
        noise = rng.random((h, w)) < 0.15
        blocks[noise] = rng.integers(0, len(pool), int(noise.sum()))
        ang = pool[blocks]
    ang = np.ascontiguousarray(ang, np.float32)
    ang[np.isin(ang, AMBIGUOUS_ANGLES)] = 0                 # a uniform draw could hit one of the two; the pools never hold them
    return mag, np.ascontiguousarray(ang, np.float32), thr


# ---- cropTemplates -------------------------------------------------------------------------
def crop_cases():
    """(name, templates, features): un-cropped pyramids (absolute features per level, offsets that differ per level)."""
    out = []
    for i, (levels, M, x0, y0) in enumerate([(1, 1, 10, 20), (2, 2, 101, 57), (3, 2, 33, 64), (2, 1, 0, 1), (3, 1, 255, 129)]):
        rng = np.random.default_rng(9000 + i)
        t = np.zeros(levels * M, TEMPLATE_DTYPE)
        fs = []
        for k in range(levels * M):
            lv = k // M
            n = int(rng.integers(1, 20))
            f = np.zeros(n, FEATURE_DTYPE)
            f["x"] = (x0 >> lv) + rng.integers(0, max(1, 90 >> lv), n)
            f["y"] = (y0 >> lv) + rng.integers(0, max(1, 70 >> lv), n)
            f["label"] = rng.integers(0, 8, n)
            t[k]["width"] = t[k]["height"] = -1
            t[k]["pyramid_level"], t[k]["feat_begin"], t[k]["feat_count"] = lv, sum(len(a) for a in fs), n
            fs.append(f)
        out.append((f"crop_L{levels}_M{M}_{x0}_{y0}", t, np.concatenate(fs)))
    return out


def check_crop_case(case):
    _, t, f = case
    assert len(f) > 0 and f["x"].min() >= 0 and f["y"].min() >= 0        # << of a negative int, min over nothing: undefined


# ---- the two back ends ---------------------------------------------------------------------------------------------------
class OracleBackend:
    """oracle_py under the method names of reference_py.Ref."""

    def __init__(self, O):
        self.O = O
        for k in ("spread", "response_maps", "linearize", "similarity", "similarity_local", "quantized_normals", "hysteresis_gradient",
                  "crop_templates"):
            setattr(self, k, getattr(O, k))

    def build_linear_memories(self, q, T, stride):
        out = self.O.build_linear_memories(q, T)
        assert out.shape[1] == stride
        return out

    def total_similarity(self, lms, templs, w, h, T):
        b = TemplateBank("obj", 1, len(templs))
        b.add_pyramid([dict(width=int(t["width"][0]), height=int(t["height"][0]), offset_x=0, offset_y=0, pyramid_level=0,
                            features=np.stack([f["x"], f["y"], f["label"]], 1)) for t, f in templs])
        return self.O.total_similarity(lms, b, 0, w, h, T)

    def match(self, case, threshold):
        banks, keep = matched_banks(case)
        if not banks:
            return np.zeros(0, MATCH_DTYPE)
        m, n = self.O.match_quantized(case["qs"], case["w0"], case["h0"], case["T"], banks, threshold)
        assert n == len(m)
        m = m.copy()
        m["class_idx"] = np.array(keep, np.int32)[m["class_idx"]]
        return m


class ReferenceBackend:
    """One build of the compiled reference (reference_py.Ref)."""

    def __init__(self, R):
        self.R = R
        for k in ("spread", "response_maps", "linearize", "build_linear_memories", "similarity", "similarity_local", "quantized_normals",
                  "hysteresis_gradient", "crop_templates"):
            setattr(self, k, getattr(R, k))

    def total_similarity(self, lms, templs, w, h, T):
        return self.R.add_similarities([self.R.similarity(lm, t, f, w, h, T) for lm, (t, f) in zip(lms, templs)])

    def match_lists(self, case, threshold):
        """(final, raw) with class_idx mapped to the index in sorted class order."""
        fin, raw = self.R.match_quantized(case["qs"], case["w0"], case["h0"], case["T"], case["banks"], threshold, case["class_ids"])
        srt = [b.class_id for b in sorted_banks(case)]
        remap = np.array([srt.index(b.class_id) for b in case["banks"]], np.int32)
        fin, raw = fin.copy(), raw.copy()
        fin["class_idx"], raw["class_idx"] = remap[fin["class_idx"]], remap[raw["class_idx"]]
        return fin, raw

    def match(self, case, threshold):
        return canonical(self.match_lists(case, threshold)[1])


# ---- one case on one back end ------------------------------------------------------------------------------------------
def _with_inputs(out, *ins):
    out["__in__"] = digest(np.concatenate([digest(a) for a in ins]))
    return out


def _refusable(out, key, fn):
    try:
        out[key] = fn()
    except AssertionError:                                  # the reference's CV_Assert: both sides must refuse
        out[key + "_refused"] = np.ones(1, np.uint8)


def compute_spread(B, case):
    q = spread_input(case)
    out = {"spread": B.spread(q, case[3])}
    _refusable(out, "maps", lambda: B.response_maps(out["spread"]))
    return _with_inputs(out, q)


def compute_lut(B, case=None):
    s = np.arange(256, dtype=np.uint8).reshape(16, 16)      # all 256 spread bytes
    return _with_inputs({"maps": B.response_maps(s)}, s)


def linearize_input(case):
    _, w, h, T, dens, seed = case
    rng = np.random.default_rng(seed)
    return synth.random_quantized(rng, w, h, dens), rng.integers(0, 5, (h, w)).astype(np.uint8)


def compute_linearize(B, case):
    _, w, h, T, dens, seed = case
    q, m = linearize_input(case)
    out = {}
    _refusable(out, "lin", lambda: B.linearize(m, T))
    _refusable(out, "lm", lambda: B.build_linear_memories(q, T, lm_stride(w, h, T)))
    return _with_inputs(out, q, m)


def _sim_lm(B, w, h, T, dens, seed):
    q = synth.random_quantized(np.random.default_rng(seed), w, h, dens)
    return q, B.build_linear_memories(q, T, lm_stride(w, h, T))


def compute_similarity(B, case):
    name, w, h, T, dens, seed, width, height, feats = case
    q, lm = _sim_lm(B, w, h, T, dens, seed)
    t, f = _templ(width, height, feats)
    return _with_inputs({"sim": B.similarity(lm, t, f, w, h, T)}, q, t, f)


def compute_local(B, case):
    name, w, h, T, dens, seed, feats, cx, cy = case
    q, lm = _sim_lm(B, w, h, T, dens, seed)
    t, f = _templ(40, 40, feats)
    return _with_inputs({"loc": B.similarity_local(lm, t, f, w, h, T, cx, cy)}, q, t, f, np.array([cx, cy]))


def total_cases():
    """(name, first, second): two non-Q2 similarity cases of one geometry; totals with one and with two modalities."""
    cs = [c for c in similarity_cases() if c[0].startswith("sim_") and c[0].split("_n")[-1] in ("1", "8", "63")]
    return [(f"total_{a[0][4:]}_{b[0].split('_')[-1]}", a, b) for a, b in zip(cs, cs[1:]) if a[1:4] == b[1:4]]


def compute_total(B, case):
    _, a, b = case
    w, h, T = a[1:4]
    qa, lma = _sim_lm(B, w, h, T, a[4], a[5])
    qb, lmb = _sim_lm(B, w, h, T, 0.3, b[5] + 50)
    ta, tb = _templ(a[6], a[7], a[8]), _templ(b[6], b[7], b[8])
    out = {"one": B.total_similarity([lma], [ta], w, h, T), "two": B.total_similarity([lma, lmb], [ta, tb], w, h, T)}
    return _with_inputs(out, qa, qb, *ta, *tb)


def coarse_templates(bank, p):
    """[(template record, its features)] of pyramid p at the coarsest level, one per modality."""
    t, f, _ = bank.arrays()
    L, M = bank.levels, bank.modalities
    out = []
    for m in range(M):
        hdr = t[(p * L + L - 1) * M + m:(p * L + L - 1) * M + m + 1].copy()
        fr = f[int(hdr["feat_begin"][0]):int(hdr["feat_begin"][0]) + int(hdr["feat_count"][0])].copy()
        hdr["feat_begin"] = 0
        out.append((hdr, fr))
    return out


def compute_match(B, case):
    """The canonical match list per threshold, and the u16 total similarity map of every pyramid at the coarsest level
    (classes in std::map order)."""
    L, M, T = len(case["T"]), case["M"], case["T"][-1]
    wl, hl = case["w0"] >> (L - 1), case["h0"] >> (L - 1)
    out = {f"matches_{thr:g}": B.match(case, thr) for thr in case["thresholds"]}
    lms = [B.build_linear_memories(case["qs"][(L - 1) * M + m], T, lm_stride(wl, hl, T)) for m in range(M)]
    out["sims"] = np.stack([B.total_similarity(lms, coarse_templates(b, p), wl, hl, T) for b in sorted_banks(case) for p in range(b.n_pyramids)])
    ins = list(case["qs"])
    for b in case["banks"]:
        ins += list(b.arrays()[:2])
    return _with_inputs(out, *ins)


def compute_normals(B, case):
    d = normals_input(case)
    return _with_inputs({"qn": B.quantized_normals(d, case[4], case[5])}, d)


def compute_hysteresis(B, case):
    mag, ang, thr = hysteresis_input(case)
    return _with_inputs({"q": B.hysteresis_gradient(mag, ang, thr)}, mag, ang)


def compute_crop(B, case):
    _, t, f = case
    to, fo, bb = B.crop_templates(t, f)
    return _with_inputs({"templates": to, "features": fo, "bb": np.array(bb, np.int32)}, t, f)


def groups():
    """group -> (list of (name, case), compute).  The whole case list, in one place."""
    mc = match_cases()
    return {
        "spread": ([(c[0], c) for c in spread_cases()], compute_spread),
        "lut": ([("lut_all_256_bytes", None)], compute_lut),
        "linearize": ([(c[0], c) for c in linearize_cases()], compute_linearize),
        "similarity": ([(c[0], c) for c in similarity_cases()], compute_similarity),
        "local": ([(c[0], c) for c in local_cases()], compute_local),
        "total": ([(c[0], c) for c in total_cases()], compute_total),
        "match": ([(k, v) for k, v in mc.items()], compute_match),
        "normals": ([(c[0], c) for c in normals_cases()], compute_normals),
        "hysteresis": ([(c[0], c) for c in hysteresis_cases()], compute_hysteresis),
        "crop": ([(c[0], c) for c in crop_cases()], compute_crop),
    }


def simd_takes(group, case):
    """The SIMD build's spread needs w % 16 == 0 (aligned 16-byte stores at every row start): decided by the case alone."""
    if group in ("spread", "linearize"):
        return case[1] % 16 == 0
    return True


def same(a, b):
    """Two output dicts agree bit for bit; returns the first key that does not, or None."""
    if sorted(a) != sorted(b):
        return f"keys {sorted(a)} != {sorted(b)}"
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return k
    return None


# ======================================================================================================================
# The ICP half: icpCloudToCloud_Ex and its helpers, detection(), depthTo3d, nonMaximumSuppression
# ======================================================================================================================
FLT_MAX = float(np.finfo(np.float32).max)
RUN_ALL = (0.0, -3.0e38)                                    # every iteration runs; the suite's other two: (0.3, 0.01), (0.5, 0.01)
EDGE_INDICES = (0, 63, 64, 255, 256, -1)                    # first / last lane of a wave, of a 256-thread workgroup, last point


def fbits(a):
    """float32 -> uint32 bit patterns; every NaN as the one quiet NaN (a NaN's sign and payload carry no meaning)."""
    a = np.ascontiguousarray(a, np.float32)
    out = a.view(np.uint32).copy()
    out[np.isnan(a)] = 0x7FC00000
    return out


@functools.lru_cache(maxsize=None)
def _object_pool(seed, n, noise):
    rng = np.random.default_rng(seed)
    R, t = synth.object_pose(tz=650.0)
    depth, _, mask = synth.render(640, 480, R, t, seed=seed, noise=True, background=False)
    ys, xs = np.nonzero(mask)
    sel = rng.choice(len(ys), size=min(n, len(ys)), replace=False)
    sel.sort()
    z = depth[ys[sel], xs[sel]].astype(np.float32)
    ref = np.stack([(xs[sel] - 320.0) / 608.0 * z, (ys[sel] - 240.0) / 608.0 * z, z], 1).astype(np.float32)
    dR = synth.rot_z(0.02) @ synth.rot_x(-0.015) @ synth.rot_y(0.01)
    c = ref.mean(0)
    model = ((ref - c) @ dR.T + c + np.array([1.5, -2.0, 1.0])).astype(np.float32)
    model += rng.normal(0, noise, model.shape).astype(np.float32)
    return ref, model


def object_clouds(seed, n=6000, noise=0.3):
    """A paired cloud: reference = points on the synthetic object, model = rigidly perturbed copy (the clouds of
    tests/test_gpu_icp.py)."""
    ref, model = _object_pool(seed, n, noise)
    return ref.copy(), model.copy()


def _shuffled(seed, n):
    """n pairs of the object clouds in random order: both ends of the arrays are inliers, not the object's outline."""
    ref, model = object_clouds(1 + seed % 4, 1500)             # four renders serve every case; the seed picks and orders the points
    p = np.random.default_rng(seed + 1000).permutation(len(ref))[:n]
    return ref[p].copy(), model[p].copy()


def _invalidate(a, n):
    """z > 900 and z = NaN at the edge indices; and the bound itself: z = 900 is valid, the next float is not."""
    for k, i in enumerate(EDGE_INDICES):
        if i < n:
            a[i, 2] = np.float32(950.0 + k) if k % 2 == 0 else np.float32(np.nan)
    a[n // 2, 2] = np.float32(900.0)
    a[n // 2 + 1, 2] = np.nextafter(np.float32(900.0), np.float32(1000.0))


def icp_cases():
    """(name, kind, n_model, n_ref, seed, icp_it_thr, dist_mean_thr, dist_diff_thr)."""
    out = []
    sizes = [3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1500]
    for i, n in enumerate(sizes):
        out.append((f"icp_clean_{n}", "clean", n, n, 100 + i, 8, *RUN_ALL))
    out.append(("icp_clean_257_1025", "clean", 257, 1025, 120, 8, *RUN_ALL))
    out.append(("icp_clean_1024_1500", "clean", 1024, 1500, 121, 8, *RUN_ALL))
    out.append(("icp_refused_2_2", "clean", 2, 2, 122, 8, *RUN_ALL))
    for i, n in enumerate((65, 257, 1025)):
        for kind in ("invalid_model", "invalid_ref", "invalid_both", "nan_valid_model", "nan_valid_ref", "far", "all_invalid_model", "all_invalid_ref"):
            out.append((f"icp_{kind}_{n}", kind, n, n, 200 + 10 * i + len(kind), 3 if kind.startswith("all_invalid") else 8, *RUN_ALL))
        out.append((f"icp_identical_{n}", "identical", n, n, 300 + i, 8, 0.0, 0.01))
        out.append((f"icp_growing_{n}", "growing", n, n, 310 + i, 8, 0.0, 0.0))     # the reference's default thresholds: only a rise ends it
        for it in (0, 1, 2):
            out.append((f"icp_clean_{n}_it{it}", "clean", n, n, 320 + i, it, *RUN_ALL))
        for a, b in ((0.3, 0.01), (0.5, 0.01)):
            out.append((f"icp_clean_{n}_thr{a:g}", "clean", n, n, 330 + i, 8, a, b))
        out.append((f"tie_icp_duplicate_ref_{n}", "tie", n, n, 340 + i, 8, *RUN_ALL))
    return out


def icp_input(case):
    """(ref, model) float32 clouds of a case."""
    _, kind, nm, nr, seed, *_ = case
    ref, model = _shuffled(seed, max(nm, nr))
    model = model[:nm].copy()
    rng = np.random.default_rng(seed + 5)
    if kind in ("invalid_model", "invalid_both"):
        _invalidate(model, nm)
    if kind in ("invalid_ref", "invalid_both"):
        _invalidate(ref[::-1] if kind == "invalid_both" else ref, nr)     # both: the mirrored indices, so that pairs lose one side each
    if kind == "nan_valid_model":
        model[1] = (np.nan, np.nan, 500.0)                    # "valid" (z <= 900) and poisons the first centroid
    if kind == "nan_valid_ref":
        ref[1] = (np.nan, np.nan, 500.0)
    if kind == "far":
        # sparse points in a 600 mm cube, every model point 8 to 12 mm from its partner: after the first pass the squared
        # distances (~100) are above 3 * dist_mean (~30), so fewer than 3 pairs survive
        ref = np.stack([rng.uniform(-300, 300, nr), rng.uniform(-300, 300, nr), rng.uniform(300, 800, nr)], 1).astype(np.float32)
        d = rng.normal(size=(nm, 3))
        d *= (rng.uniform(8, 12, nm) / np.linalg.norm(d, axis=1))[:, None]
        model = (ref[:nm] + d).astype(np.float32)
    if kind == "all_invalid_model":                           # copyPoints turns every point into (0, 0, 0), which is valid
        model[:, 2] = np.float32(950.0)
    if kind == "all_invalid_ref":                             # the reference cloud is used as it is: counter == 0, FLT_MAX
        ref[:, 2] = np.float32(950.0)
    if kind == "identical":
        model = ref[:nm].copy()
    if kind == "growing":
        # model point i lies on reference point i + 1 of the cloud sorted by x.  The first pass trusts the pairing by index
        # and shifts the model towards its partners; the nearest-neighbour passes pull it back onto the points it lies on, so
        # the mean distance of the index pairs, which is what the loop watches, goes up again
        pool = object_clouds(1 + seed % 4, 1500)[0]
        pool = pool[np.argsort(pool[:, 0], kind="stable")][::len(pool) // (nr + 1)][:nr + 1]
        ref = pool[:nr].copy()
        model = (pool[1:nm + 1] + rng.normal(0, 0.05, (nm, 3))).astype(np.float32)
    if kind == "tie":
        ref[nr // 3] = ref[nr // 7]                          # two reference points at one place: every search near them ties
    return np.ascontiguousarray(ref, np.float32), np.ascontiguousarray(model, np.float32)


def nn_ties(O, ref, model, it, dist_mean_thr, dist_diff_thr):
    """How many searches of the loop (over the iterations actually run, from the oracle's brute-force trace) find two
    reference points at exactly the smallest float32 squared distance of a model point."""
    ref, model = np.ascontiguousarray(ref, np.float32), np.ascontiguousarray(model, np.float32)
    if len(model) < 3 or len(ref) < 3 or it < 1:
        return 0
    r = O.icp(ref, model, it, dist_mean_thr, dist_diff_thr, accum64=False, use_kdtree=False, trace=True)
    state = O.copy_points(model)
    ties = 0
    for row in r["trace"]:
        if np.isnan(row[0]):                                  # the pass never reached the SVD: the loop had ended
            break
        Ropt, Topt = row[11:20], row[20:23]
        if np.isfinite(Ropt).all() and np.isfinite(Topt).all():
            state = O.transform_points(state, Ropt, Topt, in_place=True)
        ties += O.nn_tie_count(ref, state)
    return ties


def check_icp_case(O, case):
    name, kind, nm, nr, seed, it, a, b = case
    ref, model = icp_input(case)
    assert len(ref) == nr and len(model) == nm and nm <= nr, name
    ties = nn_ties(O, ref, model, it, a, b)
    assert (ties > 0) if name.startswith("tie_") else (ties == 0), (name, ties)
    # the cases that are there for one path of the loop take it (the oracle's reading; the comparison decides if it is right)
    r = O.icp(ref, model, it, a, b, use_kdtree=False)
    if kind == "far":
        assert r["iters"] == it and r["n_corr_last"] < 3, (name, r["iters"], r["n_corr_last"])
    if kind == "identical":
        assert r["iters"] == 0 and r["dist_mean"] == 0, name
    if kind == "growing":
        dm = [O.icp(ref, model, i, *RUN_ALL, use_kdtree=False)["dist_mean"] for i in range(it + 1)]
        assert 0 < r["iters"] < it and dm[r["iters"]] > dm[r["iters"] - 1], (name, r["iters"], dm)
    if kind == "all_invalid_ref":
        assert O.icp(ref, model, 0, a, b)["dist_mean"] == np.float32(FLT_MAX), name


def _icp_state(r):
    return np.concatenate([fbits(r["R"]).ravel(), fbits(r["T"]), fbits([r["dist_mean"], r["px_ratio"]])])


def compute_icp(B, case):
    """The result of every prefix icp_it_thr = 0 .. N (the prefix runs are the per-iteration trace): R, T, dist_mean and
    px_ratio as bit patterns, and `iter` on exit."""
    name, kind, nm, nr, seed, it, a, b = case
    ref, model = icp_input(case)
    runs = [B.icp(ref, model, i, a, b) for i in range(it + 1)]
    out = {"states": np.stack([_icp_state(r) for r in runs]), "iters": np.array([r["iters"] for r in runs], np.int32)}
    return _with_inputs(out, ref, model, np.array([it]), np.array([a, b], np.float32))


# ---- the helpers of the loop, one by one -----------------------------------------------------------------------------
def helper_cases():
    return [(f"helpers_{kind}_{n}", kind, n, 400 + i) for i, n in enumerate((4, 65, 257, 1025)) for kind in ("clean", "invalid_both", "nan_valid_model")]


def compute_helpers(B, case):
    name, kind, n, seed = case
    ref, model = icp_input((name, kind, n, n, seed, 0, 0.0, 0.0))
    R = (synth.rot_z(0.3) @ synth.rot_x(-0.2)).astype(np.float32)
    T = np.array([3.5, -20.25, 100.125], np.float32)          # lifts some z above 900: they turn invalid
    out = {"mean_model": fbits(B.get_mean(model)), "mean_ref": fbits(B.get_mean(ref)), "copy": fbits(B.copy_points(model)),
           "transform_fresh": fbits(B.transform_points(model, R, T, False)), "transform_in_place": fbits(B.transform_points(model, R, T, True))}
    moved = B.transform_points(B.copy_points(model), R, T, True)
    for k, thr in (("all", FLT_MAX), ("3", 3.0), ("none", -1.0)):
        ratio, dm = B.l2dist_clouds(model, ref, thr)
        out["l2_" + k] = fbits([ratio, dm])
    out["l2_short_model"] = fbits(B.l2dist_clouds(model[:n // 2], ref))
    for k, thr in (("all", FLT_MAX), ("9", 9.0), ("none", -1.0)):   # the threshold meets SQUARED distances here
        cr, cm = B.points_corresponding(ref, model, thr)
        out["pairs_" + k] = np.concatenate([fbits(cr).ravel(), fbits(cm).ravel()])
        out["n_pairs_" + k] = np.array([len(cm)], np.int32)
    return _with_inputs(out, ref, model)


# ---- detection() -----------------------------------------------------------------------------------------------------
DET_W, DET_H = 176, 56                                      # a frame that just holds the largest crop and room to place it
MODEL_K = (608.0, 608.0, 320.0, 240.0)                      # initInternalMat: the model's intrinsics are fixed
SCENE_K = (571.3, 569.9, 91.25, 26.5)


def _det_surface(rng, dx, dy):
    yy, xx = np.mgrid[0:DET_H, 0:DET_W].astype(np.float64)
    z = 600 + 40 * np.sin((xx - dx) / 17.0) + 30 * np.cos((yy - dy) / 9.0) + 0.5 * (xx - dx) + rng.normal(0, 0.6, (DET_H, DET_W))
    return np.clip(np.rint(z), 1, 65535).astype(np.uint16)


def detection_cases():
    """(name, seed, rect_model, rect_ref, K, holes, icp_it_thr, dist_mean_thr, dist_diff_thr, rotated)."""
    out = []
    crops = [(63, 3), (64, 4), (65, 5), (130, 41), (64, 41), (65, 3), (130, 4), (63, 5)]
    for i, (cw, ch) in enumerate(crops):
        rm = (3 + i, 2 + i % 3, cw, ch)
        rr = (DET_W - cw, DET_H - ch, cw, ch) if i % 2 == 0 else (7 + 2 * i, 1 + i % 4, cw, ch)   # even: flush right and bottom
        K = SCENE_K if i % 3 else MODEL_K
        thr = (8, *RUN_ALL) if i % 2 == 0 else (10, 0.5, 0.01)
        out.append((f"det_{cw}x{ch}", 500 + i, rm, rr, K, "some", *thr, i % 2 == 1))
    out.append(("det_model_flush_130x41", 520, (DET_W - 130, DET_H - 41, 130, 41), (0, 0, 130, 41), SCENE_K, "some", 8, *RUN_ALL, True))
    out.append(("det_no_holes_65x5", 521, (10, 10, 65, 5), (20, 30, 65, 5), MODEL_K, "none", 8, *RUN_ALL, False))
    out.append(("det_two_valid_pairs_64x4", 522, (5, 5, 64, 4), (30, 40, 64, 4), SCENE_K, "all_but_2", 8, *RUN_ALL, True))
    out.append(("det_no_valid_pair_63x3", 523, (5, 5, 63, 3), (30, 40, 63, 3), SCENE_K, "all", 8, *RUN_ALL, True))
    out.append(("det_refused_rect_leaves_frame", 524, (DET_W - 64, 5, 65, 5), (30, 40, 65, 5), SCENE_K, "some", 8, *RUN_ALL, False))
    return out


def detection_input(case):
    """(model_depth, scene_depth, r_match, t_match): u16 frames in mm with holes (0) and pixels beyond 900 mm."""
    name, seed, rm, rr, K, holes, it, a, b, rotated = case
    rng = np.random.default_rng(seed)
    model = _det_surface(rng, 0.0, 0.0)
    scene = _det_surface(rng, rr[0] - rm[0] + 1.5, rr[1] - rm[1] - 0.5)     # the crops see nearly the same piece of surface
    if holes == "some":
        for img in (model, scene):
            img[rng.random(img.shape) < 0.04] = 0
            img[rng.random(img.shape) < 0.03] = rng.integers(901, 3000)
            img[rng.random(img.shape) < 0.01] = 900               # float(900) * float(1/1000.0) * 1000 = 900.00006: beyond the bound
    elif holes in ("all", "all_but_2"):
        keep = [(1, 2), (2, 40)] if holes == "all_but_2" else []
        crop = scene[rr[1]:rr[1] + rr[3], rr[0]:rr[0] + rr[2]]
        saved = [crop[y, x] for y, x in keep]
        crop[:] = 0
        crop[::2, ::3] = 2000
        for (y, x), v in zip(keep, saved):
            crop[y, x] = v
    r_match = (synth.rot_z(0.4) @ synth.rot_y(-0.3) @ synth.rot_x(0.2)).astype(np.float32) if rotated else np.eye(3, dtype=np.float32)
    t_match = np.array([12.5, -7.25, 640.0], np.float32) if rotated else np.array([1.0, 2.0, 3.0], np.float32)
    return model, scene, r_match, t_match


def detection_clouds(O, case):
    """The two clouds detection() hands to icpCloudToCloud_Ex, from the oracle's pieces (for check_detection_case only)."""
    name, seed, rm, rr, K, *_ = case
    model, scene, _, _ = detection_input(case)
    with np.errstate(invalid="ignore"):
        p_ref = (O.depth_to_3d(scene, *K) * np.float32(1000))[rr[1]:rr[1] + rr[3], rr[0]:rr[0] + rr[2]].reshape(-1, 3)
        p_mod = (O.depth_to_3d(model, *MODEL_K) * np.float32(1000))[rm[1]:rm[1] + rm[3], rm[0]:rm[0] + rm[2]].reshape(-1, 3)
        ok = (p_ref[:, 2] <= 900) & (p_mod[:, 2] <= 900)
    p_ref, p_mod = np.ascontiguousarray(p_ref[ok]), np.ascontiguousarray(p_mod[ok])
    if len(p_ref):
        p_mod = O.transform_points(p_mod, np.eye(3, dtype=np.float32), O.get_mean(p_ref) - O.get_mean(p_mod), True)
    return p_ref, p_mod


def check_detection_case(O, case):
    name, seed, rm, rr, K, holes, it, a, b, rotated = case
    assert rm[2:] == rr[2:], name                              # one crop size: matToVec walks both crops with one loop
    inside = all(0 <= r[0] and 0 <= r[1] and r[0] + r[2] <= DET_W and r[1] + r[3] <= DET_H for r in (rm, rr))
    assert inside != name.startswith("det_refused"), name
    if not inside:
        return
    p_ref, p_mod = detection_clouds(O, case)
    model, scene, r_match, t_match = detection_input(case)
    assert O.detection(model, scene, K, rm, rr, it, a, b, r_match, t_match)["n_points"] == len(p_ref), name
    assert (len(p_ref) < 3) == (holes in ("all", "all_but_2")), (name, len(p_ref))
    assert nn_ties(O, p_ref, p_mod, it, a, b) == 0, name


def compute_detection(B, case):
    name, seed, rm, rr, K, holes, it, a, b, rotated = case
    model, scene, r_match, t_match = detection_input(case)
    out = {}
    try:
        r = B.detection(model, scene, K, rm, rr, it, a, b, r_match, t_match)
        out["pose"] = np.concatenate([fbits(r["R_final"]).ravel(), fbits(r["T_final"]), _icp_state(r["icp"])])
        out["counts"] = np.array([r["n_points"], r["icp"]["iters"]], np.int32)
    except AssertionError:                                  # the reference's CV_Assert on the ROI: both sides must refuse
        out["refused"] = np.ones(1, np.uint8)
    return _with_inputs(out, model, scene, r_match, t_match, np.array(rm + rr), np.array(K), np.array([it]), np.array([a, b], np.float32))


# ---- cup_d2pc::depthTo3d ---------------------------------------------------------------------------------------------
def depth3d_cases():
    """(name, w, h, K, seed)."""
    return [(f"d3d_{w}x{h}_{'K' if k else 'Kint'}", w, h, (SCENE_K if k else MODEL_K), 600 + 10 * i + j)
            for i, w in enumerate((63, 64, 65, 130)) for j, h in enumerate((3, 4, 5)) for k in (0, 1) if k == (i + j) % 2 or (w, h) == (65, 5)]


def depth3d_input(case):
    _, w, h, K, seed = case
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 65536, (h, w)).astype(np.uint16)
    d[rng.random((h, w)) < 0.2] = 0
    d.ravel()[[0, 1, 2, w - 1, w * h - 1]] = (0, 1, 65535, 65535, 1)
    return d


def compute_depth3d(B, case):
    d = depth3d_input(case)
    return _with_inputs({"points": fbits(B.depth_to_3d(d, *case[3]))}, d, np.array(case[3]))


# ---- nonMaximumSuppression -------------------------------------------------------------------------------------------
def nms_cases():
    """(name, t [n, 3], n_points [n], icp_dist [n], th_obj_dist).  Translations are small integers, so that every distance
    is exact in whatever order cv::norm forms it."""
    f = np.float32
    five_t = [(0, 0, 600), (30, 40, 600), (0, 0, 651), (300, 0, 600), (330, 40, 600)]          # |t1-t0| = 50, |t2-t0| = 51, |t4-t3| = 50
    out = [("nms_none", np.zeros((0, 3), f), [], [], 60.0), ("nms_one", [(1, 2, 3)], [100], [0.5], 60.0)]
    out.append(("nms_five_both_sides_of_50", five_t, [100, 100, 100, 100, 100], [0.9, 0.5, 0.1, 0.4, 0.6], 50.5))
    out.append(("nms_five_at_the_distance", five_t, [100, 100, 100, 100, 100], [0.9, 0.5, 0.1, 0.4, 0.6], 50.0))   # `<`: 50 is not near
    out.append(("nms_five_all_near", five_t, [100, 100, 100, 100, 100], [0.9, 0.5, 0.1, 0.4, 0.6], 1000.0))
    # the 0.85 rule: more than int(float(n) * 0.85) points, 85 of 100 and 17 of 21 (17.85 truncates); `>` decides
    out.append(("nms_size_rule_100", [(0, 0, 600)] * 4, [100, 85, 86, 84], [0.9, 0.1, 0.5, 0.05], 10.0))
    out.append(("nms_size_rule_21", [(0, 0, 600)] * 4, [21, 17, 18, 16], [0.9, 0.1, 0.5, 0.05], 10.0))
    out.append(("nms_equal_icp_dist", [(0, 0, 600), (1, 0, 600), (0, 1, 600)], [50, 50, 50], [0.5, 0.5, 0.25], 10.0))
    # the winner so far decides who is near, its opener's size decides the 0.85 rule
    out.append(("nms_winner_moves", [(0, 0, 600), (40, 0, 600), (80, 0, 600), (120, 0, 600)], [100, 90, 50, 99], [0.9, 0.5, 0.1, 0.2], 45.0))
    return [(n, np.asarray(t, f).reshape(-1, 3), np.asarray(p, np.int32), np.asarray(d, f), th) for n, t, p, d, th in out]


def check_nms_case(case):
    name, t, npts, dist, th = case
    assert np.array_equal(t, np.rint(t)) and np.abs(t).max(initial=0) < 4096, name   # sums of squares exact in float32 and in double


def compute_nms(B, case):
    name, t, npts, dist, th = case
    return _with_inputs({"winners": np.array(B.nms(t, npts, dist, th), np.int32)}, t, npts, dist, np.array([th], np.float32))


def _large(key, value):
    return value.size > 256


def recorded(out, digested=_large):
    """What tests/golden/reference_icp.npz keeps of one case's outputs, as one uint8 array: per key in sorted order the array
    itself while it is small (poses, counts, winners) or its digest beyond 256 elements (clouds, pair lists), behind a table
    of their byte lengths.  One array per case keeps the file small: the container's cost is per member.
    tests/golden/reference_extract.npz has the same layout with digested = is_image: images as digests, all else in full."""
    parts = []
    for k in sorted(out):
        v = np.ascontiguousarray(out[k])
        parts.append((digest(v) if digested(k, v) else v).tobytes())
    table = np.array([len(parts)] + [len(p) for p in parts], np.uint32).tobytes()
    return np.frombuffer(table + b"".join(parts), np.uint8).copy()


def same_as_record(out, rec, group, name, digested=_large):
    """The outputs of one case against the record; returns the first key that differs, or None."""
    a, b = recorded(out, digested), rec[f"{group}/{name}"]
    if a.tobytes() == b.tobytes():
        return None
    n = int(b[:4].view(np.uint32)[0])
    if n != len(out):
        return f"{len(out)} outputs, {n} recorded"
    lens = b[4:4 + 4 * n].view(np.uint32)
    pos = 4 + 4 * n
    for k, ln in zip(sorted(out), lens):
        v = np.ascontiguousarray(out[k])
        if (digest(v) if digested(k, v) else v).tobytes() != b[pos:pos + int(ln)].tobytes():
            return k
        pos += int(ln)
    return "layout"


def record_lengths(b):
    """The byte lengths of the members of one recorded case, in the sorted order of their keys."""
    n = int(b[:4].view(np.uint32)[0])
    return [int(v) for v in b[4:4 + 4 * n].view(np.uint32)]


def record_parts(rec, group, name, keys):
    """The recorded bytes of one case per output key; `keys` are all the keys the case's outputs have."""
    b = rec[f"{group}/{name}"]
    n = int(b[:4].view(np.uint32)[0])
    assert n == len(keys), (name, n, keys)
    lens = b[4:4 + 4 * n].view(np.uint32)
    ends = 4 + 4 * n + np.cumsum(lens)
    return {k: b[int(e - ln):int(e)].tobytes() for k, e, ln in zip(sorted(keys), ends, lens)}


class OracleIcpBackend:
    """oracle_py in the reference's float32 arithmetic (accum64 = False), on its kd-tree or its brute-force search."""

    def __init__(self, O, use_kdtree):
        self.O, self.kd = O, use_kdtree
        for k in ("get_mean", "l2dist_clouds", "copy_points", "transform_points", "depth_to_3d", "nms"):
            setattr(self, k, getattr(O, k))

    def icp(self, ref, model, it, a, b):
        return self.O.icp(ref, model, it, a, b, accum64=False, use_kdtree=self.kd)

    def points_corresponding(self, ref, model, thr):
        return self.O.points_corresponding(ref, model, thr, use_kdtree=self.kd)

    def detection(self, model, scene, K, rm, rr, it, a, b, r_match, t_match):
        r = self.O.detection(model, scene, K, rm, rr, it, a, b, r_match, t_match, accum64=False, use_kdtree=self.kd)
        if r["rc"]:
            raise AssertionError("reference CV_Assert")
        return r


class ReferenceIcpBackend:
    """The compiled ICP sources of the reference (reference_py.RefIcp)."""

    def __init__(self, R):
        for k in ("icp", "get_mean", "l2dist_clouds", "copy_points", "transform_points", "points_corresponding", "depth_to_3d", "nms"):
            setattr(self, k, getattr(R, k))
        self.R = R

    def detection(self, *args):
        r = self.R.detection(*args)
        if r["rc"]:
            raise AssertionError("reference CV_Assert")
        return r


def icp_groups():
    """group -> (list of (name, case), compute): the case list of the ICP half, in one place."""
    return {
        "icp": ([(c[0], c) for c in icp_cases()], compute_icp),
        "helpers": ([(c[0], c) for c in helper_cases()], compute_helpers),
        "detection": ([(c[0], c) for c in detection_cases()], compute_detection),
        "depth3d": ([(c[0], c) for c in depth3d_cases()], compute_depth3d),
        "nms": ([(c[0], c) for c in nms_cases()], compute_nms),
    }


# ======================================================================================================================
# Template extraction: the sort and the scattered selection, the two extractTemplate methods, quantizedOrientations with
# its magnitude, Detector::addTemplate (tests/golden/reference_extract.npz; extract_groups)
# ======================================================================================================================
# The cases sit on the reference's decision edges and on the dispatch edges fl_extract.hip states (2048-key LDS sort blocks,
# 1024-thread selection, 64-wide tiles); check_extract_cases proves on the CPU, from tests/extract_model.py and the oracle's
# stage functions, that every case is on the edge it is named for.  Excluded by construction, and asserted there:
#   * selectScatteredFeatures with fewer candidates than features, or with num_features == 0, walks past its list: the
#     reference's callers guard it (linemod.cpp:498, :802) and the select entry of both back ends refuses first;
#   * a depth list with a pixel twice and a start distance of k + 0.5 never ends (0 >= 0.25 is false at 0.5 and at -0.5);
#   * a quantized byte that is not one-hot throws in getLabel; the NORMAL_LUT and convertTo conditions of the header hold for
#     every image a case quantizes (every level of an add_template case).
EXW, EXH = 128, 96
STRONG = 55.0


def feats3(f):
    """(n, 3) int32 of a feature array (FEATURE_DTYPE / FEAT_DTYPE records or (n, 3) ints) or of a list of them."""
    if isinstance(f, list):
        return np.concatenate([feats3(a) for a in f])
    f = np.asarray(f)
    if f.dtype.names:
        return np.stack([f["x"], f["y"], f["label"]], 1).astype(np.int32)
    return f.astype(np.int32).reshape(-1, 3)


def _taken_or_refused(f):
    return {"refused": np.ones(1, np.uint8)} if f is None else {"features": feats3(f)}


# ---- select: std::stable_sort + selectScatteredFeatures on a list ------------------------------------------------------
def _select_job(name, w, h, xy, score, nf, mode=0, area=0, seed=1):
    xy = np.asarray(xy, np.int64)
    return EM.make_job(name, w, h, xy[:, 1] * w + xy[:, 0], score, num_features=nf, depth_mode=mode, area=area, seed=seed)


def _block_job(name, bw, bh, n, nf, mode, area, seed, kind="depth"):
    """n candidates packed into a bw x bh block of a 40 x 30 image, in shuffled arrival order."""
    rng = np.random.default_rng(seed)
    r = rng.permutation(EM.block_rasters(40, bw, bh))[:n]
    lab = EM.label_image(40, 30, seed)
    s = EM.depth_scores(lab, r, 40, rng) if kind == "depth" else EM.scores(kind, n, rng)
    return EM.make_job(name, 40, 30, r, s, num_features=nf, depth_mode=mode, area=area, seed=seed)


@functools.lru_cache(maxsize=None)
def select_jobs():
    """The jobs of the select group, in the form fl_dev_extract_select takes them (tests/extract_model.make_job): the start
    distance is the job's own (EM.job_distance), the candidates reach the CPU back ends in raster order."""
    out = [j for nf in (63, 31, 15, 7) for j in EM.rule_jobs(nf)]                    # n = nf - 1 (refused), nf, nf + 1, 2 nf - 1, 2 nf
    out += [EM.sort_job(n, "three", "shuffled") for n in EM.SORT_COUNTS]               # every row of SORT_COUNTS, ties everywhere
    out += [EM.sort_job(2049, "equal", "reversed"), EM.sort_job(4097, "distinct", "raster")]
    out.append(EM.deep_jobs()[2])                                                      # n = nf = 63, colour: all taken
    out.append(_block_job("all-taken-from-5.5", 8, 8, 63, 63, 2, 1008, 21))            # n = nf after the wraps 5.5 .. 0.5, ends on -0.5
    out.append(_block_job("half-3.5-nf7", 4, 3, 12, 7, 2, 28, 22))                     # 3.5, 2.5, 1.5, 0.5
    out.append(_block_job("half-2.5-nf7-all-taken", 3, 3, 7, 7, 2, 7, 23))             # n = nf: the last wrap leaves -0.5
    out.append(_block_job("half-4.5-nf31", 7, 6, 40, 31, 2, 279, 24))
    out.append(_block_job("ten-wraps", 28, 27, 756, 63, 0, 0, 25, kind="five"))        # colour: 756 / 63 + 1 = 13 on a dense block
    out.append(_block_job("ten-wraps-equal", 28, 27, 756, 63, 0, 0, 26, kind="equal"))
    # 3-4-5: the two best candidates are (5, 5) and (8, 9), the start distance is 30 / 7 + 1 = 5: 25 >= 25 keeps the second
    rng = np.random.default_rng(27)
    rest = rng.permutation(EM.block_rasters(40, 30, 20, 6, 6))[:28]
    rest = rest[(rest != 5 * 40 + 5) & (rest != 9 * 40 + 8)]
    xy = [(5, 5), (8, 9)] + [(int(r % 40), int(r // 40)) for r in rest]
    s = np.concatenate([np.array([30000.0, 20000.0], np.float32), EM.scores("three", len(rest), rng)])
    out.append(_select_job("three-four-five", 40, 30, xy, s, 7, seed=27))
    return {j["name"]: j for j in out}


def select_lists(job):
    """(x, y, label, score) of a job in raster order: the order in which the reference meets its candidates."""
    x, y, label = EM.job_xyl(job)
    o = np.argsort(job["raster"], kind="stable")
    return x[o], y[o], label[o], job["score"][o]


def select_record(job, f):
    x, y, label, score = select_lists(job)
    par = np.array([job["w"], job["h"], job["num_features"], job["depth_mode"], job["area"]], np.int32)
    return _with_inputs(_taken_or_refused(f), x, y, label, score, par, np.array([EM.job_distance(job)], np.float32))


def compute_select(B, job):
    return select_record(job, B.select_scattered_list(*select_lists(job), job["num_features"], EM.job_distance(job)))


def check_select_jobs():
    jobs = select_jobs()
    ns = {len(j["raster"]) for j in jobs.values()}
    assert set(EM.SORT_COUNTS) <= ns
    for nf in (63, 31, 15, 7):
        assert {nf - 1, nf} <= {len(j["raster"]) for j in jobs.values() if j["num_features"] == nf}
    stats = {}
    for name, j in jobs.items():
        n, nf = len(j["raster"]), j["num_features"]
        assert 1 <= nf <= 63 and (j["score"] != 0).all() and (j["raster"] >= 0).all() and (j["raster"] < j["w"] * j["h"]).all(), name
        if j["depth_mode"]:
            assert len(np.unique(j["raster"])) == n, name                      # a repeated pixel never ends from k + 0.5
        if n >= nf:
            fn = EM.select_model if n <= 800 else EM.select_walk
            stats[name] = fn(*select_lists(j), nf, EM.job_distance(j))[1]
    start = {k: float(EM.job_distance(jobs[k])) for k in jobs}
    assert start["all-taken-from-5.5"] == 5.5 and start["half-3.5-nf7"] == 3.5 and start["half-2.5-nf7-all-taken"] == 2.5 and start["half-4.5-nf31"] == 4.5
    assert start["all-taken-from-5.5"] - stats["all-taken-from-5.5"]["relaxations"] == -0.5 and stats["all-taken-from-5.5"]["wraps_after_take"] >= 1
    assert start["half-2.5-nf7-all-taken"] - stats["half-2.5-nf7-all-taken"]["relaxations"] == -0.5
    assert start["half-3.5-nf7"] - stats["half-3.5-nf7"]["relaxations"] == 0.5          # the pass at 0.5 fills the list
    assert start["half-4.5-nf31"] - stats["half-4.5-nf31"]["relaxations"] == 0.5
    assert stats["deep-all-taken"]["wraps_after_take"] >= 1
    assert stats["ten-wraps"]["relaxations"] >= 10 and stats["ten-wraps-equal"]["relaxations"] >= 10
    assert start["three-four-five"] == 5.0 and stats["three-four-five"]["kept_at_equal"] >= 1
    # equal scores: the best score is shared, and the arrival order is not the raster order that must decide
    for k in ("sort-2049-equal-reversed", "ten-wraps-equal", "sort-2049-three-shuffled"):
        s = jobs[k]["score"]
        assert (s == s.max()).sum() >= 2 and not np.array_equal(jobs[k]["raster"], np.sort(jobs[k]["raster"])), k


# ---- extract_color: ColorGradientPyramid::extractTemplate on given images ----------------------------------------------
def extract_mask(kind, w=EXW, h=EXH):
    if kind == "none":
        return None
    m = np.zeros((h, w), np.uint8)
    if kind == "rect":
        m[20:70, 30:100] = 255
    elif kind == "centre":                                  # mirror-symmetric about the middle column
        m[20:76, 24:104] = 255
    elif kind == "values":                                  # three non-zero values side by side: borders INSIDE the mask
        m[20:70, 30:64], m[20:70, 64:100], m[40:50, 50:80] = 128, 7, 1
    elif kind == "border":                                  # flush with the image's top-left and bottom-right corners
        m[0:50, 0:60], m[60:h, 100:w] = 255, 255
    elif kind == "hole":
        m[20:70, 30:100] = 255
        m[35:55, 50:80] = 0
    elif kind == "line":                                    # one pixel wide: all of it is border, none survives a 5x5 erosion
        m[48, 10:118], m[10:90, 64] = 255, 255
    else:
        raise ValueError(kind)
    return m


def extract_color_cases():
    """(name, seed, mask kind, magnitude kind, num_features, exact candidate count or None)."""
    out = [("color_edge_nomask", 30, "none", "edge", 63, None), ("color_edge_rect", 31, "rect", "edge", 63, None),
           ("color_q0_rect_nf31", 32, "rect", "q0", 31, None), ("color_mask_values", 33, "values", "edge", 63, None),
           ("color_mask_at_border_nf31", 34, "border", "edge", 31, None), ("color_mask_hole_nf15", 35, "hole", "edge", 15, None),
           ("color_mask_line_nf31", 36, "line", "edge", 31, None), ("color_mask_line_nf7", 37, "line", "q0", 7, None)]
    for nf in (63, 31):
        out += [(f"color_exactly_{nf}_of_{nf}", 40 + nf, "none", "exact", nf, nf), (f"color_refused_{nf - 1}_of_{nf}", 41 + nf, "none", "exact", nf, nf - 1)]
    out += [("color_exactly_63_in_rect", 38, "rect", "exact", 63, 63), ("color_refused_62_in_rect", 39, "rect", "exact", 63, 62)]
    return out


def extract_color_input(case):
    """(quantized, magnitude, mask).  Magnitudes are what the reference's are: integers (sums of two squares) as floats."""
    name, seed, mk, kind, nf, exact = case
    rng = np.random.default_rng(seed)
    q = (1 << rng.integers(0, 8, (EXH, EXW))).astype(np.uint8)
    q[rng.random((EXH, EXW)) < 0.3] = 0
    mask = extract_mask(mk)
    if kind == "exact":                                     # 3025 = 55^2 everywhere (not a candidate), `exact` pixels above it
        mag = np.full((EXH, EXW), 3025.0, np.float32)
        ok = q > 0 if mask is None else (q > 0) & (mask > O.erode_rect(mask, 1))
        idx = rng.permutation(np.flatnonzero(ok))[:exact]
        mag.ravel()[idx] = rng.choice(np.array([3026.0, 4000.0, 9000.0], np.float32), exact)
        assert len(idx) == exact
    else:
        mag = rng.choice(np.array([0.0, 3000.0, 3025.0, 3026.0, 4000.0, 20000.0], np.float32), (EXH, EXW))
        if kind == "q0":
            mag[q == 0] = np.float32(1.0e6)
    return q, mag, mask


def compute_extract_color(B, case):
    q, mag, mask = extract_color_input(case)
    out = _taken_or_refused(B.extract_template_color(q, mag, mask, STRONG, case[4]))
    return _with_inputs(out, q, mag, np.zeros(0, np.uint8) if mask is None else mask, np.array([case[4]]))


def check_extract_color_case(case):
    name, seed, mk, kind, nf, exact = case
    q, mag, mask = extract_color_input(case)
    assert np.isin(q, [0, 1, 2, 4, 8, 16, 32, 64, 128]).all(), name
    local = None if mask is None else np.where(mask > O.erode_rect(mask, 1), mask - O.erode_rect(mask, 1), 0)
    inb = np.ones(q.shape, bool) if local is None else local > 0
    cand = EM.color_candidates(q, mag, mask)
    assert np.array_equal(cand, inb & (q > 0) & (mag > np.float32(3025.0))), name
    if kind == "exact":
        assert cand.sum() == exact and (inb & (q > 0) & (mag == 3025)).any(), name
    else:
        assert (inb & (q > 0) & (mag == 3025)).any() and (inb & (q > 0) & (mag == 3026)).any(), name     # either side of 55^2
        assert cand.sum() > nf, name
    if kind == "q0":
        assert (inb & (q == 0) & (mag > 3025)).any(), name
    if mk == "values":
        er = O.erode_rect(mask, 1)
        assert set(np.unique(mask)) - {0, 255} and ((local > 0) & (er > 0)).any(), name      # a border between two non-zero values
    if mk == "border":
        edge = np.zeros(q.shape, bool)
        edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
        assert (edge & (mask > 0) & (local == 0)).any(), name                 # the replicated border made it interior
    if mk == "hole":
        assert local[34, 60] > 0 and local[55, 60] > 0 and mask[45, 60] == 0, name
    if mk == "line":
        assert np.array_equal(local, mask) and (O.erode_rect(mask, 2) == 0).all(), name


# ---- extract_depth: DepthNormalPyramid::extractTemplate on given images ------------------------------------------------
def extract_depth_cases():
    """(name, seed, mask kind, extract_threshold, num_features, labels in use, layout)."""
    every = (0, 1, 2, 3, 4, 5, 6, 7)
    out = []
    for thr, nf in ((2, 63), (1, 31), (0, 15)):
        out.append((f"depth_thr{thr}_nomask_nf{nf}", 50 + thr, "none", thr, nf, every, "blocks"))
        out.append((f"depth_thr{thr}_rect_nf{nf}", 53 + thr, "rect", thr, nf, every, "blocks"))
    out.append(("depth_label_absent", 56, "hole", 2, 63, (0, 1, 2, 4, 5, 7), "blocks"))
    out.append(("depth_equal_scores_across_labels", 57, "none", 2, 63, (2, 5), "halves"))
    out.append(("depth_equal_scores_masked_nf7", 58, "centre", 1, 7, (1, 6), "halves"))
    out.append(("depth_mask_values", 59, "values", 2, 31, every, "blocks"))
    out.append(("depth_mask_at_border", 60, "border", 2, 63, every, "blocks"))
    out.append(("depth_refused_mask_erodes_to_nothing", 61, "line", 0, 7, every, "blocks"))
    out.append(("depth_refused_too_few_nomask", 62, "none", 2, 63, every, "speckle"))
    return out


def extract_depth_input(case):
    name, seed, mk, thr, nf, labels, layout = case
    rng = np.random.default_rng(seed)
    if layout == "halves":                                  # two labels on mirror-image halves: equal counts, equal distances
        n = np.full((EXH, EXW), 1 << labels[0], np.uint8)
        n[:, EXW // 2:] = 1 << labels[1]
    elif layout == "speckle":                               # no pixel two steps inside its label, bar one 5 x 5 block
        n = (1 << rng.integers(0, 8, (EXH, EXW))).astype(np.uint8)
        n[10:15, 10:15] = 4
    else:
        idx = rng.choice(np.array(labels), (EXH // 12 + 1, EXW // 16 + 1)).repeat(12, 0).repeat(16, 1)[:EXH, :EXW]
        n = (1 << idx).astype(np.uint8)
        n[:, 45:48], n[40:43, :] = 0, 255                   # background and shadow, also inside every mask
    return n, extract_mask(mk)


def compute_extract_depth(B, case):
    n, mask = extract_depth_input(case)
    out = _taken_or_refused(B.extract_template_depth(n, mask, case[3], case[4]))
    return _with_inputs(out, n, np.zeros(0, np.uint8) if mask is None else mask, np.array([case[3], case[4]]))


def check_extract_depth_case(case):
    name, seed, mk, thr, nf, labels, layout = case
    n, mask = extract_depth_input(case)
    assert np.isin(n, [0, 1, 2, 4, 8, 16, 32, 64, 128, 255]).all(), name
    cand, dist, area = EM.depth_candidates(n, mask, thr)
    inside = np.ones(n.shape, bool) if mask is None else O.erode_rect(mask, 2) != 0
    assert area == (n.size if mask is None else int(inside.sum())), name
    if "refused" in name:
        assert cand.sum() < nf, name
        assert (area == 0) == (mk == "line") and (mk != "none" or cand.sum() > 0), name
        return
    assert cand.sum() >= nf, name
    if layout == "blocks":
        assert (inside & (n == 0)).any() and (inside & (n == 255)).any(), name            # labels 0 and 255 are there to be left out
    lab = np.log2(np.where(cand, n, 1).astype(np.float64)).astype(np.int64)
    if thr > 0:
        assert (cand & (dist == thr)).any() and (inside & ~cand & (n != 0) & (n != 255) & (dist == thr - 1)).any() == (thr > 1), name
    else:
        assert dist[cand].min() >= 1, name                  # a labelled pixel is never at distance 0: no score can EQUAL threshold 0
    counts = np.bincount(lab[cand], minlength=8)
    if name == "depth_label_absent":
        assert (counts == 0).sum() >= 2, name
    if layout == "halves":
        score = dist[cand] / counts[lab[cand]].astype(np.float32)
        a, b = (score[lab[cand] == l] for l in labels)
        assert counts[labels[0]] == counts[labels[1]] and a.max() == b.max() and len(np.intersect1d(a, b)) >= 2, name
    if mk == "values":
        assert set(np.unique(mask[inside])) - {0, 255}, name


# ---- orientations: quantizedOrientations, quantized image and magnitude ------------------------------------------------
def orientation_cases():
    """(name, kind, w, h, seed)."""
    return [("orient_ties_128x96", "ties", 128, 96, 70), ("orient_ties_97x61", "ties", 97, 61, 71), ("orient_weak_edge_128x96", "weak", 128, 96, 72),
            ("orient_flat_64x48", "flat", 64, 48, 73), ("orient_noise_33x18", "noise", 33, 18, 74), ("orient_noise_97x61", "noise", 97, 61, 75),
            ("orient_blocks_128x96", "blocks", 128, 96, 76)]


def orientation_input(case):
    name, kind, w, h, seed = case
    rng = np.random.default_rng(seed)
    if kind == "flat":
        return np.full((h, w, 3), 93, np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "blocks":
        return EM.block_noise_bgr(seed, w, h)
    # low contrast: small integer gradients, so that different (dx, dy) of two channels often have one squared magnitude
    # (5^2 + 0^2 = 3^2 + 4^2), and a quarter of the frame in grey, where all three channels tie
    amp = 60 if kind == "ties" else 24
    b = rng.integers(0, amp, ((h + 2) // 3, (w + 2) // 3, 3)).repeat(3, 0).repeat(3, 1)[:h, :w].astype(np.uint8) + 90
    b[: h // 2, : w // 2] = b[: h // 2, : w // 2, :1]
    return np.ascontiguousarray(b)


def orientation_channels(bgr):
    """Per channel the Sobel pair and the squared magnitude, as quantizedOrientations forms them (linemod.cpp:247-273)."""
    sm = O.gaussian7_bgr(bgr)
    dx, dy = O.sobel3_bgr(sm, False).astype(np.int32), O.sobel3_bgr(sm, True).astype(np.int32)
    return dx, dy, dx * dx + dy * dy


def fast_angles(dy, dx):
    """cv::phase in degrees per element, through the oracle's orc_fast_atan2 on the distinct pairs."""
    pairs, inv = np.unique(np.stack([dy.ravel(), dx.ravel()], 1), axis=0, return_inverse=True)
    a = np.array([O.lib().orc_fast_atan2(float(p[0]), float(p[1])) for p in pairs], np.float32)
    return a[inv.ravel()].reshape(dy.shape)


def orientation_tie_counts(bgr, weak=10.0):
    """Strong interior pixels per kind of tie among the channel magnitudes, and how many of them would get another angle bin
    from the other tied channel: {(first, other): (pixels, pixels where the choice shows)}; (0, 1, 2) is the three-way tie."""
    dx, dy, mag = orientation_channels(bgr)
    m0, m1, m2 = mag[..., 0], mag[..., 1], mag[..., 2]
    inner = np.zeros(m0.shape, bool)
    inner[1:-1, 1:-1] = True
    ang = fast_angles(dy, dx)
    bins = np.rint(ang.astype(np.float64) * (16.0 / 360.0)).astype(np.int64) & 7
    sel = {(0, 1): (m0 == m1) & (m0 > m2), (0, 2): (m0 == m2) & (m0 > m1), (1, 2): (m1 == m2) & (m1 > m0), (0, 1, 2): (m0 == m1) & (m1 == m2)}
    out = {}
    for k, s in sel.items():
        s = s & inner & (mag[..., k[0]] > weak * weak)
        shows = s & np.any([bins[..., k[0]] != bins[..., o] for o in k[1:]], axis=0)
        out[k] = (int(s.sum()), int(shows.sum()))
    return out


def compute_orientations(B, case):
    bgr = orientation_input(case)
    q, mag = B.quantized_orientations_mag(bgr, 10.0)
    return _with_inputs({"img_q": q, "img_mag": fbits(mag)}, bgr)


def orientations_defined(bgr):
    """No angle of the image is one of the two floats on which a float and a double product round apart (the header)."""
    dx, dy, mag = orientation_channels(bgr)
    return angles_unambiguous(fast_angles(dy, dx))


def check_orientation_case(case):
    name, kind, w, h, seed = case
    bgr = orientation_input(case)
    assert bgr.shape == (h, w, 3) and orientations_defined(bgr), name
    dx, dy, mag = orientation_channels(bgr)
    best = mag.max(2)
    if kind == "flat":
        assert best.max() == 0, name
    if kind == "ties":
        t = orientation_tie_counts(bgr)
        assert all(t[k][0] >= 1 for k in t), (name, t)                          # every pairwise tie and the three-way tie, above weak^2
        assert all(t[k][1] >= 1 for k in ((0, 1), (0, 2), (1, 2))), (name, t)   # and each pairwise one where the chain's choice shows
    if kind == "weak":
        # a pixel at exactly weak^2 = 100 that `>=` would let through: the vote passes there once the threshold is lowered
        ang = fast_angles(np.take_along_axis(dy, mag.argmax(2)[..., None], 2)[..., 0], np.take_along_axis(dx, mag.argmax(2)[..., None], 2)[..., 0])
        lo, at = O.hysteresis_gradient(best.astype(np.float32), ang, 99.5), O.hysteresis_gradient(best.astype(np.float32), ang, 100.0)
        assert ((best == 100) & (lo != 0) & (at == 0)).any(), name


# ---- add_template: Detector::addTemplate with the two default modalities -----------------------------------------------
def _safe_depth(d):
    d = d.copy()
    for _ in range(64):
        bad = normals_unsafe(d, 2000, 50)
        if not bad.any():
            return d
        d[bad] = 65535
    raise AssertionError("depth")


@functools.lru_cache(maxsize=None)
def add_template_cases():
    """name -> dict(bgr, depth, mask, levels, expect): expect is None (a template), or the job l * 2 + m that fails first in
    the reference's order (all colour levels, then all depth levels)."""
    out = {}

    def add(name, seed, w, h, levels, mask, expect=None):
        out[name] = dict(bgr=EM.block_noise_bgr(seed, w, h), depth=_safe_depth(EM.tilted_patch_depth(seed, w, h)), mask=mask, levels=levels, expect=expect)

    for levels, (w, h) in ((1, (EXW, EXH)), (2, (EXW, EXH)), (3, (160, 120))):
        add(f"add_L{levels}_nomask", 100 + levels, w, h, levels, None)
        add(f"add_L{levels}_mask_odd", 103 + levels, w, h, levels, EM.rect_mask(w, h, 9, 7, w - 30, h - 24))
        add(f"add_L{levels}_mask_even", 106 + levels, w, h, levels, EM.rect_mask(w, h, 12, 10, w - 30, h - 24))
    # masks of the extract_color / extract_depth groups on whole views (the kernels take no quantized images from a caller)
    for seed, mk in ((93, "values"), (90, "border"), (95, "hole")):
        add(f"add_L2_mask_{mk}", seed, EXW, EXH, 2, extract_mask(mk))
    add("add_L2_refused_depth_mask_line", 93, EXW, EXH, 2, extract_mask("line"), expect=1)       # colour passes on both levels, depth has no area
    # a job at exactly its rule, one below (refused) and one above, every other job with candidates to spare (96 x 80, two levels)
    for job, target in EM.THRESHOLD_CASES:
        c = EM.threshold_case(job, target)
        assert c is not None, (job, target)
        nf = 63 >> (job // 2)
        out[f"add_job{job}_{'colour' if job % 2 == 0 else 'depth'}_L{job // 2}_{target}_of_{nf}"] = dict(
            bgr=c["bgr"], depth=c["depth"], mask=c["mask"], levels=2, expect=job if target < nf else None, counts=tuple(c["counts"]))
    return out


def add_template_record(case, r):
    if r is None:
        out = {"refused": np.ones(1, np.uint8)}
    else:
        t, feats, bb = r
        out = {"templates": np.stack([np.asarray(t[k], np.int32) for k in ("width", "height", "offset_x", "offset_y", "pyramid_level", "feat_count")], 1),
               "features": feats3(list(feats)), "bb": np.array(bb, np.int32)}
    mask = np.zeros(0, np.uint8) if case["mask"] is None else case["mask"]
    return _with_inputs(out, case["bgr"], case["depth"], mask, np.array([case["levels"]]))


def compute_add_template(B, case):
    return add_template_record(case, B.add_template(case["bgr"], case["depth"], case["mask"], case["levels"]))


def check_add_template_cases():
    cases = add_template_cases()
    parity = set()
    for name, c in cases.items():
        h, w = c["depth"].shape
        assert c["bgr"].shape == (h, w, 3) and 1 <= c["levels"] <= 3, name
        assert not normals_unsafe(c["depth"], 2000, 50).any(), name
        src = c["bgr"]
        for l in range(c["levels"]):
            src = src if l == 0 else O.pyrdown_bgr(src)
            assert orientations_defined(src), (name, l)
        counts = EM.candidate_counts(c["bgr"], c["depth"], c["mask"], c["levels"])
        th = EM.thresholds(c["levels"])
        failing = [k for k in list(range(0, 2 * c["levels"], 2)) + list(range(1, 2 * c["levels"], 2)) if counts[k] < th[k]]
        assert (failing[0] if failing else None) == c["expect"], (name, counts, c["expect"])
        if "counts" in c:
            assert tuple(counts) == c["counts"], name
        r = O.add_template(c["bgr"], c["depth"], c["mask"], c["levels"])
        if r is not None:
            t, feats, bb = r
            raw_x = min(int((f["x"] + t[k]["offset_x"]).min()) << int(t[k]["pyramid_level"]) for k, f in enumerate(feats))
            raw_y = min(int((f["y"] + t[k]["offset_y"]).min()) << int(t[k]["pyramid_level"]) for k, f in enumerate(feats))
            assert bb[0] == raw_x - raw_x % 2 and bb[1] == raw_y - raw_y % 2, name
            parity |= {("x", raw_x % 2), ("y", raw_y % 2)}
    assert parity == {("x", 0), ("x", 1), ("y", 0), ("y", 1)}                   # min_x % 2 == 1 decides both ways, and min_y
    expects = {c["expect"] for c in cases.values()}
    assert {None, 0, 1, 2, 3} <= expects                                          # colour level 0, depth level 0, level 1 only (colour, depth)
    assert {(c["levels"], c["mask"] is None) for c in cases.values() if c["expect"] is None} >= {(l, m) for l in (1, 2, 3) for m in (True, False)}


def check_extract_cases():
    check_select_jobs()
    for c in extract_color_cases():
        check_extract_color_case(c)
    for c in extract_depth_cases():
        check_extract_depth_case(c)
    for c in orientation_cases():
        check_orientation_case(c)
    check_add_template_cases()


class OracleExtractBackend:
    """oracle_py under the method names of reference_py.Ref."""

    def __init__(self, O_):
        for k in ("select_scattered_list", "extract_template_color", "extract_template_depth", "quantized_orientations_mag", "add_template"):
            setattr(self, k, getattr(O_, k))


def extract_groups():
    """group -> (list of (name, case), compute): the case list of template extraction, in one place."""
    return {
        "select": (list(select_jobs().items()), compute_select),
        "extract_color": ([(c[0], c) for c in extract_color_cases()], compute_extract_color),
        "extract_depth": ([(c[0], c) for c in extract_depth_cases()], compute_extract_depth),
        "orientations": ([(c[0], c) for c in orientation_cases()], compute_orientations),
        "add_template": (list(add_template_cases().items()), compute_add_template),
    }


def is_image(key, value):
    """What tests/golden/reference_extract.npz keeps as a digest: the images (keys img_*); everything else in full."""
    return key.startswith("img_")
