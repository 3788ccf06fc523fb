"""GPU parity of k_scan's run loop: a wave walks `scan_run` work items (pyramid, 1024-position chunk) of a frame, with the next
item's record and the next group's offsets requested ahead.  Whatever the run length, the pruning switches and the class filter,
the match list and the raw maps are the oracle's.  Small shapes: 320x240 at T = 8 has 1200 positions, i.e. two chunks, the
second with 176 positions; 64x48 has 48 positions, i.e. four lanes of one chunk."""
import numpy as np
import pytest

from fealess_amd import api, synth
from fealess_amd.bank import TemplateBank
from util import options

pytestmark = pytest.mark.gpu

RUNS = (1, 2, 3, 8, 64)
PRUNE = (0, 1)
MID = (0, 0x7F, 0xFF)
W0, H0, T = 320, 240, [8]
THR = 70.0


def _assert_matches_equal(got, exp):
    assert len(got) == len(exp), (len(got), len(exp))
    for k in ("x", "y", "class_idx", "template_id"):
        assert np.array_equal(got[k], exp[k]), k
    assert np.array_equal(got["similarity"].view(np.uint32), exp["similarity"].view(np.uint32))


def _quantized(seed, w, h, density):
    rng = np.random.default_rng(seed)
    return [synth.random_quantized(rng, w, h, density) for _ in range(2)]


def _raw_threshold(nf, thr):
    return int(np.float32(2 * nf) + np.float32(thr) / np.float32(100.0) * np.float32(2 * nf) + np.float32(0.5))


def _check_matrix(ctx, oracle, qs, w, h, bank, thr):
    """Every run length x pruning switch: the list and every pyramid's raw map against the oracle (computed once)."""
    n = bank.n_pyramids
    exp, n_exp = oracle.match_quantized(qs, w, h, T, [bank], thr)
    assert n_exp > 0, "test is vacuous: no matches"
    lms = [oracle.build_linear_memories(qs[m], T[0]) for m in range(2)]
    exp_maps = np.stack([oracle.total_similarity(lms, bank, g, w, h, T[0]) for g in range(n)])
    det = api.Detector(ctx, 2, T)
    det.add_class(bank)
    det.finalize(w, h)
    try:
        for run in RUNS:
            for prune in PRUNE:
                for mid in MID:
                    with options(ctx, {"scan_run": run, "scan_prune": prune, "scan_prune_mid": mid}):
                        got, n_got = det.match_quantized(qs, thr)
                        maps = det.similarity_maps(0, n)
                    assert n_got == n_exp, (run, prune, mid)
                    _assert_matches_equal(got, exp)
                    assert np.array_equal(maps, exp_maps), (run, prune, mid)
    finally:
        det.close()


@pytest.mark.parametrize("n", [1, 3, 37])
def test_run_lengths_two_chunks(ctx, oracle, n):
    """Shape A.  Run lengths that do not divide the item count, a run longer than the list, a last block with idle waves."""
    qs = _quantized(100 + n, W0, H0, 0.06)
    bank = synth.make_bank("obj", n, 1, 2, W0, H0, seed=n, qs=qs, planted_frac=1.0 if n == 1 else 0.3, bbox=96)
    _check_matrix(ctx, oracle, qs, W0, H0, bank, THR)


def test_run_lengths_four_lanes(ctx, oracle):
    """Shape B: 48 positions, lanes_on = 4."""
    qs = _quantized(7, 64, 48, 0.5)
    bank = synth.make_bank("obj", 5, 1, 2, 64, 48, seed=5, qs=qs, planted_frac=0.4, bbox=24)
    _check_matrix(ctx, oracle, qs, 64, 48, bank, 60.0)


def _rand_feats(rng, n, s, labels=(0, 8)):
    return np.stack([rng.integers(0, s + 1, n), rng.integers(0, s + 1, n), rng.integers(*labels, n)], 1).astype(np.int32)


def _positions(width, height):
    W, H = W0 // T[0], H0 // T[0]
    return (H - ((height - 1) // T[0] + 1)) * W + (W - ((width - 1) // T[0] + 1)) + 1


def _stale_state_bank(qs):
    """Five kinds of pyramid, eight rounds in rotated orders, so that whatever way the items are dealt a wave meets them after
    one another.  The colour image holds labels 0 and 1 only: colour features of label 4 or 5 respond nowhere (kinds A, B).
    Returns (bank, kinds): kinds[g] in "ABCDE"."""
    rng = np.random.default_rng(31)
    def tpl(width, height, f):
        return dict(width=width, height=height, offset_x=0, offset_y=0, pyramid_level=0, features=f)
    bank, kinds = TemplateBank("obj", 1, 2), []
    orders = ["ABCDE", "BDAEC", "CEBAD", "DACBE", "EBDCA", "ACEBD", "BEADC", "DCBAE"]
    for order in orders:
        for kind in order:
            if kind == "A":      # two colour groups: the bound is missed after the first
                tl = [tpl(40, 40, _rand_feats(rng, 16, 40, (4, 6))), tpl(40, 40, _rand_feats(rng, 8, 40))]
            elif kind == "B":    # one colour group, then the depth modality is never read
                tl = [tpl(40, 40, _rand_feats(rng, 8, 40, (4, 6))), tpl(40, 40, _rand_feats(rng, 8, 40))]
            elif kind == "C":    # the colour template's positions end in chunk 0, the depth template's reach chunk 1
                tl = [tpl(200, 100, _rand_feats(rng, 4, 100)), tpl(40, 40, _rand_feats(rng, 12, 40))]
            elif kind == "D":    # a single 8-offset group per modality
                tl = [tpl(40, 40, _rand_feats(rng, 5, 40)), tpl(40, 40, _rand_feats(rng, 3, 40))]
            else:                # planted: yields candidates
                tl = synth.planted_pyramid(rng, qs, 1, 2, W0, H0, 40, nf0=30)
                assert tl is not None
            bank.add_pyramid(tl)
            kinds.append(kind)
    return bank, kinds


def _sub_map(oracle, lms, tl, keep0, keep1):
    """Raw map of a pyramid cut down to its first keep0 colour and keep1 depth features."""
    b = TemplateBank("obj", 1, 2)
    cut = [dict(tl[0], features=tl[0]["features"][:keep0]), dict(tl[1], features=tl[1]["features"][:keep1])]
    b.add_pyramid(cut)
    return oracle.total_similarity(lms, b, 0, W0, H0, T[0])


def test_no_state_survives_from_one_item_to_the_next(ctx, oracle):
    qs = _quantized(55, W0, H0, 0.12)
    qs[0] = np.where(qs[0] > 0, 1 + (qs[0] > 8), 0).astype(np.uint8)  # colour labels 0 and 1 only (kinds A and B)
    qs[1][:184] = 0                                                   # depth labels in the lowest rows only (kind C)
    bank, kinds = _stale_state_bank(qs)
    n = bank.n_pyramids
    lms = [oracle.build_linear_memories(qs[m], T[0]) for m in range(2)]
    exp, n_exp = oracle.match_quantized(qs, W0, H0, T, [bank], THR)
    exp_maps = np.stack([oracle.total_similarity(lms, bank, g, W0, H0, T[0]) for g in range(n)])
    # each kind is what it is meant to be, from the oracle's maps
    tarr, farr, _ = bank.arrays()
    seen = dict.fromkeys("ABCDE", 0)
    for g, kind in enumerate(kinds):
        t0, t1 = tarr[2 * g], tarr[2 * g + 1]
        tl = [dict(width=int(t["width"]), height=int(t["height"]), offset_x=0, offset_y=0, pyramid_level=0,
                   features=np.stack([farr["x"], farr["y"], farr["label"]], 1)[int(t["feat_begin"]):int(t["feat_begin"]) + int(t["feat_count"])])
              for t in (t0, t1)]
        nf0, nf1 = int(t0["feat_count"]), int(t1["feat_count"])
        raw_thr = _raw_threshold(nf0 + nf1, THR)
        if kind == "A":
            first = _sub_map(oracle, lms, tl, 8, 0)
            seen["A"] += int(first.max()) + 4 * (nf0 + nf1 - 8) <= raw_thr
        elif kind == "B":
            colour = _sub_map(oracle, lms, tl, nf0, 0)
            seen["B"] += nf0 == 8 and int(colour.max()) + 4 * nf1 <= raw_thr
        elif kind == "C":
            assert _positions(200, 100) <= 1024 < _positions(40, 40)
            seen["C"] += bool(exp_maps[g].reshape(-1)[1024:].any())
        elif kind == "D":
            seen["D"] += nf0 <= 8 and nf1 <= 8
        else:
            seen["E"] += bool((exp["template_id"] == g).any())
    assert all(v > 0 for v in seen.values()), seen
    assert seen["A"] >= 4 and seen["B"] >= 4 and seen["E"] >= 4, seen
    det = api.Detector(ctx, 2, T)
    det.add_class(bank)
    det.finalize(W0, H0)
    try:
        for run in (2, 3, 5, 8, 64):
            for mid in MID:
                with options(ctx, {"scan_run": run, "scan_prune_mid": mid}):
                    got, n_got = det.match_quantized(qs, THR)
                    maps = det.similarity_maps(0, n)
                assert n_got == n_exp, (run, mid)
                _assert_matches_equal(got, exp)
                assert np.array_equal(maps, exp_maps), (run, mid)
    finally:
        det.close()


def test_class_filter_inside_a_run(ctx, oracle):
    qs = _quantized(9, W0, H0, 0.06)
    banks = [synth.make_bank(name, 7, 1, 2, W0, H0, seed=i + 20, qs=qs, planted_frac=0.5, bbox=96) for i, name in enumerate("ab")]
    exp, n_exp = oracle.match_quantized(qs, W0, H0, T, banks, THR)
    assert all((exp["class_idx"] == c).any() for c in (0, 1))
    det = api.Detector(ctx, 2, T)
    for b in banks:
        det.add_class(b)
    det.finalize(W0, H0)
    try:
        for run in (3, 8, 64):                                        # 14 pyramids, 28 items: runs hold items of both classes
            with options(ctx, {"scan_run": run}):
                for c, name in enumerate("ab"):
                    det.set_class_filter([name])
                    got, n_got = det.match_quantized(qs, THR)
                    keep = exp[exp["class_idx"] == c]
                    assert n_got == len(keep) > 0, (run, name)
                    _assert_matches_equal(got, keep)
                det.set_class_filter([])
                got, n_got = det.match_quantized(qs, THR)
                assert n_got == n_exp
                _assert_matches_equal(got, exp)
    finally:
        det.close()


def test_debug_tap_in_the_middle_of_a_run(ctx, oracle):
    """fl_similarity_maps scans at 200 %: every neighbour of the tapped pyramid prunes, its own map is complete."""
    qs = _quantized(137, W0, H0, 0.06)
    bank = synth.make_bank("obj", 37, 1, 2, W0, H0, seed=37, qs=qs, planted_frac=0.3, bbox=96)
    lms = [oracle.build_linear_memories(qs[m], T[0]) for m in range(2)]
    det = api.Detector(ctx, 2, T)
    det.add_class(bank)
    det.finalize(W0, H0)
    try:
        det.match_quantized(qs, THR)
        for run in (3, 8, 64):
            with options(ctx, {"scan_run": run}):
                for first, count in ((17, 1), (16, 3), (36, 1)):
                    maps = det.similarity_maps(first, count)
                    for k in range(count):
                        e = oracle.total_similarity(lms, bank, first + k, W0, H0, T[0])
                        assert e.any() and np.array_equal(maps[k], e), (run, first, k)
    finally:
        det.close()


def test_batch_of_nine_frames(ctx, oracle):
    """Nine frames are no multiple of the eight XCD residues the blocks of a frame are dealt by."""
    rng = np.random.default_rng(90)
    frames = []
    for i in range(9):
        bgr = (rng.integers(0, 256, (H0 // 8, W0 // 8, 3)) // 32 * 32).astype(np.uint8).repeat(8, 0).repeat(8, 1)
        bgr = np.roll(bgr, 3 * i, axis=1)
        depth = (600 + 40 * rng.integers(0, 4, (H0 // 16, W0 // 16))).astype(np.uint16).repeat(16, 0).repeat(16, 1)
        frames.append((np.ascontiguousarray(bgr), np.ascontiguousarray(np.roll(depth, 5 * i, axis=0))))
    qs0 = oracle.quantize_pyramid(frames[0][0], frames[0][1], 1)
    bank = synth.make_bank("obj", 21, 1, 2, W0, H0, seed=3, qs=qs0, planted_frac=0.4, bbox=96)
    thr = 60.0
    exp0, n0 = oracle.match_images(frames[0][0], frames[0][1], T, [bank], thr)
    assert n0 > 0
    det = api.Detector(ctx, 2, T)
    det.add_class(bank)
    det.finalize(W0, H0, max_batch=9)
    try:
        single = [det.match(b, d, thr) for b, d in frames]
        assert single[0][1] == n0
        _assert_matches_equal(single[0][0], exp0)
        assert len({s[0].tobytes() for s in single}) > 1
        for run in (3, 0):
            with options(ctx, {"scan_run": run}):
                both = det.match_batch([f[0] for f in frames], [f[1] for f in frames], thr)
            for (got, n_got), (exp, n_exp) in zip(both, single):
                assert n_got == n_exp, run
                _assert_matches_equal(got, exp)
    finally:
        det.close()


def test_candidate_buffers_grow_under_a_run(ctx, oracle):
    rng = np.random.default_rng(4)
    qs = [synth.random_quantized(rng, W0, H0, 0.9)]
    bank = synth.make_bank("obj", 40, 1, 1, W0, H0, seed=9, bbox=64)
    det = api.Detector(ctx, 1, T)
    det.add_class(bank)
    det.finalize(W0, H0, max_batch=1, max_candidates=64)
    try:
        with options(ctx, {"scan_run": 8}):
            got, n = det.match_quantized(qs, -100.0, cap=1 << 17)   # raw_threshold 0: every non-zero cell is a candidate
        exp, n_exp = oracle.match_quantized(qs, W0, H0, T, det.banks, -100.0)
        assert n == n_exp > 20000
        _assert_matches_equal(got, exp)
    finally:
        det.close()


def test_scan_run_option_range(ctx):
    before = ctx.get_option("scan_run")
    for bad in (-1, 65, 1000):
        with pytest.raises(api.FealessError):
            ctx.set_option("scan_run", bad)
        assert ctx.get_option("scan_run") == before
    for good in (0, 1, 64):
        ctx.set_option("scan_run", good)
        assert ctx.get_option("scan_run") == good
    ctx.set_option("scan_run", before)
