"""k_scan's exact pruning restated in numpy (fl_scan.hip: scan_item), no GPU.

A work item is a (pyramid, 1024-position chunk) pair.  Lane i of the wave owns the chunk's positions 16 i .. 16 i + 15.  After the
first eight features of a modality, then every `step` features (inside the 8-feature groups whose bit is set in `mid`), and
between the modalities, a lane stays alive iff

    mx_tot + part + 4 * left > prune_threshold

for its own 16 positions: mx_tot its largest total of the modalities done, part its largest partial sum of the modality in
work, left the features still to come.  With `lanes` = 0 a check keeps every lane or none.  The loads of the groups that follow
run for the live lanes and their upper neighbours (a lane's bytes 16..19 are its upper neighbour's first dword), cut to the
lanes the modality has positions for, plus one.

From the oracle's linear memories and a bank, `scan(...)` gives per item the lanes alive after each check, the feature-load
instructions, the lane-loads, the distinct 64-byte lines and the candidates.  What the model leaves out: the bytes a loading lane
reads beyond `template_positions` and the tail dword of the last loading lane are taken from the oracle's arrays, zero-padded;
on the device other bytes of the workspace can follow there.  They only ever make a bound more generous, so they can keep a
lane without positions alive for a check longer than here, never change a candidate.

Run as a script, it prints the shares of items that continue after k features and the loads and lines per item under the
schedules that profiles/README.md compares, on bench-like and clutter-like scenes (CPU only, a few minutes).
"""
import numpy as np

FL_SCAN_PRUNE_MID = 0x7F


def raw_threshold(nf, threshold):
    """linemod.cpp:1487, in float as written."""
    thr100 = np.float32(threshold) / np.float32(100.0)
    return int(np.float32(2 * nf) + thr100 * np.float32(2 * nf) + np.float32(0.5))


def bank_tables(bank, w, h, T, stride):
    """Per pyramid, per modality at the coarsest level: (P, offsets padded to a multiple of 8 with None, nf), as
    fl_detector_finalize builds them.  w, h: the coarsest level's image size."""
    tarr, farr, _ = bank.arrays()
    L, M = bank.levels, bank.modalities
    W, H = w // T, h // T
    WH = W * H
    out = []
    for g in range(bank.n_pyramids):
        mods = []
        for m in range(M):
            t = tarr[(g * L + (L - 1)) * M + m]
            wf, hf = (int(t["width"]) - 1) // T + 1, (int(t["height"]) - 1) // T + 1
            P = min((H - hf) * W + (W - wf) + 1, WH)
            f = farr[int(t["feat_begin"]):int(t["feat_begin"]) + int(t["feat_count"])]
            offs = []
            for x, y, lab in zip(f["x"].tolist(), f["y"].tolist(), f["label"].tolist()):
                if x < 0 or x >= w or y < 0 or y >= h:
                    continue
                offs.append(lab * stride + ((y % T) * T + x % T) * WH + (y // T) * W + x // T)
            offs += [None] * (-len(offs) % 8)
            mods.append((P, offs, int(t["feat_count"])))
        out.append(mods)
    return out


def scan(lms, bank, w, h, T, threshold, mid=FL_SCAN_PRUNE_MID, lanes=1, step=4, prune=1):
    """lms: per modality the (8, stride) linear memories of the coarsest level (oracle.build_linear_memories).
    Returns a list of items: dict(g, chunk, checks=[(features done, alive mask as int)], ended (features done when a check
    ended the item, else None), loads, lane_loads, lines, candidates=[(x, y, raw, nf)])."""
    W, H = w // T, h // T
    WH = W * H
    stride = lms[0].shape[1]
    flat = [np.concatenate([np.ascontiguousarray(l).reshape(-1), np.zeros(2048, np.uint8)]) for l in lms]
    lane_of = np.arange(1024) // 16
    lane_ids = np.arange(64)
    items = []
    for g, mods in enumerate(bank_tables(bank, w, h, T, stride)):
        nf_all = sum(nf for _, _, nf in mods)
        pmax = max(P for P, _, _ in mods)
        thr = raw_threshold(nf_all, threshold)
        for chunk in range((WH + 1023) // 1024):
            if chunk > 0 and chunk * 1024 >= pmax:
                break
            it = dict(g=g, chunk=chunk, checks=[], ended=None, loads=0, lane_loads=0, lines=0, candidates=[])
            items.append(it)
            alive = np.ones(64, bool)
            tot = np.zeros(1024, np.int64)
            done = nf = 0
            pos = chunk * 1024 + np.arange(1024)

            def check(ok):
                nonlocal alive
                b = ok & alive
                alive = b if (lanes or not b.any()) else np.ones(64, bool)
                it["checks"].append((done, int(sum(1 << int(i) for i in np.nonzero(alive)[0]))))
                if not alive.any():
                    it["ended"] = done
                return bool(alive.any())

            over = False
            for m, (P, offs, h_nf) in enumerate(mods):
                mx_tot = np.zeros(64, np.int64)
                if prune and m > 0:
                    mx_tot = tot.reshape(64, 16).max(1)
                    if not check(mx_tot + 4 * (nf_all - nf) > thr):
                        over = True
                        break
                nf += h_nf
                if chunk * 1024 >= P:
                    continue
                lanes_on = min(64, ((P - chunk * 1024 + 15) >> 4) + 1)
                acc = np.zeros(1024, np.int64)
                for k in range(0, len(offs), 8):
                    parts = [(0, 8)] if step == 8 or k == 0 else [(s, step) for s in range(0, 8, step)]
                    for s0, n in parts:
                        need = (alive | np.concatenate([[False], alive[:-1]])) & (lane_ids < lanes_on)
                        sel = need[lane_of]
                        it["loads"] += n
                        it["lane_loads"] += n * int(need.sum())
                        for off in offs[k + s0:k + s0 + n]:
                            if off is None:                # the zero pad: one line whatever the lanes
                                it["lines"] += 1 if need.any() else 0
                                continue
                            a = off + chunk * 1024
                            a4 = a - (a & 3)               # the aligned 16 bytes a lane loads, relative to the label planes
                            first = (a4 + 16 * lane_ids[need]) // 64
                            last = (a4 + 16 * lane_ids[need] + 15) // 64
                            it["lines"] += len(np.union1d(first, last))
                            acc[sel] += flat[m][a:a + 1024][sel]
                        done += n
                        if prune and (mid >> (k >> 3)) & 1:
                            part = acc.reshape(64, 16).max(1)
                            left = nf_all - nf + max(0, h_nf - (k + s0 + n))
                            if not check(mx_tot + part + 4 * left > thr):
                                over = True
                                break
                    if over:
                        break
                if over:
                    break
                tot += np.where(pos < P, acc, 0)
            if over:
                continue
            thr_final = raw_threshold(nf, threshold)
            offset = T // 2 + (T % 2 - 1)
            for j in np.nonzero((tot > thr_final) & (pos < WH) & alive[lane_of])[0]:
                p = int(pos[j])
                it["candidates"].append(((p % W) * T + offset, (p // W) * T + offset, int(tot[j]), nf))
    return items


def matches(items):
    """The items' candidates as a one-level, one-class match() returns them (linemod.cpp:1502, then the oracle's sort and
    std::unique, which ignores the template): arrays x, y, similarity (float32), template_id."""
    out = []
    for it in items:
        for x, y, raw, nf in it["candidates"]:
            sim = np.float32(raw * np.float32(100.0)) / np.float32(4 * nf) + np.float32(0.5)
            out.append((-float(sim), it["g"], y, x))
    out.sort()
    keep = [m for i, m in enumerate(out) if i == 0 or (m[0], m[2], m[3]) != (out[i - 1][0], out[i - 1][2], out[i - 1][3])]
    return dict(x=np.array([m[3] for m in keep], np.int32), y=np.array([m[2] for m in keep], np.int32),
                similarity=np.array([-m[0] for m in keep], np.float32), template_id=np.array([m[1] for m in keep], np.int32))


def alive_after(it, done):
    """Lanes alive after the check at `done` features, as a list (None: no such check)."""
    for d, mask in it["checks"]:
        if d == done:
            return [i for i in range(64) if (mask >> i) & 1]
    return None


def _scenes():
    """Three bench-like scenes (bench.py:build_bank's poses and renders) and two clutter-like ones (build_clutter's), quantised by
    the oracle at pyramid level 1."""
    import oracle_py as O
    from fealess_amd import synth
    K = (608.0, 608.0, 320.0, 240.0)
    cam = dict(fx=K[0], fy=K[1], cx=K[2], cy=K[3])
    rng = np.random.default_rng(1234)
    out = []
    for s in range(3):
        R, t = synth.object_pose(tx=float(rng.uniform(-60, 60)), ty=float(rng.uniform(-40, 40)), tz=float(rng.uniform(620, 700)),
                                 yaw=float(rng.uniform(-0.4, 0.4)), tilt=float(rng.uniform(0.25, 0.45)), roll=float(rng.uniform(-0.1, 0.2)))
        rng.uniform(size=10)                               # the two views' draws
        depth, bgr, _ = synth.render(640, 480, R_obj=R, t_obj=t, seed=100 + s, **cam)
        out.append(("bench", O.quantize_pyramid(bgr, depth, 2)[2:4]))
    rng = np.random.default_rng(4321)
    for s in range(2):
        poses = []
        for (sx, sy) in [(-170.0, -50.0), (10.0, 60.0), (175.0, -35.0)]:
            poses.append(synth.object_pose(tx=sx + float(rng.uniform(-25, 25)), ty=sy + float(rng.uniform(-25, 25)), tz=float(rng.uniform(620, 720)),
                                           yaw=float(rng.uniform(-0.6, 0.6)), tilt=float(rng.uniform(0.2, 0.5)), roll=float(rng.uniform(-0.15, 0.25))))
        depth, bgr, _ = synth.render_clutter(640, 480, poses, seed=500 + s, **cam)
        rng.uniform(size=3 * 4 * 5)                        # the views' draws
        out.append(("clutter", O.quantize_pyramid(bgr, depth, 2)[2:4]))
    return out


def main(n_templates=300):
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import oracle_py as O
    from fealess_amd import synth
    from fealess_amd.bank import TemplateBank
    rng = np.random.default_rng(7)
    bank = TemplateBank("obj", 1, 2)
    for _ in range(n_templates):
        tl = synth.random_pyramid(rng, 2, 2, 640, 480)
        bank.add_pyramid(tl[2:4])                          # the level-1 templates: 31 + 31 features in an 80-pixel window
    rows = {}
    for kind, qs in _scenes():
        lms = [O.build_linear_memories(q, 8) for q in qs]
        for label, kw in (("groups of 8, per-wave check", dict(lanes=0, step=8)), ("groups of 8, dead lanes stop", dict(lanes=1, step=8)),
                          ("8, then groups of 4, dead lanes stop", dict(lanes=1, step=4)), ("8, then groups of 2, dead lanes stop", dict(lanes=1, step=2))):
            items = scan(lms, bank, 320, 240, 8, 75.0, **kw)
            r = rows.setdefault((kind, label), [0, 0, 0, 0, {}])
            r[0] += len(items)
            r[1] += sum(i["loads"] for i in items)
            r[2] += sum(i["lane_loads"] for i in items)
            r[3] += sum(i["lines"] for i in items)
            if kw == dict(lanes=1, step=2):
                for i in items:
                    for d, mask in i["checks"]:
                        if d <= 16:
                            c = r[4].setdefault(d, [0, 0])
                            c[0] += mask != 0
                            c[1] += bin(mask).count("1")
    for (kind, label), (n, loads, ll, lines, cont) in rows.items():
        print(f"{kind:8s} {label:40s} items {n}  loads/item {loads / n:.1f}  lane-loads/item {ll / n:.1f}  lines/item {lines / n:.0f}")
        for d in sorted(cont):
            print(f"         after {d:2d} features: {100.0 * cont[d][0] / n:.1f} % of the items continue, {cont[d][1] / max(1, cont[d][0]):.1f} live lanes in those")


if __name__ == "__main__":
    main()
