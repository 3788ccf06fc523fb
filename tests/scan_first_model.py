"""k_scan's schedule with a streamed first piece restated in numpy (fl_scan.hip: scan_item), no GPU.

tests/scan_prune_model.py with one more argument: `first`, the features of a modality's first piece (8, 12, 14 or 16).  A
modality with more than eight padded features adds its first `first` features in one piece, with no check inside, and checks
the bound once behind it; a modality with eight adds those.  The rest of the second group follows in pieces that end at the
multiples of `step`, then the groups of eight cut into pieces of `step`, as before.  The check behind a piece is enabled by the
bit of `mid` of the 8-feature group that holds the piece's last feature: for `first` > 8 the first check goes by bit 1.  `first`
= 8 is scan_prune_model.scan, item for item (tests/test_scan_first_model_cpu.py).

Leaving out the checks behind 8 and 12 features is exact for the same reason every check is: a check only ever removes lanes
that cannot reach the threshold, so fewer checks keep a superset of lanes alive.

Run as a script, it prints scan_prune_model's table extended by the `first` schedules: loads, lane-loads and lines per item
and the share of items that end at the check behind the first piece (CPU only, a few minutes).
"""
import numpy as np

from scan_prune_model import FL_SCAN_PRUNE_MID, _scenes, alive_after, bank_tables, matches, raw_threshold  # noqa: F401

FIRSTS = (8, 12, 14, 16)


def pieces(n_pad, first, step):
    """[(start, count, bit of mid)] for a modality of n_pad padded features."""
    if n_pad <= 0:
        return []
    out = []
    if first > 8 and n_pad > 8:
        out.append((0, first, 1))
        s = first
        while s < 16:
            e = min(16, (s // step + 1) * step)
            out.append((s, e - s, 1))
            s = e
        k0 = 16
    else:
        out.append((0, 8, 0))
        k0 = 8
    for k in range(k0, n_pad, 8):
        for s in range(0, 8, step):
            out.append((k + s, step, k >> 3))
    return out


def scan(lms, bank, w, h, T, threshold, mid=FL_SCAN_PRUNE_MID, lanes=1, step=4, prune=1, first=8):
    """As scan_prune_model.scan; every item also has `first_end` (the item ended at the check behind a first piece) and
    `trips` (pieces loaded: the dependent vector round trips)."""
    assert first in FIRSTS and step in (8, 4, 2)
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
            it = dict(g=g, chunk=chunk, checks=[], ended=None, first_end=False, trips=0, loads=0, lane_loads=0, lines=0,
                      candidates=[])
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
                for s0, n, bit in pieces(len(offs), first, step):
                    need = (alive | np.concatenate([[False], alive[:-1]])) & (lane_ids < lanes_on)
                    sel = need[lane_of]
                    it["trips"] += 1
                    it["loads"] += n
                    it["lane_loads"] += n * int(need.sum())
                    for off in offs[s0:s0 + n]:
                        if off is None:                    # the zero pad: one line whatever the lanes
                            it["lines"] += 1 if need.any() else 0
                            continue
                        a = off + chunk * 1024
                        a4 = a - (a & 3)                   # the aligned 16 bytes a lane loads, relative to the label planes
                        lo = (a4 + 16 * lane_ids[need]) // 64
                        hi = (a4 + 16 * lane_ids[need] + 15) // 64
                        it["lines"] += len(np.union1d(lo, hi))
                        acc[sel] += flat[m][a:a + 1024][sel]
                    done += n
                    if prune and (mid >> bit) & 1:
                        part = acc.reshape(64, 16).max(1)
                        left = nf_all - nf + max(0, h_nf - (s0 + n))
                        if not check(mx_tot + part + 4 * left > thr):
                            it["first_end"] = s0 == 0
                            over = True
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
    schedules = [("groups of 8, per-wave check", dict(lanes=0, step=8)), ("groups of 8, dead lanes stop", dict(lanes=1, step=8)),
                 ("8, then groups of 4, dead lanes stop", dict(lanes=1, step=4)), ("8, then groups of 2, dead lanes stop", dict(lanes=1, step=2))]
    for first in (12, 14, 16):
        for step in (4, 2):
            schedules.append((f"first {first}, then pieces to multiples of {step}", dict(lanes=1, step=step, first=first)))
    rows = {}
    for kind, qs in _scenes():
        lms = [O.build_linear_memories(q, 8) for q in qs]
        for label, kw in schedules:
            items = scan(lms, bank, 320, 240, 8, 75.0, **kw)
            r = rows.setdefault((kind, label), [0, 0, 0, 0, 0, 0, 0])
            r[0] += len(items)
            r[1] += sum(i["loads"] for i in items)
            r[2] += sum(i["lane_loads"] for i in items)
            r[3] += sum(i["lines"] for i in items)
            r[4] += sum(i["first_end"] for i in items)
            r[5] += sum(i["trips"] for i in items)
            r[6] += sum(i["trips"] == 1 for i in items)
    for (kind, label), (n, loads, ll, lines, fe, trips, one) in rows.items():
        print(f"{kind:8s} {label:44s} items {n}  loads/item {loads / n:.1f}  lane-loads/item {ll / n:.1f}  lines/item {lines / n:.0f}  "
              f"pieces/item {trips / n:.2f}  ended by the first piece's check {100.0 * fe / n:.1f} %  after one piece {100.0 * one / n:.1f} %")


if __name__ == "__main__":
    main()
