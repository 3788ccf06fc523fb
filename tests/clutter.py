"""Cluttered test scenes: three instances of the object in front of a textured, non-planar background, and a bank of near
views of every instance trained with the ORACLE's Detector::addTemplate (so that the templates under test do not come from
the library under test), padded with random pyramids.  Modelled on bench.py's clutter workload (build_clutter), at test size.

Frames (all 640 x 480, one background):
  a  three separated instances (the bench layout);
  b  two instances overlapping: the nearer one hides part of the other;
  c  frame a shifted horizontally (np.roll), so that one instance crosses the image border;
  d  the background alone.
"""
import numpy as np

from fealess_amd import synth
from fealess_amd.bank import TemplateBank

W, H = 640, 480
LEVELS, T = 2, [5, 8]
K = (synth.FX, synth.FY, synth.CX, synth.CY)
FRAMES = ("a", "b", "c", "d")
SHIFT_C = 150                      # frame c = frame a rolled right by this many columns


def _tl_from_oracle(ex):
    """oracle.add_template's (templates, features, bb) -> the template dicts of TemplateBank.add_pyramid."""
    t, feats, _ = ex
    return [dict(width=int(h["width"]), height=int(h["height"]), offset_x=int(h["offset_x"]), offset_y=int(h["offset_y"]),
                 pyramid_level=int(h["pyramid_level"]), features=np.stack([f["x"], f["y"], f["label"]], 1).astype(np.int32))
            for h, f in zip(t, feats)]


def _shift(a, dx, dy):
    """a moved by (dx, dy) whole pixels, zero-filled."""
    out = np.zeros_like(a)
    h, w = a.shape[:2]
    out[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = a[max(-dy, 0):h - max(dy, 0), max(-dx, 0):w - max(dx, 0)]
    return out


def build(oracle, views=8, n_random=100, seed=4321):
    """Returns dict(bank, K, frames={name: (bgr, depth)}, masks={name: visible mask per instance}, full_masks_b (the masks of
    frame b's instances before compositing), poses, n_trained)."""
    rng = np.random.default_rng(seed)
    poses = []
    for (sx, sy) in [(-170.0, -50.0), (10.0, 60.0), (175.0, -35.0)]:
        poses.append(synth.object_pose(tx=sx + float(rng.uniform(-25, 25)), ty=sy + float(rng.uniform(-25, 25)),
                                       tz=float(rng.uniform(620, 720)), yaw=float(rng.uniform(-0.6, 0.6)),
                                       tilt=float(rng.uniform(0.2, 0.5)), roll=float(rng.uniform(-0.15, 0.25))))
    depth_a, bgr_a, masks_a = synth.render_clutter(W, H, poses, seed=500)
    depth_d, bgr_d, _ = synth.render_clutter(W, H, [], seed=500)          # the same wall, texture and noise, no instance
    # b: instance 1 where it is in a, instance 2 moved by whole pixels to just behind it (its depth 60 mm farther away), both
    # composited over the background of a by depth: instance 1 hides a fifth of instance 2.  A pixel shift keeps the labels
    # that the near views of instance 2 were trained on.
    frames = {"a": (bgr_a, depth_a), "d": (bgr_d, depth_d)}
    nrng = np.random.default_rng(seed + 1)
    zbuf = np.full((H, W), np.inf)
    bgr_b, depth_b = bgr_d.astype(np.float64), depth_d.astype(np.float64)
    masks_b, full_b = [], []
    for j, dx, dy, dz in ((1, 0, 0, 0), (2, -90, 40, 60)):
        R, t = poses[j]
        d_j, c_j, m_j = synth.render(W, H, R, t, seed=900 + j, noise=False, background=False)
        d_j, c_j, m_j = _shift(d_j, dx, dy), _shift(c_j, dx, dy), _shift(m_j, dx, dy)
        z = np.where(m_j, d_j.astype(np.float64) + dz, np.inf)
        win = z < zbuf
        zbuf = np.where(win, z, zbuf)
        depth_b = np.where(win, z + nrng.integers(-1, 2, size=z.shape), depth_b)
        bgr_b = np.where(win[..., None], c_j + nrng.normal(0, 1.5, size=c_j.shape), bgr_b)
        masks_b = [m & ~win for m in masks_b] + [win]
        full_b.append(m_j)
    frames["b"] = (np.clip(np.rint(bgr_b), 0, 255).astype(np.uint8), np.clip(np.rint(depth_b), 0, 65535).astype(np.uint16))
    frames["c"] = (np.roll(bgr_a, SHIFT_C, axis=1), np.roll(depth_a, SHIFT_C, axis=1))
    masks = {"a": masks_a, "b": masks_b, "c": [np.roll(m, SHIFT_C, axis=1) for m in masks_a], "d": []}

    bank = TemplateBank("obj", LEVELS, 2)
    n_trained = 0
    for j, (R, t) in enumerate(poses):
        for v in range(views):
            dR = synth.rot_z(np.deg2rad(rng.uniform(-1.5, 1.5))) @ synth.rot_x(np.deg2rad(rng.uniform(-1.5, 1.5)))
            tt = t + np.array([rng.uniform(-8, 8), rng.uniform(-8, 8), rng.uniform(-5, 5)])
            s = 5000 + 10 * j + v
            d_bg, bgr_v, mask = synth.render(W, H, dR @ R, tt, seed=s, noise=False, background=True)
            ex = oracle.add_template(bgr_v, d_bg, (mask * 255).astype(np.uint8), LEVELS)
            if ex is None:
                continue
            d_obj, _, _ = synth.render(W, H, dR @ R, tt, seed=s, noise=False, background=False)
            bank.add_pyramid(_tl_from_oracle(ex), synth.pose13(dR @ R, tt),
                             (d_obj.astype(np.uint32) * 10).clip(0, 65535).astype(np.uint16))
            n_trained += 1
    for _ in range(n_random):                 # no depth render: never refined
        bank.add_pyramid(synth.random_pyramid(rng, LEVELS, 2, W, H), None, None)
    return dict(bank=bank, K=K, frames=frames, masks=masks, full_masks_b=full_b, poses=poses, n_trained=n_trained)
