"""Seeded synthetic camera frames for the tools that work on full frames (camera footage is not shipped): per hand a constellation
of 21 bright discs drifting over a dim noise background.  tools.track_frames tracks the sequence, tools.train --frame_size trains on
it (one hand per frame, the discs' centres as joints)."""
import argparse

import numpy as np


def frame_size_arg(text):
    parts = text.lower().split("x")
    if len(parts) != 2 or not all(p.isdigit() and int(p) > 0 for p in parts):
        raise argparse.ArgumentTypeError(f"--frame_size wants HSxWS (e.g. 1080x1920), not {text!r}")
    return int(parts[0]), int(parts[1])


def synthetic_sequence(n, hs, ws, hands, seed=0, spin=0.0, return_joints=False):
    """n frames uint8 [n][hs][ws][3] and the first frame's hand boxes fp32 [hands][4] (pixel-index coordinates, the bounds of each
    hand's 21 joints); with ``return_joints`` also the discs' centres fp32 [n][hands][21][2] (the frames are the same either way).
    Every hand is a fixed constellation of 21 discs, about a fifth of the frame's short side across, whose centre drifts on a seeded
    smooth path that stays inside the frame; ``spin`` degrees per frame turn it about that centre."""
    rng = np.random.RandomState(seed)
    span = max(8.0, min(hs, ws) / 5.0)
    frames = rng.randint(0, 32, size=(n, hs, ws, 3)).astype(np.uint8)
    shape = rng.uniform(-0.5, 0.5, size=(hands, 21, 2)) * span
    start = np.stack([rng.uniform(span, ws - span, size=hands), rng.uniform(span, hs - span, size=hands)], 1)
    phase, speed = rng.uniform(0, 2 * np.pi, size=(hands, 2)), rng.uniform(0.02, 0.08, size=(hands, 2))
    r = max(2, int(span / 16))
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    disc = (255 * np.clip(1.25 - np.hypot(xx, yy) / r, 0, 1)).astype(np.uint8)
    boxes = np.zeros((hands, 4), np.float32)
    every = np.zeros((n, hands, 21, 2), np.float32)
    for t in range(n):
        drift = 0.5 * span * np.sin(phase + speed * t) - 0.5 * span * np.sin(phase)
        turned = shape
        if spin:
            c, s = np.cos(np.deg2rad(spin * t)), np.sin(np.deg2rad(spin * t))
            turned = shape @ np.array([[c, s], [-s, c]])
        joints = turned + np.clip(start + drift, [span, span], [ws - span, hs - span])[:, None, :]
        every[t] = joints
        if t == 0:
            boxes[:, :2], boxes[:, 2:] = joints.min(1), joints.max(1)
        for x, y in np.rint(joints.reshape(-1, 2)).astype(int):
            y0, y1, x0, x1 = max(y - r, 0), min(y + r + 1, hs), max(x - r, 0), min(x + r + 1, ws)
            if y0 < y1 and x0 < x1:
                patch = disc[y0 - (y - r):y1 - (y - r), x0 - (x - r):x1 - (x - r), None]
                frames[t, y0:y1, x0:x1] = np.maximum(frames[t, y0:y1, x0:x1], patch)
    return (frames, boxes, every) if return_joints else (frames, boxes)
