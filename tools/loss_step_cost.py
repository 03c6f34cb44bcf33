#!/usr/bin/env python3
"""What the visibility-weighted loss and hard-keypoint mining cost per training step: the plain TrainStep
(lh_gaussian_target + lh_mse_heatmap) against use_target_weight (lh_gaussian_target_w + lh_joints_mse: the same passes), ohkm_topk=8
(plane sums, select, gradient: one more read of the selected planes) and both, alternated in ONE process on R50 64 x 256^2 bf16.
Every joint is visible and in frame, so all forms train on the same planes.  Device events around `steps` replays, after a warm-up;
median over the rounds.  --coord_loss_weight L adds a leg: the plain step plus the integral-regression coordinate loss
(lh_integral_l1 behind lh_mse_heatmap: one more read of the heat-maps, one read and write of their gradient).
--frames times another pair instead, by the same method: the step on ready uint8 crops, TrainStep(input_u8=(256, 256)), against the step
that crops its hand ROIs from 32 full frames of 1080 x 1920 on the device, TrainStep(frames=(32, 1080, 1920)) (lh_box_affine +
lh_frames_crop_to_nhwc4 in the uint8 kernel's place, lh_affine_points_inv in front of the target render, lh_affine_points behind the
decode), the same with roi_aug=(30, 0.25, 0.1, 0.5) (lh_roi_perturb + lh_roi_affine, a new draw copied in per replay), and both with
crop_jitter=(0.5, 0.5, 0.5, 0.5) (lh_frames_crop_jitter_to_nhwc4: the grey-mean launch and ColorJitter in the crop, a new draw per
replay), and the frames leg with surfaces=True (the 32 frames bound in place: lh_frames_crop_surfaces_to_nhwc4 through the surface
table): seeded boxes of 200..400 frame pixels, two per frame.
usage (GPU box): python tools/loss_step_cost.py [steps] [rounds] [--coord_loss_weight L | --frames]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from lighthand_amd.runtime import TrainStep  # noqa: E402

argv = sys.argv[1:]
coord = None
if "--coord_loss_weight" in argv:
    k = argv.index("--coord_loss_weight")
    coord = float(argv[k + 1])
    del argv[k:k + 2]
frames_legs = "--frames" in argv
if frames_legs:
    argv.remove("--frames")
steps = int(argv[0]) if len(argv) > 0 else 30
rounds = int(argv[1]) if len(argv) > 1 else 5
dev = torch.device("cuda", 0)
batch = 64


def timed(step, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def frames_main():
    """The --frames legs (module docstring)."""
    import numpy as np
    n, hs, ws = 32, 1080, 1920
    rng = np.random.RandomState(0)
    side = rng.uniform(200, 400, size=(batch, 1))
    centre = np.stack([rng.uniform(250, ws - 250, size=batch), rng.uniform(250, hs - 250, size=batch)], 1)
    boxes = torch.from_numpy(np.concatenate([centre - side / 2, centre + side / 2], 1).astype(np.float32)).to(dev)
    jt = torch.from_numpy((centre[:, None, :] + rng.uniform(-0.4, 0.4, size=(batch, 21, 2)) * side[:, None, :]).astype(np.float32)).to(dev)
    index = (torch.arange(batch, dtype=torch.int32) % n).to(dev)
    frames = torch.randint(0, 256, (n, hs, ws, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    crops = torch.randint(0, 256, (batch, 256, 256, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
    crop_joints = torch.from_numpy(rng.uniform(20, 236, size=(batch, 21, 2)).astype(np.float32)).to(dev)
    legs = [("uint8 crops", dict(input_u8=(256, 256)), lambda st: st(crops, crop_joints)),
            ("frames", dict(frames=(n, hs, ws)), lambda st: st(frames=frames, boxes=boxes, frame_index=index, joints=jt)),
            ("frames+roi_aug", dict(frames=(n, hs, ws), roi_aug=(30.0, 0.25, 0.1, 0.5)),
             lambda st: st(frames=frames, boxes=boxes, frame_index=index, joints=jt)),
            ("frames+crop_jitter", dict(frames=(n, hs, ws), crop_jitter=(0.5, 0.5, 0.5, 0.5)),
             lambda st: st(frames=frames, boxes=boxes, frame_index=index, joints=jt)),
            ("frames+roi_aug+crop_jitter", dict(frames=(n, hs, ws), roi_aug=(30.0, 0.25, 0.1, 0.5), crop_jitter=(0.5, 0.5, 0.5, 0.5)),
             lambda st: st(frames=frames, boxes=boxes, frame_index=index, joints=jt)),
            # the frames leg with the 32 frames bound where they lie (lh_frames_crop_surfaces_to_nhwc4 in the crop's place)
            ("frames surfaces", dict(frames=(n, hs, ws), surfaces=True),
             lambda st: st(surfaces=frames.reshape(n, -1), boxes=boxes, frame_index=index, joints=jt))]
    forms = {}
    for tag, kw, first in legs:
        step = TrainStep(bench.build_model(depth=50, precision="bf16"), batch, 256, 256, lr=1e-3, **kw)
        first(step)
        timed(step, 10)
        forms[tag] = step
    ms = {tag: [] for tag in forms}
    for _ in range(rounds):
        for tag, step in forms.items():
            ms[tag].append(timed(step, steps))
    med = {tag: statistics.median(v) for tag, v in ms.items()}
    print(f"r50 bs{batch} 256^2 bf16, {n} frames of {hs} x {ws} ({frames.numel() / 1e6:.0f} MB) against {crops.numel() / 1e6:.1f} MB of crops:", flush=True)
    for tag, v in ms.items():
        print(f"  {tag:26s} {med[tag]:7.3f} ms/step median ({med[tag] - med['uint8 crops']:+.3f} vs uint8 crops; rounds: "
              f"{', '.join(f'{x:.3f}' for x in v)})", flush=True)


if frames_legs:
    frames_main()
    sys.exit(0)
images, joints = bench.synthetic_batch(batch, 256, dev)
forms = {}
legs = [("plain", {}), ("weighted", dict(use_target_weight=True)), ("ohkm-8", dict(ohkm_topk=8)),
        ("weighted+ohkm-8", dict(use_target_weight=True, ohkm_topk=8))]
if coord is not None:
    legs.append((f"coord-{coord:g}", dict(coord_loss_weight=coord)))
for tag, kw in legs:
    step = TrainStep(bench.build_model(depth=50, precision="bf16"), batch, 256, 256, lr=1e-3, **kw)
    step(images, joints)
    timed(step, 10)                                                   # warm-up (capture happened in the first call)
    forms[tag] = step
ms = {tag: [] for tag in forms}
for _ in range(rounds):
    for tag, step in forms.items():
        ms[tag].append(timed(step, steps))
med = {tag: statistics.median(v) for tag, v in ms.items()}
print(f"r50 bs{batch} 256^2 bf16, heat-maps {forms['plain'].plan.out_nchw.numel() * 4 / 1e6:.0f} MB:", flush=True)
for tag, v in ms.items():
    print(f"  {tag:16s} {med[tag]:7.3f} ms/step median ({med[tag] - med['plain']:+.3f} vs plain; rounds: {', '.join(f'{x:.3f}' for x in v)})",
          flush=True)
