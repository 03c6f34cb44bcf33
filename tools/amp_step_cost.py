#!/usr/bin/env python3
"""What dynamic loss scaling costs per training step: the static loss_scale=1024 step against the dynamic one
(lh_amp_check over the gradient arena + lh_amp_update + lh_adam_apply_guarded in place of lh_adam_step), alternated in ONE process,
on R50 64 x 256^2 fp16 and HRNet-W32 32 x 256^2 fp16.  The dynamic step starts at 1024 and never grows, so both forms do the same
arithmetic; its skipped steps are reported (a skipped update is cheaper and would flatter it).  Device events around `steps` replays,
after a warm-up; median over the rounds.
usage (GPU box): python tools/amp_step_cost.py [steps] [rounds] [configs: r50,hrnet32]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from lighthand_amd.amp import DynamicLossScale  # noqa: E402
from lighthand_amd.runtime import TrainStep  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
configs = sys.argv[3].split(",") if len(sys.argv) > 3 else ["r50", "hrnet32"]
dev = torch.device("cuda", 0)
SHAPES = {"r50": (dict(depth=50), 64), "hrnet32": (dict(hrnet_width=32), 32)}


def timed(step, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


for cfg in configs:
    kw, batch = SHAPES[cfg]
    images, joints = bench.synthetic_batch(batch, 256, dev)
    forms = {}
    for tag, scale in (("static-1024", 1024.0), ("dynamic", DynamicLossScale(init_scale=1024.0, growth_interval=10 ** 9))):
        step = TrainStep(bench.build_model(precision="fp16", **kw), batch, 256, 256, lr=1e-3, loss_scale=scale)
        step(images, joints)
        timed(step, 10)                                                   # warm-up (capture happened in the first call)
        forms[tag] = step
    ms = {tag: [] for tag in forms}
    for _ in range(rounds):
        for tag, step in forms.items():
            ms[tag].append(timed(step, steps))
    med = {tag: statistics.median(v) for tag, v in ms.items()}
    arena = forms["dynamic"].arena.numel
    print(f"{cfg} bs{batch} 256^2 fp16, arena {arena / 1e6:.1f} M params ({arena * 4 / 1e6:.0f} MB of gradients checked):", flush=True)
    for tag, v in ms.items():
        print(f"  {tag:12s} {med[tag]:7.3f} ms/step median (rounds: {', '.join(f'{x:.3f}' for x in v)})", flush=True)
    print(f"  dynamic - static = {med['dynamic'] - med['static-1024']:+.3f} ms/step; dynamic skipped "
          f"{forms['dynamic'].scaler.skipped_steps} steps, scale {forms['dynamic'].scaler.scale:g}", flush=True)
    del forms
    torch.cuda.empty_cache()
