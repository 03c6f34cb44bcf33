#!/usr/bin/env python3
"""What one plan consists of, as ONE JSON document: its pack / forward / backward lists entry by entry, the profile attribution, the
gradient marks and the table members -- to compare an engine refactor against its parent commit (run both with LH_AUTOTUNE=0, diff the
outputs).  --step also runs one captured step on a fixed synthetic batch and adds sha256 sums of what it computed.
usage: plan_dump.py [r18|r50|hrnet_w32] [bf16|fp16|fp32] [train|infer] [batch] [size] [--bucket BYTES] [--step]"""
import argparse
import hashlib
import json
import sys
import torch
sys.path.insert(0, ".")
from bench import build_model, synthetic_batch          # noqa: E402


def sha(t):
    return hashlib.sha256(t.detach().float().cpu().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", nargs="?", default="r50")
    ap.add_argument("precision", nargs="?", default="bf16")
    ap.add_argument("mode", nargs="?", default="train", choices=["train", "infer"])
    ap.add_argument("batch", nargs="?", type=int, default=2)
    ap.add_argument("size", nargs="?", type=int, default=256)
    ap.add_argument("--bucket", type=int, default=None, help="wgrad_bucket_bytes (a data-parallel plan)")
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    train, b, hw = a.mode == "train", a.batch, a.size
    model = build_model(hrnet_width=int(a.model[7:]), precision=a.precision) if a.model.startswith("hrnet") else build_model(int(a.model[1:]), a.precision)
    model.train(train)
    step = None
    if a.step and train:
        from lighthand_amd import parallel
        from lighthand_amd.runtime import TrainStep
        step = TrainStep(model, b, hw, hw, lr=1e-3, grad_sync=parallel.GradSync(world_size=1, bucket_bytes=a.bucket) if a.bucket else None)
    elif a.step:
        from lighthand_amd.runtime import InferStep
        step = InferStep(model, b, hw, hw)
    plan = step.plan if step else model.plan(b, hw, hw, training=train, backward=train, wgrad_bucket_bytes=a.bucket)
    entry = lambda c: c.kind if not hasattr(c, "fn") else (c.fn.__name__, c.what, len(c.args), c.lane, c.slane, c.mtag)
    where = {id(c): f"{name}[{i}]" for name in ("packs", "fwd", "bwd") for i, c in enumerate(getattr(plan, name))}
    doc = {name: [entry(c) for c in getattr(plan, name)] for name in ("packs", "fwd", "bwd")}
    doc["profile_meta"] = [(lst, where.get(id(c), c.what), kname, flops, nbytes) for lst, c, kname, flops, nbytes in plan.profile_meta]
    doc["bwd_marks"] = getattr(plan, "bwd_marks", [])
    doc["wgrad_tables"] = [names for _, _, names in plan.wgrad_tables]
    doc["n_groups"], doc["n_l2_touch"] = plan._n_groups, getattr(plan, "_n_l2_touch", 0)
    if step:
        images, joints = synthetic_batch(b, hw, "cuda")
        step(images, joints) if train else step(images)
        torch.cuda.synchronize()
        doc["sha256"] = dict(heatmap=sha(plan.out_nchw), grad=sha(model.arena().flat_grad) if train else None,
                             bn_running=sha(torch.cat([v.flatten().float() for k, v in model.named_buffers() if "running" in k])))
    print(json.dumps(doc, indent=1))


main()
