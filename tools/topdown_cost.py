#!/usr/bin/env python3
"""What top-down inference on full frames costs per captured inference step (README): InferStep(input_u8=(256, 256)) --
the crops already exist -- against InferStep(frames=(32, 1080, 1920)) with two hand boxes per frame and against the same with
track=True, alternated in ONE process on R50 64 x 256^2 bf16.  The frame legs add lh_box_affine, lh_affine_points [and
lh_keypoints_to_boxes] and swap the uint8 input kernel for lh_frames_crop_to_nhwc4, which writes the same bytes but gathers them from
199 MB of frames.  Two more legs price the oriented ROIs and the One-Euro filter against the track=True leg of the same run:
oriented + track swaps lh_box_affine / lh_keypoints_to_boxes for lh_roi_affine / lh_keypoints_to_rois (seeded directions, every second
box mirrored), oriented + track + smooth adds the lh_one_euro launch; the upright leg runs the oriented kernels with rot = (1, 0) and
no mirror, which separates the cost of the two sibling launches from that of gathering along turned rows.  Two legs price the
antialiased crop (antialias=True: lh_frames_crop_area_to_nhwc4 in the crop's place) against the frames leg: with the boxes above
(187..625 frame px into 256: 1..3 samples per axis) and with large boxes of half extent 300..500 px (3..5 per axis).  Two legs price
NV12 frames (frame_format="nv12": lh_frames_crop_yuv_to_nhwc4 in the crop's place, 100 MB of frames, tight layout, BT.709 limited)
against the frames and the frames+antialias legs, same boxes.  Four legs price what reaches the crop from a decoder, against the nv12
leg: "nv12 copy" pays a device-to-device copy of all 32 frames into ``step.frames`` in front of every replay (what a pipeline whose
decoder sits on the same GPU pays with a frame buffer), "nv12 surfaces" binds the 32 frames where they lie in front of every replay
(InferStep(surfaces=True): 32 addresses instead of 99.5 MB), "yuv420p surfaces" and "p010 surfaces" do the same for the planar and the
10-bit format (lh_frames_crop_surfaces_to_nhwc4 in the crop's place in all three).  One leg prices track management against the
oriented + track leg of the same run: ManagedInferStep(oriented + track) adds the lh_tracks_manage launch and hands over a full detection
list (64 boxes, two per frame, seeded) in front of every replay, three small copies and a fill.  Two legs price motion-aware tracking,
ManagedInferStep(manage_tracks=False, ...): "oriented+track+motion" adds the lh_rois_predict launch (motion=True) and is reported against
the oriented + track leg, "oriented+track+motion+gate" adds smooth= and smooth_gate=True on top (lh_one_euro_gated in lh_one_euro's place)
and is reported against that and against the oriented + track + smooth leg.  Two legs price the skeleton overlay,
ManagedInferStep(manage_tracks=False, oriented + track + smooth, overlay=True): "oriented+track+smooth+overlay" adds the lh_draw_hands launch
on the RGB frames and is reported against the oriented + track + smooth leg, "nv12 surf o+t+s+overlay" does the same on 32 NV12 surfaces of
its own, drawn in place, against "nv12 surf o+t+s", the same step without the overlay.  Device events around `steps` replays, after a
warm-up; median over the rounds.
usage (GPU box): python tools/topdown_cost.py [steps] [rounds]"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from lighthand_amd.runtime import InferStep, ManagedInferStep  # noqa: E402


def timed(step, n, feed=None):
    """``feed``: what every call passes (the legs that copy or bind frames in front of each replay); None: a bare replay."""
    feed = feed or {}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        step(**feed)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    batch, size, n_frames, hs, ws = 64, 256, 32, 1080, 1920
    rng = np.random.RandomState(0)
    model = bench.build_model(depth=50, precision="bf16").eval()
    crops = torch.from_numpy(rng.randint(0, 256, size=(batch, size, size, 3)).astype(np.uint8)).cuda()
    frames = torch.from_numpy(rng.randint(0, 256, size=(n_frames, hs, ws, 3)).astype(np.uint8)).cuda()
    # two hands per frame: boxes of 150..500 px around centres inside the frame (a hand at arm's length to close to the camera)
    centre = np.stack([rng.uniform(200, ws - 200, size=batch), rng.uniform(200, hs - 200, size=batch)], 1)
    half = rng.uniform(75, 250, size=(batch, 1))
    boxes = torch.from_numpy(np.concatenate([centre - half, centre + half], 1).astype(np.float32)).cuda()
    index = (torch.arange(batch, dtype=torch.int32) // 2).cuda()
    rot = torch.from_numpy(rng.normal(size=(batch, 2)).astype(np.float32)).cuda()
    mirror = (torch.arange(batch, dtype=torch.int32) % 2).cuda()
    # a hand close to the camera: half extents of 300..500 px (drawn after everything above, which keeps its numbers)
    half_l = rng.uniform(300, 500, size=(batch, 1))
    large = torch.from_numpy(np.concatenate([centre - half_l, centre + half_l], 1).astype(np.float32)).cuda()

    forms = {"uint8 crops": InferStep(model, batch, size, size, input_u8=(size, size)),
             "frames": InferStep(model, batch, size, size, frames=(n_frames, hs, ws)),
             "frames+track": InferStep(model, batch, size, size, frames=(n_frames, hs, ws), track=True),
             "oriented+track": InferStep(model, batch, size, size, frames=(n_frames, hs, ws), track=True, oriented=True),
             "oriented upright": InferStep(model, batch, size, size, frames=(n_frames, hs, ws), track=True, oriented=True),
             "oriented+track+smooth": InferStep(model, batch, size, size, frames=(n_frames, hs, ws), track=True, oriented=True,
                                                smooth=(1.0, 0.007)),
             "frames+antialias": InferStep(model, batch, size, size, frames=(n_frames, hs, ws), antialias=True),
             "frames+antialias large": InferStep(model, batch, size, size, frames=(n_frames, hs, ws), antialias=True)}
    forms["nv12"] = InferStep(model, batch, size, size, frames=(n_frames, hs, ws), frame_format="nv12")
    forms["nv12+antialias"] = InferStep(model, batch, size, size, frames=(n_frames, hs, ws), frame_format="nv12", antialias=True)
    nv12 = torch.from_numpy(rng.randint(0, 256, size=(n_frames, hs * 3 // 2, ws)).astype(np.uint8)).cuda()   # drawn last: see above
    for tag in ("nv12", "nv12+antialias"):
        forms[tag](frames=nv12, boxes=boxes, frame_index=index)
    forms["uint8 crops"](crops)
    for tag in ("frames", "frames+track"):
        forms[tag](frames=frames, boxes=boxes, frame_index=index)
    for tag in ("oriented+track", "oriented+track+smooth"):
        forms[tag](frames=frames, boxes=boxes, frame_index=index, rot=rot, mirror=mirror)
    forms["oriented upright"](frames=frames, boxes=boxes, frame_index=index)
    forms["frames+antialias"](frames=frames, boxes=boxes, frame_index=index)
    forms["frames+antialias large"](frames=frames, boxes=large, frame_index=index)
    from lighthand_amd.topdown import crop_taps_host
    for tag in ("frames+antialias", "frames+antialias large"):
        taps = crop_taps_host(forms[tag].plan.crop_mat.cpu().numpy())
        print(f"  {tag}: {int(taps.min())}..{int(taps.max())} samples per axis, {float(taps.prod(1).mean()):.1f} per crop pixel on average", flush=True)
    # what a decoder hands over per replay (after every draw above): the same 99.5 MB as 32 frames of their own, and the RGB bytes
    # read as 32 tight p010 frames (both are hs * ws * 3 bytes)
    planes = list(nv12.reshape(n_frames, -1).unbind(0))
    wide = list(frames.reshape(n_frames, -1).unbind(0))
    forms["nv12 copy"] = InferStep(model, batch, size, size, frames=(n_frames, hs, ws), frame_format="nv12")
    feeds = {"nv12 copy": dict(frames=nv12.clone())}
    for tag, fmt, src in (("nv12 surfaces", "nv12", planes), ("yuv420p surfaces", "yuv420p", planes), ("p010 surfaces", "p010", wide)):
        forms[tag] = InferStep(model, batch, size, size, frames=(n_frames, hs, ws), frame_format=fmt, surfaces=True)
        feeds[tag] = dict(surfaces=src)
    for tag, feed in feeds.items():
        forms[tag](boxes=boxes, frame_index=index, **feed)
    # a detector's output per replay (drawn after every draw above): as many boxes as slots, two per frame, any score
    det_c = np.stack([rng.uniform(200, ws - 200, size=batch), rng.uniform(200, hs - 200, size=batch)], 1)
    det_h = rng.uniform(75, 250, size=(batch, 1))
    dets = (torch.from_numpy(np.concatenate([det_c - det_h, det_c + det_h], 1).astype(np.float32)).cuda(), index.clone(),
            torch.from_numpy(rng.uniform(0, 1, size=batch).astype(np.float32)).cuda())
    forms["oriented+track+manage"] = ManagedInferStep(model, batch, size, size, frames=(n_frames, hs, ws), track=True, oriented=True)
    feeds["oriented+track+manage"] = dict(detections=dets)
    forms["oriented+track+manage"](frames=frames, boxes=boxes, frame_index=index, rot=rot, mirror=mirror, detections=dets)
    motion = dict(frames=(n_frames, hs, ws), track=True, oriented=True, manage_tracks=False, motion=True)
    forms["oriented+track+motion"] = ManagedInferStep(model, batch, size, size, **motion)
    forms["oriented+track+motion+gate"] = ManagedInferStep(model, batch, size, size, smooth=(1.0, 0.007), smooth_gate=True, **motion)
    for tag in ("oriented+track+motion", "oriented+track+motion+gate"):
        forms[tag](frames=frames, boxes=boxes, frame_index=index, rot=rot, mirror=mirror)
    smooth = dict(frames=(n_frames, hs, ws), track=True, oriented=True, manage_tracks=False, smooth=(1.0, 0.007))
    forms["oriented+track+smooth+overlay"] = ManagedInferStep(model, batch, size, size, overlay=True, **smooth)
    forms["oriented+track+smooth+overlay"](frames=frames, boxes=boxes, frame_index=index, rot=rot, mirror=mirror)
    for tag, extra in (("nv12 surf o+t+s", {}), ("nv12 surf o+t+s+overlay", dict(overlay=True))):
        forms[tag] = ManagedInferStep(model, batch, size, size, frame_format="nv12", surfaces=True, **smooth, **extra)
        forms[tag](surfaces=list(nv12.clone().reshape(n_frames, -1).unbind(0)), boxes=boxes, frame_index=index, rot=rot, mirror=mirror)
    against = {"oriented+track+smooth+overlay": "oriented+track+smooth", "nv12 surf o+t+s+overlay": "nv12 surf o+t+s", "nv12 surf o+t+s": "nv12 surfaces"}
    for tag, step in forms.items():
        timed(step, 10, feeds.get(tag))                                   # warm-up (capture happened in the first call)
    ms = {tag: [] for tag in forms}
    for _ in range(rounds):
        for tag, step in forms.items():
            ms[tag].append(timed(step, steps, feeds.get(tag)))
    med = {tag: statistics.median(v) for tag, v in ms.items()}
    print(f"r50 bs{batch} {size}^2 bf16 inference, {n_frames} frames of {hs} x {ws}, {batch // n_frames} boxes each:", flush=True)
    for tag, v in ms.items():
        if tag in against:
            print(f"  {tag:30s} {med[tag]:7.3f} ms/step median ({med[tag] - med[against[tag]]:+.3f} vs {against[tag]}; rounds: "
                  f"{', '.join(f'{x:.3f}' for x in v)})", flush=True)
            continue
        if tag == "oriented+track+manage":
            print(f"  {tag:22s} {med[tag]:7.3f} ms/step median ({med[tag] - med['oriented+track']:+.3f} vs oriented+track; rounds: "
                  f"{', '.join(f'{x:.3f}' for x in v)})", flush=True)
            continue
        if tag.startswith("oriented+track+motion"):
            print(f"  {tag:26s} {med[tag]:7.3f} ms/step median ({med[tag] - med['oriented+track']:+.3f} vs oriented+track, "
                  f"{med[tag] - med['oriented+track+smooth']:+.3f} vs oriented+track+smooth; rounds: {', '.join(f'{x:.3f}' for x in v)})", flush=True)
            continue
        if tag in feeds:
            print(f"  {tag:22s} {med[tag]:7.3f} ms/step median ({med[tag] - med['nv12']:+.3f} vs nv12; rounds: {', '.join(f'{x:.3f}' for x in v)})",
                  flush=True)
            continue
        print(f"  {tag:22s} {med[tag]:7.3f} ms/step median ({med[tag] - med['uint8 crops']:+.3f} vs uint8 crops, {med[tag] - med['frames']:+.3f} "
              f"vs frames, {med[tag] - med['frames+track']:+.3f} vs frames+track; rounds: {', '.join(f'{x:.3f}' for x in v)})", flush=True)


if __name__ == "__main__":
    main()
