#!/usr/bin/env python3
"""Top-down inference on full camera frames, closed loop: every frame is cropped at the hand boxes ON THE DEVICE, the keypoints are
decoded and taken back to frame coordinates, and the next frame's boxes are the bounds of this frame's keypoints -- one replay of a
captured graph plus one device-to-device copy per frame, no host arithmetic in between (runtime.InferStep(frames=..., track=True)).

    track_frames.py --synthetic N --frame_size HSxWS [--hands 2] [--flip_test] [--dark_decode]
                    [--oriented] [--mirror] [--one_euro MIN_CUTOFF BETA] [--spin DEG_PER_FRAME] [--antialias [N]]
                    [--frame_format nv12|nv21|yuv420p|p010 [--yuv_matrix bt601|bt709] [--yuv_range limited|full]
                     [--chroma_siting left|center]] [--surfaces] [--detect_every N [--max_lost M]]
                    [--motion [--motion_cutoff HZ] [--motion_lead F] [--coast N]] [--smooth_gate [--gate_min_score S] [--no_size_norm]]

``--synthetic N`` renders a seeded sequence of N frames: per hand a cluster of 21 bright discs drifting over a dim noise background
(camera footage is not shipped; a real loop copies each captured frame into ``step.frames`` and its detector's boxes into
``step.boxes`` once, then calls ``step()`` / ``step.advance()`` per frame).  Prints ONE JSON line: frames per second, the number of
(frame, hand) slots that were lost (too few confident joints: the box is kept), and the options.  The weights
are seeded random ones, so the keypoints mean nothing and their confidences are far below InferStep's default ``track_min_score``:
the tool sets the threshold to the median confidence of the first frame (a replay of a probe step), so about half of the joints count,
the boxes move from frame to frame and some slots are lost -- the loop runs as it would with a trained model.

``--oriented`` follows oriented ROIs (InferStep(oriented=True): the crop is turned so that wrist -> middle-finger MCP points up),
``--mirror`` marks every second hand as a left one (its crop is mirrored; needs ``--oriented``), ``--one_euro MIN_CUTOFF BETA``
filters the keypoints (InferStep(smooth=...)); the line then also gives the mean distance between ``preds`` and ``smooth_preds``.
``--spin DEG_PER_FRAME`` turns every synthetic constellation about its centre.  ``--antialias [N]`` averages up to N (8 when N is left
out) samples per axis over each crop pixel's footprint where a ROI is minified (InferStep(antialias=N)).  ``--frame_format nv12`` hands
the step what a video decoder does: the synthetic frames are encoded to NV12 on the host (topdown.rgb_to_nv12_host, with
``--yuv_matrix`` / ``--yuv_range``) and the crop converts each sample back (InferStep(frame_format="nv12", yuv=..., chroma_siting=...)).
``--frame_format nv21 | yuv420p | p010`` encode with topdown.rgb_to_yuv420_host in the tight layout of that format.  ``--surfaces``
allocates one device tensor per synthetic frame, as a decoder on the same GPU leaves its surfaces, and binds the frame's tensor in
front of every replay in place of the copy into ``step.frames`` (InferStep(surfaces=True), ``step(surfaces=[tensor])``).
``--detect_every N`` manages the tracks on the device (runtime.ManagedInferStep(manage_tracks=dict(max_lost=M))): the detector is the scene's own
ground truth, the bounds of each hand's joints jittered by a few pixels with the tool's seed, handed over as ``detections=`` on every
N-th frame; hand 0 leaves the scene for the middle fifth of the sequence (its region is painted over with the background) and is
detected once more on the frame it re-enters.  The line then also counts the slots that were seeded by a detection, suppressed as
duplicates and expired after ``--max_lost`` lost frames in a row (default 0: never).
``--motion`` predicts each next ROI from the box's low-passed velocity (runtime.ManagedInferStep(motion=dict(cutoff=HZ, lead=F, coast=N)):
``--motion_cutoff`` Hz, default 10; ``--motion_lead`` frames of lead, default 1; ``--coast N`` replays a lost slot keeps moving, default 0);
the line then also gives the mean speed of the found slots in frame px / s and the number of coasted slots.  ``--smooth_gate``, on top of
``--one_euro``, gates the filter per joint at ``--gate_min_score`` (default: the tracking threshold) and measures speed in hand sizes
unless ``--no_size_norm`` (ManagedInferStep(smooth_gate=dict(min_score=S, by_size=...))).
``--overlay_out DIR`` draws the tracked hands into the frames on the device (runtime.ManagedInferStep(overlay=...): ROI outline, bones,
joint discs; ``--overlay_smooth`` draws the filtered keypoints) and writes every ``--overlay_every``-th annotated frame after its replay:
packed RGB as binary PPM, a 4:2:0 frame as its raw surface bytes beside a one-line sidecar with format, size and pitches.
With none of these the sequence and the line are what they were; the new keys appear only with the new options."""
import argparse
import json
import os
import time

from lighthand_amd.tools.synthetic_frames import frame_size_arg as _frame_size, synthetic_sequence  # noqa: F401  (the renderer is shared with tools.train)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", default=0, type=int, help="number of seeded synthetic frames to render and track")
    ap.add_argument("--frame_size", default=(1080, 1920), type=_frame_size, help="HSxWS of the camera frames")
    ap.add_argument("--hands", default=2, type=int, help="hand boxes per frame (slots of the captured step)")
    ap.add_argument("--depth", default=50, type=int)
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--size", default=256, type=int, help="side of the square crop the model reads")
    ap.add_argument("--flip_test", action="store_true", help="average with the flipped-back heat-maps of the mirrored crop")
    ap.add_argument("--dark_decode", action="store_true", help="DARK decode in place of the plain arg-max")
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--oriented", action="store_true", help="oriented ROIs: the crop follows the hand's rotation in the image plane")
    ap.add_argument("--mirror", action="store_true", help="every second hand is a left one: its crop is mirrored (needs --oriented)")
    ap.add_argument("--one_euro", nargs=2, type=float, default=None, metavar=("MIN_CUTOFF", "BETA"), help="One-Euro filter of the keypoints")
    ap.add_argument("--spin", default=0.0, type=float, metavar="DEG_PER_FRAME", help="turn each synthetic constellation about its centre")
    ap.add_argument("--antialias", nargs="?", type=int, const=8, default=None, metavar="N",
                    help="area sampling of minified ROIs: at most N (1..8, default 8) samples per crop pixel and axis")
    ap.add_argument("--frame_format", default="rgb", choices=["rgb", "nv12", "nv21", "yuv420p", "p010"],
                    help="what the frame buffer holds: packed RGB or a 4:2:0 format under its decoder's name")
    ap.add_argument("--yuv_matrix", default="bt709", choices=["bt601", "bt709"], help="luma coefficients of NV12 frames")
    ap.add_argument("--yuv_range", default="limited", choices=["limited", "full"], help="quantisation range of NV12 frames")
    ap.add_argument("--chroma_siting", default="left", choices=["left", "center"], help="horizontal position of NV12's chroma samples")
    ap.add_argument("--surfaces", action="store_true", help="one device tensor per frame, bound in place (no copy into a frame buffer)")
    ap.add_argument("--detect_every", default=0, type=int, metavar="N", help="manage the tracks on the device; ground-truth detections every N-th frame")
    ap.add_argument("--max_lost", default=0, type=int, metavar="M", help="with --detect_every: a slot lost M frames in a row is emptied (0: never)")
    ap.add_argument("--motion", action="store_true", help="predict the next ROI from the box's velocity")
    ap.add_argument("--motion_cutoff", default=10.0, type=float, metavar="HZ", help="with --motion: cut-off of the velocity's low-pass")
    ap.add_argument("--motion_lead", default=1.0, type=float, metavar="F", help="with --motion: frames of lead")
    ap.add_argument("--coast", default=0, type=int, metavar="N", help="with --motion: replays in a row a lost slot keeps moving")
    ap.add_argument("--smooth_gate", action="store_true", help="with --one_euro: gate the filter per joint by confidence")
    ap.add_argument("--gate_min_score", default=None, type=float, metavar="S", help="with --smooth_gate: the gate (default: the tracking threshold)")
    ap.add_argument("--no_size_norm", action="store_true", help="with --smooth_gate: keep the filter's speed in frame pixels per second")
    ap.add_argument("--overlay_out", default=None, metavar="DIR", help="draw the tracked hands into the frames on the device and write them here")
    ap.add_argument("--overlay_every", default=1, type=int, metavar="N", help="with --overlay_out: write every N-th frame")
    ap.add_argument("--overlay_smooth", action="store_true", help="with --overlay_out and --one_euro: draw the filtered keypoints")
    return ap


def write_overlay_frame(directory, t, frame, frame_format, hs, ws, layout=None):
    """One annotated frame (a uint8 device tensor) -> its file's name: packed RGB as a binary PPM (``frame_%05d.ppm``); a 4:2:0 frame as
    its raw surface bytes (``frame_%05d.<format>``) beside a one-line sidecar (``.txt``) with format, size and pitches.  The copy to the
    host is this tool's, after the replay: the step itself never moves a frame."""
    data = frame.cpu().numpy().reshape(-1)
    if frame_format == "rgb":
        name = os.path.join(directory, f"frame_{t:05d}.ppm")
        with open(name, "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (ws, hs))
            f.write(data[:hs * ws * 3].tobytes())
        return name
    name = os.path.join(directory, f"frame_{t:05d}.{frame_format}")
    with open(name, "wb") as f:
        f.write(data.tobytes())
    with open(name + ".txt", "w") as f:
        pitch = f" pitch={layout.pitch} c_pitch={layout.c_pitch} cb_offset={layout.cb_offset} cr_offset={layout.cr_offset}" if layout is not None else f" pitch={ws}"
        f.write(f"format={frame_format} width={ws} height={hs}{pitch} bytes={data.size}\n")
    return name


def main(argv=None):
    import torch

    from lighthand_amd.runtime import InferStep, ManagedInferStep
    from lighthand_amd.modeling.simplebaseline.config import default_config
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.synthetic < 1:
        raise SystemExit("camera footage is not shipped: pass --synthetic N")
    if args.hands < 1:
        ap.error("--hands must be >= 1")
    if args.mirror and not args.oriented:
        ap.error("--mirror needs --oriented")
    if args.antialias is not None and not 1 <= args.antialias <= 8:
        ap.error("--antialias takes 1..8")
    if args.detect_every < 0 or args.max_lost < 0 or (args.max_lost and not args.detect_every):
        ap.error("--detect_every N >= 1 turns track management on; --max_lost M >= 0 needs it")
    if not args.motion and (args.motion_cutoff, args.motion_lead, args.coast) != (10.0, 1.0, 0):
        ap.error("--motion_cutoff / --motion_lead / --coast need --motion")
    if args.smooth_gate and not args.one_euro:
        ap.error("--smooth_gate needs --one_euro")
    if not args.smooth_gate and (args.gate_min_score is not None or args.no_size_norm):
        ap.error("--gate_min_score / --no_size_norm need --smooth_gate")
    if args.overlay_out is None and (args.overlay_every != 1 or args.overlay_smooth):
        ap.error("--overlay_every / --overlay_smooth need --overlay_out")
    if args.overlay_every < 1 or (args.overlay_smooth and not args.one_euro):
        ap.error("--overlay_every N >= 1; --overlay_smooth needs --one_euro")
    hs, ws = args.frame_size
    if args.detect_every:
        import numpy as np
        frames, boxes, joints = synthetic_sequence(args.synthetic, hs, ws, args.hands, args.seed, spin=args.spin, return_joints=True)
        rng = np.random.RandomState(args.seed + 1)
        truth = np.concatenate([joints.min(2), joints.max(2)], 2)                 # [n][hands][4]
        truth = (truth + rng.uniform(-3, 3, size=truth.shape)).astype(np.float32)
        away = range(2 * args.synthetic // 5, 3 * args.synthetic // 5)          # hand 0 is out of the scene on these frames
        for t in away:
            x0, y0, x1, y1 = np.rint(truth[t, 0] + (-8, -8, 8, 8)).astype(int).clip(0, [ws, hs, ws, hs])
            frames[t, y0:y1, x0:x1] = rng.randint(0, 32, size=(y1 - y0, x1 - x0, 3))
    else:
        frames, boxes = synthetic_sequence(args.synthetic, hs, ws, args.hands, args.seed, spin=args.spin)
    torch.manual_seed(args.seed)
    model = get_pose_net(default_config(args.depth), is_train=True).cuda().set_precision(args.precision)
    model.eval()
    options = dict(frames=(1, hs, ws), flip_test=args.flip_test, post_process="dark" if args.dark_decode else False)
    if args.oriented:
        options["oriented"] = True
    if args.antialias is not None:
        options["antialias"] = args.antialias
    if args.frame_format == "nv12":
        from lighthand_amd.topdown import rgb_to_nv12_host
        if hs % 2 or ws % 2:
            ap.error("--frame_format nv12 needs even frame sides")
        frames = rgb_to_nv12_host(frames, args.yuv_matrix, args.yuv_range)
        options.update(frame_format="nv12", yuv=(args.yuv_matrix, args.yuv_range), chroma_siting=args.chroma_siting)
    elif args.frame_format != "rgb":
        from lighthand_amd.topdown import rgb_to_yuv420_host
        if hs % 2 or ws % 2:
            ap.error(f"--frame_format {args.frame_format} needs even frame sides")
        frames = rgb_to_yuv420_host(frames, args.frame_format, args.yuv_matrix, args.yuv_range)
        options.update(frame_format=args.frame_format, yuv=(args.yuv_matrix, args.yuv_range), chroma_siting=args.chroma_siting)
    elif (args.yuv_matrix, args.yuv_range, args.chroma_siting) != ("bt709", "limited", "left"):
        ap.error("--yuv_matrix / --yuv_range / --chroma_siting need --frame_format nv12")
    if args.surfaces:
        options["surfaces"] = True
    mirror = torch.arange(args.hands, dtype=torch.int32) % 2 if args.mirror else None
    seq = torch.from_numpy(frames).pin_memory()
    if args.surfaces:                                              # what a decoder on this GPU leaves behind: one tensor per frame
        surfaces = [f.cuda().reshape(-1) for f in seq]
        feed = lambda t: dict(surfaces=surfaces[t:t + 1])          # noqa: E731
    else:
        feed = lambda t: dict(frames=seq[t:t + 1])                 # noqa: E731
    probe = InferStep(model, args.hands, args.size, args.size, **options)
    probe(boxes=torch.from_numpy(boxes), mirror=mirror, **feed(0))
    score = float(probe.maxvals.median())                          # random weights: see the module docstring
    del probe
    if args.one_euro:
        options["smooth"] = tuple(args.one_euro)
    if args.detect_every:
        options["manage_tracks"] = dict(max_lost=args.max_lost)
    managed = bool(args.detect_every or args.motion or args.smooth_gate or args.overlay_out)
    if managed and not args.detect_every:
        options["manage_tracks"] = False
    if args.motion:
        options["motion"] = dict(cutoff=args.motion_cutoff, lead=args.motion_lead, coast=args.coast)
    if args.smooth_gate:
        options["smooth_gate"] = dict(min_score=score if args.gate_min_score is None else args.gate_min_score, by_size=not args.no_size_norm)
    if args.overlay_out:                                           # the ROI outline is on: a follower's lag is visible
        options["overlay"] = dict(source="smooth" if args.overlay_smooth else "raw")
        os.makedirs(args.overlay_out, exist_ok=True)
        written = []
    step = (ManagedInferStep if managed else InferStep)(model, args.hands, args.size, args.size, track=True, track_min_score=score, **options)
    step.boxes.copy_(torch.from_numpy(boxes))
    lost = torch.zeros(args.hands, dtype=torch.int64, device=step.lost.device)
    moved = torch.zeros((), dtype=torch.float64, device=step.lost.device)
    step(mirror=mirror, **feed(0))                                 # capture; the loop below starts from the first frame's boxes again
    step.boxes.copy_(torch.from_numpy(boxes))
    if args.overlay_out and args.surfaces:
        surfaces[0].copy_(seq[0].reshape(-1))                      # the capture call drew on it in place
    if args.oriented:
        step.rot.copy_(torch.tensor([1.0, 0.0]).expand(args.hands, 2))
    if args.one_euro:
        step.reset_filter()
    if args.detect_every:
        step.reset_tracks()
        counts = torch.zeros(3, dtype=torch.int64, device=step.lost.device)      # seeded, suppressed, expired
        on_frame_0, given = torch.zeros(args.hands, dtype=torch.int32), 0
    if args.motion:
        step.reset_motion()
        speed = torch.zeros(2, dtype=torch.float64, device=step.lost.device)      # sum of the found slots' speeds, their number
        coasted = torch.zeros((), dtype=torch.int64, device=step.lost.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.synthetic):
        if args.detect_every:
            hands = [h for h in range(args.hands) if (t % args.detect_every == 0 and not (h == 0 and t in away)) or (h == 0 and t and t == away.stop)]
            dets = (torch.from_numpy(truth[t, hands]), on_frame_0[:len(hands)], torch.ones(len(hands))) if hands else None
            given += len(hands)
            step(detections=dets, **feed(t))
            emptied = (step.next_boxes == 0).all(1) & step.valid & (step.dup_of < 0) & (step.seeded < 0)
            counts += torch.stack([(step.seeded >= 0).sum(), (step.dup_of >= 0).sum(), emptied.sum()])
        else:
            step(**feed(t))
        lost += step.lost
        if args.overlay_out and t % args.overlay_every == 0:
            written.append(write_overlay_frame(args.overlay_out, t, surfaces[t] if args.surfaces else step.frames[0], args.frame_format, hs, ws,
                                               step.plan.frame_layout))
        if args.motion:
            found = step.lost == 0
            speed += torch.stack([(step.velocity.norm(dim=-1) * found).sum().double(), found.sum().double()])
            coasted += (step.coasted > 0).sum()
        if args.one_euro:
            moved += (step.smooth_preds - step.preds).norm(dim=-1).mean().double()
        step.advance()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    result = {"frames_per_s": round(args.synthetic / dt, 2), "frames": args.synthetic, "slots": args.synthetic * args.hands,
              "slots_lost": int(lost.sum()), "frame_size": [hs, ws], "hands": args.hands, "depth": args.depth,
              "precision": args.precision, "size": args.size, "track_min_score": score, "flip_test": args.flip_test, "dark_decode": args.dark_decode, "seed": args.seed}
    if args.oriented:
        result["oriented"] = True
    if args.mirror:
        result["mirror"] = mirror.tolist()
    if args.one_euro:
        result["one_euro"] = list(args.one_euro)
        result["smooth_mean_dist"] = float(moved) / args.synthetic
    if args.spin:
        result["spin"] = args.spin
    if args.antialias is not None:
        result["antialias"] = args.antialias
    if args.frame_format != "rgb":
        result.update(frame_format=args.frame_format, yuv_matrix=args.yuv_matrix, yuv_range=args.yuv_range, chroma_siting=args.chroma_siting)
    if args.surfaces:
        result["surfaces"] = True
    if args.detect_every:
        seeded, suppressed, expired = counts.tolist()
        result.update(detect_every=args.detect_every, max_lost=args.max_lost, detections=given, slots_seeded=seeded, slots_suppressed=suppressed,
                      slots_expired=expired)
    if args.motion:
        result.update(motion=dict(cutoff=args.motion_cutoff, lead=args.motion_lead, coast=args.coast),
                      mean_speed_px_s=float(speed[0] / speed[1].clamp(min=1)), slots_coasted=int(coasted))
    if args.smooth_gate:
        result["smooth_gate"] = step.smooth_gate
    if args.overlay_out:
        result.update(overlay_out=args.overlay_out, overlay_files=written, overlay_smooth=args.overlay_smooth)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
