#!/usr/bin/env python3
"""Training entry point with the reference's flag surface (src/tools/train.py + src/utils/argparser.py:27-100)
running the hot loop on the HIP engine.

Same flags / defaults as the reference (``--root --name --root_path --model --dataset --view --batch_size
--milestone --count --num_our --ratio_of_other --ratio_of_aug --epoch --lr`` and the booleans ``--scale --plt
--transfer --eval --test --logger --reset --rot --optim --color --D3``), same seeds (9001), Adam(lr) +
CosineAnnealingLR(T_max=epoch) stepped per epoch, best-validation-loss checkpoint
``<root_path>/<root>/<name>/checkpoint-good/state_dict.bin`` with the reference's dict keys, early stop on
``--count``.  New flags (they do not change existing semantics): ``--depth`` (ResNet depth, the reference
hard-codes 50), ``--hrnet_width``, ``--precision {fp32,bf16,fp16}``, ``--size``, ``--synthetic N`` (seeded
synthetic samples; the reference's datasets are not redistributable), ``--no_graph``, ``--transfer_from PATH`` (where
``--transfer`` reads its checkpoint; default: the reference's ``output/<model>/frei/ori/checkpoint-good/state_dict.bin``),
``--drop_last`` (skip the short last batch: the reference trains and validates on it, src/tools/train.py:27-38 builds both
loaders with the default ``drop_last=False``), ``--lr_resume_fix`` (on resume, continue the cosine schedule where the saved run
left it; the reference builds a FRESH ``CosineAnnealingLR`` behind ``optimizer.load_state_dict``, src/tools/train.py:50-58, and
that is the default here too), ``--loss_scale {auto,dynamic,<float>}`` (``auto``: the static default of ``TrainStep``, 1024 for
fp16 and none otherwise; ``dynamic``: torch.amp.GradScaler-style dynamic scaling on the device -- the checkpoint then also holds
``scaler_state_dict`` and a resume restores it, and the per-epoch line reports the scale and the skipped steps),
``--rot_factor DEG`` / ``--scale_factor F`` / ``--shift_factor F`` (online geometric augmentation of raw uint8 frames: per sample
and step a rotation ~ U[-DEG, DEG] degrees about the frame centre, a scale ~ U[1-F, 1+F] and a shift ~ U[-F, F] x the size,
warped on the device in the fused input kernel with a black border, the joints moved to match before the target is rendered;
the reference bakes one fixed +-20 degree rotation into a second copy of its dataset offline, src/tools/processing_aug.py.  All
default to 0 = off, the same step as without them; with float-tensor datasets a factor is an error.  The reference's boolean
``--rot`` is read nowhere there and stays a no-op here), ``--use_target_weight`` (the loss weights every joint plane by upstream's
``target_weight``: 0 for a joint that is invisible -- a third column of ``joint_2d`` -- or whose Gaussian patch left the map, e.g.
after the online warp; the reference computes this weight, src/tools/dataset.py:171-186, and never applies it) and ``--ohkm_topk K``
(online hard-keypoint mining, upstream's JointsOHKMMSELoss: per sample only the K joints with the largest loss count).  Both default
to off = the reference's objective; validation then scores the loss with the same criterion, PCK / EPE stay as they are.
``--synthetic_invisible F``: the fraction of synthetic joints marked invisible under ``--use_target_weight`` (default 0.1).
``--unbiased_target`` / ``--dark_decode`` (DARK, Zhang et al. 2020; both off by default): the target Gaussian is rendered around the
joint's real-valued position instead of the rounded cell (in the step and in the validation loss), and the validation keypoints
are decoded with the Taylor step on the log of the blurred map instead of the hard arg-max.
``--coord_loss_weight L`` / ``--soft_argmax_beta B`` / ``--soft_decode`` (integral regression, Sun et al. 2018; off by default): the
step adds L x the L1 distance between the soft-arg-max under softmax(B * heat-map) and the joint, in input pixels, to the heat-map
loss (every joint, whatever ``--ohkm_topk`` selects; weighted like the heat-map loss under ``--use_target_weight``); the validation
loss stays the heat-map loss, and ``--soft_decode`` decodes the validation keypoints with that soft-arg-max (not with ``--dark_decode``).
``--frame_size HSxWS`` (with ``--synthetic N``; off by default = the tool as it was): train on hand ROIs cropped from full frames on
the device (TrainStep(frames=...)): the samples are seeded HS x WS frames of one hand each, a constellation of 21 discs whose centres
are the joints in FRAME coordinates and whose bounds are the hand box (tools.synthetic_frames, the renderer of tools.track_frames).
``--roi_rot DEG`` / ``--roi_scale S`` / ``--roi_shift F`` / ``--roi_mirror P`` perturb the ROI per sample and step (TrainStep(roi_aug=):
the frame is sampled once, so the margin of a turned or shrunk crop is real context), ``--oriented``, ``--antialias [N]`` and
``--frame_format nv12 [--yuv_matrix --yuv_range --chroma_siting]`` are InferStep's crop options, so the model trains on the crop it is
deployed behind; validation crops the un-augmented ROI with the same options and scores loss / PCK / EPE in crop coordinates.
``--ratio_of_aug`` > 0 turns on ColorJitter(0.5 x 4) on the crops (TrainStep(crop_jitter=)) for the samples with
``idx < len(dataset) * ratio_of_aug``, as on raw uint8 images; validation never jitters.

Datasets (src/tools/train.py:24-38 builds them from files this repository cannot ship): ``main(args, train_set=,
val_set=)`` takes any ``torch.utils.data.Dataset`` whose samples are tuples starting with ``(image, joint_2d)`` --
the reference's ``CustomDataset`` yields ``(image, joint_2d, heatmap)`` and fits as it is; the heatmap is re-rendered on
the device from ``joint_2d``.  ``image`` is either a normalised float tensor ``[3, S, S]`` or a RAW uint8 frame
``[H, W, 3]``: raw frames go through the fused device pipeline (ToTensor, Resize(S), ColorJitter(0.5 x 4) on the
samples with ``idx < len(dataset) * ratio_of_aug`` -- the reference's rule, src/tools/dataset.py:133 -- Normalize).

What changes vs the reference loop (src/utils/method.py:160-183): the per-iteration ``loss.item()`` and
full-heatmap D2H + NumPy arg-max are replaced by device-resident loss / keypoints that are read once per
logging interval; everything else (BN momentum, loss, decode rule, optimizer) is the same arithmetic.

Multi-GPU: launch with ``python -m torch.distributed.run --nproc-per-node N -m lighthand_amd.tools.train ...``
(one process per GPU, gradients averaged by bucketed RCCL all-reduce; see lighthand_amd/parallel.py).
"""
import argparse
import os
import random
import time

import numpy as np
import torch


def parse_args(argv=None, phase="train"):
    p = argparse.ArgumentParser()
    p.add_argument("--root", default="simplebaseline/ours", type=str, help="You write down to store the directory path")
    p.add_argument("--name", default="84k", type=str, help="You write down to store the directory path")
    p.add_argument("--root_path", default="output", type=str, help="The root directory to save location which you want")
    known, _ = p.parse_known_args(argv)
    p.add_argument("--model", default="ours", type=str)
    p.add_argument("--dataset", default=known.root.split("/")[-1], type=str)
    p.add_argument("--view", default="wrist", type=str)
    p.add_argument("--batch_size", default=32, type=int)
    p.add_argument("--milestone", default=10, type=int)
    p.add_argument("--count", default=30, type=int)
    p.add_argument("--num_our", default=300000, type=int)
    p.add_argument("--ratio_of_other", default=0, type=float)
    p.add_argument("--ratio_of_aug", default=0.6, type=float)
    p.add_argument("--epoch", default=100, type=int)
    p.add_argument("--lr", default=0.001, type=float)
    for flag in ("scale", "plt", "transfer", "eval", "test", "logger", "reset", "rot", "optim", "color", "D3"):
        p.add_argument("--" + flag, action="store_true")
    # additions of this engine
    p.add_argument("--depth", default=50, type=int, choices=[18, 34, 50, 101, 152])
    p.add_argument("--hrnet_width", default=48, type=int)
    p.add_argument("--precision", default="bf16", choices=["fp32", "bf16", "fp16"])
    p.add_argument("--size", default=256, type=int)
    p.add_argument("--synthetic", default=0, type=int, help="train on N seeded synthetic samples")
    p.add_argument("--val_synthetic", default=0, type=int)
    p.add_argument("--no_graph", action="store_true")
    p.add_argument("--transfer_from", default=None, type=str, help="checkpoint --transfer loads (default: the reference's path)")
    p.add_argument("--drop_last", action="store_true", help="skip the short last batch of the training epoch (reference: trained on)")
    p.add_argument("--lr_resume_fix", action="store_true", help="resume the cosine schedule at the saved epoch (reference: fresh schedule)")
    p.add_argument("--loss_scale", default="auto", type=_loss_scale_arg,
                   help="auto (static: 1024 for fp16, none otherwise), dynamic (GradScaler-style, on the device) or a static factor")
    p.add_argument("--rot_factor", default=0.0, type=float, help="online rotation of raw uint8 frames: U[-DEG, DEG] degrees (0 = off)")
    p.add_argument("--scale_factor", default=0.0, type=float, help="online scale of raw uint8 frames: U[1-F, 1+F] (0 = off)")
    p.add_argument("--shift_factor", default=0.0, type=float, help="online shift of raw uint8 frames: U[-F, F] x the size (0 = off)")
    p.add_argument("--use_target_weight", action="store_true",
                   help="weight the loss by joint visibility (joint_2d column 2) x patch-inside-the-map (default: off, the reference's loss)")
    p.add_argument("--ohkm_topk", default=0, type=int, help="online hard-keypoint mining: the K hardest joints per sample (0 = off)")
    p.add_argument("--synthetic_invisible", default=0.1, type=float,
                   help="fraction of --synthetic joints marked invisible (read under --use_target_weight only)")
    p.add_argument("--unbiased_target", action="store_true",
                   help="DARK's target encoding: the Gaussian around the joint's real-valued position (default: the rounded cell)")
    p.add_argument("--dark_decode", action="store_true", help="decode the validation keypoints with DARK (default: hard arg-max)")
    p.add_argument("--coord_loss_weight", default=0.0, type=float,
                   help="integral regression: weight of the L1 loss on the soft-arg-max coordinates, input pixels (0 = off)")
    p.add_argument("--soft_argmax_beta", default=100.0, type=float, help="softmax temperature of the soft-arg-max (heat-map x beta)")
    p.add_argument("--soft_decode", action="store_true", help="decode the validation keypoints with the soft-arg-max (default: hard arg-max)")
    from lighthand_amd.tools.synthetic_frames import frame_size_arg
    p.add_argument("--frame_size", default=None, type=frame_size_arg, metavar="HSxWS",
                   help="train on hand ROIs cropped from synthetic HS x WS frames on the device (needs --synthetic; default: off)")
    p.add_argument("--roi_rot", default=0.0, type=float, help="ROI augmentation: rotation U[-DEG, DEG] degrees (needs --frame_size)")
    p.add_argument("--roi_scale", default=0.0, type=float, help="ROI augmentation: extents x U[1-S, 1+S] (needs --frame_size)")
    p.add_argument("--roi_shift", default=0.0, type=float, help="ROI augmentation: centre shift U[-F, F] x the extents (needs --frame_size)")
    p.add_argument("--roi_mirror", default=0.0, type=float, help="ROI augmentation: probability of mirroring the crop (needs --frame_size)")
    p.add_argument("--oriented", action="store_true", help="oriented ROI launch of the frame crop (needs --frame_size)")
    p.add_argument("--antialias", nargs="?", type=int, const=8, default=None, metavar="N",
                   help="area sampling of minified ROIs: at most N (1..8, default 8) samples per crop pixel and axis (needs --frame_size)")
    p.add_argument("--frame_format", default="rgb", choices=["rgb", "nv12", "nv21", "yuv420p", "p010"],
                   help="what the frame buffer holds: packed RGB or a 4:2:0 format under its decoder's name (needs --frame_size)")
    p.add_argument("--yuv_matrix", default="bt709", choices=["bt601", "bt709"], help="luma coefficients of NV12 frames")
    p.add_argument("--yuv_range", default="limited", choices=["limited", "full"], help="quantisation range of NV12 frames")
    p.add_argument("--chroma_siting", default="left", choices=["left", "center"], help="horizontal position of NV12's chroma samples")
    p.add_argument("--surfaces", action="store_true",
                   help="bind each batch's frames in place as surfaces instead of copying them into the step's buffer (needs --frame_size)")
    args = p.parse_args(argv)
    roi_flags = any((args.roi_rot, args.roi_scale, args.roi_shift, args.roi_mirror))
    if args.frame_size is None:
        if roi_flags or args.oriented or args.antialias is not None or args.frame_format != "rgb" or args.surfaces:
            p.error("--roi_rot / --roi_scale / --roi_shift / --roi_mirror / --oriented / --antialias / --frame_format / --surfaces need "
                    "--frame_size HSxWS")
    else:
        if not args.synthetic:
            p.error("--frame_size renders synthetic frames: pass --synthetic N")
        if any((args.rot_factor, args.scale_factor, args.shift_factor)):
            p.error("--rot_factor / --scale_factor / --shift_factor warp ready crops: with --frame_size use --roi_rot / --roi_scale / --roi_shift")
        if args.coord_loss_weight > 0 and not args.use_target_weight:
            p.error("--coord_loss_weight with --frame_size needs --use_target_weight")
        if args.antialias is not None and not 1 <= args.antialias <= 8:
            p.error("--antialias takes 1..8")
        if args.frame_format != "rgb" and (args.frame_size[0] % 2 or args.frame_size[1] % 2):
            p.error(f"--frame_format {args.frame_format} needs even frame sides")
        if min(args.roi_rot, args.roi_scale, args.roi_shift, args.roi_mirror) < 0 or args.roi_scale >= 1 or args.roi_mirror > 1:
            p.error("--roi_rot, --roi_shift >= 0, 0 <= --roi_scale < 1, 0 <= --roi_mirror <= 1")
    if args.frame_format == "rgb" and (args.yuv_matrix, args.yuv_range, args.chroma_siting) != ("bt709", "limited", "left"):
        p.error("--yuv_matrix / --yuv_range / --chroma_siting need --frame_format nv12")
    if args.soft_decode and args.dark_decode:
        p.error("--soft_decode and --dark_decode are two decodes: pass one")
    if not (args.coord_loss_weight >= 0 and np.isfinite(args.coord_loss_weight)):
        p.error("--coord_loss_weight must be a finite number >= 0")
    if not (args.soft_argmax_beta > 0 and np.isfinite(args.soft_argmax_beta)):
        p.error("--soft_argmax_beta must be a finite number > 0")
    args.phase = phase
    args.model = args.root.split("/")[0]                  # src/tools/dataset.py:59 overwrites it from the name
    args.name = os.path.join(args.root, args.name)
    args.output_dir = os.path.join(args.root_path, args.name)      # src/utils/pre_argparser.py:9
    args.logging_steps, args.num_workers, args.device = 100, 8, "cuda"
    if args.D3:
        raise SystemExit("--D3 (3-D joint regression) is outside the heatmap-regression path this engine covers")
    return args


def build_model(args):
    from lighthand_amd.modeling.hrnet.pose_hrnet import get_hrnet, hrnet_cfg
    from lighthand_amd.modeling.simplebaseline.config import default_config
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    if args.model == "hrnet":
        return get_hrnet(hrnet_cfg(args.hrnet_width), is_train=True)
    return get_pose_net(default_config(args.depth), is_train=True)


class SyntheticHands(torch.utils.data.Dataset):
    """Seeded stand-in for CustomDataset (src/tools/dataset.py:103-163): returns (image[3,S,S] ~ N(0,1) like
    a normalised crop, joint_2d[21,2] uniform in [20, S-20]).  Heatmaps are rendered on the device.  ``invisible=F`` appends a
    visibility column (joint_2d[21,3]): 0 for a seeded fraction F of the joints, 1 for the others."""

    def __init__(self, n, size, seed, invisible=None):
        rng = np.random.RandomState(seed)
        self.images = torch.from_numpy(rng.randn(n, 3, size, size).astype(np.float32))
        self.joints = torch.from_numpy(rng.uniform(20, size - 20, size=(n, 21, 2)).astype(np.float32))
        if invisible is not None:                    # drawn after the images and joints: those stay what they are without it
            vis = torch.from_numpy((rng.uniform(size=(n, 21, 1)) >= invisible).astype(np.float32))
            self.joints = torch.cat([self.joints, vis], 2)

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return self.images[i], self.joints[i]


class SyntheticFrames(torch.utils.data.Dataset):
    """Seeded full frames of one hand each (--frame_size): (frame uint8 [hs, ws, 3] -- or NV12 [rows, ws] with ``nv12=(matrix, range)``,
    or the bytes of ``frame_format`` "nv21" / "yuv420p" / "p010" in its tight layout with that pair --, joint_2d[21, 2] in FRAME
    coordinates, box[4] = the joints' bounds).  ``invisible``: as SyntheticHands'."""

    def __init__(self, n, frame_size, seed, invisible=None, nv12=None, frame_format="nv12"):
        from lighthand_amd.tools.synthetic_frames import synthetic_sequence
        from lighthand_amd.topdown import rgb_to_yuv420_host
        frames, _, joints = synthetic_sequence(n, frame_size[0], frame_size[1], 1, seed, return_joints=True)
        joints = joints[:, 0]
        self.frames = torch.from_numpy(rgb_to_yuv420_host(frames, frame_format, *nv12) if nv12 else frames)
        self.boxes = torch.from_numpy(np.concatenate([joints.min(1), joints.max(1)], 1).astype(np.float32))
        self.joints = torch.from_numpy(joints)
        if invisible is not None:
            rng = np.random.RandomState(seed + 77)
            self.joints = torch.cat([self.joints, torch.from_numpy((rng.uniform(size=(n, 21, 1)) >= invisible).astype(np.float32))], 2)

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return self.frames[i], self.joints[i], self.boxes[i]


def frame_options(args):
    """The crop options --frame_size's steps share (TrainStep and the validation InferStep), without ``frames=`` itself."""
    opt = dict(oriented=bool(args.oriented))
    if args.antialias is not None:
        opt["antialias"] = args.antialias
    if args.frame_format != "rgb":
        opt.update(frame_format=args.frame_format, yuv=(args.yuv_matrix, args.yuv_range), chroma_siting=args.chroma_siting)
    if getattr(args, "surfaces", False):
        opt["surfaces"] = True
    return opt


def _frames_feed(st, frames):
    """A batch of frames on the device as the step's input: copied into its buffer, or under --surfaces bound row by row where it lies."""
    return dict(surfaces=frames.reshape(frames.shape[0], -1)) if st.surfaces else dict(frames=frames)


def roi_aug(args):
    """(rotation, scale, shift, mirror_prob) for TrainStep(roi_aug=) from --roi_rot / --roi_scale / --roi_shift / --roi_mirror, None
    when all are 0."""
    factors = (args.roi_rot, args.roi_scale, args.roi_shift, args.roi_mirror)
    return factors if any(factors) else None


class _WithAugFlag(torch.utils.data.Dataset):
    """(image, joint_2d, ...) -> (image, joint_2d, jitter?) with the reference's rule for the colour augmentation: the
    FIXED subset idx < len(dataset) * ratio_of_aug is jittered (src/tools/dataset.py:133).  joint_2d keeps a third column
    (visibility, read by --use_target_weight) when the dataset has one."""

    def __init__(self, base, ratio_of_aug):
        # the reference compares the sample index with len(self.meta) * ratio_of_aug (dataset.py:133), and len(meta) can
        # differ from __len__ (= num_our): a dataset that carries `meta` supplies the limit the same way
        meta = getattr(base, "meta", None)
        self.base, self.limit = base, (len(meta) if meta is not None else len(base)) * ratio_of_aug

    def __len__(self):
        return len(self.base)

    def __getitem__(self, i):
        s = self.base[i]
        return s[0], torch.as_tensor(s[1], dtype=torch.float32)[:, :3], i < self.limit


class _FramesWithAugFlag(torch.utils.data.Dataset):
    """(frame, joint_2d, box) -> (frame, joint_2d, box, jitter?): _WithAugFlag's rule for the samples of --frame_size."""

    def __init__(self, base, ratio_of_aug):
        self.base, self.limit = base, len(base) * ratio_of_aug

    def __len__(self):
        return len(self.base)

    def __getitem__(self, i):
        return tuple(self.base[i]) + (i < self.limit,)


def _sample_kind(ds):
    """'u8' for raw uint8 HWC frames, 'f32' for normalised [3, S, S] float tensors; (H, W) of a raw frame."""
    img = torch.as_tensor(ds[0][0])
    if img.dtype == torch.uint8:
        if img.dim() != 3 or img.shape[2] != 3:
            raise SystemExit(f"raw frames must be uint8 [H, W, 3], got {tuple(img.shape)}")
        return "u8", (int(img.shape[0]), int(img.shape[1]))
    if img.dim() != 3 or img.shape[0] != 3:
        raise SystemExit(f"normalised images must be float [3, S, S], got {tuple(img.shape)}")
    return "f32", None


def geometric_aug(args, kind):
    """(rotation, scale, shift) for TrainStep(geometric_aug=) from --rot_factor / --scale_factor / --shift_factor, None when all are 0
    (--rot is not read: the reference declares it and never uses it).  The warp runs in the uint8 input kernel: with a float-tensor
    dataset ('f32') a factor is an error."""
    factors = (args.rot_factor, args.scale_factor, args.shift_factor)
    if not any(factors):
        return None
    if kind != "u8":
        raise SystemExit("--rot_factor / --scale_factor / --shift_factor warp raw uint8 frames on the device; this dataset yields "
                         "normalised float tensors -- pass uint8 [H, W, 3] frames or drop the factors")
    return factors


def _loss_scale_arg(v):
    if v in ("auto", "dynamic"):
        return v
    try:
        return float(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--loss_scale takes auto, dynamic or a number, not {v!r}")


def save_checkpoint(model, args, epoch, optimizer, best_loss, count, ment="good", scaler=None):
    """Same file name and dict keys as src/tools/dataset.py:340-367; only rank 0 writes.  With a dynamic loss scale (``scaler``,
    --loss_scale dynamic) one more key, ``scaler_state_dict`` (torch.amp.GradScaler's format)."""
    d = os.path.join(args.output_dir, "checkpoint-{}".format(ment))
    if int(os.environ.get("RANK", "0")) != 0:
        return d
    os.makedirs(d, exist_ok=True)
    sd = {"epoch": epoch, "optimizer_state_dict": optimizer.state_dict(), "best_loss": best_loss, "count": count,
          "model_state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()}}
    if scaler is not None:
        sd["scaler_state_dict"] = scaler.state_dict()
    torch.save(sd, os.path.join(d, "state_dict.bin"))
    return d


def load_scaler_state(scaler, args):
    """--loss_scale dynamic on a resume (the checkpoint logic of load_model_state): the saved scale and growth tracker, when the
    checkpoint holds them.  Returns True when a state was loaded."""
    ckpt = os.path.join(args.output_dir, "checkpoint-good", "state_dict.bin")
    if args.reset or not os.path.isfile(ckpt):
        return False
    state = torch.load(ckpt, map_location="cpu").get("scaler_state_dict")
    if state:
        scaler.load_state_dict(state)
    return bool(state)


def resume_checkpoint(model, path):
    """src/utils/dir.py:38-47: strict=False load, epoch + 1."""
    sd = torch.load(path, map_location="cpu")
    model.load_state_dict(sd["model_state_dict"], strict=False)
    return sd["best_loss"], sd["epoch"] + 1, sd["count"], sd.get("optimizer_state_dict")


def transfer_path(args):
    """Where --transfer reads its weights: src/utils/argparser.py:167-175 hard-codes output/<model>/frei/ori (relative to the
    working directory, NOT --root_path)."""
    return args.transfer_from or os.path.join(f"output/{args.model}/frei/ori", "checkpoint-good/state_dict.bin")


def load_model_state(model, args):
    """The checkpoint logic of load_model (src/utils/argparser.py:100-189) on an already built model: resume from
    <output_dir>/checkpoint-good/state_dict.bin unless --reset, THEN (--transfer) overwrite the weights with those of the transfer
    checkpoint, keeping the resumed epoch / best loss / count / optimizer state (the reference discards the transfer checkpoint's:
    `_, _, _model, _, _ = resume_checkpoint(...)`, :169).  A missing transfer checkpoint is an error, as in the reference (torch.load).
    Returns (best_loss, first epoch, count, optimizer_state | None)."""
    best_loss, epo, count, opt_state = np.inf, 0, 0, None
    ckpt = os.path.join(args.output_dir, "checkpoint-good", "state_dict.bin")
    if os.path.isfile(ckpt) and not args.reset:
        best_loss, epo, count, opt_state = resume_checkpoint(model, ckpt)
    if args.transfer:
        resume_checkpoint(model, transfer_path(args))
        if int(os.environ.get("RANK", "0")) == 0:
            print("Transfer_Loading ===> %s" % transfer_path(args))
    return best_loss, epo, count, opt_state


def make_scheduler(optimizer, args, epo, opt_state):
    """Optimizer state + learning-rate schedule at (re)start, src/tools/train.py:45-58: the saved optimizer state is loaded unless
    --optim, THEN a fresh CosineAnnealingLR(T_max=args.epoch) is built on the optimizer -- on a resume its param_groups carry the
    saved run's `lr` and `initial_lr`, so the schedule restarts its cosine from the saved learning rate (what the installed PyTorch
    does with such a group is the reference's behaviour, not restated here).  --lr_resume_fix instead fast-forwards a schedule that
    starts at args.lr by the epochs already run.  Call it AFTER the TrainStep exists (the fused Adam binds the arena there)."""
    if opt_state and not args.optim:
        optimizer.load_state_dict(opt_state)
    if getattr(args, "lr_resume_fix", False):
        for g in optimizer.param_groups:
            g["lr"] = args.lr
            g.pop("initial_lr", None)
        scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=args.epoch)
        for _ in range(epo):
            scheduler.step()
        return scheduler
    return torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=args.epoch)


def run_epochs(args, epo, train_loader, train_batch, validate_fn, save_fn, optimizer, scheduler, stopper, log=print, rank=0, world=1,
               scaler=None):
    """The epoch loop of src/tools/train.py:60-117 with the device work behind three callables: train_batch(it, batch) runs one
    iteration (any batch size: the short last batch included) and returns a callable that reads the running loss (called once per
    logging interval: the only device->host read of the loop), validate_fn() -> (val_loss, pck, epe), save_fn(epoch, best, count).
    Same order as the reference: train, validate, best / count bookkeeping, checkpoint on improvement, break on count == --count,
    THEN scheduler.step().  ``scaler``: a dynamic loss scale, whose scale and skipped steps the per-epoch line reports."""
    for epoch in range(epo, args.epoch):
        t0, seen = time.time(), 0
        for it, batch in enumerate(train_loader):
            read_loss = train_batch(it, batch)
            seen += len(batch[0])
            if it % args.logging_steps == 0 and rank == 0:
                log(f"epoch {epoch} iter {it}/{len(train_loader)} loss {float(read_loss()):.6f} "
                    f"{world * seen / (time.time() - t0 + 1e-9):.0f} img/s lr {optimizer.param_groups[0]['lr']:.2e}")
        val_loss, pck, epe = validate_fn()
        if rank == 0:
            amp = f" loss scale {scaler.scale:g} skipped {scaler.skipped_steps}" if scaler is not None else ""
            log(f"epoch {epoch} valid loss {val_loss:.6f} pck {pck:.2f}% epe {epe * 0.26:.2f} mm{amp}")     # method.py:131
        improved, stop = stopper.update(val_loss)     # val_loss is rank-invariant (reduce_validation): collective decision
        if improved:
            save_fn(epoch, stopper.best_loss, stopper.count)
        if stop:
            break
        scheduler.step()
    return stopper.best_loss


def validate(model, loader, args, u8_step=None, frames_step=None):
    """Runner.run validation branch (src/utils/method.py:218-287): loss, PCK@0.2 (bbox-normalised), EPE.
    ``u8_step``: an InferStep(input_u8=...) of the model for loaders that yield raw uint8 frames, or a callable
    batch size -> InferStep (the short last batch of the loader needs a step of its own shape).
    ``frames_step`` (--frame_size): a callable batch size -> InferStep(frames=(b, hs, ws), ...) for loaders that yield (frame, joint_2d
    in frame coordinates, box): the un-augmented ROI is cropped, and the joints are taken into the crop (lh_affine_points_inv) before
    loss, PCK and EPE are scored there."""
    from lighthand_amd.heatmap import JointsMSELoss, WeightedJointsMSELoss, max_preds_device, render_targets
    from lighthand_amd.metrics import device_pck_epe
    model.eval()
    # the loss the step trains with (--use_target_weight / --ohkm_topk), so the best-checkpoint decision follows the objective
    use_weight, topk = getattr(args, "use_target_weight", False), getattr(args, "ohkm_topk", 0)
    unbiased, decode = getattr(args, "unbiased_target", False), "dark" if getattr(args, "dark_decode", False) else False
    beta = getattr(args, "soft_argmax_beta", 100.0)
    if getattr(args, "soft_decode", False):
        decode = "soft"
    crit = WeightedJointsMSELoss(topk) if use_weight or topk else JointsMSELoss(False)
    acc = torch.zeros(5, device="cuda")          # loss*b, b, pck*b, epe sum, epe count -- reduced on the device
    with torch.no_grad():
        for batch in loader:
            images, joints3 = batch[0].cuda(non_blocking=True), batch[1][..., :3].float().cuda(non_blocking=True)
            joints = joints3[..., :2].contiguous()
            if frames_step is not None:
                from lighthand_amd.topdown import affine_points_inv
                st = frames_step(images.shape[0])
                st.refresh_weights()
                st(boxes=batch[2].cuda(non_blocking=True), **_frames_feed(st, images))
                pred = st.heatmaps
                joints = affine_points_inv(joints, st.plan.crop_mat, st.plan.src_frame)
                joints3 = torch.cat([joints, joints3[..., 2:]], 2)
            elif images.dtype == torch.uint8:
                st = u8_step(images.shape[0]) if callable(u8_step) and not hasattr(u8_step, "heatmaps") else u8_step
                st.refresh_weights()
                st(images)
                pred = st.heatmaps
            else:
                pred = model(images)
            hs = pred.shape[-1]
            if use_weight:
                target, weight = render_targets(joints3, size=hs, return_weight=True, unbiased=unbiased)
            else:
                target, weight = render_targets(joints, size=hs, unbiased=unbiased), None
            loss = crit(pred, target, weight)
            kp, _, _ = max_preds_device(pred, scale=float(args.size // hs), post_process=decode, soft_argmax_beta=beta)
            b = images.shape[0]
            pck, esum, ecnt = device_pck_epe(kp, joints, T=0.2)
            acc += torch.stack([loss * b, torch.tensor(float(b), device="cuda"), pck * b, esum, ecnt])
    model.train()
    return reduce_validation(acc)


def reduce_validation(acc):
    """acc = [loss*b, b, pck*b, epe sum, epe count] of THIS rank's validation shard.  Summed over the data-parallel
    ranks first, so every rank derives the same (loss, pck, epe) and therefore the same best-checkpoint / early-stop
    decision: a rank leaving the epoch loop alone would leave the others inside the next bucketed all-reduce."""
    from lighthand_amd import parallel
    a = parallel.all_reduce_sum_(acc).tolist()     # the only host read of the validation pass
    return a[0] / max(a[1], 1), 100.0 * a[2] / max(a[1], 1), a[3] / max(a[4], 1)


class EarlyStop:
    """best-loss / patience bookkeeping of the reference loop (src/tools/train.py:84-112)."""

    def __init__(self, best_loss, count, patience):
        self.best_loss, self.count, self.patience = best_loss, count, patience

    def update(self, val_loss):
        """Returns (improved, stop)."""
        if self.best_loss > val_loss:
            self.best_loss, self.count = val_loss, 0
            return True, False
        self.count += 1
        return False, self.count == self.patience


def main(args, train_set=None, val_set=None):
    """``train_set`` / ``val_set``: any Dataset of (image, joint_2d, ...) samples (module docstring); without them
    ``--synthetic N`` builds seeded synthetic ones.  Under torch.distributed every rank must be given ITS shard."""
    from lighthand_amd import parallel
    from lighthand_amd.amp import DynamicLossScale
    from lighthand_amd.optim import Adam
    from lighthand_amd.options import PlanOptions
    from lighthand_amd.runtime import InferStep, TrainStep

    # a geometric factor with float samples is refused before any device work (synthetic samples are float tensors)
    geo = geometric_aug(args, _sample_kind(train_set)[0] if train_set is not None else "f32")
    seed = 9001                                           # src/tools/train.py:15-22
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)
    rank, world, local = parallel.init_distributed()
    torch.cuda.set_device(local)
    # synthetic samples carry a visibility column only where it is read: their default shape stays [21, 2]
    invisible = args.synthetic_invisible if args.use_target_weight else None
    frame_size = getattr(args, "frame_size", None)
    if frame_size is not None:
        if train_set is not None or val_set is not None:
            raise SystemExit("--frame_size renders its own synthetic frames: it takes no train_set / val_set")
        nv12 = (args.yuv_matrix, args.yuv_range) if args.frame_format != "rgb" else None
        fmt = dict(frame_format=args.frame_format) if args.frame_format not in ("rgb", "nv12") else {}
        train_set = SyntheticFrames(args.synthetic, frame_size, seed + rank, invisible=invisible, nv12=nv12, **fmt)
        val_set = SyntheticFrames(args.val_synthetic or max(args.batch_size, max(args.synthetic, args.batch_size * 8) // 8), frame_size,
                                  seed + 1000, invisible=invisible, nv12=nv12, **fmt)
    if train_set is None:
        if not args.synthetic:
            raise SystemExit("the reference's datasets (LightHand99K / FreiHAND / ...) are not shipped: pass --synthetic N, or call "
                             "lighthand_amd.tools.train.main(args, train_set=, val_set=) with Datasets of (image, joint_2d) samples")
        train_set = SyntheticHands(args.synthetic, args.size, seed + rank, invisible=invisible)
    if val_set is None:
        val_set = SyntheticHands(args.val_synthetic or max(args.batch_size, max(args.synthetic, args.batch_size * 8) // 8), args.size, seed + 1000,
                                 invisible=invisible)
    if frame_size is not None:
        kind = val_kind = "frames"
        raw_hw = val_hw = None
        workers = 0
        train_set = _FramesWithAugFlag(train_set, args.ratio_of_aug)
    else:
        kind, raw_hw = _sample_kind(train_set)
        val_kind, val_hw = _sample_kind(val_set)
        train_set = _WithAugFlag(train_set, args.ratio_of_aug)
        workers = args.num_workers if not isinstance(train_set.base, SyntheticHands) else 0
    # persistent workers: a worker is forked from THIS process, which by the first epoch holds a HIP context and hundreds of
    # GB of mappings (~20 s per fork measured on the GPU box) -- fork them once per loader, not once per epoch
    # the reference builds both loaders with drop_last=False (src/tools/train.py:27-38): the short last batch is trained on and
    # validated on.  Data-parallel training keeps whole batches only (every rank must take part in every bucket's exchange, and the
    # reference has no multi-GPU loop to be faithful to); --drop_last asks for that on one GPU too.
    kw = dict(batch_size=args.batch_size, pin_memory=True, num_workers=workers, persistent_workers=workers > 0)
    train_loader = torch.utils.data.DataLoader(train_set, shuffle=True, drop_last=bool(args.drop_last or world > 1), **kw)
    val_loader = torch.utils.data.DataLoader(val_set, shuffle=False, drop_last=False, **kw)

    model = build_model(args).cuda().set_precision(args.precision)
    best_loss, epo, count, opt_state = load_model_state(model, args)
    optimizer = Adam(model.parameters(), lr=args.lr)
    # one dynamic loss scale for the full-size step and the short last batch's step
    scaler = DynamicLossScale() if args.loss_scale == "dynamic" else None
    if scaler is not None:
        load_scaler_state(scaler, args)
    loss_scale = scaler if scaler is not None else None if args.loss_scale == "auto" else args.loss_scale
    sync = parallel.GradSync(world) if world > 1 else None
    # raw uint8 frames: ToTensor / Resize / ColorJitter(0.5, 0.5, 0.5, 0.5) / Normalize fused on the device (dataset.py:128-159)
    jitter = (0.5, 0.5, 0.5, 0.5) if kind == "u8" and args.ratio_of_aug > 0 else None
    crop_jitter = (0.5, 0.5, 0.5, 0.5) if kind == "frames" and args.ratio_of_aug > 0 else None      # the same chain on the frame crops
    loss_kw = dict(use_target_weight=args.use_target_weight, ohkm_topk=args.ohkm_topk,
                   target_encoding="unbiased" if args.unbiased_target else "quantised",
                   coord_loss_weight=args.coord_loss_weight, soft_argmax_beta=args.soft_argmax_beta)

    def frame_kw(b):
        """--frame_size: one frame per slot (frame_index stays the plan's arange), the crop options and the two augmentations."""
        if frame_size is None:
            return {}
        return dict(frames=(b,) + tuple(frame_size), roi_aug=roi_aug(args), crop_jitter=crop_jitter, **frame_options(args))

    step = TrainStep(model, args.batch_size, args.size, args.size, optimizer=optimizer, use_graph=not args.no_graph, grad_sync=sync,
                     input_u8=raw_hw, color_jitter=jitter, loss_scale=loss_scale, geometric_aug=geo, **loss_kw, **frame_kw(args.batch_size))
    scheduler = make_scheduler(optimizer, args, epo, opt_state)       # src/tools/train.py:50-58, in the reference's order
    steps = {args.batch_size: step}

    def step_for(b):
        """The short last batch of an epoch runs on a step of its own shape (plans are per static shape): eager launches, the
        library's static kernel choice (one batch per epoch is not worth a measurement), the same optimizer -- moments and step
        count live in the optimizer, so full and short batches update one Adam state, as in the reference loop."""
        st = steps.get(b)
        if st is None:
            st = steps[b] = TrainStep(model, b, args.size, args.size, optimizer=optimizer, use_graph=False, grad_sync=sync,
                                      input_u8=raw_hw, color_jitter=jitter, loss_scale=loss_scale, geometric_aug=geo, **loss_kw, **frame_kw(b),
                                      plan_options=PlanOptions.from_env().replace(autotune=False))
        return st

    val_steps = {}

    def val_step_for(b):
        if b not in val_steps:
            if frame_size is not None:
                val_steps[b] = InferStep(model, b, args.size, args.size, frames=(b,) + tuple(frame_size), **frame_options(args))
            else:
                val_steps[b] = InferStep(model, b, args.size, args.size, input_u8=val_hw)
        return val_steps[b]

    def train_batch(it, batch):
        if frame_size is not None:                 # (frame, joints in frame coordinates, box, jitter?)
            images, joints, boxes, aug = batch
            st = step_for(images.shape[0])
            st(boxes=boxes.cuda(non_blocking=True), joints=joints.cuda(non_blocking=True), aug=aug if crop_jitter else None,
               **_frames_feed(st, images.cuda(non_blocking=True)))
            return lambda: st.loss
        images, joints, aug = batch
        st = step_for(images.shape[0])
        st(images.cuda(non_blocking=True), joints.cuda(non_blocking=True), aug=aug if jitter else None)
        return lambda: st.loss

    stopper = EarlyStop(best_loss, count, args.count)
    return run_epochs(args, epo, train_loader, train_batch,
                      lambda: validate(model, val_loader, args, val_step_for if val_kind == "u8" else None,
                                       frames_step=val_step_for if frame_size is not None else None),
                      lambda epoch, best, cnt: save_checkpoint(model, args, epoch, optimizer, best, cnt, "good", scaler=scaler),
                      optimizer, scheduler, stopper, rank=rank, world=world, scaler=scaler)


if __name__ == "__main__":
    main(parse_args())
