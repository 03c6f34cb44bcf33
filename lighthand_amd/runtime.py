"""hipGraph-captured training / inference steps: the fast path of the engine.

The reference's hot loop (src/utils/method.py:160-183) is, per iteration: H2D, forward,
JointsMSELoss, ``.item()``, full-heatmap D2H + NumPy arg-max, zero_grad, backward, Adam.
``TrainStep`` runs the same work as ONE replay of a captured HIP graph over static buffers:
weight packs -> forward -> Gaussian target render (from joints) -> MSE loss + dL/dheatmap ->
arg-max decode (kept on the device) -> backward -> [gradient all-reduce] -> fused Adam.
Loss and keypoints stay on the device; ``.loss`` / ``.preds`` are read only when the caller
asks (no per-iteration stream sync).
"""
import math
import numbers

import torch

from . import _lib, heatmap, topdown
from ._lib import LightHandError, check
from .amp import DynamicLossScale
from .optim import Adam


def sample_color_jitter(n, brightness=0.5, contrast=0.5, saturation=0.5, hue=0.5, mask=None, generator=None):
    """torchvision ColorJitter.get_params per image (host side): factor ~ U[max(0, 1 - v), 1 + v] for brightness /
    contrast / saturation, hue ~ U[-h, h], op order = randperm(4).  ``mask`` (bool [n], optional) selects the samples
    that are jittered at all; the others get order -1 (skip).  The reference jitters a FIXED subset of its dataset, the
    samples with idx < len(meta) * ratio_of_aug (src/tools/dataset.py:133): the loader computes that flag per sample
    (lighthand_amd.tools.train) and hands it in here -- it is not a per-batch random draw.
    Returns (factors fp32 [n][4], order int32 [n][4]) CPU tensors for Plan.jitter_factors / jitter_order."""
    g = generator
    u = torch.rand(n, 4, generator=g)
    lo = torch.tensor([max(0.0, 1 - brightness), max(0.0, 1 - contrast), max(0.0, 1 - saturation), -hue])
    hi = torch.tensor([1 + brightness, 1 + contrast, 1 + saturation, hue])
    factors = (lo + (hi - lo) * u).to(torch.float32)
    order = torch.stack([torch.randperm(4, generator=g) for _ in range(n)]).to(torch.int32)
    if mask is not None:
        order[~torch.as_tensor(mask, dtype=torch.bool).cpu()] = -1
    return factors, order


def sample_affine(n, rotation=0.0, scale=0.0, shift=0.0, prob=1.0, mask=None, generator=None, size=(256, 256)):
    """Per-image random affine warp (host side, seeded like ``sample_color_jitter``): rotation ~ U[-rotation, rotation] degrees
    about the frame centre ((w-1)/2, (h-1)/2) with cv2.getRotationMatrix2D's sign (the reference's offline augmentation,
    src/tools/processing_aug.py), isotropic scale ~ U[1-scale, 1+scale], shift ~ U[-shift*w, shift*w] x U[-shift*h, shift*h].
    Coordinates are output pixel indices of the h x w frame (``size``), the joints' convention.  A sample is drawn with
    probability ``prob`` and only where ``mask`` (bool [n], optional) is set; the others -- and every sample when all three
    factors are 0 -- get the exact identity.  The matrices are formed in float64 and rounded to fp32.
    Returns (inv, fwd) CPU fp32 tensors [n][6] = [a b c d e f] for Plan.warp_inv / warp_fwd: ``fwd`` maps a joint into the
    warped frame, ``inv`` maps an output pixel back to where it samples."""
    h, w = size
    u = torch.rand(n, 5, generator=generator, dtype=torch.float64)
    theta = torch.deg2rad((2 * u[:, 0] - 1) * rotation)
    s = 1 + (2 * u[:, 1] - 1) * scale
    tx, ty = (2 * u[:, 2] - 1) * shift * w, (2 * u[:, 3] - 1) * shift * h
    drawn = u[:, 4] < prob
    if mask is not None:
        drawn &= torch.as_tensor(mask, dtype=torch.bool).cpu()
    if not (rotation or scale or shift):
        drawn[:] = False
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    al, be = s * torch.cos(theta), s * torch.sin(theta)
    # forward: p' = s R (p - c) + c + t, R = [[cos, sin], [-sin, cos]]
    fwd = torch.stack([al, be, (1 - al) * cx - be * cy + tx, -be, al, be * cx + (1 - al) * cy + ty], 1)
    # inverse: A^-1 = [[al, -be], [be, al]] / s^2, translation -A^-1 t
    s2 = al * al + be * be
    ia, ib, ic, idd = al / s2, -be / s2, be / s2, al / s2
    inv = torch.stack([ia, ib, -(ia * fwd[:, 2] + ib * fwd[:, 5]), ic, idd, -(ic * fwd[:, 2] + idd * fwd[:, 5])], 1)
    eye = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float64)
    fwd[~drawn], inv[~drawn] = eye, eye
    return (inv + 0.0).to(torch.float32), (fwd + 0.0).to(torch.float32)          # + 0.0: no signed zeros


def _geometric_aug_spec(geometric_aug):
    """TrainStep(geometric_aug=): (rotation, scale, shift) or a dict of rotation / scale / shift / prob / generator."""
    keys = ("rotation", "scale", "shift", "prob", "generator")
    spec = dict(geometric_aug) if isinstance(geometric_aug, dict) else dict(zip(keys[:3], geometric_aug))
    unknown = set(spec) - set(keys)
    if unknown:
        raise LightHandError(f"geometric_aug: unknown keys {sorted(unknown)} (known: {', '.join(keys)})")
    out = {"rotation": 0.0, "scale": 0.0, "shift": 0.0, "prob": 1.0, "generator": None}
    out.update(spec)
    return out


def _ptr(t):
    return None if t is None else t.data_ptr()


def _is_number(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool) and math.isfinite(v)


def _check_beta(soft_argmax_beta):
    if not _is_number(soft_argmax_beta) or soft_argmax_beta <= 0:
        raise ValueError(f"soft_argmax_beta must be a finite number > 0, not {soft_argmax_beta!r}")


def _antialias_taps(antialias):
    """InferStep / InferPipeline(antialias=): False -> 1 (the plain crop), True -> 8, an integer 1..8 -> itself: the most samples per
    crop pixel and axis (lh_frames_crop_area_to_nhwc4's max_taps)."""
    if isinstance(antialias, bool):
        return 8 if antialias else 1
    if not isinstance(antialias, numbers.Integral) or not 1 <= antialias <= 8:
        raise ValueError(f"antialias must be False, True (= 8) or an integer 1..8, not {antialias!r}")
    return int(antialias)


_FRAME_DEFAULTS = dict(frame_format="rgb", yuv=("bt709", "limited"), chroma_siting="left", frame_layout=None)


def _is_frame_default(key, value):
    default = _FRAME_DEFAULTS[key]
    if default is None or isinstance(default, str):
        return value is None if default is None else value == default
    return isinstance(value, (tuple, list)) and tuple(value) == default


def _check_frames(frames, input_u8, box_padding, track, min_score, min_joints, min_side, antialias=False, frame_format="rgb",
                  yuv=("bt709", "limited"), chroma_siting="left", frame_layout=None, surfaces=False):
    """InferStep / InferPipeline(frames=, box_padding=, track*=, antialias=, frame_format=, yuv=, chroma_siting=, frame_layout=,
    surfaces=): refuse what cannot run, before any device work.  Returns the (n_frames, hs, ws) tuple of ints, or None."""
    taps = _antialias_taps(antialias)
    given = dict(frame_format=frame_format, yuv=yuv, chroma_siting=chroma_siting, frame_layout=frame_layout)
    topdown.check_frame_format(frame_format)
    topdown.csc12(yuv)
    topdown.chroma_siting_code(chroma_siting)
    if not isinstance(surfaces, bool):
        raise ValueError(f"surfaces must be False or True, not {surfaces!r}")
    if frames is None:
        if surfaces:
            raise ValueError("surfaces=True reads full frames in place: pass frames=(n_frames, hs, ws)")
        for key, value in given.items():
            if not _is_frame_default(key, value):
                raise ValueError(f"{key}={value!r} describes full frames: pass frames=(n_frames, hs, ws)")
        if antialias is not False:
            raise ValueError(f"antialias={antialias!r} samples hand ROIs on full frames ({taps} taps): pass frames=(n_frames, hs, ws)")
        if track:
            raise ValueError("track=True follows hand boxes on full frames: pass frames=(n_frames, hs, ws)")
        return None
    if input_u8:
        raise ValueError("frames= and input_u8= are two input paths: pass one of them")
    ok = isinstance(frames, (tuple, list)) and len(frames) == 3 and all(isinstance(v, numbers.Integral) and not isinstance(v, bool) and v > 0
                                                                        for v in frames)
    if not ok:
        raise ValueError(f"frames must be (n_frames, hs, ws), three positive integers, not {frames!r}")
    if not _is_number(box_padding) or box_padding <= 0:
        raise ValueError(f"box_padding must be a finite number > 0, not {box_padding!r}")
    if frame_format != "rgb":
        topdown.frame_layout_of(frame_format, int(frames[1]), int(frames[2]), frame_layout)
    else:
        for key in ("yuv", "chroma_siting", "frame_layout"):
            if not _is_frame_default(key, given[key]):
                raise ValueError(f"{key}={given[key]!r} describes NV12 frames: pass frame_format='nv12' (or 'nv21' / 'yuv420p' / 'p010')")
    if track:
        if not _is_number(min_score):
            raise ValueError(f"track_min_score must be a finite number, not {min_score!r}")
        if not isinstance(min_joints, numbers.Integral) or isinstance(min_joints, bool) or min_joints < 1:
            raise ValueError(f"track_min_joints must be an integer >= 1, not {min_joints!r}")
        if not _is_number(min_side) or min_side < 0:
            raise ValueError(f"track_min_side must be a finite number >= 0, not {min_side!r}")
    return tuple(int(v) for v in frames)


class _SurfaceBinding:
    """bind_surfaces / unbind_surfaces of a step built with ``frames=..., surfaces=True``: the step owns no frame buffer but
    ``plan.surface_table`` (int64 [n_frames] on the device), the addresses of the frames, which its crop launch reads at every
    replay -- so the surfaces change between replays of one captured graph with no recapture."""

    surfaces = False
    _surface_refs = None

    def _own_surfaces(self, n_frames):
        self.surfaces = True
        self._surface_refs = [None] * n_frames                     # a bound tensor lives until its entry is rebound or cleared

    def bind_surfaces(self, surfaces, start=0):
        """Frame ``start + i`` <- ``surfaces[i]``: a sequence of CUDA uint8 tensors, or one tensor [k][...] bound row by row.  Each is
        checked on the host (topdown.check_surface: on the step's device, uint8, contiguous, at least topdown.surface_bytes(layout)
        bytes, 2-byte aligned for 16-bit samples); any violation raises ValueError and writes nothing.  The addresses reach the table
        with one stream-ordered copy on the current stream.  A surface may be overwritten or freed only after that stream has passed
        the replay that reads it; the step holds a reference until the entry is rebound or cleared.  A tensor of more than one
        dimension is always k surfaces, one per row: ONE surface shaped [rows][pitch] goes in as ``[surface]`` (or flattened)."""
        if not self.surfaces:
            raise ValueError("surfaces are the input of a step built with frames=(n_frames, hs, ws), surfaces=True")
        table = self.plan.surface_table
        rows = torch.is_tensor(surfaces) and surfaces.dim() > 1
        seq = list(surfaces.unbind(0)) if rows else [surfaces] if torch.is_tensor(surfaces) else list(surfaces)
        if isinstance(start, bool) or not isinstance(start, numbers.Integral) or start < 0 or not seq or start + len(seq) > table.shape[0]:
            raise ValueError(f"bind_surfaces: {len(seq)} surfaces from frame {start!r} on do not fit the step's {table.shape[0]} frames"
                             + (f" (a tensor {tuple(surfaces.shape)} is bound row by row: pass one surface as [surface])" if rows else ""))
        try:
            addresses = [topdown.check_surface(t, table.device, self.plan.frame_layout) for t in seq]
        except ValueError as e:
            if rows:                                                # name the likely cause: one surface taken for k rows
                raise ValueError(f"{e} (a tensor {tuple(surfaces.shape)} is bound row by row, {len(seq)} surfaces of "
                                 f"{seq[0].numel()} bytes: pass one surface as [surface])") from None
            raise
        table[start:start + len(seq)].copy_(torch.tensor(addresses, dtype=torch.int64), non_blocking=True)      # from pageable memory
        self._surface_refs[start:start + len(seq)] = seq

    def unbind_surfaces(self, indices=None):
        """Zero the table entries of ``indices`` (None: all) and drop the references: such a frame is empty, its slots crop black."""
        if not self.surfaces:
            raise ValueError("surfaces are the input of a step built with frames=(n_frames, hs, ws), surfaces=True")
        table = self.plan.surface_table
        if indices is None:
            indices = range(table.shape[0])
        indices = [int(i) for i in indices]
        if any(i < 0 or i >= table.shape[0] for i in indices):
            raise ValueError(f"unbind_surfaces: indices within 0..{table.shape[0] - 1}, not {indices!r}")
        if indices:
            table[torch.tensor(indices, dtype=torch.int64).to(table.device)] = 0
        for i in indices:
            self._surface_refs[i] = None


def _check_roi(model, frames, oriented, track_axis, track_min_axis, smooth):
    """InferStep / InferPipeline(oriented=, track_axis=, track_min_axis=, smooth=): refuse what cannot run, before any device work.
    The joint count is the model's ``final_layer.out_channels`` (both model families end in that convolution); a model without one
    leaves the upper range of ``track_axis`` to lh_keypoints_to_rois' own argument check.  Returns smooth as (min_cutoff, beta,
    d_cutoff) floats, or None."""
    if oriented and frames is None:
        raise ValueError("oriented=True turns hand ROIs on full frames: pass frames=(n_frames, hs, ws)")
    if smooth is not None and frames is None:
        raise ValueError("smooth= filters keypoints in frame coordinates: pass frames=(n_frames, hs, ws)")
    if oriented:
        ok = isinstance(track_axis, (tuple, list)) and len(track_axis) == 2 and all(
            isinstance(v, numbers.Integral) and not isinstance(v, bool) and v >= 0 for v in track_axis) and track_axis[0] != track_axis[1]
        if not ok:
            raise ValueError(f"track_axis must be two different joint numbers (from, to), not {track_axis!r}")
        joints = getattr(getattr(model, "final_layer", None), "out_channels", None)
        if isinstance(joints, numbers.Integral) and max(track_axis) >= joints:
            raise ValueError(f"track_axis {tuple(track_axis)!r} names a joint the model does not have ({joints} joints)")
        if not _is_number(track_min_axis) or track_min_axis <= 0:
            raise ValueError(f"track_min_axis must be a finite number > 0, not {track_min_axis!r}")
    if smooth is None:
        return None
    if not isinstance(smooth, (tuple, list)) or len(smooth) not in (2, 3) or not all(_is_number(v) for v in smooth):
        raise ValueError(f"smooth must be (min_cutoff, beta) or (min_cutoff, beta, d_cutoff), finite numbers, not {smooth!r}")
    min_cutoff, beta, d_cutoff = (tuple(smooth) + (1.0,))[:3]
    if min_cutoff <= 0 or d_cutoff <= 0 or beta < 0:
        raise ValueError(f"smooth wants cut-offs > 0 and beta >= 0, not {smooth!r}")
    return float(min_cutoff), float(beta), float(d_cutoff)


def sample_roi_aug(n, rotation=0.0, scale=0.0, shift=0.0, mirror_prob=0.0, prob=1.0, mask=None, generator=None):
    """Per-slot random perturbation of a hand ROI (host side, seeded like ``sample_affine``), the rows of Plan.roi_aug that lh_roi_perturb
    reads: angle ~ U[-rotation, rotation] degrees (positive turns the crop's +x axis towards the frame's +y, topdown.rot_from_angle's
    sign), k ~ U[1-scale, 1+scale] on the ROI's extents, tx, ty ~ U[-shift, shift] as fractions of the ROI's extents along its own
    axes, flip ~ Bernoulli(mirror_prob).  A slot is drawn with probability ``prob`` and only where ``mask`` (bool [n], optional) is
    set; the others -- and every slot when all four factors are 0 -- get the exact identity row (1, 0, 1, 0, 0, 0), which the kernel
    copies bit for bit.  (c, s) = (cos, sin) are formed in float64 and rounded to fp32.
    Returns a CPU fp32 tensor [n][6] = (c, s, k, tx, ty, flip)."""
    u = torch.rand(n, 6, generator=generator, dtype=torch.float64)
    theta = torch.deg2rad((2 * u[:, 0] - 1) * rotation)
    k = 1 + (2 * u[:, 1] - 1) * scale
    tx, ty = (2 * u[:, 2] - 1) * shift, (2 * u[:, 3] - 1) * shift
    flip = (u[:, 4] < mirror_prob).to(torch.float64)
    drawn = u[:, 5] < prob
    if mask is not None:
        drawn &= torch.as_tensor(mask, dtype=torch.bool).cpu()
    if not (rotation or scale or shift or mirror_prob):
        drawn[:] = False
    rows = torch.stack([torch.cos(theta), torch.sin(theta), k, tx, ty, flip], 1)
    rows[~drawn] = torch.tensor(topdown.ROI_AUG_IDENTITY, dtype=torch.float64)
    return (rows + 0.0).to(torch.float32)          # + 0.0: no signed zeros


def _roi_aug_spec(roi_aug):
    """TrainStep(roi_aug=): (rotation_deg, scale, shift), (rotation_deg, scale, shift, mirror_prob), or a dict of rotation / scale /
    shift / mirror_prob / prob / generator."""
    keys = ("rotation", "scale", "shift", "mirror_prob", "prob", "generator")
    if isinstance(roi_aug, dict):
        spec = dict(roi_aug)
    elif isinstance(roi_aug, (tuple, list)) and len(roi_aug) in (3, 4):
        spec = dict(zip(keys[:4], roi_aug))
    else:
        raise ValueError(f"roi_aug must be (rotation_deg, scale, shift[, mirror_prob]) or a dict of {', '.join(keys)}, not {roi_aug!r}")
    unknown = set(spec) - set(keys)
    if unknown:
        raise ValueError(f"roi_aug: unknown keys {sorted(unknown)} (known: {', '.join(keys)})")
    out = {"rotation": 0.0, "scale": 0.0, "shift": 0.0, "mirror_prob": 0.0, "prob": 1.0, "generator": None}
    out.update(spec)
    for key in keys[:5]:
        if not _is_number(out[key]) or out[key] < 0:
            raise ValueError(f"roi_aug: {key} must be a finite number >= 0, not {out[key]!r}")
    if out["scale"] >= 1:
        raise ValueError(f"roi_aug: scale must stay below 1 (the extents are multiplied by 1 - scale .. 1 + scale), not {out['scale']!r}")
    if out["mirror_prob"] > 1 or out["prob"] > 1:
        raise ValueError(f"roi_aug: mirror_prob and prob are probabilities in 0..1, not {out['mirror_prob']!r} / {out['prob']!r}")
    return out


def _check_train_frames(model, frames, input_u8=None, geometric_aug=None, color_jitter=None, targets_from_joints=True, box_padding=1.25,
                        oriented=False, antialias=False, frame_format="rgb", yuv=("bt709", "limited"), chroma_siting="left",
                        frame_layout=None, roi_aug=None, coord_loss_weight=0.0, use_target_weight=False, crop_jitter=None, surfaces=False):
    """TrainStep(frames=, box_padding=, oriented=, antialias=, frame_format=, yuv=, chroma_siting=, frame_layout=, roi_aug=,
    crop_jitter=): refuse what cannot run, before any device work (no device is touched here).  The options shared with InferStep
    follow _check_frames' / _check_roi's rules.  Returns (frames as a tuple of ints or None, the roi_aug spec or None), and with the
    ``crop_jitter`` keyword a third value: the validated (brightness, contrast, saturation, hue) tuple of floats, or None."""
    checked = _check_frames(frames, input_u8, box_padding, False, 0.0, 1, 0.0, antialias, frame_format, yuv, chroma_siting, frame_layout,
                            surfaces)
    _check_roi(model, checked, oriented, (0, 1), 1.0, None)
    if checked is None:
        if roi_aug is not None:
            raise ValueError("roi_aug perturbs hand ROIs on full frames: pass frames=(n_frames, hs, ws)")
        if crop_jitter is not None:
            raise ValueError("crop_jitter jitters hand ROIs cropped from full frames: pass frames=(n_frames, hs, ws) (color_jitter= is "
                             "the uint8 input's)")
        return None, None
    if geometric_aug is not None:
        raise ValueError("frames= and geometric_aug= are two augmentations of two input paths: with frames pass roi_aug=, which samples "
                         "the frame itself")
    if color_jitter is not None:
        raise ValueError("frames= and color_jitter=: color_jitter runs in the uint8 input kernel; the frame crop's ColorJitter is "
                         "crop_jitter=(brightness, contrast, saturation, hue)")
    if not targets_from_joints:
        raise ValueError("frames= needs targets_from_joints=True: the target is rendered from the joints taken into the crop")
    if coord_loss_weight > 0 and not use_target_weight:
        raise ValueError("coord_loss_weight > 0 with frames= needs use_target_weight=True: the joints of an empty slot lie off the map "
                         "and must carry weight 0 in the coordinate term")
    spec = None if roi_aug is None else _roi_aug_spec(roi_aug)
    if crop_jitter is None:
        return checked, spec
    if (not isinstance(crop_jitter, (tuple, list)) or len(crop_jitter) != 4 or not all(_is_number(v) and v >= 0 for v in crop_jitter)
            or crop_jitter[3] > 0.5):
        raise ValueError(f"crop_jitter must be (brightness, contrast, saturation, hue), torchvision ColorJitter ranges: four finite "
                         f"numbers >= 0, hue <= 0.5, not {crop_jitter!r}")
    return checked, spec, tuple(float(v) for v in crop_jitter)


class TrainStep(_SurfaceBinding):
    def __init__(self, model, batch, height, width, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 optimizer=None, decode=True, use_graph=True, grad_sync=None, targets_from_joints=True,
                 input_u8=None, color_jitter=None, loss_scale=None, geometric_aug=None, plan_options=None,
                 use_target_weight=False, ohkm_topk=0, target_encoding="quantised", coord_loss_weight=0.0, soft_argmax_beta=100.0,
                 frames=None, box_padding=1.25, oriented=False, antialias=False, frame_format="rgb", yuv=("bt709", "limited"),
                 chroma_siting="left", frame_layout=None, roi_aug=None, crop_jitter=None, surfaces=False):
        """``coord_loss_weight`` = L > 0 (opt-in, integral regression; 0 = the step as it was: the same launches and buffers) adds
        L * mean |soft-arg-max(beta * heat-map) * 4 - joint| to the loss and its gradient to ``plan.dout_nchw`` (lh_integral_l1 right
        behind the MSE kernel, on the joints the target was rendered from, weighted by ``target_weight`` under ``use_target_weight``,
        with the step's loss scale).  The coordinate term covers EVERY joint whatever ``ohkm_topk`` says: mining selects planes of
        the MSE term only.  ``coord_loss`` holds the coordinate term alone, ``soft_preds`` the soft-arg-max keypoints and
        ``coord_joint_loss`` [B, J] the weighted L1 distance of every joint (lh_integral_l1's joint_loss); ``preds`` stays the arg-max.  Data parallel needs nothing new: the normaliser 2*b*j is a constant every rank shares.

        Training on hand ROIs cropped from full frames, opt-in (``frames=None``: the step as it was, the same launches and buffers):
        ``frames=(n_frames, hs, ws)`` makes the static inputs ``frames`` / ``boxes`` / ``frame_index`` (and ``rot`` / ``mirror`` under
        ``oriented`` or ``roi_aug``) with InferStep's meaning and launches -- ``box_padding``, ``oriented``, ``antialias``,
        ``frame_format`` / ``yuv`` / ``chroma_siting`` / ``frame_layout`` as there, so the crop a model is trained on is the crop it is
        deployed behind, bit for bit.  ``joints`` are FRAME coordinates (``step.joints`` keeps them): lh_affine_points_inv takes them
        through the inverse of ``plan.crop_mat`` into ``joints_crop``, which the target is rendered from (and lh_integral_l1 reads).
        ``preds`` stays in crop coordinates, ``frame_preds`` (with ``decode``) is ``preds`` through ``crop_mat``; ``valid`` is
        ``src_frame >= 0``.  An empty slot's joints lie at topdown.POINT_OFF: a zero target and, under ``use_target_weight``, weight 0.
        ``roi_aug=(rotation_deg, scale, shift[, mirror_prob])`` or a dict that may also carry prob / generator: every call draws one
        perturbation per slot (sample_roi_aug) into ``plan.roi_aug``; lh_roi_perturb moves, scales, turns and mirrors the caller's
        ROI in front of lh_roi_affine, so the crop samples the frame once and its margin is real context.  The caller's ``boxes`` /
        ``rot`` / ``mirror`` are never written.  A mirrored ROI needs no joint permutation (a hand has no left / right joint pairs).
        ``crop_jitter=(brightness, contrast, saturation, hue)``: torchvision ColorJitter ranges (the reference: 0.5 each), the frames'
        ``color_jitter``: every call draws factors and an op order per slot (sample_color_jitter, ``aug`` as on the uint8 path) into
        ``plan.jitter_factors`` / ``plan.jitter_order`` and lh_frames_crop_jitter_to_nhwc4 applies them to the crop between the sample
        and Normalize; contrast blends with the grey mean of the slot's own crop, black outside the frame included.  None: the
        launches and buffers without it.
        ``frame_format`` "nv21" / "yuv420p" / "p010" and ``surfaces=True`` (``bind_surfaces`` / ``unbind_surfaces`` /
        ``step(surfaces=seq, ...)``; ``step.frames`` is then None): as InferStep's, with every option above; the crop launch is
        lh_frames_crop_surfaces_to_nhwc4, under ``crop_jitter`` with its grey-mean launch in front."""
        if not _is_number(coord_loss_weight) or coord_loss_weight < 0:
            raise ValueError(f"coord_loss_weight must be a finite number >= 0, not {coord_loss_weight!r}")
        checked = _check_train_frames(model, frames, input_u8, geometric_aug, color_jitter, targets_from_joints, box_padding, oriented,
                                      antialias, frame_format, yuv, chroma_siting, frame_layout, roi_aug, coord_loss_weight,
                                      use_target_weight, crop_jitter, surfaces)
        frames, roi_aug = checked[:2]
        crop_jitter = checked[2] if crop_jitter is not None else None
        self.lib = _lib.load()
        _check_beta(soft_argmax_beta)
        if coord_loss_weight > 0 and not targets_from_joints:
            raise LightHandError("coord_loss_weight needs targets_from_joints=True: the coordinate loss reads the joints the target is rendered from")
        self.coord_loss_weight, self.soft_argmax_beta = float(coord_loss_weight), float(soft_argmax_beta)
        # target_encoding="unbiased" (opt-in, DARK): the target Gaussian is evaluated around the joint's real-valued heat-map
        # position (lh_gaussian_target_sub) instead of placed around the rounded cell; "quantised" = the step as it was
        if target_encoding not in ("quantised", "unbiased"):
            raise ValueError(f'target_encoding must be "quantised" or "unbiased", not {target_encoding!r}')
        if target_encoding == "unbiased" and not targets_from_joints:
            raise LightHandError('target_encoding="unbiased" needs targets_from_joints=True: the encoding is applied where the target is rendered')
        self.target_encoding = target_encoding
        # geometric_aug=(rotation, scale, shift) or a dict that may also carry prob / generator: a random affine warp of the
        # uint8 input per image and step (sample_affine), the joints moved to match (joints_aug) before the target render
        if geometric_aug is not None:
            if not input_u8:
                raise LightHandError("geometric_aug warps the uint8 input pipeline: it needs input_u8=(hs, ws)")
            if not targets_from_joints:
                raise LightHandError("geometric_aug needs targets_from_joints=True: the target is rendered from the warped joints")
            geometric_aug = _geometric_aug_spec(geometric_aug)
        self.model = model
        self._model_generation = getattr(model, "_lh_generation", 0)
        model.train()
        # uint8 input rewires the plan's image launch: such a step owns its plan (model(x) in train mode keeps the float one)
        owner = ("train", "frames") if frames else ("train", "u8") if input_u8 else None
        if grad_sync is not None:               # data parallel: one set of measured kernel choices for all ranks
            from . import parallel
            self.plan = parallel.plan_with_shared_tuning(
                lambda: model.plan(batch, height, width, training=True, backward=True, wgrad_bucket_bytes=grad_sync.bucket_bytes, owner=owner,
                                   options=plan_options))
        else:
            self.plan = model.plan(batch, height, width, training=True, backward=True, owner=owner, options=plan_options)
        self.arena = model.arena()
        dev = self.arena.device
        out = self.plan.out_nchw
        self.images = self.plan.img_nchw                               # static input: fp32 NCHW
        # input_u8=(hs, ws): feed raw uint8 HWC frames instead; ToTensor/Resize/Normalize run fused on the device
        # color_jitter=(brightness, contrast, saturation, hue): torchvision ColorJitter ranges (reference: 0.5 each,
        # src/tools/dataset.py:139-141) applied inside the fused input kernel; factors are drawn per batch on the host
        self.color_jitter = color_jitter
        self.geometric_aug = geometric_aug
        self.images_u8 = self.plan.use_uint8_input(*input_u8, jitter=color_jitter is not None,
                                                   warp=geometric_aug is not None) if input_u8 else None
        self.joints = torch.zeros(batch, out.shape[1], 2, dtype=torch.float32, device=dev)
        # the joints through this step's forward matrices: what the model is asked to predict (self.joints keeps the caller's)
        self.joints_aug = torch.zeros_like(self.joints) if geometric_aug is not None else None
        # frames=(n_frames, hs, ws): the input is hand ROIs on full frames (the docstring); joints_crop takes joints_aug's place
        self.frames = self.boxes = self.frame_index = self.rot = self.mirror = self.joints_crop = self.frame_preds = None
        self.roi_aug, self.oriented = roi_aug, False
        self.crop_jitter = crop_jitter
        self.antialias = _antialias_taps(antialias)
        self.frame_format = frame_format if frames else None
        if frames:
            self.images = None                                         # the inputs of such a step are frames / boxes / frame_index
            self.oriented = bool(oriented) or roi_aug is not None      # a turned ROI needs the oriented launch
            extra = dict(frame_format="nv12", yuv=yuv, chroma_siting=chroma_siting, frame_layout=frame_layout) if frame_format == "nv12" else {}
            if surfaces or frame_format not in ("rgb", "nv12"):
                extra = dict(frame_format=frame_format, frame_layout=frame_layout, surfaces=surfaces)
                if frame_format != "rgb":
                    extra.update(yuv=yuv, chroma_siting=chroma_siting)
                if surfaces:
                    self._own_surfaces(frames[0])
            self.frames = self.plan.use_frame_input(*frames, padding=float(box_padding), oriented=self.oriented, max_taps=self.antialias,
                                                    perturb=roi_aug is not None, **extra, **(dict(jitter=True) if crop_jitter else {}))
            self.boxes, self.frame_index = self.plan.boxes, self.plan.frame_index
            self.rot, self.mirror = self.plan.rot, self.plan.mirror
            self.joints_crop = torch.zeros_like(self.joints)
            if decode:
                self.frame_preds = torch.zeros_like(self.joints)
        self.target = torch.zeros_like(out)
        self.targets_from_joints = targets_from_joints
        # use_target_weight / ohkm_topk (opt-in extensions, off = the step as it was: the same launches and buffers): the loss is
        # lh_joints_mse in place of lh_mse_heatmap.  use_target_weight renders the target with lh_gaussian_target_w: a joint
        # that is invisible (column 2 of the caller's joints, kept in `vis`; ones when the caller passes two columns) or whose
        # patch left the map -- tested on the WARPED joints under geometric_aug -- gets weight 0 and a zero map, so it
        # contributes neither loss nor gradient.  ohkm_topk = K keeps, per sample, the K joints with the largest loss (weights
        # of 1 without use_target_weight).  Data parallel needs no new collective: the loss normaliser (b*j*hw, or b*K*hw
        # with mining) is a constant every rank shares, so averaging the ranks' gradients stays the gradient of the mean loss.
        self.use_target_weight, self.ohkm_topk = bool(use_target_weight), int(ohkm_topk)
        if self.use_target_weight and not targets_from_joints:
            raise LightHandError("use_target_weight needs targets_from_joints=True: the weight is computed where the target is rendered")
        if not 0 <= self.ohkm_topk <= out.shape[1]:
            raise LightHandError(f"ohkm_topk={ohkm_topk} must lie in 0..{out.shape[1]} (the joints of a sample)")
        self.vis = self.target_weight = self.joint_loss = self._jmse_ws = None
        if self.use_target_weight or self.ohkm_topk:
            self.vis = torch.ones(batch, out.shape[1], dtype=torch.float32, device=dev)
            self.target_weight = torch.ones(batch, out.shape[1], 1, dtype=torch.float32, device=dev)
            self.joint_loss = torch.zeros(batch, out.shape[1], dtype=torch.float32, device=dev)
            self._jmse_ws = torch.empty(self.lib.lh_joints_mse_workspace_bytes(batch, out.shape[1]), dtype=torch.uint8, device=dev)
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.preds = torch.zeros(batch, out.shape[1], 2, dtype=torch.float32, device=dev)
        self.maxvals = torch.zeros(batch, out.shape[1], 1, dtype=torch.float32, device=dev)
        self.decode = decode
        self.coord_loss = self.soft_preds = self.coord_joint_loss = self._integral_ws = None
        if self.coord_loss_weight > 0:
            self._integral_ws = torch.zeros(self.lib.lh_integral_l1_workspace_bytes(batch, out.shape[1]), dtype=torch.uint8, device=dev)
            self.coord_loss = self._integral_ws[:4].view(torch.float32)[0]       # the fold writes the coordinate term alone here
            self.soft_preds = torch.zeros(batch, out.shape[1], 2, dtype=torch.float32, device=dev)
            self.coord_joint_loss = torch.zeros(batch, out.shape[1], dtype=torch.float32, device=dev)
        self._mse_ws = torch.empty(self.lib.lh_mse_workspace_bytes(out.numel()), dtype=torch.uint8, device=dev)
        self._patch = heatmap._patch_on(dev)
        self.optimizer = optimizer or Adam(model.parameters(), lr=lr, betas=betas, eps=eps)
        self.optimizer.bind_arena(self.arena)
        self.grad_sync = grad_sync                                     # parallel.GradSync or None
        self.grad_scale = 1.0 if grad_sync is None else 1.0 / grad_sync.world_size
        # static loss scaling (fp16 plans: 1024 by default): the loss GRADIENT is multiplied by S where it is formed
        # (lh_mse_heatmap), every gradient of the backward pass carries S, Adam divides it out again -- the loss value, the
        # moments and the update are those of the unscaled step, but heat-map gradients of 1e-7 no longer flush to zero in
        # the 16-bit backward pass.  bf16 / fp32 need none (fp32's exponent range).
        # loss_scale="dynamic" or an amp.DynamicLossScale: torch.amp.GradScaler's dynamic scaling, decided on the device inside the
        # step (Adam.step(amp=...)): the update is skipped when a gradient is inf / NaN, the scale backs off / grows, and
        # lh_mse_heatmap reads the new scale at the next replay.  Data parallel: the check reads the ALL-REDUCED gradients -- an
        # inf / NaN of any rank survives the sum (and the bf16 bucket staging), so every rank takes the same decision and keeps the
        # same scale without a collective of its own.  Pass one instance to several steps (e.g. a short last batch) to share it.
        self.scaler = None
        if isinstance(loss_scale, str):
            if loss_scale != "dynamic":
                raise ValueError(f"loss_scale must be None, a number, 'dynamic' or a DynamicLossScale, not {loss_scale!r}")
            loss_scale = DynamicLossScale(device=dev)
        if isinstance(loss_scale, DynamicLossScale):
            self.scaler = loss_scale
            self.loss_scale = "dynamic"
            self._loss_scale_dev = self.scaler.scale_tensor
        else:
            if loss_scale is None:
                loss_scale = 1024.0 if self.plan.tdtype == torch.float16 else 1.0
            self.loss_scale = float(loss_scale)
            self._loss_scale_dev = torch.tensor([self.loss_scale], dtype=torch.float32, device=dev) if self.loss_scale != 1.0 else None
            self.grad_scale /= self.loss_scale
        self.graphs = None
        self.use_graph = use_graph
        self.heat_scale = float(height // out.shape[2])               # x4 of method.py:157
        self.steps = 0

    # ---- the work of one iteration, enqueued on the current stream --------------------------------
    def _render_target(self, stream):
        out = self.plan.out_nchw
        b, j, hs = self.joints.shape[0], self.joints.shape[1], out.shape[2]
        joints = self.joints
        if self.joints_aug is not None:
            check(self.lib.lh_affine_points(self.joints.data_ptr(), 2, self.plan.warp_fwd.data_ptr(), self.joints_aug.data_ptr(), 2, b, j,
                                            stream), "lh_affine_points")
            joints = self.joints_aug
        if self.joints_crop is not None:                               # frame -> crop through this step's matrix (behind the matrix launch)
            check(self.lib.lh_affine_points_inv(self.joints.data_ptr(), 2, self.plan.crop_mat.data_ptr(), self.plan.src_frame.data_ptr(),
                                                self.joints_crop.data_ptr(), 2, b, j, stream), "lh_affine_points_inv")
            joints = self.joints_crop
        if self.target_encoding == "unbiased":
            check(self.lib.lh_gaussian_target_sub(joints.data_ptr(), 2, _ptr(self.vis) if self.use_target_weight else None, 1, heatmap.RADIUS,
                                                  float(heatmap.SIGMA), self.target.data_ptr(),
                                                  self.target_weight.data_ptr() if self.use_target_weight else None, b, j, hs, stream),
                  "lh_gaussian_target_sub")
            return
        if self.use_target_weight:
            check(self.lib.lh_gaussian_target_w(joints.data_ptr(), 2, self.vis.data_ptr(), 1, self._patch.data_ptr(), heatmap.RADIUS,
                                                self.target.data_ptr(), self.target_weight.data_ptr(), b, j, hs, stream),
                  "lh_gaussian_target_w")
            return
        check(self.lib.lh_gaussian_target(joints.data_ptr(), 2, self._patch.data_ptr(), heatmap.RADIUS,
                                          self.target.data_ptr(), b, j, hs, stream), "lh_gaussian_target")

    def _fwd_loss(self, stream):
        # the target only depends on the joints: it is rendered on the weight-pack side stream, under the stem
        # (on frames the joints go through the crop matrix, which the forward list writes: the render follows it on the main stream)
        side = self._render_target if self.targets_from_joints and self.frame_format is None else None
        rendered = self.plan.refresh_packs(stream, overlap=True, side_work=side)
        self.plan.run_forward(stream)
        self._fwd_loss_tail(stream, target_done=rendered)

    def _fwd_loss_tail(self, stream, target_done=False):
        p, out = self.plan, self.plan.out_nchw
        if self.targets_from_joints and not target_done:
            self._render_target(stream)
        aux = None
        if self.decode and torch.cuda.current_stream().cuda_stream == stream:
            # the arg-max decode only reads the heat-maps: on a side stream under the loss kernels
            aux = self._aux_stream = getattr(self, "_aux_stream", None) or torch.cuda.Stream()
            aux.wait_event(torch.cuda.current_stream().record_event())
        if self._jmse_ws is not None:
            check(self.lib.lh_joints_mse(out.data_ptr(), self.target.data_ptr(), self.target_weight.data_ptr() if self.use_target_weight else None,
                                         out.shape[0], out.shape[1], out.shape[2] * out.shape[3], self.ohkm_topk, self.loss.data_ptr(),
                                         self.joint_loss.data_ptr(), p.dout_nchw.data_ptr(), _ptr(self._loss_scale_dev),
                                         self._jmse_ws.data_ptr(), stream), "lh_joints_mse")
        else:
            check(self.lib.lh_mse_heatmap(out.data_ptr(), self.target.data_ptr(), out.numel(), self.loss.data_ptr(),
                                          p.dout_nchw.data_ptr(), _ptr(self._loss_scale_dev), self._mse_ws.data_ptr(), stream), "lh_mse_heatmap")
        if self._integral_ws is not None:
            joints = self.joints_crop if self.joints_crop is not None else self.joints_aug if self.joints_aug is not None else self.joints
            check(self.lib.lh_integral_l1(out.data_ptr(), joints.data_ptr(), 2, self.target_weight.data_ptr() if self.use_target_weight else None,
                                          out.shape[0], out.shape[1], out.shape[2], out.shape[3], self.soft_argmax_beta, self.heat_scale,
                                          self.coord_loss_weight, self.soft_preds.data_ptr(), self.coord_joint_loss.data_ptr(),
                                          self.loss.data_ptr(), 1, p.dout_nchw.data_ptr(), 1, _ptr(self._loss_scale_dev),
                                          self._integral_ws.data_ptr(), stream), "lh_integral_l1")
        if self.decode:
            check(self.lib.lh_heatmap_argmax(out.data_ptr(), out.shape[0] * out.shape[1], out.shape[2], out.shape[3],
                                             self.heat_scale, self.preds.data_ptr(), self.maxvals.data_ptr(), None,
                                             aux.cuda_stream if aux is not None else stream), "lh_heatmap_argmax")
            if self.frame_preds is not None:
                check(self.lib.lh_affine_points(self.preds.data_ptr(), 2, p.crop_mat.data_ptr(), self.frame_preds.data_ptr(), 2, out.shape[0],
                                                out.shape[1], aux.cuda_stream if aux is not None else stream), "lh_affine_points")
            if aux is not None:
                torch.cuda.current_stream().wait_event(aux.record_event())

    def _enqueue_all(self):
        stream = torch.cuda.current_stream().cuda_stream
        self._fwd_loss(stream)
        self.plan.run_backward(stream)
        self._adam_step()

    def _capture(self):
        """One graph for the whole step; with gradient synchronisation through torch.distributed one graph per backward
        segment, so that each gradient bucket's all-reduce (an eager call on the side stream) starts as soon as its
        segment has been replayed; with the C-ABI communicator again one graph, collectives included."""
        warm = torch.cuda.Stream()
        warm.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(warm):          # warm-up outside capture (allocations, lazy state)
            self._enqueue_all() if self.grad_sync is None else self._eager_synced()
        torch.cuda.current_stream().wait_stream(warm)
        torch.cuda.synchronize()
        self.graphs = []
        if self.grad_sync is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._enqueue_all()
            self.graphs.append((g, None))
            return
        if getattr(self.grad_sync, "comm", None) is not None:
            # C-ABI communicator (lh_comm_*): the bucket all-reduces are stream-ordered RCCL launches that a hipGraph can
            # hold, so the whole data-parallel step -- backward segments, the all-reduces on the side stream, Adam -- is
            # ONE captured graph (no host work between segments)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._eager_synced()
            self.graphs.append((g, None))
            return
        segs = self.grad_sync.segments(self.plan)
        for i, (lo, hi, bucket) in enumerate(segs):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                stream = torch.cuda.current_stream().cuda_stream
                if i == 0:
                    self._fwd_loss(stream)
                self.plan.run_backward(stream, lo, hi)
            self.graphs.append((g, bucket))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._adam_step()
        self.graphs.append((g, "adam"))

    def _eager_synced(self):
        stream = torch.cuda.current_stream().cuda_stream
        self._fwd_loss(stream)
        for lo, hi, bucket in self.grad_sync.segments(self.plan):
            self.plan.run_backward(stream, lo, hi)
            if bucket is not None:
                self.grad_sync.launch(self.arena.flat_grad, bucket)
        self.grad_sync.wait_all()
        self._adam_step()

    def _adam_step(self):
        if self.scaler is None:
            self.optimizer.step(grad_scale=self.grad_scale)
        else:
            self.optimizer.step(grad_scale=self.grad_scale, amp=self.scaler)

    def _optimizer_snapshot(self):
        """Adam moments and device step counters as they are BEFORE the warm-up / capture iterations: a resumed run
        (optimizer.load_state_dict before the first step, src/tools/train.py:50) must keep them."""
        st = self.optimizer.state.get("flat")
        moments = {k: st[k].clone() for k in ("exp_avg", "exp_avg_sq")} if st and "exp_avg" in st else None
        steps = {gi: d["step"].clone() for gi, d in self.optimizer._dev.items()}
        return moments, steps, self.scaler._snapshot() if self.scaler is not None else None

    def _optimizer_restore(self, snap):
        """Undo the warm-up iteration on the optimizer side (weights / BN buffers are restored by ``__call__``), the dynamic loss
        scale's included: capture must not consume a growth tick or a backoff."""
        moments, steps, scaler = snap
        if scaler is not None:
            self.scaler._restore(scaler)
        st = self.optimizer.state.get("flat")
        if st and "exp_avg" in st:
            for k in ("exp_avg", "exp_avg_sq"):
                st[k].copy_(moments[k]) if moments is not None else st[k].zero_()
        for gi, d in self.optimizer._dev.items():
            d["step"].copy_(steps[gi]) if gi in steps else d["step"].zero_()

    def close(self):
        """Release what the step owns outside PyTorch (the C-ABI communicator of a data-parallel step)."""
        if self.grad_sync is not None:
            self.grad_sync.close()

    def sync_hyper(self):
        """Push lr / betas / eps changes (e.g. CosineAnnealingLR.step()) to the device-side Adam state."""
        for gi, group in enumerate(self.optimizer.param_groups):
            st = self.optimizer._dev.get(gi)
            if st is not None:
                self.optimizer._sync_hyper(st, group)

    @property
    def valid(self):
        """bool [batch]: the slots whose ROI and frame index were usable in the last run (None without ``frames``).  Under
        ``surfaces=True`` it does not say whether the frame's surface was bound: that is the caller's matter."""
        return None if self.frame_format is None else self.plan.src_frame >= 0

    def __call__(self, images=None, joints=None, target=None, aug=None, frames=None, boxes=None, frame_index=None, rot=None, mirror=None,
                 surfaces=None):
        """``joints``: [batch, J, >=2]; under ``use_target_weight`` a third column is the visibility (two columns = all visible).
        A step built with ``frames=`` takes ``frames`` / ``boxes`` / ``frame_index`` (and ``rot`` / ``mirror`` under ``oriented`` or
        ``roi_aug``) in place of ``images``, copied into the static buffers as InferStep does; its ``joints`` are frame coordinates.
        ``aug`` (bool [batch], optional; uint8 input with color_jitter, or frames with crop_jitter): which samples are jittered this step
        (the reference's fixed --ratio_of_aug subset, src/tools/dataset.py:133); None = all of them."""
        if getattr(self.model, "_lh_generation", 0) != self._model_generation:
            raise LightHandError("the model's parameter storages were re-created (.to() / .cuda() / .float()) after this TrainStep "
                                 "was built: its graph still trains the old buffers -- build a new TrainStep")
        if self.frame_format is None:
            if (frames is not None or boxes is not None or frame_index is not None or rot is not None or mirror is not None
                    or surfaces is not None):
                raise ValueError("frames / boxes / frame_index / rot / mirror are the inputs of TrainStep(frames=(n_frames, hs, ws))")
        elif images is not None or target is not None:
            raise ValueError("a step built with frames= takes frames / boxes / frame_index and joints, not images or target")
        elif (rot is not None or mirror is not None) and not self.oriented:
            raise ValueError("rot / mirror are the inputs of TrainStep(frames=..., oriented=True) or roi_aug=")
        if self.surfaces and frames is not None:
            raise ValueError("a step built with surfaces=True owns no frame buffer: pass surfaces= (or bind_surfaces), not frames=")
        if surfaces is not None:
            self.bind_surfaces(surfaces)                            # refuses a step built without surfaces=True
        if self.graphs is not None:
            self.sync_hyper()
        for dst, src in ((self.frames, frames), (self.boxes, boxes), (self.frame_index, frame_index), (self.rot, rot), (self.mirror, mirror)):
            if src is not None:
                dst.copy_(src, non_blocking=True)
        if self.roi_aug is not None:
            g = self.roi_aug                       # read by the replay from the plan's buffer, never baked into the graph
            self.plan.roi_aug.copy_(sample_roi_aug(self.joints.shape[0], g["rotation"], g["scale"], g["shift"], g["mirror_prob"],
                                                   prob=g["prob"], generator=g["generator"]), non_blocking=True)
        if self.crop_jitter is not None:
            f, o = sample_color_jitter(self.joints.shape[0], *self.crop_jitter, mask=aug)
            self.plan.jitter_factors.copy_(f, non_blocking=True)
            self.plan.jitter_order.copy_(o, non_blocking=True)
        if images is not None:
            (self.images_u8 if images.dtype == torch.uint8 and self.images_u8 is not None else self.images).copy_(images, non_blocking=True)
        if self.color_jitter is not None and self.images_u8 is not None:
            f, o = sample_color_jitter(self.joints.shape[0], *self.color_jitter, mask=aug)
            self.plan.jitter_factors.copy_(f, non_blocking=True)
            self.plan.jitter_order.copy_(o, non_blocking=True)
        if self.geometric_aug is not None:
            g = self.geometric_aug                 # read by the replay from the plan's buffers, never baked into the graph
            inv, fwd = sample_affine(self.joints.shape[0], g["rotation"], g["scale"], g["shift"], prob=g["prob"],
                                     generator=g["generator"], size=(self.plan.h, self.plan.w))
            self.plan.warp_inv.copy_(inv, non_blocking=True)
            self.plan.warp_fwd.copy_(fwd, non_blocking=True)
        if joints is not None:
            self.joints.copy_(joints[..., :2], non_blocking=True)
            if self.use_target_weight:             # column 2 = visibility; two columns = every joint visible
                self.vis.copy_(joints[..., 2], non_blocking=True) if joints.shape[-1] >= 3 else self.vis.fill_(1.0)
        if target is not None:
            self.target.copy_(target, non_blocking=True)
        if not self.use_graph:
            self._enqueue_all() if self.grad_sync is None else self._eager_synced()
        else:
            if self.graphs is None:
                snap = self.arena.flat.clone()
                bufs = {k: v.clone() for k, v in self.model.named_buffers()}
                opt_snap = self._optimizer_snapshot()
                self._capture()
                self._optimizer_restore(opt_snap)
                self.arena.flat.copy_(snap)                       # warm-up / capture must not train
                for k, v in self.model.named_buffers():
                    v.copy_(bufs[k])
            for g, bucket in self.graphs:
                if bucket == "adam":
                    self.grad_sync.wait_all()
                g.replay()
                if bucket is not None and bucket != "adam":
                    self.grad_sync.launch(self.arena.flat_grad, bucket)
        self.steps += 1
        return self.loss


class InferStep(_SurfaceBinding):
    """Eval-mode forward + arg-max decode as one captured graph (wearable_eval_2d / pred_store path,
    src/utils/argparser.py:246-281).  ``bn_train=True`` reproduces the reference quirk of running
    ``pred_store`` without ``model.eval()`` (batch statistics at evaluation time).

    The TEST block of the reference's configs, opt-in and inside the same graph:
    ``flip_test`` (TEST.FLIP_TEST) runs the forward a second time on the batch mirrored horizontally (lh_nhwc4_mirror in place
    of the image launch) and decodes the average of the plain heat-maps and the flipped-back mirrored ones
    (lh_heatmap_flip_merge); ``heatmaps`` is then that merged buffer.  Both passes run the plan of ``batch``, so with
    ``bn_train`` each pass normalises with its own batch statistics and updates the running ones, as two model() calls do.
    ``shift_heatmap`` (TEST.SHIFT_HEATMAP) shifts the flipped-back maps by one column before the average; it only applies to
    the flip test.  ``post_process`` (TEST.POST_PROCESS): ``True`` / ``"quarter"`` adds the quarter-pixel refinement
    (lh_heatmap_refine) to the decode, ``"dark"`` the DARK decode with a blur of ``blur_kernel`` taps (lh_heatmap_dark) in its
    place, ``"soft"`` overwrites ``preds`` with the soft-arg-max under softmax(``soft_argmax_beta`` * heat-map)
    (lh_heatmap_soft_argmax; ``maxvals`` stays the arg-max's); each reads the merged maps under the flip test.

    Top-down inference on full frames, opt-in (``frames=None``: the step as it was, the same launches and buffers):
    ``frames=(n_frames, hs, ws)`` makes the static inputs ``frames`` (uint8 [n_frames][hs][ws][3], shared by all slots), ``boxes``
    (fp32 [batch][4] = x0 y0 x1 y1 in frame pixel-index coordinates) and ``frame_index`` (int32 [batch]); the graph turns every box,
    padded by ``box_padding`` at the crop's aspect ratio, into a matrix (lh_box_affine), crops the frames through it
    (lh_frames_crop_to_nhwc4) and, after the decode -- flip-test merge and ``post_process`` included -- takes the keypoints back to
    the frame through the same matrix (lh_affine_points): ``preds`` are then FRAME coordinates, ``crop_preds`` keeps the crop's,
    ``valid`` is ``src_frame >= 0`` (a slot whose box is degenerate / not finite or whose frame index is out of range is empty:
    a black crop, preds (0, 0)).  ``track=True`` ends the graph with lh_keypoints_to_boxes: ``next_boxes`` = the bounds of the joints
    with maxval >= ``track_min_score``, at least ``track_min_side`` wide, and ``lost`` = 1 where fewer than ``track_min_joints``
    joints qualify (``next_boxes`` then repeats the box); ``advance()`` copies ``next_boxes`` into ``boxes`` on the device, so frame
    t+1 is replayed with no host arithmetic.  The graph never writes ``boxes``: the box behind ``preds`` stays readable.

    Oriented, mirrored ROIs and a temporal filter, opt-in on top of ``frames=`` (both off: the launches above, nothing else):
    ``oriented=True`` adds the static inputs ``rot`` (fp32 [batch][2], the frame direction of each crop's +x axis, any length,
    (1, 0) = upright; topdown.rot_from_angle) and ``mirror`` (int32 [batch], non-zero = a left hand: the crop's x axis is flipped),
    filled through ``rot=`` / ``mirror=``; a box is then the ROI's centre and its extents along the ROI's own axes, and lh_roi_affine
    writes the matrix in lh_box_affine's place.  The decode stays in crop coordinates and lh_affine_points maps back through the same
    matrix, mirror included, so ``flip_test`` and every ``post_process`` compose.  With ``track=True`` the graph ends with
    lh_keypoints_to_rois in lh_keypoints_to_boxes' place: ``next_rot`` turns the next crop so that joint ``track_axis[0]`` ->
    ``track_axis[1]`` (wrist -> middle-finger MCP) points up, when both are confident and at least ``track_min_axis`` frame pixels
    apart (otherwise the orientation is kept), ``next_boxes`` bounds the confident joints along that direction, and ``advance()``
    copies both.  ``mirror`` is the caller's: the graph never writes it.
    ``smooth=(min_cutoff, beta)`` or ``(min_cutoff, beta, d_cutoff=1.0)`` makes lh_one_euro the last launch: ``smooth_preds`` is the
    One-Euro filter of ``preds`` (frame pixels; ``beta`` multiplies a speed in frame pixels per second), ``preds`` stays raw and the next ROI is computed
    from the raw keypoints (a filtered ROI lags).  ``dt`` (fp32 [batch], seconds since the slot's previous frame, 1/30 until
    written; ``dt=`` takes a tensor or one number) is an input.  One call is one frame.  A slot that is empty, or lost under
    ``track=True``, passes its keypoints through and starts fresh when it is found again; ``reset_filter(slots=None)`` does the same
    by hand (a scene cut, a new hand in the slot).
    ``antialias=True`` (= 8) or an integer 1..8, on top of ``frames=``: the crop launch becomes lh_frames_crop_area_to_nhwc4, which
    averages up to that many samples per axis over each crop pixel's footprint wherever a ROI is minified (more than 1 + 1/64 frame
    pixels per crop pixel; topdown.crop_taps_host gives the counts, topdown.frames_crop_host the rule), so the network does not see
    texture that aliases with every sub-pixel move of the box.  A ROI that is not minified is cropped bit for bit as before, and
    ``False`` / 1 is the step as it was.  The matrix, the map-back and the flip test's mirror are untouched, so it composes with
    every option above; ``step.antialias`` keeps the number.
    ``frame_format="nv12"``, on top of ``frames=``: ``frames`` is what a video decoder or a camera stack hands over, uint8
    [n_frames][rows][pitch] -- hs rows of luma, then hs/2 rows of interleaved CbCr, on a row pitch that may be wider than ws
    (``frame_layout`` = topdown.nv12_layout(hs, ws, pitch, luma_rows); None: the tight layout, rows = hs*3/2, pitch = ws) -- and the
    crop launch becomes lh_frames_crop_yuv_to_nhwc4: every sample, the single one or each tap under ``antialias``, reads luma and
    bilinear chroma and is converted to RGB on the spot, so no pass over whole frames runs.  ``yuv=(standard, range)`` ("bt601" /
    "bt709", "limited" / "full"; or 12 coefficients: topdown.yuv_matrix) picks the conversion, ``chroma_siting`` "left" (H.264 / HEVC)
    or "center" (JPEG / MPEG-1) where the chroma samples sit.  hs and ws must be even.  topdown.frames_crop_nv12_host states the
    rule; the matrix and everything after the crop are untouched, so it composes with every option above.  ``step.frame_format``
    keeps the choice; "rgb" is the step as it was.
    ``frame_format`` "nv21" (Android camera stacks), "yuv420p" (software decoders: three planes) and "p010" (10-bit HEVC / AV1:
    16-bit little-endian samples, the 10 data bits on top): ``frames`` is uint8 [n_frames][frame_bytes] in ``frame_layout`` =
    topdown.yuv420_layout(frame_format, hs, ws, pitch, luma_rows, chroma_pitch) (None: tight), and the crop launch is
    lh_frames_crop_surfaces_to_nhwc4, which finds every sample through that plane descriptor and then follows the NV12 rule
    (topdown.frames_crop_yuv420_host); for p010 ``yuv=(standard, range)`` means topdown.yuv_matrix(standard, range, bits=10).
    ``surfaces=True``, on top of ``frames=`` and for every ``frame_format``: the step owns no frame buffer (``step.frames`` is None)
    but ``plan.surface_table``, the device addresses of the frames, which the crop launch reads at every replay: a decoder's
    surfaces are cropped where they lie, with no copy.  ``bind_surfaces(tensors, start=0)`` / ``unbind_surfaces(indices=None)`` fill
    and clear it, ``step(surfaces=seq, ...)`` binds and replays; the captured graph stays the same.  An unbound frame is empty: its
    slots crop exactly black (``valid`` keeps meaning ``src_frame >= 0``: whether a surface is bound is the caller's matter).  A
    surface may be overwritten or freed only after the step's stream has passed the replay that reads it."""

    _serial = 0

    def __init__(self, model, batch, height, width, bn_train=False, use_graph=True, input_u8=None, slot=0,
                 flip_test=False, shift_heatmap=True, post_process=False, plan_options=None, blur_kernel=11, soft_argmax_beta=100.0,
                 frames=None, box_padding=1.25, track=False, track_min_score=0.1, track_min_joints=8, track_min_side=16.0,
                 oriented=False, track_axis=(0, 9), track_min_axis=4.0, smooth=None, antialias=False, frame_format="rgb",
                 yuv=("bt709", "limited"), chroma_siting="left", frame_layout=None, surfaces=False):
        if not shift_heatmap and not flip_test:
            raise ValueError("shift_heatmap=False applies to the flip test: pass flip_test=True")
        frames = _check_frames(frames, input_u8, box_padding, track, track_min_score, track_min_joints, track_min_side, antialias,
                               frame_format, yuv, chroma_siting, frame_layout, surfaces)
        self.antialias = _antialias_taps(antialias)                 # samples per crop pixel and axis at most; 1 = the plain crop
        self.frame_format = frame_format if frames else None        # what the frames hold; None: the step takes no frames
        smooth = _check_roi(model, frames, oriented, track_axis, track_min_axis, smooth)
        post_process = heatmap.decode_mode(post_process)
        _check_beta(soft_argmax_beta)
        self.soft_argmax_beta = float(soft_argmax_beta)
        self.lib = _lib.load()
        # a plan of its own (never the one model(x) runs): use_uint8_input rewires the plan's image launch, and a pipeline
        # slot replays asynchronously on its own stream -- neither may happen to the plan model.forward() uses
        InferStep._serial += 1
        self.plan = model.plan(batch, height, width, training=bn_train, backward=False, slot=slot,
                               owner=("infer", "frames" if frames else "u8" if input_u8 else "f32", InferStep._serial), options=plan_options)
        out = self.plan.out_nchw
        dev = out.device
        # input_u8=(hs, ws): raw uint8 HWC frames; ToTensor / Resize / Normalize run fused on the device (dataset.py:128-159)
        self.images = self.plan.use_uint8_input(*input_u8) if input_u8 else self.plan.img_nchw
        self.frames = self.boxes = self.frame_index = self.crop_preds = self.next_boxes = self.lost = None
        self.track = bool(track) and frames is not None
        self.track_min_score, self.track_min_joints, self.track_min_side = float(track_min_score), int(track_min_joints), float(track_min_side)
        self.oriented, self.smooth = bool(oriented) and frames is not None, smooth
        self.rot = self.mirror = self.next_rot = self.dt = self.smooth_preds = None
        if self.oriented:
            self.track_axis, self.track_min_axis = (int(track_axis[0]), int(track_axis[1])), float(track_min_axis)
        if frames:
            self.images = None                                      # the inputs of such a step are frames / boxes / frame_index
            if surfaces or frame_format not in ("rgb", "nv12"):
                extra = dict(frame_format=frame_format, frame_layout=frame_layout, surfaces=surfaces)
                if frame_format != "rgb":
                    extra.update(yuv=yuv, chroma_siting=chroma_siting)
                self.frames = self.plan.use_frame_input(*frames, padding=float(box_padding), oriented=self.oriented, max_taps=self.antialias,
                                                        **extra)
                if surfaces:
                    self._own_surfaces(frames[0])
            elif frame_format == "nv12":                            # the RGB step calls use_frame_input as it always did
                self.frames = self.plan.use_frame_input(*frames, padding=float(box_padding), oriented=self.oriented, max_taps=self.antialias,
                                                        frame_format="nv12", yuv=yuv, chroma_siting=chroma_siting, frame_layout=frame_layout)
            else:
                self.frames = self.plan.use_frame_input(*frames, padding=float(box_padding), oriented=self.oriented, max_taps=self.antialias)
            self.boxes, self.frame_index = self.plan.boxes, self.plan.frame_index
            self.rot, self.mirror = self.plan.rot, self.plan.mirror
            self.crop_preds = torch.zeros(batch, out.shape[1], 2, dtype=torch.float32, device=dev)
            if self.track:
                self.next_boxes = self.boxes.clone()
                self.lost = torch.ones(batch, dtype=torch.int32, device=dev)
                if self.oriented:
                    self.next_rot = self.rot.clone()
            if smooth:
                self.dt = torch.full((batch,), 1.0 / 30.0, dtype=torch.float32, device=dev)
                self.smooth_preds = torch.zeros(batch, out.shape[1], 2, dtype=torch.float32, device=dev)
                # the filter's state: the last filtered keypoints, their filtered derivative, and whether the slot has seen a frame
                self._xhat, self._dxhat = torch.zeros_like(self.smooth_preds), torch.zeros_like(self.smooth_preds)
                self._seen = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.flip_test, self.shift_heatmap, self.post_process, self.blur_kernel = flip_test, shift_heatmap, post_process, int(blur_kernel)
        # flip test: the plain pass's maps are copied here, and the merge writes over them in place
        self.heatmaps = torch.zeros_like(out) if flip_test else out
        self.preds = torch.zeros(batch, out.shape[1], 2, dtype=torch.float32, device=dev)
        self.maxvals = torch.zeros(batch, out.shape[1], 1, dtype=torch.float32, device=dev)
        self.idx = torch.zeros(batch, out.shape[1], dtype=torch.int32, device=dev) if post_process in ("quarter", "dark") else None
        self.scale = float(height // out.shape[2])
        self.use_graph = use_graph
        self.graph = None
        self._packed = False

    def _enqueue(self):
        s = torch.cuda.current_stream().cuda_stream
        self.plan.run_forward(s)
        out, hm = self.plan.out_nchw, self.heatmaps
        bj, h, w = out.shape[0] * out.shape[1], out.shape[2], out.shape[3]
        preds = self.preds if self.frame_format is None else self.crop_preds      # the decode works in crop coordinates
        if self.flip_test:
            hm.copy_(out)
            self.plan.run_forward(s, mirrored=True)
            check(self.lib.lh_heatmap_flip_merge(hm.data_ptr(), out.data_ptr(), bj, h, w, int(self.shift_heatmap), self.scale,
                                                 hm.data_ptr(), preds.data_ptr(), self.maxvals.data_ptr(), _ptr(self.idx), s),
                  "lh_heatmap_flip_merge")
        else:
            check(self.lib.lh_heatmap_argmax(hm.data_ptr(), bj, h, w, self.scale, preds.data_ptr(), self.maxvals.data_ptr(),
                                             _ptr(self.idx), s), "lh_heatmap_argmax")
        if self.post_process == "quarter":
            check(self.lib.lh_heatmap_refine(hm.data_ptr(), self.idx.data_ptr(), self.maxvals.data_ptr(), bj, h, w, self.scale,
                                             preds.data_ptr(), s), "lh_heatmap_refine")
        elif self.post_process == "dark":
            check(self.lib.lh_heatmap_dark(hm.data_ptr(), self.idx.data_ptr(), self.maxvals.data_ptr(), bj, h, w, self.blur_kernel,
                                           self.scale, preds.data_ptr(), s), "lh_heatmap_dark")
        elif self.post_process == "soft":
            check(self.lib.lh_heatmap_soft_argmax(hm.data_ptr(), bj, h, w, self.soft_argmax_beta, self.scale, preds.data_ptr(), s),
                  "lh_heatmap_soft_argmax")
        if self.frame_format is not None:
            p = self.plan
            check(self.lib.lh_affine_points(preds.data_ptr(), 2, p.crop_mat.data_ptr(), self.preds.data_ptr(), 2, out.shape[0], out.shape[1], s),
                  "lh_affine_points")
            if self.track and self.oriented:
                check(self.lib.lh_keypoints_to_rois(self.preds.data_ptr(), self.maxvals.data_ptr(), self.boxes.data_ptr(), self.rot.data_ptr(),
                                                    p.src_frame.data_ptr(), out.shape[0], out.shape[1], self.track_axis[0], self.track_axis[1],
                                                    self.track_min_score, self.track_min_joints, self.track_min_side, self.track_min_axis,
                                                    self.next_boxes.data_ptr(), self.next_rot.data_ptr(), self.lost.data_ptr(), s),
                      "lh_keypoints_to_rois")
            elif self.track:
                check(self.lib.lh_keypoints_to_boxes(self.preds.data_ptr(), self.maxvals.data_ptr(), self.boxes.data_ptr(), p.src_frame.data_ptr(),
                                                     out.shape[0], out.shape[1], self.track_min_score, self.track_min_joints,
                                                     self.track_min_side, self.next_boxes.data_ptr(), self.lost.data_ptr(), s),
                      "lh_keypoints_to_boxes")
            if self.smooth:
                check(self.lib.lh_one_euro(self.preds.data_ptr(), p.src_frame.data_ptr(), _ptr(self.lost), self.dt.data_ptr(), out.shape[0],
                                           out.shape[1], self.smooth[0], self.smooth[1], self.smooth[2], self._xhat.data_ptr(),
                                           self._dxhat.data_ptr(), self._seen.data_ptr(), self.smooth_preds.data_ptr(), s), "lh_one_euro")

    @property
    def valid(self):
        """bool [batch]: the slots whose box and frame index were usable in the last run (None without ``frames``).  Under
        ``surfaces=True`` it does not say whether the frame's surface was bound: that is the caller's matter."""
        return None if self.frame_format is None else self.plan.src_frame >= 0

    def advance(self):
        """boxes <- next_boxes (and rot <- next_rot with ``oriented=True``), on the device (``track=True``): the next call crops where
        this one found the hand.  On a step built without
        ``track`` it raises LightHandError (a call the step cannot serve, as a stale ticket of InferPipeline.result; the ValueErrors
        are for bad argument values)."""
        if not self.track:
            raise LightHandError("advance() needs InferStep(frames=..., track=True)")
        self.boxes.copy_(self.next_boxes, non_blocking=True)
        if self.oriented:
            self.rot.copy_(self.next_rot, non_blocking=True)

    def reset_filter(self, slots=None):
        """Forget the One-Euro filter's state of ``slots`` (indices or a mask; None: all), on the device: their next frame passes
        through unfiltered and starts the filter again.  LightHandError on a step built without ``smooth=``, as advance()'s."""
        if not self.smooth:
            raise LightHandError("reset_filter() needs InferStep(frames=..., smooth=(min_cutoff, beta))")
        if slots is None:
            self._seen.zero_()
        else:
            self._seen[torch.as_tensor(slots, device=self._seen.device)] = 0

    def refresh_weights(self):
        self.plan.refresh_packs(torch.cuda.current_stream().cuda_stream)
        self._packed = True

    def __call__(self, images=None, frames=None, boxes=None, frame_index=None, rot=None, mirror=None, dt=None, surfaces=None):
        if self.frame_format is None:
            if frames is not None or boxes is not None or frame_index is not None or surfaces is not None:
                raise ValueError("frames / boxes / frame_index are the inputs of InferStep(frames=(n_frames, hs, ws))")
        elif images is not None:
            raise ValueError("a step built with frames= takes frames / boxes / frame_index, not images")
        if self.surfaces and frames is not None:
            raise ValueError("a step built with surfaces=True owns no frame buffer: pass surfaces= (or bind_surfaces), not frames=")
        if surfaces is not None:
            self.bind_surfaces(surfaces)                            # refuses a step built without surfaces=True
        if (rot is not None or mirror is not None) and not self.oriented:
            raise ValueError("rot / mirror are the inputs of InferStep(frames=..., oriented=True)")
        if dt is not None and not self.smooth:
            raise ValueError("dt is the input of InferStep(frames=..., smooth=(min_cutoff, beta))")
        if images is not None:
            self.images.copy_(images, non_blocking=True)
        for dst, src in ((self.frames, frames), (self.boxes, boxes), (self.frame_index, frame_index), (self.rot, rot), (self.mirror, mirror)):
            if src is not None:
                dst.copy_(src, non_blocking=True)
        if dt is not None:
            self.dt.copy_(dt, non_blocking=True) if torch.is_tensor(dt) else self.dt.fill_(float(dt))
        if not self._packed:
            self.refresh_weights()
        if not self.use_graph:
            self._enqueue()
            return self.preds
        if self.graph is None:
            warm = torch.cuda.Stream()
            warm.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(warm):
                self._enqueue()
            torch.cuda.current_stream().wait_stream(warm)
            torch.cuda.synchronize()
            if self.smooth:
                self._seen.zero_()                                  # the warm-up run is not a frame: the first replay starts the filter
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._enqueue()
        self.graph.replay()
        return self.preds


class InferPipeline:
    """``depth`` batches in flight: one InferStep (own activation buffers, weight packs and captured graph) per slot, each on
    a stream of its own.  The stage 3-4 launches of one batch are latency-bound chains of one wave of tiles; a second batch
    fills the machine under them: R50 256x256 bs 64 bf16, 29.9 k img/s with one batch in flight, 33.3 k with two (MI355X).
    Eval-mode only (the batch-statistics quirk of ``pred_store`` updates the running statistics, which slots would race on).
    ``flip_test`` / ``shift_heatmap`` / ``post_process`` / ``blur_kernel`` / ``soft_argmax_beta``: as InferStep's, for every slot.
    ``frames`` / ``box_padding`` / ``track`` / ``track_min_*``: as InferStep's; every slot owns its frame buffer and boxes, and
    ``submit(frames=, boxes=, frame_index=)`` fills them (``steps[i]`` gives a slot's ``valid`` / ``next_boxes`` / ``lost``).
    ``oriented`` / ``track_axis`` / ``track_min_axis`` / ``smooth``: as InferStep's; every slot owns its ROIs and its filter state
    (one slot is one video stream: ``submit(rot=, mirror=, dt=)``, ``steps[i].smooth_preds`` / ``next_rot`` / ``reset_filter()``).
    ``antialias``: as InferStep's, for every slot.
    ``frame_format`` / ``yuv`` / ``chroma_siting`` / ``frame_layout``: as InferStep's; every slot owns its NV12 buffer.
    ``surfaces``: as InferStep's; every slot owns its surface table, and ``submit(surfaces=seq, ...)`` binds on the slot that runs
    the ticket (the slot keeps the references until it is bound again, ``depth`` submits later).

        pipe = InferPipeline(model, 64, 256, 256, depth=2)
        t0 = pipe.submit(images0); t1 = pipe.submit(images1)
        preds0, maxvals0 = pipe.result(t0)          # valid until `depth` more batches have been submitted
    """

    def __init__(self, model, batch, height, width, depth=2, input_u8=None, flip_test=False, shift_heatmap=True, post_process=False,
                 blur_kernel=11, soft_argmax_beta=100.0, frames=None, box_padding=1.25, track=False, track_min_score=0.1,
                 track_min_joints=8, track_min_side=16.0, oriented=False, track_axis=(0, 9), track_min_axis=4.0, smooth=None,
                 antialias=False, frame_format="rgb", yuv=("bt709", "limited"), chroma_siting="left", frame_layout=None, surfaces=False):
        if depth < 1:
            raise ValueError("depth must be >= 1")
        _check_roi(model, _check_frames(frames, input_u8, box_padding, track, track_min_score, track_min_joints, track_min_side, antialias,
                                        frame_format, yuv, chroma_siting, frame_layout, surfaces),
                   oriented, track_axis, track_min_axis, smooth)
        self.steps = [InferStep(model, batch, height, width, bn_train=False, input_u8=input_u8, slot=i, flip_test=flip_test,
                                shift_heatmap=shift_heatmap, post_process=post_process, blur_kernel=blur_kernel,
                                soft_argmax_beta=soft_argmax_beta, frames=frames, box_padding=box_padding, track=track,
                                track_min_score=track_min_score, track_min_joints=track_min_joints, track_min_side=track_min_side,
                                oriented=oriented, track_axis=track_axis, track_min_axis=track_min_axis, smooth=smooth,
                                antialias=antialias, frame_format=frame_format, yuv=yuv, chroma_siting=chroma_siting,
                                frame_layout=frame_layout, surfaces=surfaces)
                      for i in range(depth)]
        self.streams = [torch.cuda.Stream() for _ in range(depth)]
        self.events = [None] * depth
        self.count = 0

    def refresh_weights(self):
        """After the model's weights changed: every slot rebuilds its packs at its next submit."""
        for s in self.steps:
            s._packed = False

    def submit(self, images=None, frames=None, boxes=None, frame_index=None, rot=None, mirror=None, dt=None, surfaces=None):
        i = self.count % len(self.steps)
        st = self.streams[i]
        st.wait_stream(torch.cuda.current_stream())          # the caller's copy of `images` into place is ordered before
        # the surfaces are READ by the slot's replay on `st` (nothing copies them): the same rule, or the allocator hands a surface's
        # block out once the slot drops its reference at its next submit while this replay may still be reading it
        bound = [surfaces] if torch.is_tensor(surfaces) else list(surfaces) if surfaces is not None else []
        if surfaces is not None and not torch.is_tensor(surfaces):
            surfaces = bound                                  # (an iterator is walked once)
        for t in [images, frames, boxes, frame_index, rot, mirror, dt] + bound:
            if torch.is_tensor(t) and t.is_cuda:
                # the slot's copy of an input runs on `st`: tell the caching allocator, or a caller that drops the batch right
                # after submit() gets the same block back for the next batch while this copy is still queued
                t.record_stream(st)
        with torch.cuda.stream(st):
            self.steps[i](images, frames, boxes, frame_index, rot, mirror, dt, surfaces)
            self.events[i] = st.record_event()
        self.count += 1
        return self.count - 1

    def result(self, ticket):
        if ticket < self.count - len(self.steps) or ticket >= self.count:
            raise LightHandError(f"ticket {ticket} is not in flight (submitted so far: {self.count}, depth {len(self.steps)})")
        i = ticket % len(self.steps)
        torch.cuda.current_stream().wait_event(self.events[i])
        return self.steps[i].preds, self.steps[i].maxvals

    def map(self, batches):
        """Yields (preds, maxvals) clones for every batch of the iterable, in order, keeping `depth` batches in flight.  A batch is
        an image tensor, or a dict of submit()'s keyword arguments (frames / boxes / frame_index / rot / mirror / dt)."""
        pending = []
        for images in batches:
            pending.append(self.submit(**images) if isinstance(images, dict) else self.submit(images))
            if len(pending) == len(self.steps):
                p, m = self.result(pending.pop(0))
                yield p.clone(), m.clone()
        for t in pending:
            p, m = self.result(t)
            yield p.clone(), m.clone()

