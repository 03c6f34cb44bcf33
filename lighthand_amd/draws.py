"""The per-step random draws of the training augmentations, on the host: CPU torch only, no device code.  ``lighthand_amd.runtime``
re-exports the samplers; TrainStep calls them through that module."""
import math
import numbers

import torch

from ._lib import LightHandError
from .topdown import ROI_AUG_IDENTITY


def _is_number(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool) and math.isfinite(v)


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
    rows[~drawn] = torch.tensor(ROI_AUG_IDENTITY, dtype=torch.float64)
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
