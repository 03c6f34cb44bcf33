"""Heatmap target render, MSE heatmap loss and arg-max keypoint decode on the HIP device.

Mirrors the three free functions the reference's training loop uses
(``CustomDataset.generate_target`` src/tools/dataset.py:165-212, ``JointsMSELoss``
src/utils/loss.py:306-325, ``get_max_preds`` src/utils/loss.py:327-355) with the same
names, arguments and error behaviour; the arithmetic runs in liblighthand_hip.  ``WeightedJointsMSELoss`` and the
``return_weight`` option of the renderers are opt-in extensions (upstream's target_weight and OHKM loss), as is DARK's
sub-pixel coding (Zhang et al. 2020): ``unbiased=True`` of the renderers and ``post_process="dark"`` of the decoders, and integral
regression (Sun et al. 2018): ``IntegralL1Loss`` and ``post_process="soft"``.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import check

HEATMAP_SIZE = 64
SIGMA = 2
RADIUS = 3 * SIGMA


def _stream():
    return torch.cuda.current_stream().cuda_stream


def gaussian_patch_host(radius=RADIUS, sigma=SIGMA):
    """The (2r+1)^2 patch, evaluated on the host with numpy float32 exactly like the reference
    (dataset.py:188-193) so the rendered values are bit-identical to the reference's."""
    size = 2 * radius + 1
    x = np.arange(0, size, 1, np.float32)
    y = x[:, np.newaxis]
    c = size // 2
    return np.exp(-((x - c) ** 2 + (y - c) ** 2) / (2 * sigma ** 2)).astype(np.float32)


_patch_cache = {}


def _patch_on(device):
    key = str(device)
    if key not in _patch_cache:
        _patch_cache[key] = torch.from_numpy(gaussian_patch_host()).to(device)
    return _patch_cache[key]


def render_targets(joints, size=HEATMAP_SIZE, out=None, return_weight=False, unbiased=False):
    """joints: device tensor [B, J, >=2] (pixel coordinates in the 256x256 frame) ->
    float32 [B, J, size, size] Gaussian targets (sigma 2, 13x13 patch, clipped assignment).
    ``return_weight=True`` (an extension: the reference computes this weight and never uses it) returns
    ``(target, target_weight [B, J, 1])``: column 2 of ``joints``, when present, is the visibility, weight = (vis > 0.5 ? vis : 0)
    x (some part of the patch lies inside the map), and a joint of weight 0 gets a zero map.
    ``unbiased=True`` (an extension: DARK's target encoding) keeps the 13x13 window where it is and evaluates the Gaussian
    around the joint's real-valued position x / 4 instead of the rounded cell (lh_gaussian_target_sub)."""
    if not joints.is_cuda:
        raise _lib.LightHandError("render_targets needs a HIP device tensor")
    j = joints.to(torch.float32).contiguous()
    b, nj, stride = j.shape
    if out is None:
        out = torch.empty(b, nj, size, size, dtype=torch.float32, device=j.device)
    if unbiased:
        weight = torch.empty(b, nj, 1, dtype=torch.float32, device=j.device) if return_weight else None
        vis = j.data_ptr() + 8 if return_weight and stride >= 3 else None
        check(_lib.load().lh_gaussian_target_sub(j.data_ptr(), stride, vis, stride, RADIUS, float(SIGMA), out.data_ptr(),
                                                 None if weight is None else weight.data_ptr(), b, nj, size, _stream()),
              "lh_gaussian_target_sub")
        return (out, weight) if return_weight else out
    patch = _patch_on(j.device)
    if return_weight:
        weight = torch.empty(b, nj, 1, dtype=torch.float32, device=j.device)
        vis = j.data_ptr() + 8 if stride >= 3 else None
        check(_lib.load().lh_gaussian_target_w(j.data_ptr(), stride, vis, stride, patch.data_ptr(), RADIUS, out.data_ptr(),
                                               weight.data_ptr(), b, nj, size, _stream()), "lh_gaussian_target_w")
        return out, weight
    check(_lib.load().lh_gaussian_target(j.data_ptr(), stride, patch.data_ptr(), RADIUS, out.data_ptr(), b, nj, size, _stream()),
          "lh_gaussian_target")
    return out


def generate_target(joints, device="cuda", return_weight=False, unbiased=False):
    """Per-sample form with the reference's signature: joints [21, >=2] (array-like) ->
    torch.float32 [21, 64, 64] (returned on the CPU like the reference's dataset method).  ``return_weight=True`` returns
    ``(target, target_weight [21, 1])`` as upstream's generate_target does (column 2 = visibility when present);
    ``unbiased``: as ``render_targets``'s."""
    if return_weight:
        j = torch.as_tensor(np.asarray(joints, dtype=np.float32)[:, :3].copy()).to(device)
        target, weight = render_targets(j[None], return_weight=True, unbiased=unbiased)
        return target[0].cpu(), weight[0].cpu()
    j = torch.as_tensor(np.asarray(joints, dtype=np.float32)[:, :2].copy()).to(device)
    return render_targets(j[None], unbiased=unbiased)[0].cpu()


def render_targets_host(joints, size=HEATMAP_SIZE, weighted=False, unbiased=False):
    """The three renderers in numpy (lh_gaussian_target, lh_gaussian_target_w, lh_gaussian_target_sub): joints [B, J, >=2] (column 2,
    when present and ``weighted``, is the visibility) -> (target fp32 [B, J, size, size], weight fp32 [B, J, 1]; ones when not
    ``weighted``).  The window and the skip test are the kernel's, in fp32: centre int(v * 0.25 + 0.5) truncated toward zero, a patch
    wholly outside the map is skipped, weight = (vis > 0.5 ? vis : 0) x (not skipped), a joint of weight 0 gets a zero map.  The
    quantised value is the patch's, the unbiased one exp(-(d^2) / (2 sigma^2)) around v * 0.25 (numpy's expf: the last bit may differ
    from the device's)."""
    F = np.float32
    jt = np.asarray(joints, np.float32)
    b, nj = jt.shape[:2]
    out, weight = np.zeros((b, nj, size, size), np.float32), np.ones((b, nj, 1), np.float32)
    patch = gaussian_patch_host()
    ys, xs = np.mgrid[0:size, 0:size]
    for i in range(b):
        for k in range(nj):
            jx, jy = jt[i, k, 0], jt[i, k, 1]
            mx, my = int(jx * F(0.25) + F(0.5)), int(jy * F(0.25) + F(0.5))
            x0, y0, x1, y1 = mx - RADIUS, my - RADIUS, mx + RADIUS + 1, my + RADIUS + 1
            skip = x0 >= size or y0 >= size or x1 < 0 or y1 < 0
            draw = not skip
            if weighted:
                v = jt[i, k, 2] if jt.shape[2] >= 3 else F(1)
                weight[i, k, 0] = (v if v > 0.5 else F(0)) * F(0 if skip else 1)
                draw = weight[i, k, 0] > 0
            if not draw:
                continue
            inside = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
            if unbiased:
                dx, dy = xs.astype(np.float32) - jx * F(0.25), ys.astype(np.float32) - jy * F(0.25)
                val = np.exp(-(dx * dx + dy * dy) / F(2 * SIGMA * SIGMA)).astype(np.float32)
            else:
                val = np.zeros((size, size), np.float32)
                iy0, iy1, ix0, ix1 = max(0, y0), min(y1, size), max(0, x0), min(x1, size)
                val[iy0:iy1, ix0:ix1] = patch[iy0 - y0:iy1 - y0, ix0 - x0:ix1 - x0]
            out[i, k] = np.where(inside, val, F(0))
    return out, weight


class GenerateHeatmap:
    """The reference's alternate renderer (src/utils/dataset_loader.py:22-53), same constructor and call: points
    ``[num_parts, >=2]`` already in heat-map coordinates -> float32 ``[num_parts, res, res]`` (CPU, like the reference);
    ``render(points)`` is the batched device form ``[B, J, >=2] -> [B, J, res, res]``.  sigma = output_res / 64 must be an
    integer (the reference instantiates it with output_res = 64)."""

    def __init__(self, output_res, num_parts, device="cuda"):
        if output_res % 64:
            raise ValueError("GenerateHeatmap on the device needs output_res = 64 * k (sigma = output_res / 64 integral)")
        self.output_res, self.num_parts, self.device = output_res, num_parts, device
        sigma = self.output_res / 64
        self.sigma = sigma
        size = 6 * sigma + 3
        x = np.arange(0, size, 1, float)
        y = x[:, np.newaxis]
        x0, y0 = 3 * sigma + 1, 3 * sigma + 1
        self.g = np.exp(-((x - x0) ** 2 + (y - y0) ** 2) / (2 * sigma ** 2))       # float64, as in the reference
        self._patch = {}

    def render(self, points, out=None):
        if not points.is_cuda:
            raise _lib.LightHandError("GenerateHeatmap.render needs a HIP device tensor")
        p = points.to(torch.float32).contiguous()
        b, nj, stride = p.shape
        if out is None:
            out = torch.empty(b, nj, self.output_res, self.output_res, dtype=torch.float32, device=p.device)
        key = str(p.device)
        if key not in self._patch:
            self._patch[key] = torch.from_numpy(self.g.astype(np.float32)).to(p.device)
        check(_lib.load().lh_gaussian_target_alt(p.data_ptr(), stride, self._patch[key].data_ptr(), int(self.sigma), out.data_ptr(),
                                                 b, nj, self.output_res, _stream()), "lh_gaussian_target_alt")
        return out

    def __call__(self, p):
        pts = torch.as_tensor(np.asarray(p, dtype=np.float32)[:, :2].copy()).to(self.device)
        return self.render(pts[None])[0].cpu().numpy()


class _MseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, target):
        lib = _lib.load()
        p = output.detach().to(torch.float32).contiguous()
        g = target.detach().to(torch.float32).contiguous()
        if p.shape != g.shape:
            raise ValueError(f"prediction {tuple(p.shape)} and target {tuple(g.shape)} differ")
        n = p.numel()
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        grad = torch.empty_like(p)
        ws = torch.empty(lib.lh_mse_workspace_bytes(n), dtype=torch.uint8, device=p.device)
        check(lib.lh_mse_heatmap(p.data_ptr(), g.data_ptr(), n, loss.data_ptr(), grad.data_ptr(), None, ws.data_ptr(), _stream()),
              "lh_mse_heatmap")
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        return grad * gout, None


class JointsMSELoss(nn.Module):
    """0.5 * MSE per joint averaged over joints (== 0.5 * mean over all elements).  The
    ``target_weight`` argument is accepted and ignored exactly like the reference does with
    ``use_target_weight=False`` (src/utils/method.py:49)."""

    def __init__(self, use_target_weight=False):
        super().__init__()
        self.use_target_weight = use_target_weight

    def forward(self, output, target, target_weight=None):
        if not output.is_cuda:
            raise _lib.LightHandError("JointsMSELoss runs on the HIP device only")
        return _MseFn.apply(output, target)


class _WeightedMseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, target, target_weight, topk):
        lib = _lib.load()
        p = output.detach().to(torch.float32).contiguous()
        g = target.detach().to(torch.float32).contiguous()
        if p.shape != g.shape or p.dim() < 3:
            raise ValueError(f"prediction {tuple(p.shape)} and target {tuple(g.shape)} must be one [B, J, ...] shape")
        b, j = p.shape[:2]
        hw = p[0, 0].numel()
        w = None
        if target_weight is not None:
            w = target_weight.detach().to(torch.float32).contiguous()
            if w.numel() != b * j:
                raise ValueError(f"target_weight {tuple(w.shape)} does not hold one weight per joint plane ({b} x {j})")
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        joint_loss = torch.empty(b, j, dtype=torch.float32, device=p.device)
        grad = torch.empty_like(p)
        ws = torch.empty(lib.lh_joints_mse_workspace_bytes(b, j), dtype=torch.uint8, device=p.device)
        check(lib.lh_joints_mse(p.data_ptr(), g.data_ptr(), None if w is None else w.data_ptr(), b, j, hw, int(topk), loss.data_ptr(),
                                joint_loss.data_ptr(), grad.data_ptr(), None, ws.data_ptr(), _stream()), "lh_joints_mse")
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(joint_loss)
        return loss, joint_loss

    @staticmethod
    def backward(ctx, gout, _gjoint):
        (grad,) = ctx.saved_tensors
        return grad * gout, None, None, None


class WeightedJointsMSELoss(nn.Module):
    """An extension without a reference oracle (the reference computes ``target_weight`` and drops it; ``JointsMSELoss`` above
    stays its drop-in): the SimpleBaseline / HRNet code line's ``JointsMSELoss(use_target_weight=True)`` -- every joint plane's
    prediction and target are multiplied by its weight, loss = 0.5 * mean over all elements -- and, with ``topk`` >= 1, its
    ``JointsOHKMMSELoss``: per sample only the ``topk`` joints with the largest loss count, loss = mean over samples of their mean.
    ``target_weight``: [B, J, 1] / [B, J] or None (ones).  ``joint_loss`` holds the per-joint losses [B, J] of the last call."""

    def __init__(self, topk=0):
        super().__init__()
        if topk < 0:
            raise ValueError("topk must be >= 0 (0 = no hard-keypoint mining)")
        self.topk = int(topk)
        self.joint_loss = None

    def forward(self, output, target, target_weight=None):
        if not output.is_cuda:
            raise _lib.LightHandError("WeightedJointsMSELoss runs on the HIP device only")
        loss, self.joint_loss = _WeightedMseFn.apply(output, target, target_weight, self.topk)
        return loss


class _IntegralL1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, joints, target_weight, beta, scale):
        lib = _lib.load()
        p = output.detach().to(torch.float32).contiguous()
        if p.dim() != 4:
            raise ValueError(f"prediction {tuple(p.shape)} must be [B, J, H, W]")
        b, j, h, w = p.shape
        g = joints.detach().to(torch.float32).contiguous()
        if g.dim() != 3 or tuple(g.shape[:2]) != (b, j) or g.shape[2] < 2:
            raise ValueError(f"joints {tuple(g.shape)} must be [{b}, {j}, >=2]")
        wt = None
        if target_weight is not None:
            wt = target_weight.detach().to(torch.float32).contiguous()
            if wt.numel() != b * j:
                raise ValueError(f"target_weight {tuple(wt.shape)} does not hold one weight per joint plane ({b} x {j})")
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        preds = torch.empty(b, j, 2, dtype=torch.float32, device=p.device)
        joint_loss = torch.empty(b, j, dtype=torch.float32, device=p.device)
        grad = torch.empty_like(p) if ctx.needs_input_grad[0] else None      # no gradient wanted: the kernel skips that pass
        ws = torch.empty(lib.lh_integral_l1_workspace_bytes(b, j), dtype=torch.uint8, device=p.device)
        check(lib.lh_integral_l1(p.data_ptr(), g.data_ptr(), g.shape[2], None if wt is None else wt.data_ptr(), b, j, h, w, float(beta),
                                 float(scale), 1.0, preds.data_ptr(), joint_loss.data_ptr(), loss.data_ptr(), 0,
                                 None if grad is None else grad.data_ptr(), 0, None, ws.data_ptr(), _stream()), "lh_integral_l1")
        if grad is not None:
            ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(preds, joint_loss)
        return loss, preds, joint_loss

    @staticmethod
    def backward(ctx, gout, _gpreds, _gjoint):
        (grad,) = ctx.saved_tensors
        return grad * gout, None, None, None, None


class IntegralL1Loss(nn.Module):
    """An extension without a reference oracle: the coordinate loss of integral regression (Sun et al. 2018).  The prediction of a
    plane is the expected position under softmax(``beta`` * heat-map), times ``scale`` (heat-map cells -> input pixels); the loss is
    the L1 distance to ``joints`` [B, J, >=2] (input pixels), weighted per joint by ``target_weight`` ([B, J, 1] / [B, J] or None
    = ones) and averaged over the 2 * B * J coordinates (lh_integral_l1 with lambda = 1).  ``preds`` [B, J, 2] and ``joint_loss``
    [B, J] hold the last call's outputs; the gradient reaches the heat-maps through autograd."""

    def __init__(self, beta=100.0, scale=1.0):
        super().__init__()
        if not (beta > 0 and np.isfinite(beta)):
            raise ValueError(f"beta must be positive and finite, not {beta!r}")
        if not np.isfinite(scale):
            raise ValueError(f"scale must be finite, not {scale!r}")
        self.beta, self.scale = float(beta), float(scale)
        self.preds = self.joint_loss = None

    def forward(self, output, joints, target_weight=None):
        if not output.is_cuda:
            raise _lib.LightHandError("IntegralL1Loss runs on the HIP device only")
        loss, self.preds, self.joint_loss = _IntegralL1Fn.apply(output, joints, target_weight, self.beta, self.scale)
        return loss


def decode_mode(post_process):
    """The ``post_process`` option of the decoders -> None (plain arg-max), "quarter", "dark" or "soft".  ``True`` means "quarter"."""
    if isinstance(post_process, str):
        if post_process in ("quarter", "dark", "soft"):
            return post_process
    elif post_process is None or isinstance(post_process, (bool, np.bool_)):
        return "quarter" if post_process else None
    raise ValueError(f'post_process must be False, True, "quarter", "dark" or "soft", not {post_process!r}')


def dark_refine_device(heatmaps, idx, maxvals, preds, scale=1.0, blur_kernel=11):
    """The DARK launch on its own, for callers that hold the outputs of an arg-max or a flip merge at the same ``scale``:
    ``preds`` [B, J, 2] is refined in place from ``heatmaps`` float32 [B, J, H, W] (contiguous, only read)."""
    b, j, h, w = heatmaps.shape
    check(_lib.load().lh_heatmap_dark(heatmaps.data_ptr(), idx.data_ptr(), maxvals.data_ptr(), b * j, h, w, int(blur_kernel),
                                       float(scale), preds.data_ptr(), _stream()), "lh_heatmap_dark")
    return preds


def max_preds_device(heatmaps, scale=1.0, post_process=False, blur_kernel=11, soft_argmax_beta=100.0):
    """Device overload: heatmaps float32 [B, J, H, W] on the device ->
    (preds [B, J, 2], maxvals [B, J, 1], flat indices [B, J]) device tensors.  ``post_process=True`` / ``"quarter"`` adds the
    opt-in quarter-pixel refinement (an extension: the reference's TEST.POST_PROCESS flag exists but is unused);
    ``post_process="dark"`` the DARK decode instead: a second-order Taylor step on the log of the map blurred with a Gaussian of
    ``blur_kernel`` taps (lh_heatmap_dark: maps of at most 96 x 96, ``blur_kernel`` odd in 3..17); ``post_process="soft"`` the
    soft-arg-max: preds is the expectation under softmax(``soft_argmax_beta`` * heat-map) (lh_heatmap_soft_argmax), while maxvals
    and the indices stay the arg-max's."""
    mode = decode_mode(post_process)
    if heatmaps.dim() != 4:
        raise AssertionError("batch_images should be 4-ndim")
    hm = heatmaps.to(torch.float32).contiguous()
    b, j, h, w = hm.shape
    preds = torch.empty(b, j, 2, dtype=torch.float32, device=hm.device)
    maxvals = torch.empty(b, j, 1, dtype=torch.float32, device=hm.device)
    idx = torch.empty(b, j, dtype=torch.int32, device=hm.device)
    check(_lib.load().lh_heatmap_argmax(hm.data_ptr(), b * j, h, w, float(scale), preds.data_ptr(), maxvals.data_ptr(),
                                         idx.data_ptr(), _stream()), "lh_heatmap_argmax")
    if mode == "quarter":
        check(_lib.load().lh_heatmap_refine(hm.data_ptr(), idx.data_ptr(), maxvals.data_ptr(), b * j, h, w, float(scale),
                                            preds.data_ptr(), _stream()), "lh_heatmap_refine")
    elif mode == "dark":
        dark_refine_device(hm, idx, maxvals, preds, scale, blur_kernel)
    elif mode == "soft":
        check(_lib.load().lh_heatmap_soft_argmax(hm.data_ptr(), b * j, h, w, float(soft_argmax_beta), float(scale), preds.data_ptr(),
                                                  _stream()), "lh_heatmap_soft_argmax")
    return preds, maxvals, idx


def flip_merge_device(heatmaps, heatmaps_mirrored, shift=True, scale=1.0, out=None):
    """Flip test for callers that run their own forwards: heatmaps float32 [B, J, H, W] of the plain batch and
    ``heatmaps_mirrored`` of the same batch mirrored horizontally, on the device ->
    (preds [B, J, 2], maxvals [B, J, 1], flat indices [B, J], merged [B, J, H, W]) device tensors.  merged = (heatmaps +
    flipped-back mirrored maps, shifted one column when ``shift``) * 0.5 (SimpleBaseline's flip test; TEST.SHIFT_HEATMAP), decoded
    like ``max_preds_device``.  ``out``: a float32 [B, J, H, W] buffer for merged (may be ``heatmaps`` itself)."""
    if heatmaps.dim() != 4 or heatmaps_mirrored.shape != heatmaps.shape:
        raise AssertionError("heatmaps and heatmaps_mirrored should be 4-ndim of one shape")
    a = heatmaps.to(torch.float32).contiguous()
    m = heatmaps_mirrored.to(torch.float32).contiguous()
    b, j, h, w = a.shape
    if out is None:
        out = torch.empty_like(a)
    if out.shape != a.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 tensor of shape {tuple(a.shape)}")
    preds = torch.empty(b, j, 2, dtype=torch.float32, device=a.device)
    maxvals = torch.empty(b, j, 1, dtype=torch.float32, device=a.device)
    idx = torch.empty(b, j, dtype=torch.int32, device=a.device)
    check(_lib.load().lh_heatmap_flip_merge(a.data_ptr(), m.data_ptr(), b * j, h, w, int(bool(shift)), float(scale), out.data_ptr(),
                                            preds.data_ptr(), maxvals.data_ptr(), idx.data_ptr(), _stream()), "lh_heatmap_flip_merge")
    return preds, maxvals, idx, out


def soft_argmax_device(heatmaps, beta=100.0, scale=1.0):
    """Opt-in differentiable-style decode (an extension: the reference only has the hard arg-max): heatmaps float32
    [B, J, H, W] on the device -> expected (x, y) under softmax(beta * heatmap), [B, J, 2] device tensor."""
    if heatmaps.dim() != 4:
        raise AssertionError("batch_images should be 4-ndim")
    hm = heatmaps.to(torch.float32).contiguous()
    b, j, h, w = hm.shape
    preds = torch.empty(b, j, 2, dtype=torch.float32, device=hm.device)
    check(_lib.load().lh_heatmap_soft_argmax(hm.data_ptr(), b * j, h, w, float(beta), float(scale), preds.data_ptr(), _stream()),
          "lh_heatmap_soft_argmax")
    return preds


def get_max_preds(batch_heatmaps, post_process=False, blur_kernel=11, soft_argmax_beta=100.0):
    """Reference signature (src/utils/loss.py:327-355): numpy [B, J, H, W] -> (preds float32
    [B, J, 2], maxvals [B, J, 1]) numpy arrays; device tensors are accepted too and then
    device tensors are returned (no host round trip).  ``post_process`` (default off = reference behaviour) enables
    the quarter-pixel refinement (``True`` / ``"quarter"``), the DARK decode (``"dark"``, with ``blur_kernel``) or the soft-arg-max
    (``"soft"``, with ``soft_argmax_beta``), as ``max_preds_device``'s."""
    decode_mode(post_process)
    if isinstance(batch_heatmaps, torch.Tensor):
        p, m, _ = max_preds_device(batch_heatmaps, post_process=post_process, blur_kernel=blur_kernel, soft_argmax_beta=soft_argmax_beta)
        return p, m
    assert isinstance(batch_heatmaps, np.ndarray), "batch_heatmaps should be numpy.ndarray"
    assert batch_heatmaps.ndim == 4, "batch_images should be 4-ndim"
    p, m, _ = max_preds_device(torch.from_numpy(np.ascontiguousarray(batch_heatmaps, dtype=np.float32)).cuda(),
                               post_process=post_process, blur_kernel=blur_kernel, soft_argmax_beta=soft_argmax_beta)
    return p.cpu().numpy(), m.cpu().numpy().astype(batch_heatmaps.dtype)
