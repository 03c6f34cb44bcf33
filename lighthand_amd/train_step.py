"""TrainStep: one training iteration as one replay of a captured HIP graph (the overview is lighthand_amd.runtime's docstring)."""
import torch

from . import _lib, heatmap
from ._lib import LightHandError, check
from .amp import DynamicLossScale
from .draws import _geometric_aug_spec, _is_number
from .frame_input import FrameInput, _check_beta, _check_train_frames, _FrameStep, _ptr
from .optim import Adam


class TrainStep(_FrameStep):
    _frame_inputs = "frames / boxes / frame_index / rot / mirror"
    _frames_take = "frames / boxes / frame_index and joints, not images or target"
    _rot_also, _rot_first = " or roi_aug=", True

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
        fi = FrameInput.check(frames, input_u8, box_padding=box_padding, oriented=oriented, antialias=antialias, frame_format=frame_format,
                              yuv=yuv, chroma_siting=chroma_siting, frame_layout=frame_layout, surfaces=surfaces)
        _, roi_aug, crop_jitter = _check_train_frames(
            model, fi, geometric_aug=geometric_aug, color_jitter=color_jitter, targets_from_joints=targets_from_joints, roi_aug=roi_aug,
            coord_loss_weight=coord_loss_weight, use_target_weight=use_target_weight, crop_jitter=crop_jitter)
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
        owner = ("train", "frames") if fi.frames else ("train", "u8") if input_u8 else None
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
        self.color_jitter, self.geometric_aug = color_jitter, geometric_aug
        self.images_u8 = self.plan.use_uint8_input(*input_u8, jitter=color_jitter is not None,
                                                   warp=geometric_aug is not None) if input_u8 else None
        self.joints = torch.zeros(batch, out.shape[1], 2, dtype=torch.float32, device=dev)
        # the joints through this step's forward matrices: what the model is asked to predict (self.joints keeps the caller's)
        self.joints_aug = torch.zeros_like(self.joints) if geometric_aug is not None else None
        # frames=(n_frames, hs, ws): the input is hand ROIs on full frames (the docstring); joints_crop takes joints_aug's place
        self.roi_aug, self.crop_jitter = roi_aug, crop_jitter
        self._use_frame_input(fi, perturb=roi_aug is not None, jitter=crop_jitter is not None)
        self.joints_crop = torch.zeros_like(self.joints) if fi.frames else None
        self.frame_preds = torch.zeros_like(self.joints) if fi.frames and decode else None
        # the ColorJitter ranges drawn from at every call: the crop's, or the uint8 input's (a step has one of the two inputs)
        self._jitter = crop_jitter if crop_jitter is not None else color_jitter if self.images_u8 is not None else None
        # the samplers are looked up on lighthand_amd.runtime at every call: that module is where a caller replaces one
        from . import runtime
        self._draws = runtime
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
        self._check_call(images is not None or target is not None, frames, boxes, frame_index, rot, mirror, surfaces)
        if self.graphs is not None:
            self.sync_hyper()
        self._copy_frame_inputs(frames, boxes, frame_index, rot, mirror)
        if self.roi_aug is not None:
            g = self.roi_aug                       # read by the replay from the plan's buffer, never baked into the graph
            self.plan.roi_aug.copy_(self._draws.sample_roi_aug(self.joints.shape[0], g["rotation"], g["scale"], g["shift"], g["mirror_prob"],
                                                               prob=g["prob"], generator=g["generator"]), non_blocking=True)
        if images is not None:
            (self.images_u8 if images.dtype == torch.uint8 and self.images_u8 is not None else self.images).copy_(images, non_blocking=True)
        if self._jitter is not None:
            f, o = self._draws.sample_color_jitter(self.joints.shape[0], *self._jitter, mask=aug)
            self.plan.jitter_factors.copy_(f, non_blocking=True)
            self.plan.jitter_order.copy_(o, non_blocking=True)
        if self.geometric_aug is not None:
            g = self.geometric_aug                 # read by the replay from the plan's buffers, never baked into the graph
            inv, fwd = self._draws.sample_affine(self.joints.shape[0], g["rotation"], g["scale"], g["shift"], prob=g["prob"],
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
