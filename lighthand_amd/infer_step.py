"""InferStep: eval-mode forward + decode as one captured HIP graph; InferPipeline: several of them in flight."""
import ctypes

import torch

from . import _lib, heatmap, overlay as _overlay, topdown
from ._lib import LightHandError, check
from .frame_input import FrameInput, _check_beta, _check_manage_tracks, _check_motion, _check_smooth_gate, _check_tracking, _FrameStep, _ptr


class InferStep(_FrameStep):
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
    surface may be overwritten or freed only after the step's stream has passed the replay that reads it.
    Track management -- duplicate tracks, expiry, a detector's boxes -- is ManagedInferStep's, below, and so are motion prediction
    (``motion=``) and the gated filter (``smooth_gate=``)."""

    _serial = 0
    _frame_inputs = "frames / boxes / frame_index"
    _frames_take = "frames / boxes / frame_index, not images"
    _rot_also, _rot_first = "", False
    _manage_tracks_option, _detections = False, None               # ManagedInferStep(manage_tracks=) / its call's detections=
    _motion_option, _smooth_gate_option = None, None               # ManagedInferStep(motion=, smooth_gate=)
    _overlay_option, overlay, overlay_table = None, None, None     # ManagedInferStep(overlay=)

    def __init__(self, model, batch, height, width, bn_train=False, use_graph=True, input_u8=None, slot=0,
                 flip_test=False, shift_heatmap=True, post_process=False, plan_options=None, blur_kernel=11, soft_argmax_beta=100.0,
                 frames=None, box_padding=1.25, track=False, track_min_score=0.1, track_min_joints=8, track_min_side=16.0,
                 oriented=False, track_axis=(0, 9), track_min_axis=4.0, smooth=None, antialias=False, frame_format="rgb",
                 yuv=("bt709", "limited"), chroma_siting="left", frame_layout=None, surfaces=False):
        if not shift_heatmap and not flip_test:
            raise ValueError("shift_heatmap=False applies to the flip test: pass flip_test=True")
        fi = FrameInput.check(frames, input_u8, box_padding=box_padding, oriented=oriented, antialias=antialias, frame_format=frame_format,
                              yuv=yuv, chroma_siting=chroma_siting, frame_layout=frame_layout, surfaces=surfaces)
        smooth = _check_tracking(model, fi, track=track, track_min_score=track_min_score, track_min_joints=track_min_joints,
                                 track_min_side=track_min_side, track_axis=track_axis, track_min_axis=track_min_axis, smooth=smooth)
        self.manage_tracks = _check_manage_tracks(fi, track, self._manage_tracks_option, batch)        # ManagedInferStep's
        self.motion = _check_motion(fi, track, self._motion_option)                                    # ManagedInferStep's, as well
        self.smooth_gate = _check_smooth_gate(smooth, self._smooth_gate_option, track_min_score)
        if self._overlay_option not in (None, False) and fi.frames is None:
            raise ValueError("overlay= draws the tracked hands into full frames: pass frames=(n_frames, hs, ws)")
        post_process = heatmap.decode_mode(post_process)
        _check_beta(soft_argmax_beta)
        self.soft_argmax_beta = float(soft_argmax_beta)
        self.lib = _lib.load()
        # a plan of its own (never the one model(x) runs): use_uint8_input rewires the plan's image launch, and a pipeline
        # slot replays asynchronously on its own stream -- neither may happen to the plan model.forward() uses
        InferStep._serial += 1
        self.plan = model.plan(batch, height, width, training=bn_train, backward=False, slot=slot,
                               owner=("infer", "frames" if fi.frames else "u8" if input_u8 else "f32", InferStep._serial), options=plan_options)
        out = self.plan.out_nchw
        dev = out.device
        # input_u8=(hs, ws): raw uint8 HWC frames; ToTensor / Resize / Normalize run fused on the device (dataset.py:128-159)
        self.images = self.plan.use_uint8_input(*input_u8) if input_u8 else self.plan.img_nchw
        self.crop_preds = self.next_boxes = self.lost = self.next_rot = self.dt = self.smooth_preds = None
        self.det_boxes = self.det_frame = self.det_score = self.lost_count = self.dup_of = self.seeded = self.det_state = None
        self.velocity = self.coasted = None
        self.track, self.smooth = bool(track) and fi.frames is not None, smooth
        self.track_min_score, self.track_min_joints, self.track_min_side = float(track_min_score), int(track_min_joints), float(track_min_side)
        self._use_frame_input(fi)
        if self.oriented:
            self.track_axis, self.track_min_axis = (int(track_axis[0]), int(track_axis[1])), float(track_min_axis)
        if fi.frames:
            self.crop_preds = torch.zeros(batch, out.shape[1], 2, dtype=torch.float32, device=dev)
            if self.track:
                self.next_boxes = self.boxes.clone()
                self.lost = torch.ones(batch, dtype=torch.int32, device=dev)
                if self.oriented:
                    self.next_rot = self.rot.clone()
                if self.manage_tracks:
                    k = self.manage_tracks["max_detections"]
                    self._n_frames = fi.frames[0]
                    self.det_boxes = torch.zeros(k, 4, dtype=torch.float32, device=dev)
                    self.det_frame = torch.full((k,), -1, dtype=torch.int32, device=dev)
                    self.det_score = torch.zeros(k, dtype=torch.float32, device=dev)
                    self.lost_count = torch.zeros(batch, dtype=torch.int32, device=dev)       # state: replays in a row a slot has been lost
                    self.dup_of, self.seeded = (torch.full((batch,), -1, dtype=torch.int32, device=dev) for _ in range(2))
                    self.det_state = torch.full((k,), -1, dtype=torch.int32, device=dev)
            if smooth or self.motion:
                self.dt = torch.full((batch,), 1.0 / 30.0, dtype=torch.float32, device=dev)
            if self.motion:
                # the predictor's state: the centre of the last box the hand was found in, its low-passed velocity (frame px / s),
                # whether the slot has seen a frame, and the replays in a row it has coasted
                self._centre, self.velocity = (torch.zeros(batch, 2, dtype=torch.float32, device=dev) for _ in range(2))
                self._motion_seen, self.coasted = (torch.zeros(batch, dtype=torch.int32, device=dev) for _ in range(2))
            if smooth:
                self.smooth_preds = torch.zeros(batch, out.shape[1], 2, dtype=torch.float32, device=dev)
                # the filter's state: the last filtered keypoints, their filtered derivative, and whether the slot has seen a frame
                self._xhat, self._dxhat = torch.zeros_like(self.smooth_preds), torch.zeros_like(self.smooth_preds)
                self._seen = torch.zeros(batch, dtype=torch.int32, device=dev)
                if self.smooth_gate:                                # per joint in _seen's place, and the seconds a joint has gone without an update
                    self._seen_j = torch.zeros(batch, out.shape[1], dtype=torch.int32, device=dev)
                    self._gap = torch.zeros(batch, out.shape[1], dtype=torch.float32, device=dev)
        self.flip_test, self.shift_heatmap, self.post_process, self.blur_kernel = flip_test, shift_heatmap, post_process, int(blur_kernel)
        # flip test: the plain pass's maps are copied here, and the merge writes over them in place
        self.heatmaps = torch.zeros_like(out) if flip_test else out
        self.preds = torch.zeros(batch, out.shape[1], 2, dtype=torch.float32, device=dev)
        self.maxvals = torch.zeros(batch, out.shape[1], 1, dtype=torch.float32, device=dev)
        self.idx = torch.zeros(batch, out.shape[1], dtype=torch.int32, device=dev) if post_process in ("quarter", "dark") else None
        self.scale = float(height // out.shape[2])
        if self._overlay_option not in (None, False):
            self._use_overlay(fi, track_min_score)
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
            if self.manage_tracks:
                mt = self.manage_tracks
                check(self.lib.lh_tracks_manage(self.preds.data_ptr(), self.maxvals.data_ptr(), p.src_frame.data_ptr(), self.frame_index.data_ptr(),
                                                out.shape[0], out.shape[1], self._n_frames, self.det_boxes.data_ptr(), self.det_frame.data_ptr(),
                                                self.det_score.data_ptr(), mt["max_detections"], self.track_min_score, self.track_min_side,
                                                mt["dup_overlap"], mt["match_overlap"], mt["det_min_score"], mt["max_lost"],
                                                self.next_boxes.data_ptr(), _ptr(self.next_rot), self.lost.data_ptr(), self.lost_count.data_ptr(),
                                                self.dup_of.data_ptr(), self.seeded.data_ptr(), self.det_state.data_ptr(), s), "lh_tracks_manage")
            if self.motion:
                mo = self.motion
                check(self.lib.lh_rois_predict(self.next_boxes.data_ptr(), self.lost.data_ptr(), p.src_frame.data_ptr(), _ptr(self.seeded),
                                               self.dt.data_ptr(), out.shape[0], mo["cutoff"], mo["lead"], mo["max_shift"], mo["coast"],
                                               self._centre.data_ptr(), self.velocity.data_ptr(), self._motion_seen.data_ptr(),
                                               self.coasted.data_ptr(), s), "lh_rois_predict")
            if self.smooth_gate:                                    # in lh_one_euro's place, never beside it
                sizes = self.next_boxes if self.track else self.boxes
                check(self.lib.lh_one_euro_gated(self.preds.data_ptr(), self.maxvals.data_ptr(), sizes.data_ptr(), p.src_frame.data_ptr(),
                                                 _ptr(self.lost), self.dt.data_ptr(), out.shape[0], out.shape[1], self.smooth[0], self.smooth[1],
                                                 self.smooth[2], self.smooth_gate["min_score"], int(self.smooth_gate["by_size"]),
                                                 self._xhat.data_ptr(), self._dxhat.data_ptr(), self._seen_j.data_ptr(), self._gap.data_ptr(),
                                                 self.smooth_preds.data_ptr(), s), "lh_one_euro_gated")
            elif self.smooth:
                check(self.lib.lh_one_euro(self.preds.data_ptr(), p.src_frame.data_ptr(), _ptr(self.lost), self.dt.data_ptr(), out.shape[0],
                                           out.shape[1], self.smooth[0], self.smooth[1], self.smooth[2], self._xhat.data_ptr(),
                                           self._dxhat.data_ptr(), self._seen.data_ptr(), self.smooth_preds.data_ptr(), s), "lh_one_euro")
            if self.overlay and not self._warming:                  # the last launch of the graph, behind the filter
                self._enqueue_overlay(s)

    _warming = False                                               # the eager run in front of the capture is not a frame: it draws nothing

    def _use_overlay(self, fi, track_min_score):
        """ManagedInferStep(overlay=): the resolved options (``self.overlay``), the topology and palette on the device, the frames'
        layout, and with target="surfaces" the second surface table (``overlay_table``, zeros: every destination unbound)."""
        dev = self.preds.device
        o = _overlay.resolve_overlay(self._overlay_option, self.preds.shape[1], track_min_score, fi.frame_format, fi.yuv, self.smooth)
        self._ov_layout = topdown.frame_layout_of(fi.frame_format, fi.frames[1], fi.frames[2], fi.frame_layout)
        self._ov_desc = topdown.frames_layout_struct(self._ov_layout, fi.yuv, fi.chroma_siting)
        self._ov_tables = [torch.from_numpy(o[k]).to(dev) for k in ("parents", "groups", "palette")]
        self._ov_frames = fi.frames
        if o["target"] == "surfaces":
            self.overlay_table = torch.zeros(fi.frames[0], dtype=torch.int64, device=dev)
            self._overlay_refs = [None] * fi.frames[0]
        self.overlay = o

    def _enqueue_overlay(self, s):
        o, p = self.overlay, self.plan
        n, hs, ws = self._ov_frames
        table = self.overlay_table if o["target"] == "surfaces" else p.surface_table if self.surfaces else None
        frames, stride = (None, 0) if table is not None else (self.frames.data_ptr(), self.frames.stride(0))
        src = self.smooth_preds if o["source"] == "smooth" else self.preds
        check(self.lib.lh_draw_hands(frames, stride, _ptr(table), ctypes.byref(self._ov_desc), n, hs, ws, src.data_ptr(), self.maxvals.data_ptr(),
                                     p.src_frame.data_ptr(), _ptr(self.lost), p.crop_mat.data_ptr(), self.boxes.data_ptr(), src.shape[0],
                                     src.shape[1], p.h, p.w, self._ov_tables[0].data_ptr(), self._ov_tables[1].data_ptr(),
                                     self._ov_tables[2].data_ptr(), self._ov_tables[2].shape[0] - 2, o["min_score"], o["line_radius"],
                                     o["joint_radius"], o["by_size"], o["opacity"], int(o["draw_roi"]), s), "lh_draw_hands")

    def bind_overlay_surfaces(self, surfaces, start=0):
        """Destination ``start + i`` of the overlay <- ``surfaces[i]`` (ManagedInferStep(overlay=dict(target="surfaces"))): bind_surfaces'
        rules and checks on the second table, same layout as the frames; also on a step that crops a frame buffer.  The kernel never
        reads the source frames, so the caller decides what a destination holds beforehand (a copy of the frame, as a rule).  A
        destination may be reused only after the step's stream has passed the replay that draws on it."""
        if self.overlay_table is None:
            raise ValueError("overlay surfaces are the destinations of a step built with overlay=dict(target='surfaces')")
        self._bind_table(self.overlay_table, self._overlay_refs, self._ov_layout, surfaces, start, "bind_overlay_surfaces")

    def unbind_overlay_surfaces(self, indices=None):
        """Zero the overlay table's entries of ``indices`` (None: all) and drop the references: nothing is drawn for such a frame."""
        if self.overlay_table is None:
            raise ValueError("overlay surfaces are the destinations of a step built with overlay=dict(target='surfaces')")
        self._unbind_table(self.overlay_table, self._overlay_refs, indices, "unbind_overlay_surfaces")

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
        for state in (self._seen,) + ((self._seen_j, self._gap) if self.smooth_gate else ()):
            if slots is None:
                state.zero_()
            else:
                state[torch.as_tensor(slots, device=state.device)] = 0

    def reset_motion(self, slots=None):
        """Forget the motion state of ``slots`` (indices or a mask; None: all), on the device: ``velocity`` and ``coasted`` go to zero and
        their next frame starts the predictor again, with no shift.  LightHandError on a step built without ``motion=``, as advance()'s."""
        if not self.motion:
            raise LightHandError("reset_motion() needs ManagedInferStep(frames=..., track=True, motion=True)")
        for state in (self._motion_seen, self.velocity, self.coasted, self._centre):
            if slots is None:
                state.zero_()
            else:
                state[torch.as_tensor(slots, device=state.device)] = 0

    def reset_tracks(self, slots=None):
        """Zero ``lost_count`` of ``slots`` (indices or a mask; None: all), on the device: their expiry starts counting again.
        LightHandError on a step built without ``manage_tracks=``, as advance()'s."""
        if not self.manage_tracks:
            raise LightHandError("reset_tracks() needs ManagedInferStep(frames=..., track=True, manage_tracks=True)")
        if slots is None:
            self.lost_count.zero_()
        else:
            self.lost_count[torch.as_tensor(slots, device=self.lost_count.device)] = 0

    def _copy_detections(self, detections):
        """The detection list of this call: ``detections`` = (boxes [n][4], frame [n], score [n]), n <= max_detections, tensors or
        array-likes; the entries behind them, or all of them without ``detections``, are empty (frame -1)."""
        n = 0
        if detections is not None:
            if not isinstance(detections, (tuple, list)) or len(detections) != 3:
                raise ValueError("detections must be (boxes [n][4], frame [n], score [n])")
            dev = self.det_boxes.device
            boxes = torch.as_tensor(detections[0], dtype=torch.float32).reshape(-1, 4)
            frame, score = torch.as_tensor(detections[1], dtype=torch.int32).reshape(-1), torch.as_tensor(detections[2], dtype=torch.float32).reshape(-1)
            n = boxes.shape[0]
            if frame.shape[0] != n or score.shape[0] != n or n > self.det_boxes.shape[0]:
                raise ValueError(f"detections: boxes [n][4], frame [n] and score [n] with n <= max_detections = {self.det_boxes.shape[0]}, got "
                                 f"{tuple(boxes.shape)} / {tuple(frame.shape)} / {tuple(score.shape)}")
            if n:
                self.det_boxes[:n].copy_(boxes.to(dev, non_blocking=True), non_blocking=True)
                self.det_frame[:n].copy_(frame.to(dev, non_blocking=True), non_blocking=True)
                self.det_score[:n].copy_(score.to(dev, non_blocking=True), non_blocking=True)
        self.det_frame[n:].fill_(-1)

    def refresh_weights(self):
        self.plan.refresh_packs(torch.cuda.current_stream().cuda_stream)
        self._packed = True

    def __call__(self, images=None, frames=None, boxes=None, frame_index=None, rot=None, mirror=None, dt=None, surfaces=None):
        self._check_call(images is not None, frames, boxes, frame_index, rot, mirror, surfaces)
        if dt is not None and not (self.smooth or self.motion):
            raise ValueError("dt is the input of InferStep(frames=..., smooth=(min_cutoff, beta))")
        if images is not None:
            self.images.copy_(images, non_blocking=True)
        self._copy_frame_inputs(frames, boxes, frame_index, rot, mirror)
        if dt is not None:
            self.dt.copy_(dt, non_blocking=True) if torch.is_tensor(dt) else self.dt.fill_(float(dt))
        if self.manage_tracks:
            self._copy_detections(self._detections)
            self._detections = None
        if not self._packed:
            self.refresh_weights()
        if not self.use_graph:
            self._enqueue()
            return self.preds
        if self.graph is None:
            lost_count = self.lost_count.clone() if self.manage_tracks else None
            warm = torch.cuda.Stream()
            warm.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(warm):
                self._warming = True
                try:
                    self._enqueue()
                finally:
                    self._warming = False
            torch.cuda.current_stream().wait_stream(warm)
            torch.cuda.synchronize()
            if self.smooth:
                self._seen.zero_()                                  # the warm-up run is not a frame: the first replay starts the filter
                if self.smooth_gate:
                    self._seen_j.zero_()
                    self._gap.zero_()
            if self.manage_tracks:
                self.lost_count.copy_(lost_count)                   # nor does it count towards a slot's expiry
            if self.motion:
                self.reset_motion()                                 # nor is it a frame the predictor has seen
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
    Track management: ManagedInferPipeline, below.

        pipe = InferPipeline(model, 64, 256, 256, depth=2)
        t0 = pipe.submit(images0); t1 = pipe.submit(images1)
        preds0, maxvals0 = pipe.result(t0)          # valid until `depth` more batches have been submitted
    """

    _step_class, _step_extra = InferStep, {}                        # ManagedInferPipeline's slots are ManagedInferSteps

    def __init__(self, model, batch, height, width, depth=2, input_u8=None, flip_test=False, shift_heatmap=True, post_process=False,
                 blur_kernel=11, soft_argmax_beta=100.0, frames=None, box_padding=1.25, track=False, track_min_score=0.1,
                 track_min_joints=8, track_min_side=16.0, oriented=False, track_axis=(0, 9), track_min_axis=4.0, smooth=None,
                 antialias=False, frame_format="rgb", yuv=("bt709", "limited"), chroma_siting="left", frame_layout=None, surfaces=False):
        # every option from input_u8 on is InferStep's of the same name, for every slot: slot 0's constructor refuses what cannot run
        options = {k: v for k, v in locals().items() if k not in ("self", "model", "batch", "height", "width", "depth")}
        if depth < 1:
            raise ValueError("depth must be >= 1")
        self.steps = [self._step_class(model, batch, height, width, bn_train=False, slot=i, **options, **self._step_extra) for i in range(depth)]
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
            self._call_step(self.steps[i], images, frames, boxes, frame_index, rot, mirror, dt, surfaces)
            self.events[i] = st.record_event()
        self.count += 1
        return self.count - 1

    def _call_step(self, step, *inputs):
        step(*inputs)

    def result(self, ticket):
        if ticket < self.count - len(self.steps) or ticket >= self.count:
            raise LightHandError(f"ticket {ticket} is not in flight (submitted so far: {self.count}, depth {len(self.steps)})")
        i = ticket % len(self.steps)
        torch.cuda.current_stream().wait_event(self.events[i])
        return self.steps[i].preds, self.steps[i].maxvals

    def map(self, batches):
        """Yields (preds, maxvals) clones for every batch of the iterable, in order, keeping `depth` batches in flight.  A batch is
        an image tensor, or a dict of submit()'s keyword arguments (frames / boxes / frame_index / rot / mirror / dt; ManagedInferPipeline: also detections)."""
        pending = []
        for images in batches:
            pending.append(self.submit(**images) if isinstance(images, dict) else self.submit(images))
            if len(pending) == len(self.steps):
                p, m = self.result(pending.pop(0))
                yield p.clone(), m.clone()
        for t in pending:
            p, m = self.result(t)
            yield p.clone(), m.clone()


class ManagedInferStep(InferStep):
    """InferStep(frames=..., track=True) that manages its tracks on the device: every argument of InferStep, and
    ``manage_tracks=True`` (the default here) or a dict, on top of ``frames=..., track=True`` (``False``: InferStep as it is): lh_tracks_manage runs
    behind lh_keypoints_to_boxes / lh_keypoints_to_rois and in front of lh_one_euro and edits ``next_boxes`` / ``next_rot`` / ``lost`` in
    place, per frame (the slots with that ``frame_index``), so ``advance()`` hands on managed tracks with no host arithmetic.  Of the
    live slots whose keypoint bounds overlap by more than ``dup_overlap`` of the smaller box, the one with the larger sum of confident
    maxvals stays and the others are emptied (``dup_of`` names the winner; a zero box, ``lost`` = 1); a slot lost for ``max_lost``
    replays in a row is emptied too (``lost_count`` counts them; 0: never).  The step owns a detection list of ``max_detections``
    entries, ``det_boxes`` fp32 [K][4] / ``det_frame`` int32 [K] / ``det_score`` fp32 [K], filled through ``detections=(boxes, frame,
    score)`` (n <= K rows; the rest is padded with frame -1): a detection of at least ``det_min_score`` that no kept slot and no
    better detection covers by more than ``match_overlap`` takes the lowest slot of its frame that was not kept -- ``next_boxes`` is its
    box, ``next_rot`` (1, 0), ``seeded`` names it, ``det_state`` says what became of every entry (the slot, -1 invalid, -2 tracked, -3
    repeated, -4 no room) -- and ``lost`` stays 1 for that frame, so the filter starts fresh on the next.  A call without
    ``detections=`` runs with an empty list: a list never seeds twice.  ``reset_tracks(slots=None)`` zeroes ``lost_count``.  The
    defaults (0.5 / 0.5 / 0.0 / 0, MediaPipe's similarity threshold for the overlaps) are a design choice, not measured.  ``mirror`` and
    ``frame_index`` stay the caller's; topdown.manage_tracks_host states the rule.
    Motion-aware tracking, opt-in and with or without ``manage_tracks`` (both None: the launches above, nothing else):
    ``motion=True`` or a dict, on top of ``frames=..., track=True``: lh_rois_predict runs behind the launches above and in front of the
    filter and moves ``next_boxes`` to where the hand will be -- the box's centre is differenced against the last one over ``dt``,
    low-passed at ``cutoff`` Hz (the One-Euro derivative filter) into ``velocity`` (fp32 [batch][2], frame px / s), and the box is
    shifted by ``lead`` x velocity x dt, at most ``max_shift`` of its larger side per axis; a lost slot moves on along its last
    velocity for up to ``coast`` replays in a row (``coasted`` counts them) before the track is forgotten.  An empty slot, one that
    track management emptied or a detection just seeded, and a ``dt`` that is not finite and > 0 start the predictor fresh;
    ``reset_motion(slots=None)`` does the same by hand.  ``next_rot``, ``lost`` and ``advance()`` are untouched, a translation serves
    upright and oriented ROIs alike, and coasting moves the box but invents no keypoints.  ``step.dt`` and ``dt=`` exist with
    ``motion`` as with ``smooth``.  topdown.rois_predict_host states the rule.
    ``smooth_gate=True`` or a dict, on top of ``smooth=``: lh_one_euro_gated runs in lh_one_euro's place.  A joint whose maxval is
    below ``min_score`` (default: ``track_min_score``) holds its filtered position instead of dragging the filter after a guess, and
    its next confident frame is filtered over the whole time it was away; with ``by_size`` (default True) ``beta`` multiplies a
    speed in hand sizes per second (the larger side of ``next_boxes``, or of ``boxes`` without ``track``, at least 1 px), so one
    ``beta`` serves near and far hands.  With ``min_score=-3.0e38, by_size=False`` it is lh_one_euro bit for bit.
    topdown.one_euro_gated_host states the rule.  The defaults of both (10 Hz / 1.0 / 0.5 / 0; ``track_min_score`` / True) are design
    choices, not measured.
    Skeleton overlay, opt-in on top of ``frames=`` and with or without ``track`` / ``manage_tracks`` / ``motion`` / ``smooth`` (None: the
    launches above, nothing else, nothing allocated): ``overlay=True`` or a dict makes lh_draw_hands the LAST launch of the graph,
    behind the filter: every slot's ROI outline (the crop's quad through ``plan.crop_mat``, so oriented and mirrored ROIs come out
    turned; a lost slot draws it alone, in the palette's last row), bones and joint discs are drawn into the frames in place, on the
    pixels around each hand only -- no pass over whole frames, no copy to the host.  The dict: ``min_score`` (default
    ``track_min_score``) gates joints and bones, ``line_radius`` (1.0) / ``joint_radius`` (2.5) in frame pixels plus ``by_size`` (0.0)
    times the larger side of the slot's box, ``opacity`` (1.0), ``draw_roi`` (True), ``source`` "raw" (``preds``) or "smooth"
    (``smooth_preds``; needs ``smooth=``), ``parents`` / ``groups`` (int [j]; default: the 21-joint hand tree, topdown.HAND_PARENTS /
    HAND_GROUPS) and ``palette`` (fp32 [n_groups + 2][3] in the frames' own plane space, topdown.overlay_palette converts RGB rows;
    the last two rows colour the outline of a live and of a lost slot).  ``target`` "inplace" draws on what the crop read
    (``step.frames``, or the bound surfaces under ``surfaces=True``); "surfaces" draws on a second table, ``bind_overlay_surfaces(tensors,
    start=0)`` / ``unbind_overlay_surfaces()``, for callers whose source frames must stay clean (a decoder's reference frames): the
    kernel never reads the source, so the caller decides what a destination holds beforehand, and an unbound destination is skipped.
    In-place drawing changes what a later replay crops if the caller does not bring new frames; a surface may be reused only after
    the step's stream has passed the replay; chroma siting is ignored (a chroma texel takes the mean coverage of its 2 x 2 luma
    block).  The eager run in front of the capture draws nothing, so the first call draws once.  ``step.overlay`` keeps the resolved
    options (None when off); topdown.draw_hands_host states the rule.
    The keywords live on this class, so InferStep's own signatures stay as they are."""

    def __init__(self, *args, manage_tracks=True, motion=None, smooth_gate=None, overlay=None, **kwargs):
        self._manage_tracks_option, self._motion_option, self._smooth_gate_option = manage_tracks, motion, smooth_gate
        self._overlay_option = overlay
        super().__init__(*args, **kwargs)

    def __call__(self, *args, detections=None, **kwargs):
        if detections is not None and not self.manage_tracks:
            raise ValueError("detections are the input of ManagedInferStep(frames=..., track=True, manage_tracks=True)")
        self._detections = detections
        try:
            return super().__call__(*args, **kwargs)
        finally:
            self._detections = None


class ManagedInferPipeline(InferPipeline):
    """InferPipeline whose slots are ManagedInferSteps: every argument of InferPipeline and ``manage_tracks`` as ManagedInferStep's, for
    every slot.  Every slot owns its detection list and its ``lost_count``; ``submit(detections=...)`` fills the list of the slot that
    runs the ticket (``steps[i].dup_of`` / ``seeded`` / ``det_state`` / ``reset_tracks()``).  ``motion`` / ``smooth_gate``: as
    ManagedInferStep's, for every slot; every slot owns its motion state and its filter state (``steps[i].velocity`` / ``coasted`` /
    ``reset_motion()``).  ``overlay``: as ManagedInferStep's, for every slot; every slot draws on its own frames (or its own
    overlay table: ``steps[i].bind_overlay_surfaces``)."""

    _step_class = ManagedInferStep

    def __init__(self, *args, manage_tracks=True, motion=None, smooth_gate=None, overlay=None, **kwargs):
        self._step_extra = dict(manage_tracks=manage_tracks, motion=motion, smooth_gate=smooth_gate, overlay=overlay)
        self._detections = None
        super().__init__(*args, **kwargs)

    def submit(self, *args, detections=None, **kwargs):
        self._detections = detections
        try:
            return super().submit(*args, **kwargs)
        finally:
            self._detections = None

    def _call_step(self, step, *inputs):
        for t in self._detections if isinstance(self._detections, (tuple, list)) else ():
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(torch.cuda.current_stream())       # the slot's copy of the list runs on its stream: as submit()'s inputs
        step(*inputs, detections=self._detections)
