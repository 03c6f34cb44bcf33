"""What TrainStep and InferStep share on the way in: the frame-crop options as one validated record (``FrameInput``), the rules that
refuse what cannot run before any device work, and ``_FrameStep``, the part of a step that owns frames / boxes / frame_index /
rot / mirror or a surface table."""
import dataclasses
import numbers

import torch

from . import topdown
from .draws import _is_number, _roi_aug_spec


def _ptr(t):
    return None if t is None else t.data_ptr()


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


def _is_frame_default(key, value):
    default = FrameInput.__dataclass_fields__[key].default
    if default is None or isinstance(default, str):
        return value is None if default is None else value == default
    return isinstance(value, (tuple, list)) and tuple(value) == default


@dataclasses.dataclass(frozen=True)
class FrameInput:
    """The frame-crop options of a step, validated once per constructor: ``frames`` = (n_frames, hs, ws) ints or None (the step takes
    no frames), ``taps`` the resolved ``antialias``, the rest as the steps' arguments of the same names."""
    frames: tuple = None
    box_padding: float = 1.25
    oriented: bool = False
    taps: int = 1
    frame_format: str = "rgb"
    yuv: tuple = ("bt709", "limited")
    chroma_siting: str = "left"
    frame_layout: tuple = None
    surfaces: bool = False

    @classmethod
    def check(cls, frames=None, input_u8=None, box_padding=1.25, oriented=False, antialias=False, frame_format="rgb",
              yuv=("bt709", "limited"), chroma_siting="left", frame_layout=None, surfaces=False):
        """TrainStep / InferStep(frames=, box_padding=, oriented=, antialias=, frame_format=, yuv=, chroma_siting=, frame_layout=,
        surfaces=): refuse what cannot run, before any device work, and return the record.  ``oriented`` without frames is for
        the steps' own rules to refuse (tracking's come first)."""
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
            return cls(None, box_padding, bool(oriented), taps)
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
        return cls(tuple(int(v) for v in frames), float(box_padding), bool(oriented), taps, frame_format, yuv, chroma_siting, frame_layout, surfaces)

    def plan_kwargs(self, perturb=False, jitter=False):
        """The keyword arguments of Plan.use_frame_input behind (n_frames, hs, ws), all of them for every format: the plan reads
        ``yuv`` / ``chroma_siting`` / ``frame_layout`` only where the format has them, and their defaults are the only values ``check``
        lets through elsewhere.  ``perturb`` / ``jitter``: TrainStep's roi_aug / crop_jitter; a turned ROI needs the oriented launch."""
        return dict(padding=self.box_padding, oriented=self.oriented or perturb, max_taps=self.taps, frame_format=self.frame_format,
                    yuv=self.yuv, chroma_siting=self.chroma_siting, frame_layout=self.frame_layout, surfaces=self.surfaces, perturb=perturb,
                    jitter=jitter)


_ORIENTED_WANTS_FRAMES = "oriented=True turns hand ROIs on full frames: pass frames=(n_frames, hs, ws)"


def _check_tracking(model, fi, track, track_min_score, track_min_joints, track_min_side, track_axis, track_min_axis, smooth):
    """InferStep(track=, track_min_*=, oriented=, track_axis=, track_min_axis=, smooth=) behind FrameInput.check: refuse what cannot
    run, before any device work.  The joint count is the model's ``final_layer.out_channels`` (both model families end in that
    convolution); a model without one leaves the upper range of ``track_axis`` to lh_keypoints_to_rois' own argument check.  Returns
    smooth as (min_cutoff, beta, d_cutoff) floats, or None."""
    if track and fi.frames is None:
        raise ValueError("track=True follows hand boxes on full frames: pass frames=(n_frames, hs, ws)")
    if track:
        if not _is_number(track_min_score):
            raise ValueError(f"track_min_score must be a finite number, not {track_min_score!r}")
        if not isinstance(track_min_joints, numbers.Integral) or isinstance(track_min_joints, bool) or track_min_joints < 1:
            raise ValueError(f"track_min_joints must be an integer >= 1, not {track_min_joints!r}")
        if not _is_number(track_min_side) or track_min_side < 0:
            raise ValueError(f"track_min_side must be a finite number >= 0, not {track_min_side!r}")
    if fi.oriented and fi.frames is None:
        raise ValueError(_ORIENTED_WANTS_FRAMES)
    if smooth is not None and fi.frames is None:
        raise ValueError("smooth= filters keypoints in frame coordinates: pass frames=(n_frames, hs, ws)")
    if fi.oriented:
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


MANAGE_TRACKS_MAX = 1024           # slots, and detections, of one lh_tracks_manage launch (its static LDS arrays)


def _check_manage_tracks(fi, track, manage_tracks, batch):
    """ManagedInferStep / ManagedInferPipeline(manage_tracks=) behind _check_tracking: refuse what cannot run, before any device work.  False / None:
    None (the step as it was).  True or a dict of ``max_detections`` (1..1024, default: the batch), ``dup_overlap`` (0.5),
    ``match_overlap`` (0.5), ``det_min_score`` (0.0), ``max_lost`` (0: nothing expires) -> the dict with every key, as ints / floats."""
    if manage_tracks is None or manage_tracks is False:
        return None
    if manage_tracks is not True and not isinstance(manage_tracks, dict):
        raise ValueError(f"manage_tracks must be False, True or a dict of options, not {manage_tracks!r}")
    if not track or fi.frames is None:
        raise ValueError("manage_tracks= manages the slots of a tracked step: pass frames=(n_frames, hs, ws), track=True")
    given = {} if manage_tracks is True else dict(manage_tracks)
    unknown = sorted(set(given) - {"max_detections"} - set(topdown.MANAGE_TRACKS_DEFAULTS), key=str)
    if unknown:
        raise ValueError(f"manage_tracks: unknown keys {unknown!r}; it takes max_detections, " + ", ".join(topdown.MANAGE_TRACKS_DEFAULTS))
    if not isinstance(batch, numbers.Integral) or not 1 <= batch <= MANAGE_TRACKS_MAX:
        raise ValueError(f"manage_tracks serves a batch of 1..{MANAGE_TRACKS_MAX} slots, not {batch!r}")
    out = dict(topdown.MANAGE_TRACKS_DEFAULTS, max_detections=batch)
    out.update(given)
    for key in ("max_detections", "max_lost"):
        v = out[key]
        if not isinstance(v, numbers.Integral) or isinstance(v, bool) or v < 0:
            raise ValueError(f"manage_tracks: {key} must be an integer >= 0, not {v!r}")
        out[key] = int(v)
    if not 1 <= out["max_detections"] <= MANAGE_TRACKS_MAX:
        raise ValueError(f"manage_tracks: max_detections must be within 1..{MANAGE_TRACKS_MAX}, not {out['max_detections']!r}")
    for key in ("dup_overlap", "match_overlap", "det_min_score"):
        v = out[key]
        if not _is_number(v) or v < 0:
            raise ValueError(f"manage_tracks: {key} must be a finite number >= 0, not {v!r}")
        out[key] = float(v)
    return out


def _check_motion(fi, track, motion):
    """ManagedInferStep / ManagedInferPipeline(motion=) behind _check_tracking: refuse what cannot run, before any device work.  None /
    False: None (the step as it was).  True or a dict of ``cutoff`` (Hz, > 0; 10.0), ``lead`` (>= 0; 1.0), ``max_shift`` (>= 0, in box
    sides; 0.5) and ``coast`` (an integer >= 0; 0) -> the dict with every key, as floats / int."""
    if motion is None or motion is False:
        return None
    if motion is not True and not isinstance(motion, dict):
        raise ValueError(f"motion must be None, True or a dict of options, not {motion!r}")
    if not track or fi.frames is None:
        raise ValueError("motion= predicts the next ROI of a tracked step: pass frames=(n_frames, hs, ws), track=True")
    given = {} if motion is True else dict(motion)
    unknown = sorted(set(given) - set(topdown.MOTION_DEFAULTS), key=str)
    if unknown:
        raise ValueError(f"motion: unknown keys {unknown!r}; it takes " + ", ".join(topdown.MOTION_DEFAULTS))
    out = dict(topdown.MOTION_DEFAULTS)
    out.update(given)
    if not _is_number(out["cutoff"]) or not 0 < out["cutoff"] <= 3.0e38:
        raise ValueError(f"motion: cutoff must be a finite number > 0 (Hz), not {out['cutoff']!r}")
    for key in ("lead", "max_shift"):
        if not _is_number(out[key]) or not 0 <= out[key] <= 3.0e38:
            raise ValueError(f"motion: {key} must be a finite number >= 0, not {out[key]!r}")
    if not isinstance(out["coast"], numbers.Integral) or isinstance(out["coast"], bool) or not 0 <= out["coast"] < 2 ** 31:
        raise ValueError(f"motion: coast must be an integer >= 0, not {out['coast']!r}")
    return dict(cutoff=float(out["cutoff"]), lead=float(out["lead"]), max_shift=float(out["max_shift"]), coast=int(out["coast"]))


def _check_smooth_gate(smooth, smooth_gate, track_min_score):
    """ManagedInferStep / ManagedInferPipeline(smooth_gate=) behind _check_tracking (``smooth`` is what it returned): refuse what cannot
    run, before any device work.  None / False: None (lh_one_euro as it was).  True or a dict of ``min_score`` (finite; default: the
    step's ``track_min_score``) and ``by_size`` (a bool; True) -> the dict with both keys."""
    if smooth_gate is None or smooth_gate is False:
        return None
    if smooth_gate is not True and not isinstance(smooth_gate, dict):
        raise ValueError(f"smooth_gate must be None, True or a dict of options, not {smooth_gate!r}")
    if smooth is None:
        raise ValueError("smooth_gate= gates the One-Euro filter: pass frames=(n_frames, hs, ws), smooth=(min_cutoff, beta)")
    given = {} if smooth_gate is True else dict(smooth_gate)
    unknown = sorted(set(given) - {"min_score", "by_size"}, key=str)
    if unknown:
        raise ValueError(f"smooth_gate: unknown keys {unknown!r}; it takes min_score, by_size")
    min_score, by_size = given.get("min_score", track_min_score), given.get("by_size", True)
    if not _is_number(min_score) or abs(min_score) > 3.0e38:
        raise ValueError(f"smooth_gate: min_score must be a finite number, not {min_score!r}")
    if not isinstance(by_size, bool):
        raise ValueError(f"smooth_gate: by_size must be False or True, not {by_size!r}")
    return dict(min_score=float(min_score), by_size=by_size)


def _check_train_frames(model, frames, input_u8=None, geometric_aug=None, color_jitter=None, targets_from_joints=True, roi_aug=None,
                        coord_loss_weight=0.0, use_target_weight=False, crop_jitter=None, **frame_options):
    """TrainStep(frames=, roi_aug=, crop_jitter=) against the step's other options: refuse what cannot run, before any device work (no
    device is touched here).  ``frames`` is a FrameInput, or the ``frames=`` argument itself with ``input_u8`` and the frame-crop
    options as keywords, which FrameInput.check then validates first.  Always returns three values: frames as a tuple of ints or None, the
    roi_aug spec or None, crop_jitter as (brightness, contrast, saturation, hue) floats or None."""
    fi = frames if isinstance(frames, FrameInput) else FrameInput.check(frames, input_u8, **frame_options)
    if fi.frames is None:
        if fi.oriented:
            raise ValueError(_ORIENTED_WANTS_FRAMES)
        if roi_aug is not None:
            raise ValueError("roi_aug perturbs hand ROIs on full frames: pass frames=(n_frames, hs, ws)")
        if crop_jitter is not None:
            raise ValueError("crop_jitter jitters hand ROIs cropped from full frames: pass frames=(n_frames, hs, ws) (color_jitter= is "
                             "the uint8 input's)")
        return None, None, None
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
    if crop_jitter is not None and (not isinstance(crop_jitter, (tuple, list)) or len(crop_jitter) != 4
                                    or not all(_is_number(v) and v >= 0 for v in crop_jitter) or crop_jitter[3] > 0.5):
        raise ValueError(f"crop_jitter must be (brightness, contrast, saturation, hue), torchvision ColorJitter ranges: four finite "
                         f"numbers >= 0, hue <= 0.5, not {crop_jitter!r}")
    return fi.frames, spec, None if crop_jitter is None else tuple(float(v) for v in crop_jitter)


class _FrameStep:
    """The part of TrainStep / InferStep that reads full frames.  ``_use_frame_input`` makes the plan's frame buffers the step's
    inputs; ``_check_call`` / ``_copy_frame_inputs`` are the head of ``__call__``.  bind_surfaces / unbind_surfaces serve a step built
    with ``frames=..., surfaces=True``: it owns no frame buffer but ``plan.surface_table`` (int64 [n_frames] on the device), the
    addresses of the frames, which its crop launch reads at every replay -- so the surfaces change between replays of one captured
    graph with no recapture."""

    surfaces = False
    _surface_refs = None

    def _use_frame_input(self, fi, perturb=False, jitter=False):
        """The one call of Plan.use_frame_input (``perturb`` / ``jitter``: TrainStep's roi_aug / crop_jitter).  Without frames the five
        inputs are None and ``frame_format`` says so; with them ``images`` is None, the inputs of such a step are frames / boxes /
        frame_index."""
        options = fi.plan_kwargs(perturb, jitter)
        self.antialias = fi.taps                                    # samples per crop pixel and axis at most; 1 = the plain crop
        self.frame_format = fi.frame_format if fi.frames else None  # what the frames hold; None: the step takes no frames
        self.oriented = options["oriented"]
        self.frames = self.boxes = self.frame_index = self.rot = self.mirror = None
        if not fi.frames:
            return
        self.images = None
        self.frames = self.plan.use_frame_input(*fi.frames, **options)
        if fi.surfaces:
            self._own_surfaces(fi.frames[0])
        self.boxes, self.frame_index = self.plan.boxes, self.plan.frame_index
        self.rot, self.mirror = self.plan.rot, self.plan.mirror

    @property
    def valid(self):
        """bool [batch]: the slots whose box (ROI) and frame index were usable in the last run (None without ``frames``).  Under
        ``surfaces=True`` it does not say whether the frame's surface was bound: that is the caller's matter."""
        return None if self.frame_format is None else self.plan.src_frame >= 0

    def _check_call(self, others, frames, boxes, frame_index, rot, mirror, surfaces):
        """Refuse the inputs the step was not built for (``others``: the inputs of a step without frames were given) and bind
        ``surfaces``.  The class words the refusals: ``_frame_inputs`` the frame inputs it names, ``_frames_take`` what a step built
        with frames= takes, ``_rot_also`` who else fills rot / mirror, and ``_rot_first`` whether unasked rot / mirror are refused
        before ``surfaces`` are looked at (TrainStep) or after they are bound (InferStep)."""
        no_rot = (rot is not None or mirror is not None) and not self.oriented and ValueError(
            f"rot / mirror are the inputs of {type(self).__name__}(frames=..., oriented=True){self._rot_also}")
        if self.frame_format is None:
            if frames is not None or boxes is not None or frame_index is not None or surfaces is not None or (no_rot and self._rot_first):
                raise ValueError(f"{self._frame_inputs} are the inputs of {type(self).__name__}(frames=(n_frames, hs, ws))")
        elif others:
            raise ValueError(f"a step built with frames= takes {self._frames_take}")
        if no_rot and self._rot_first:
            raise no_rot
        if self.surfaces and frames is not None:
            raise ValueError("a step built with surfaces=True owns no frame buffer: pass surfaces= (or bind_surfaces), not frames=")
        if surfaces is not None:
            self.bind_surfaces(surfaces)                            # refuses a step built without surfaces=True
        if no_rot:
            raise no_rot

    def _copy_frame_inputs(self, frames, boxes, frame_index, rot, mirror):
        for dst, src in ((self.frames, frames), (self.boxes, boxes), (self.frame_index, frame_index), (self.rot, rot), (self.mirror, mirror)):
            if src is not None:
                dst.copy_(src, non_blocking=True)

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
        self._bind_table(self.plan.surface_table, self._surface_refs, self.plan.frame_layout, surfaces, start, "bind_surfaces")

    @staticmethod
    def _bind_table(table, refs, layout, surfaces, start, who):
        """bind_surfaces on one table of addresses and its list of references (InferStep's overlay table is the other one)."""
        rows = torch.is_tensor(surfaces) and surfaces.dim() > 1
        seq = list(surfaces.unbind(0)) if rows else [surfaces] if torch.is_tensor(surfaces) else list(surfaces)
        if isinstance(start, bool) or not isinstance(start, numbers.Integral) or start < 0 or not seq or start + len(seq) > table.shape[0]:
            raise ValueError(f"{who}: {len(seq)} surfaces from frame {start!r} on do not fit the step's {table.shape[0]} frames"
                             + (f" (a tensor {tuple(surfaces.shape)} is bound row by row: pass one surface as [surface])" if rows else ""))
        try:
            addresses = [topdown.check_surface(t, table.device, layout) for t in seq]
        except ValueError as e:
            if rows:                                                # name the likely cause: one surface taken for k rows
                raise ValueError(f"{e} (a tensor {tuple(surfaces.shape)} is bound row by row, {len(seq)} surfaces of "
                                 f"{seq[0].numel()} bytes: pass one surface as [surface])") from None
            raise
        table[start:start + len(seq)].copy_(torch.tensor(addresses, dtype=torch.int64), non_blocking=True)      # from pageable memory
        refs[start:start + len(seq)] = seq

    def unbind_surfaces(self, indices=None):
        """Zero the table entries of ``indices`` (None: all) and drop the references: such a frame is empty, its slots crop black."""
        if not self.surfaces:
            raise ValueError("surfaces are the input of a step built with frames=(n_frames, hs, ws), surfaces=True")
        self._unbind_table(self.plan.surface_table, self._surface_refs, indices, "unbind_surfaces")

    @staticmethod
    def _unbind_table(table, refs, indices, who):
        if indices is None:
            indices = range(table.shape[0])
        indices = [int(i) for i in indices]
        if any(i < 0 or i >= table.shape[0] for i in indices):
            raise ValueError(f"{who}: indices within 0..{table.shape[0] - 1}, not {indices!r}")
        if indices:
            table[torch.tensor(indices, dtype=torch.int64).to(table.device)] = 0
        for i in indices:
            refs[i] = None
