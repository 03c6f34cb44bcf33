"""CPU: lighthand_amd.runtime as the import surface of the modules it was split into -- the names callers import from it, the
signatures of the steps (literal lists, copied from runtime.py as it was in one file) -- and the single call of
Plan.use_frame_input: the full keyword set the steps now always pass binds to the same arguments as the keyword sets they used to
choose by hand, for every frame format, with and without surfaces, a layout, roi_aug and crop_jitter."""
import inspect
import itertools

import pytest

REQ = inspect.Parameter.empty
YUV = ("bt709", "limited")
_FRAME_TAIL = [("frame_format", "rgb"), ("yuv", YUV), ("chroma_siting", "left"), ("frame_layout", None)]
_CALL = [(k, None) for k in ("images", "frames", "boxes", "frame_index", "rot", "mirror", "dt", "surfaces")]
_INFER_FRAMES = [("frames", None), ("box_padding", 1.25), ("track", False), ("track_min_score", 0.1), ("track_min_joints", 8),
                 ("track_min_side", 16.0), ("oriented", False), ("track_axis", (0, 9)), ("track_min_axis", 4.0), ("smooth", None),
                 ("antialias", False)] + _FRAME_TAIL + [("surfaces", False)]
SIGNATURES = {
    ("TrainStep", "__init__"): [
        ("model", REQ), ("batch", REQ), ("height", REQ), ("width", REQ), ("lr", 1e-3), ("betas", (0.9, 0.999)), ("eps", 1e-8), ("optimizer", None),
        ("decode", True), ("use_graph", True), ("grad_sync", None), ("targets_from_joints", True), ("input_u8", None), ("color_jitter", None),
        ("loss_scale", None), ("geometric_aug", None), ("plan_options", None), ("use_target_weight", False), ("ohkm_topk", 0),
        ("target_encoding", "quantised"), ("coord_loss_weight", 0.0), ("soft_argmax_beta", 100.0), ("frames", None), ("box_padding", 1.25),
        ("oriented", False), ("antialias", False)] + _FRAME_TAIL + [("roi_aug", None), ("crop_jitter", None), ("surfaces", False)],
    ("TrainStep", "__call__"): [(k, None) for k in ("images", "joints", "target", "aug", "frames", "boxes", "frame_index", "rot", "mirror",
                                                    "surfaces")],
    ("InferStep", "__init__"): [
        ("model", REQ), ("batch", REQ), ("height", REQ), ("width", REQ), ("bn_train", False), ("use_graph", True), ("input_u8", None), ("slot", 0),
        ("flip_test", False), ("shift_heatmap", True), ("post_process", False), ("plan_options", None), ("blur_kernel", 11),
        ("soft_argmax_beta", 100.0)] + _INFER_FRAMES,
    ("InferStep", "__call__"): _CALL,
    ("InferPipeline", "__init__"): [
        ("model", REQ), ("batch", REQ), ("height", REQ), ("width", REQ), ("depth", 2), ("input_u8", None), ("flip_test", False),
        ("shift_heatmap", True), ("post_process", False), ("blur_kernel", 11), ("soft_argmax_beta", 100.0)] + _INFER_FRAMES,
    ("InferPipeline", "submit"): _CALL,
}
NAMES = ("TrainStep", "InferStep", "InferPipeline", "sample_color_jitter", "sample_affine", "sample_roi_aug", "_antialias_taps",
         "_check_train_frames")


@pytest.mark.parametrize("cls, method", list(SIGNATURES))
def test_signatures_are_the_ones_before_the_split(cls, method):
    from lighthand_amd import runtime
    params = list(inspect.signature(getattr(getattr(runtime, cls), method)).parameters.values())
    assert params[0].name == "self" and all(p.kind is p.POSITIONAL_OR_KEYWORD for p in params)
    assert [(p.name, p.default) for p in params[1:]] == SIGNATURES[cls, method]
    assert all(type(p.default) is type(want) for p, (_, want) in zip(params[1:], SIGNATURES[cls, method]) if want is not REQ)


def test_runtime_exports_every_name_callers_import_and_they_are_the_modules_own():
    from lighthand_amd import draws, frame_input, infer_step, runtime, train_step
    homes = dict(TrainStep=train_step, InferStep=infer_step, InferPipeline=infer_step, sample_color_jitter=draws, sample_affine=draws,
                 sample_roi_aug=draws, _antialias_taps=frame_input, _check_train_frames=frame_input)
    assert sorted(homes) == sorted(NAMES)
    for name in NAMES:
        assert getattr(runtime, name) is getattr(homes[name], name), name
    assert not [n for n, v in vars(runtime).items() if inspect.isfunction(v) and v.__module__ == runtime.__name__]      # re-exports only


# ------------------------------------------------------------------------------------------------ the single use_frame_input call
FRAMES = (3, 96, 128)
PADDING, TAPS = 1.5, 4


def keywords_before_the_split(step, frames, box_padding, oriented, taps, frame_format, yuv, chroma_siting, frame_layout, surfaces, roi_aug,
                              crop_jitter):
    """The keyword arguments TrainStep.__init__ / InferStep.__init__ passed to use_frame_input when each chose what to leave out."""
    if step == "train":
        extra = dict(frame_format="nv12", yuv=yuv, chroma_siting=chroma_siting, frame_layout=frame_layout) if frame_format == "nv12" else {}
        if surfaces or frame_format not in ("rgb", "nv12"):
            extra = dict(frame_format=frame_format, frame_layout=frame_layout, surfaces=surfaces)
            if frame_format != "rgb":
                extra.update(yuv=yuv, chroma_siting=chroma_siting)
        return dict(padding=float(box_padding), oriented=bool(oriented) or roi_aug, max_taps=taps, perturb=roi_aug, **extra,
                    **(dict(jitter=True) if crop_jitter else {}))
    if surfaces or frame_format not in ("rgb", "nv12"):
        extra = dict(frame_format=frame_format, frame_layout=frame_layout, surfaces=surfaces)
        if frame_format != "rgb":
            extra.update(yuv=yuv, chroma_siting=chroma_siting)
        return dict(padding=float(box_padding), oriented=oriented, max_taps=taps, **extra)
    if frame_format == "nv12":
        return dict(padding=float(box_padding), oriented=oriented, max_taps=taps, frame_format="nv12", yuv=yuv, chroma_siting=chroma_siting,
                    frame_layout=frame_layout)
    return dict(padding=float(box_padding), oriented=oriented, max_taps=taps)


class _RecordingPlan:
    boxes = frame_index = rot = mirror = None

    def use_frame_input(self, *args, **kwargs):
        self.calls = getattr(self, "calls", []) + [(args, kwargs)]


def _cases():
    from lighthand_amd import topdown
    for frame_format, surfaces in itertools.product(topdown.FRAME_FORMATS, (False, True)):
        layouts = [None]
        if frame_format != "rgb":
            layouts.append(topdown.frame_layout_of(frame_format, *FRAMES[1:]))
        if frame_format == "nv12":
            layouts.append(topdown.nv12_layout(*FRAMES[1:]))
        for layout in layouts:
            yield frame_format, surfaces, layout


def test_one_call_with_every_keyword_binds_like_the_calls_that_left_keywords_out():
    from lighthand_amd.engine import Plan
    from lighthand_amd.frame_input import FrameInput, _FrameStep
    sig = inspect.signature(Plan.use_frame_input)

    def bound(kwargs):
        b = sig.bind(None, *FRAMES, **kwargs)
        b.apply_defaults()
        return dict(b.arguments)

    seen = 0
    for frame_format, surfaces, layout in _cases():
        yuv, siting = (YUV, "left") if frame_format == "rgb" else (("bt601", "full"), "center")
        for step, oriented, roi_aug, crop_jitter in itertools.product(("infer", "train"), (False, True), (False, True), (False, True)):
            if step == "infer" and (roi_aug or crop_jitter):
                continue
            fi = FrameInput.check(FRAMES, None, box_padding=PADDING, oriented=oriented, antialias=TAPS, frame_format=frame_format, yuv=yuv,
                                  chroma_siting=siting, frame_layout=layout, surfaces=surfaces)
            owner = _FrameStep()
            owner.plan = _RecordingPlan()
            owner._use_frame_input(fi, **(dict(perturb=roi_aug, jitter=crop_jitter) if step == "train" else {}))
            (args, kwargs), = owner.plan.calls
            want = keywords_before_the_split(step, FRAMES, PADDING, oriented, TAPS, frame_format, yuv, siting, layout, surfaces, roi_aug,
                                             crop_jitter)
            assert args == FRAMES and bound(kwargs) == bound(want), (step, frame_format, surfaces, layout, oriented, roi_aug, crop_jitter)
            assert owner.surfaces is surfaces and owner.oriented is (oriented or roi_aug) and owner.frame_format == frame_format
            seen += 1
    assert seen == (1 + 3 + 3 * 2) * 2 * (2 + 8)          # layouts of rgb, nv12 and the three others; surfaces; infer and train options


def test_packed_rgb_frames_take_no_layout_with_or_without_surfaces():
    """The one combination of the enumeration that no step accepts: "rgb" has no layout to pass."""
    from lighthand_amd import topdown
    from lighthand_amd.frame_input import FrameInput
    for surfaces in (False, True):
        with pytest.raises(ValueError, match="frame_layout"):
            FrameInput.check(FRAMES, None, frame_layout=topdown.frame_layout_of("rgb", *FRAMES[1:]), surfaces=surfaces)
