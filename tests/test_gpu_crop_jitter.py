"""GPU: ColorJitter inside the frame crop -- lh_frames_crop_jitter_to_nhwc4 (the grey-mean launch and the jittered crop, both modes of
frames_crop_kernel) against the un-jittered entries (bit for bit where no op runs), against topdown.frames_crop_jitter_host (every op
order, under the criterion of test_color_jitter_input_pipeline_matches_oracle), on the closed-form contrast case, against the uint8
input kernels on whole-frame boxes, and runtime.TrainStep(frames=..., crop_jitter=...) as a captured step.  Inputs:
tests/crop_jitter_data.py (28 slots, 96 x 128 frames, 64 x 64 crops)."""
import numpy as np
import pytest
import torch

import crop_jitter_data as D
from conftest import resnet_cfg

pytestmark = pytest.mark.gpu

F = np.float32
SIZE = (D.SIZE, D.SIZE)
ZERO, ONE = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
_MODELS = {}


@pytest.fixture(autouse=True)
def _static_kernel_choice(monkeypatch):
    monkeypatch.setenv("LH_AUTOTUNE", "0")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _model(precision):
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    if precision not in _MODELS:
        torch.manual_seed(0)
        _MODELS[precision] = get_pose_net(resnet_cfg(18), True).cuda().set_precision(precision)
    return _MODELS[precision]


def _case(case):
    """frames (as the entry reads them), mat, src, the options of frames_crop / frames_crop_jitter_host and of Plan.use_frame_input."""
    from lighthand_amd import topdown as T
    frames = D.frames()
    minified = case in ("antialias", "turned")
    boxes, rot, mirror, index = D.rois(scale=(2.8, 3.2) if minified else (0.4, 1.1))
    if case == "antialias":
        rot[:] = (1, 0)
    mat, src = T.roi_affine_host(boxes, rot, mirror, index, D.N_FRAMES, SIZE, 1.0)
    opts = dict(max_taps=4 if minified else 1)
    if minified:                                              # 3 x minified: every live slot averages taps on both axes
        assert (T.crop_taps_host(mat, 4)[src >= 0] >= 3).all()
    if case == "turned":                                      # |m3| >= 0.25: the tiled walk, for most slots
        assert (np.abs(mat[src >= 0, 3]) >= 0.25).sum() >= 16
    if case == "nv12":
        frames = T.rgb_to_nv12_host(frames)
        opts.update(frame_format="nv12", frame_size=(D.HS, D.WS))
    return frames, (boxes, rot, mirror, index), mat, src, opts


def _nchw(nhwc4):
    return nhwc4[..., :3].permute(0, 3, 1, 2).float().cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. no op: the un-jittered entries' bits
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", ["rgb", "antialias", "nv12", "turned"])
def test_no_op_orders_give_the_unjittered_crop_bit_for_bit(case, precision):
    from lighthand_amd.topdown import frames_crop
    frames, _, mat, src, opts = _case(case)
    factors, _ = D.draw()                                     # non-trivial factors: only the order decides
    order = np.full((D.B, 4), -1, np.int32)
    args = (_cuda(frames), _cuda(mat), _cuda(src), SIZE)
    want = frames_crop(*args, dtype=DTYPES[precision], **opts)
    got = frames_crop(*args, dtype=DTYPES[precision], jitter=(_cuda(factors), _cuda(order)), **opts)
    torch.cuda.synchronize()
    assert got.dtype == DTYPES[precision] and torch.equal(_bits(got), _bits(want))
    assert float(want.float().abs().max()) > 1


# ------------------------------------------------------------------------------------------------ 2. every op order, through a plan
def _plan(case, jitter=True, precision="fp32"):
    _, _, _, _, opts = _case(case)
    plan = _model(precision).eval().plan(D.B, D.SIZE, D.SIZE, training=False, backward=False, owner=("crop-jitter-test", case, jitter))
    extra = dict(frame_format="nv12") if case == "nv12" else {}
    plan.use_frame_input(D.N_FRAMES, D.HS, D.WS, padding=1.0, oriented=True, max_taps=opts["max_taps"], jitter=jitter, **extra)
    return plan


def _run(plan, frames, roi, draw=None):
    boxes, rot, mirror, index = roi
    for dst, a in ((plan.frames_u8, frames), (plan.boxes, boxes), (plan.rot, rot), (plan.mirror, mirror), (plan.frame_index, index)):
        dst.copy_(_cuda(a))
    if draw is not None:
        plan.jitter_factors.copy_(_cuda(draw[0]))
        plan.jitter_order.copy_(_cuda(draw[1]))
    s = torch.cuda.current_stream().cuda_stream
    i = plan._image_call_index
    plan.fwd[i - 1](s)
    plan.fwd[i](s)
    torch.cuda.synchronize()
    return plan.img_nhwc4


@pytest.mark.parametrize("case", ["rgb", "antialias", "nv12"])
def test_every_op_order_matches_the_restatement(case):
    """All 24 permutations, an order with skips, both ends of the 0.5 ranges, a frame of grey pixels and an empty slot, fp32 destination:
    the device against frames_crop_jitter_host -- per slot fewer than 1e-3 of the values off by more than 1e-4, median below 1e-6 (the
    restatement itself keeps within half that share of its fp64 evaluation: tests/test_crop_jitter_host.py).  The padding border and
    channel 3 stay exactly zero, and a second launch on the same inputs returns the same bits (no atomics)."""
    from lighthand_amd import topdown as T
    frames, roi, mat, src, opts = _case(case)
    draw = D.draw()
    plan = _plan(case)
    assert plan.fwd[plan._image_call_index].fn is plan.lib.lh_frames_crop_jitter_to_nhwc4
    img = _run(plan, frames, roi, draw).clone()
    assert torch.equal(_bits(plan.crop_mat), _bits(_cuda(mat))) and torch.equal(plan.src_frame.cpu(), torch.from_numpy(src))
    p = plan.img_pad
    got = _nchw(img[:, p:p + D.SIZE, p:p + D.SIZE])
    want = T.frames_crop_jitter_host(frames, mat, src, SIZE, draw[0], draw[1], **opts)
    share, med = D.mismatch(got, want)
    plain = T.frames_crop_jitter_host(frames, mat, src, SIZE, draw[0], np.full_like(draw[1], -1), **opts)
    print(f"{case}: share of values off by more than 1e-4: {share:.2e} (cap 1e-3), median difference {med:.2e} (cap 1e-6)")
    assert share < 1e-3 and med < 1e-6
    assert np.array_equal(got[24], plain[24]) and np.array_equal(got[5], plain[5])          # no op; the empty slot: normalised black
    assert (np.abs(got - plain).reshape(D.B, -1).max(1)[np.r_[0:5, 6:24, 25:28]] > 0.05).all()
    border = img.clone()
    border[:, p:p + D.SIZE, p:p + D.SIZE, :3] = 0
    assert p >= 1 and not border.any()                        # the padding border and channel 3
    again = _run(plan, frames, roi, draw)
    assert torch.equal(_bits(again), _bits(img))


# ------------------------------------------------------------------------------------------------ 3. the mean covers the whole interior
@pytest.mark.parametrize("f", [0.6, 1.3])
def test_contrast_mean_counts_the_black_outside_closed_form(f):
    """Half the crop's columns lie left of a constant grey frame: mean = 0.5 * gray(c) exactly, inside clamp(f*c + (1-f)*mean), outside
    clamp((1-f)*mean) -- bit for bit, so the mean is the slot's (all 32 partials, the black half included), not one workgroup's share."""
    from lighthand_amd import topdown as T
    fr, boxes, want = D.half_outside_case(f=f)
    mat, src = T.box_affine(_cuda(boxes), torch.zeros(1, dtype=torch.int32).cuda(), 1, SIZE, padding=1.0)
    got = T.frames_crop(_cuda(fr), mat, src, SIZE, mean=ZERO, std=ONE, jitter=(_cuda(F([[1, f, 1, 0]])), _cuda(np.int32([[1, -1, -1, -1]]))))
    torch.cuda.synchronize()
    assert torch.equal(mat.cpu(), torch.tensor([[1.0, 0, -32, 0, 1, 10]]))
    got = _nchw(got)[0]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_empty_slots_stay_exactly_black():
    from lighthand_amd import topdown as T
    frames, _, mat, src, _ = _case("rgb")
    src = src.copy()
    src[[0, 9, 27]] = -1
    factors, order = D.draw()
    order[27] = (1, 3, 0, 2)
    for extra in (dict(), dict(max_taps=4)):
        got = T.frames_crop(_cuda(frames), _cuda(mat), _cuda(src), SIZE, mean=ZERO, std=ONE, jitter=(_cuda(factors), _cuda(order)), **extra)
        torch.cuda.synchronize()
        assert not got[[0, 5, 9, 27]].any() and bool(got[[1, 2, 3]].any())
        assert not got[..., 3].any()


# ------------------------------------------------------------------------------------------------ 4. against the uint8 input kernels
def test_whole_frame_crop_matches_the_uint8_jitter_pipeline():
    """Frames the size of the crop, whole-frame boxes, box_padding 1: the crop matrix is the identity and both pipelines sample the same
    bytes, so lh_frames_crop_jitter_to_nhwc4 and lh_image_u8_jitter_to_nhwc4 agree under the criterion with the same draw.  Their grey
    means are fp64 sums over different partitions (32 strips of rows here, 32 interleaved shares of the walk there): whether the
    images are bit-equal is printed, not asserted."""
    rng = np.random.RandomState(D.SEED + 7)
    u8 = rng.randint(0, 256, size=(D.B, D.SIZE, D.SIZE, 3)).astype(np.uint8)
    u8[1] = u8[1][..., :1]
    draw = D.draw()
    model = _model("fp32").eval()
    a = model.plan(D.B, D.SIZE, D.SIZE, training=False, backward=False, owner=("crop-jitter-test", "u8"))
    a.use_uint8_input(D.SIZE, D.SIZE, jitter=True).copy_(_cuda(u8))
    b = model.plan(D.B, D.SIZE, D.SIZE, training=False, backward=False, owner=("crop-jitter-test", "whole"))
    b.use_frame_input(D.B, D.SIZE, D.SIZE, padding=1.0, jitter=True).copy_(_cuda(u8))
    s = torch.cuda.current_stream().cuda_stream
    for plan in (a, b):
        plan.jitter_factors.copy_(_cuda(draw[0]))
        plan.jitter_order.copy_(_cuda(draw[1]))
    a.fwd[a._image_call_index](s)
    b.fwd[b._image_call_index - 1](s)
    b.fwd[b._image_call_index](s)
    torch.cuda.synchronize()
    assert torch.equal(b.crop_mat.cpu(), torch.tensor([1.0, 0, 0, 0, 1, 0]).expand(D.B, 6))
    share, med = D.mismatch(_nchw(b.img_nhwc4), _nchw(a.img_nhwc4))
    print(f"frame crop vs uint8 pipeline, same draw: share off by more than 1e-4 {share:.2e}, median {med:.2e}, "
          f"bit-equal: {torch.equal(_bits(a.img_nhwc4), _bits(b.img_nhwc4))}")
    assert share < 1e-3 and med < 1e-6


# ------------------------------------------------------------------------------------------------ 5. the captured step
def test_captured_step_with_crop_jitter_and_roi_aug():
    from lighthand_amd.runtime import TrainStep
    frames, (boxes, _, _, index), _, _, _ = _case("rgb")
    index = np.where(index < 0, 0, index).astype(np.int32)
    rng = np.random.RandomState(3)
    centre = (boxes[:, :2] + boxes[:, 2:]) * 0.5
    joints = (centre[:, None, :] + rng.uniform(-12, 12, size=(D.B, 21, 2))).astype(np.float32)
    args = dict(frames=_cuda(frames), boxes=_cuda(boxes), frame_index=_cuda(index), joints=_cuda(joints))

    def build(**kw):
        from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
        torch.manual_seed(1)
        model = get_pose_net(resnet_cfg(18), True).cuda().set_precision("bf16")
        return TrainStep(model, D.B, D.SIZE, D.SIZE, lr=1e-3, frames=(D.N_FRAMES, D.HS, D.WS), roi_aug=(30, 0.25, 0.1, 0.5), **kw)

    def call(st, seed, first=False, **kw):
        st.roi_aug["generator"] = torch.Generator().manual_seed(seed)          # the same ROI draw for both steps
        loss = float(st(**args, **kw) if first else st(**kw))
        torch.cuda.synchronize()
        p = st.plan.img_pad
        return st.plan.img_nhwc4[:, p:p + D.SIZE, p:p + D.SIZE].clone(), loss

    jit, plain = build(crop_jitter=(0.5,) * 4), build()
    assert jit.crop_jitter == (0.5, 0.5, 0.5, 0.5) and plain.crop_jitter is None
    # crop_jitter=None: the launch list of the step as it was; with it, one entry takes the crop's place
    what_jit, what_plain = [getattr(c, "what", None) for c in jit.plan.fwd], [getattr(c, "what", None) for c in plain.plan.fwd]
    i = plain.plan._image_call_index
    assert plain.plan.fwd[i].fn is plain.lib.lh_frames_crop_to_nhwc4 and what_plain[i] == "frame crop input pipeline"
    assert jit.plan.fwd[i].fn is jit.lib.lh_frames_crop_jitter_to_nhwc4 and jit.plan._image_call_index == i
    assert what_jit[:i] + [what_jit[i].replace(" + ColorJitter", "")] + what_jit[i + 1:] == what_plain
    assert not hasattr(plain.plan, "jitter_factors")
    mask = torch.arange(D.B) % 2 == 0
    one, loss1 = call(jit, 1, first=True)
    ref1, _ = call(plain, 1, first=True)
    two, loss2 = call(jit, 2, aug=torch.zeros(D.B, dtype=torch.bool))
    ref2, _ = call(plain, 2)
    three, loss3 = call(jit, 3, aug=mask)
    ref3, _ = call(plain, 3)
    assert jit.graphs is not None and all(np.isfinite(v) for v in (loss1, loss2, loss3))
    assert not torch.equal(one, two) and not torch.equal(two, three) and not torch.equal(one, three)
    live = jit.valid.cpu()
    assert bool(live.all())
    differs = lambda x, y: (_bits(x) != _bits(y)).flatten(1).any(1).cpu()
    assert differs(one, ref1).all()                           # aug=None: every slot is jittered
    assert torch.equal(_bits(two), _bits(ref2))               # aug all false: the step without crop_jitter, bit for bit
    assert torch.equal(differs(three, ref3), mask)            # exactly the masked-out slots are bit-equal
    assert torch.equal(jit.plan.jitter_order[~mask].cpu(), torch.full((int((~mask).sum()), 4), -1, dtype=torch.int32))
