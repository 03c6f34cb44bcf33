"""GPU: decoder surfaces and the 4:2:0 flavours of the frame crop -- lh_frames_crop_surfaces_to_nhwc4 against the numpy restatement
(topdown.frames_crop_yuv420_host; the rule: csrc/frames_crop_kernel.h, above crop_texel) for rgb / nv12 / nv21 / yuv420p / p010, from a frame
buffer and through a surface table; separate surfaces against one contiguous buffer; rebinding under one captured graph; the options
composed; InferPipeline; TrainStep; ColorJitter on a new format; the refusals that need tensors; and the launch lists of steps built
without the new arguments.  Inputs: tests/surfaces_data.py (3 frames of 36 x 52, crop 24 x 40) and, for the steps, R18 at batch 4 on
64 x 64 crops."""
import numpy as np
import pytest
import torch

import crop_jitter_data as J
import surfaces_data as D
from conftest import resnet_cfg
from test_gpu_area_crop import _calls, assert_close, input_caps

pytestmark = pytest.mark.gpu

F = np.float32
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
ALL = ("rgb",) + D.FORMATS
B, SIZE = 4, 64
FRAMES = (D.NF, D.HS, D.WS)
BOXES = [[-0.5, -0.5, D.WS - 0.5, D.HS - 0.5], [4.0, 2.0, 40.0, 30.0], [-10.0, -6.0, 60.0, 44.0], [20.0, 8.0, 50.0, 34.0]]
INDEX = [0, 1, 2, 1]


@pytest.fixture(autouse=True)
def _static_kernel_choice(monkeypatch):
    monkeypatch.setenv("LH_AUTOTUNE", "0")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _model(precision="bf16", seed=0):
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    torch.manual_seed(seed)
    return get_pose_net(resnet_cfg(18), True).cuda().set_precision(precision).eval()


def frame_bytes(fmt, seed=3):
    """(the frames of ``fmt`` as uint8 [NF][bytes], its layout or None for rgb): noise samples; p010 with random low bits."""
    if fmt == "rgb":
        return D.rgb_frames(seed + 1).reshape(D.NF, -1), None
    luma, chroma = D.samples(seed)
    L = D.layouts()[fmt]
    low = np.random.RandomState(seed + 5).randint(0, 64, luma.shape) if fmt == "p010" else None
    return D.pack(L, luma, chroma, low), L


# ------------------------------------------------------------------------------------------------ 1. the kernel against the rule
_WANT = {}


def reference(fmt):
    """(frames, layout, want, dark) of one format on the shared slots, the restatement computed once and left read-only.  Slot 8 names
    frame 3: no such frame in the 3-frame buffer, an unbound entry of the 4-entry table -- black in both."""
    if fmt not in _WANT:
        from lighthand_amd.topdown import crop_taps_host, frames_crop_yuv420_host
        frames, L = frame_bytes(fmt)
        want = frames_crop_yuv420_host(list(frames) + [None], (D.HS, D.WS), D.MAT, D.SRC, (D.H, D.W), fmt, L, max_taps=D.MAX_TAPS)
        want.setflags(write=False)
        _, lit, dark = input_caps(D.MAT, D.SRC, crop_taps_host(D.MAT, D.MAX_TAPS), D.HS, D.WS, D.H, D.W, D.NF)
        assert dark[list(D.DARK_SLOTS)].all() and 0.4 < lit < 0.8
        _WANT[fmt] = (frames, L, want, dark)
    return _WANT[fmt]


def _launch(fmt, frames, L, mode, dtype, mat=D.MAT, src=D.SRC, **kw):
    from lighthand_amd.topdown import frames_crop
    common = dict(max_taps=D.MAX_TAPS, dtype=DTYPES[dtype], frame_format=fmt, frame_size=(D.HS, D.WS), layout=L, **kw)
    if mode == "surfaces":
        out = frames_crop(None, _cuda(mat), _cuda(src), (D.H, D.W), surfaces=[_cuda(f) for f in frames] + [None], **common)
    else:
        buf = _cuda(frames.reshape(D.NF, D.HS, D.WS, 3) if fmt == "rgb" else frames)
        out = frames_crop(buf, _cuda(mat), _cuda(src), (D.H, D.W), **common)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mode", ["buffer", "surfaces"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("fmt", ALL)
def test_crops_match_the_numpy_rule(fmt, dtype, mode):
    """fp32: the restatement's bits.  bf16 / fp16: the criterion of tests/test_gpu_yuv_crop.py (assert_close).  The slots that are
    wholly outside, empty or unbound are exactly black in every dtype."""
    frames, L, want, dark = reference(fmt)
    out = _launch(fmt, frames, L, mode, dtype)
    assert out.shape == (len(D.SRC), D.H, D.W, 4) and out.dtype == DTYPES[dtype]
    got = np.transpose(out.float().cpu().numpy()[..., :3], (0, 3, 1, 2))
    print(f"{fmt} {dtype} {mode}: max |d| {float(np.abs(got - want).max()):.3e}")
    if dtype == "fp32":
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert_close(out, want, dark, dtype, D.H, D.W, 0, f"{fmt} crop from a {mode}")
    black = _launch(fmt, frames, L, mode, dtype, mat=D.MAT[list(D.DARK_SLOTS)], src=D.SRC[list(D.DARK_SLOTS)])
    assert torch.equal(_bits(out[list(D.DARK_SLOTS)]), _bits(black)) and float(black[..., :3].float().abs().min()) > 1.5
    assert torch.equal(_bits(black), _bits(black[:1].expand_as(black).contiguous())) and not bool(black[..., 3].any())


# ------------------------------------------------------------------------------------------------ 2. separate surfaces = one buffer
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("fmt", ["rgb", "nv12"])
def test_separate_surfaces_equal_the_contiguous_buffer(fmt, dtype):
    """The same bytes as three tensors of their own, bound in permuted order with the frame numbers permuted to match; one of them is a
    view that starts at an odd byte offset."""
    from lighthand_amd.topdown import frames_crop
    frames, L = frame_bytes(fmt)
    L = None if fmt == "rgb" else (D.PITCH, D.PITCH * D.LUMA_ROWS, D.PITCH * (D.LUMA_ROWS + D.HS // 2), D.LUMA_ROWS + D.HS // 2)
    buf = _cuda(frames.reshape(D.NF, D.HS, D.WS, 3) if fmt == "rgb" else frames.reshape(D.NF, L[3], L[0]))
    kw = dict(max_taps=D.MAX_TAPS, dtype=DTYPES[dtype], frame_format=fmt, frame_size=(D.HS, D.WS), layout=L)
    want = frames_crop(buf, _cuda(D.MAT), _cuda(D.SRC), (D.H, D.W), **kw)              # the entries that existed
    perm = [2, 0, 1]                                               # table entry i holds frame perm[i]
    odd = torch.empty(frames.shape[1] + 7, dtype=torch.uint8, device="cuda")
    tensors = [_cuda(frames[p]) for p in perm]
    tensors[1] = odd[3:3 + frames.shape[1]].copy_(tensors[1])
    assert tensors[1].data_ptr() % 2 == 1 and tensors[1].is_contiguous()
    where = {p: i for i, p in enumerate(perm)}
    src = np.array([where.get(int(s), s) for s in D.SRC], np.int32)
    got = frames_crop(None, _cuda(D.MAT), _cuda(src), (D.H, D.W), surfaces=tensors, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want)) and float(want.float().abs().max()) > 1


# ------------------------------------------------------------------------------------------------ 3. steps
def _inputs(fmt, seed):
    frames, L = frame_bytes(fmt, seed)
    return frames, L, dict(boxes=torch.tensor(BOXES, dtype=torch.float32).cuda(), frame_index=torch.tensor(INDEX, dtype=torch.int32).cuda())


def _buffer_feed(step, frames):
    return dict(frames=_cuda(frames).reshape(step.frames.shape))


def _same(a, b, extra=()):
    for name in ("heatmaps", "preds", "maxvals", "crop_preds") + tuple(extra):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(_bits(a.plan.img_nhwc4), _bits(b.plan.img_nhwc4)) and torch.equal(a.valid, b.valid)


def test_rebinding_under_one_captured_graph():
    from lighthand_amd.runtime import InferStep
    model = _model()
    surf, buf = InferStep(model, B, SIZE, SIZE, frames=FRAMES, surfaces=True), InferStep(model, B, SIZE, SIZE, frames=FRAMES)
    assert surf.frames is None and surf.surfaces and not buf.surfaces and surf.frame_format == "rgb"
    table = surf.plan.surface_table
    assert table.dtype == torch.int64 and tuple(table.shape) == (D.NF,) and not bool(table.any())
    set_a, _, common = _inputs("rgb", 3)
    set_b, _, _ = _inputs("rgb", 11)
    a = [_cuda(f) for f in set_a]
    surf(surfaces=a, **common)
    buf(**_buffer_feed(buf, set_a), **common)
    torch.cuda.synchronize()
    graph = surf.graph
    assert graph is not None and table.cpu().tolist() == [t.data_ptr() for t in a] and surf.valid.cpu().tolist() == [True] * B
    _same(surf, buf)
    first = surf.heatmaps.clone()
    b = torch.stack([_cuda(f) for f in set_b])                     # one tensor [k][...]: bound row by row
    surf.bind_surfaces(b)
    surf()
    buf(**_buffer_feed(buf, set_b))
    torch.cuda.synchronize()
    assert surf.graph is graph and table.cpu().tolist() == [b[i].data_ptr() for i in range(D.NF)]
    _same(surf, buf)
    assert not torch.equal(surf.heatmaps, first)
    surf.bind_surfaces([a[1]], start=1)                            # one entry: frame 1 of set A among set B
    surf()
    buf(**_buffer_feed(buf, np.stack([set_b[0], set_a[1], set_b[2]])))
    torch.cuda.synchronize()
    _same(surf, buf)
    surf.unbind_surfaces([1])                                      # an unbound frame: its slots crop black, valid keeps its meaning
    surf()
    torch.cuda.synchronize()
    assert surf.graph is graph and table.cpu().tolist()[1] == 0 and surf._surface_refs[1] is None
    p = surf.plan.img_pad
    img = surf.plan.img_nhwc4[:, p:p + SIZE, p:p + SIZE, :3].float()
    assert torch.equal(img[1], img[1][:1, :1].expand_as(img[1])) and torch.equal(img[3], img[1]) and float(img[1].abs().min()) > 1.5
    assert torch.equal(_bits(surf.plan.img_nhwc4[0]), _bits(buf.plan.img_nhwc4[0])) and surf.valid.cpu().tolist() == [True] * B
    surf.unbind_surfaces()
    assert not bool(table.any()) and surf._surface_refs == [None] * D.NF


def test_options_compose_on_surfaces():
    from lighthand_amd.runtime import InferStep
    model = _model()
    frames, L, common = _inputs("yuv420p", 5)
    options = dict(frames=FRAMES, oriented=True, track=True, antialias=4, flip_test=True, frame_format="yuv420p", frame_layout=L,
                   track_min_score=-1.0)
    surf, buf = InferStep(model, B, SIZE, SIZE, surfaces=True, **options), InferStep(model, B, SIZE, SIZE, **options)
    assert tuple(buf.frames.shape) == (D.NF, L.frame_bytes) and buf.frames.dtype == torch.uint8 and surf.antialias == 4
    rot = torch.tensor([[1.0, 0.0], [0.6, 0.8], [-3.0, 0.5], [0.0, -1.0]]).cuda()
    mirror = torch.tensor([0, 1, 0, 1], dtype=torch.int32).cuda()
    surf(surfaces=[_cuda(f) for f in frames], rot=rot, mirror=mirror, **common)
    buf(frames=_cuda(frames), rot=rot, mirror=mirror, **common)
    torch.cuda.synchronize()
    _same(surf, buf, ("next_boxes", "next_rot", "lost"))
    assert surf.lost.cpu().tolist() == [0] * B and float(surf.heatmaps.float().abs().max()) > 0


def test_pipeline_binds_on_the_slot_that_runs_the_ticket():
    from lighthand_amd.runtime import InferPipeline, InferStep
    model = _model()
    options = dict(frames=FRAMES, frame_format="nv21", frame_layout=D.layouts()["nv21"], antialias=True)
    ref = InferStep(model, B, SIZE, SIZE, **options)
    batches, want = [], []
    for seed in (40, 41, 42):
        frames, _, common = _inputs("nv21", seed)
        ref(frames=_cuda(frames), **common)
        torch.cuda.synchronize()
        want.append((ref.preds.clone(), ref.maxvals.clone()))
        batches.append(dict(surfaces=[_cuda(f) for f in frames], **common))
    pipe = InferPipeline(model, B, SIZE, SIZE, depth=2, surfaces=True, **options)
    assert [s.surfaces for s in pipe.steps] == [True, True] and all(s.frames is None for s in pipe.steps)
    got = list(pipe.map(batches))
    assert len(got) == 3 and all(torch.equal(g[0], w[0]) and torch.equal(g[1], w[1]) for g, w in zip(got, want))
    assert not torch.equal(want[0][0], want[1][0])
    with pytest.raises(ValueError, match="surfaces"):
        pipe.submit(frames=_cuda(frame_bytes("nv21")[0]))


def test_train_step_on_surfaces():
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    from lighthand_amd.runtime import TrainStep
    frames, L, common = _inputs("nv21", 7)
    rng = np.random.RandomState(2)
    centre = (np.asarray(BOXES)[:, :2] + np.asarray(BOXES)[:, 2:]) * 0.5
    joints = _cuda((centre[:, None, :] + rng.uniform(-6, 6, size=(B, 21, 2))).astype(np.float32))

    def build(**kw):
        torch.manual_seed(1)
        model = get_pose_net(resnet_cfg(18), True).cuda().set_precision("bf16")
        return TrainStep(model, B, SIZE, SIZE, lr=1e-3, frames=FRAMES, frame_format="nv21", frame_layout=L, roi_aug=(30, 0.25, 0.1, 0.5),
                         crop_jitter=(0.5, 0.5, 0.5, 0.5), **kw)
    surf, buf = build(surfaces=True), build()
    assert surf.frames is None and surf.surfaces and tuple(buf.frames.shape) == (D.NF, L.frame_bytes)
    i = surf.plan._image_call_index
    assert surf.plan.fwd[i].fn is surf.lib.lh_frames_crop_surfaces_to_nhwc4 is buf.plan.fwd[i].fn and "ColorJitter" in surf.plan.fwd[i].what
    for n, seed in enumerate((5, 6)):
        feeds = (dict(surfaces=[_cuda(f) for f in frames]), dict(frames=_cuda(frames))) if n == 0 else ({}, {})
        first = dict(joints=joints, **common) if n == 0 else {}
        out = []
        for st, feed in zip((surf, buf), feeds):
            torch.manual_seed(seed)                                # the ROI and ColorJitter draws of both steps
            loss = float(st(**first, **feed))
            torch.cuda.synchronize()
            out.append((loss, st.preds.clone(), st.maxvals.clone(), st.joints_crop.clone(), st.plan.img_nhwc4.clone()))
        assert np.isfinite(out[0][0]) and out[0][0] == out[1][0]
        assert all(torch.equal(x, y) for x, y in zip(out[0][1:4], out[1][1:4])) and torch.equal(_bits(out[0][4]), _bits(out[1][4]))
    assert surf.graphs is not None and bool(surf.valid.all())
    with pytest.raises(ValueError, match="surfaces"):
        surf(frames=_cuda(frames))


# ------------------------------------------------------------------------------------------------ 4. ColorJitter on a new format
def test_jittered_crop_of_planar_surfaces_matches_the_restatement():
    """tests/test_gpu_crop_jitter.py's inputs (28 ROIs on 96 x 128 frames, every op order) as yuv420p surfaces, under its criterion:
    per slot fewer than 1e-3 of the values off by more than 1e-4, median below 1e-6."""
    from lighthand_amd import topdown as T
    L = T.yuv420_layout("yuv420p", J.HS, J.WS, J.WS + 16, J.HS + 2, J.WS // 2 + 6)
    frames = T.rgb_to_yuv420_host(J.frames(), "yuv420p", layout=L)
    boxes, rot, mirror, index = J.rois()
    mat, src = T.roi_affine_host(boxes, rot, mirror, index, J.N_FRAMES, (J.SIZE, J.SIZE), 1.0)
    factors, order = J.draw()
    kw = dict(frame_format="yuv420p", frame_size=(J.HS, J.WS), layout=L)
    want = T.frames_crop_jitter_host(list(frames), mat, src, (J.SIZE, J.SIZE), factors, order, **kw)
    got = T.frames_crop(None, _cuda(mat), _cuda(src), (J.SIZE, J.SIZE), surfaces=[_cuda(f) for f in frames],
                        jitter=(_cuda(factors), _cuda(order)), **kw)
    torch.cuda.synchronize()
    got = got[..., :3].permute(0, 3, 1, 2).float().cpu().numpy()
    share, med = J.mismatch(got, want)
    print(f"yuv420p surfaces + ColorJitter: share of values off by more than 1e-4: {share:.2e} (cap 1e-3), median {med:.2e} (cap 1e-6)")
    assert share < 1e-3 and med < 1e-6
    plain = T.frames_crop_jitter_host(list(frames), mat, src, (J.SIZE, J.SIZE), factors, np.full_like(order, -1), **kw)
    assert np.array_equal(got[24], plain[24]) and np.array_equal(got[5], plain[5])          # no op; the empty slot
    assert (np.abs(got - plain).reshape(J.B, -1).max(1)[np.r_[0:5, 6:24, 25:28]] > 0.05).all()


# ------------------------------------------------------------------------------------------------ 5. the refusals that need tensors
def test_bind_surfaces_refuses_and_writes_nothing():
    from lighthand_amd.runtime import InferStep
    from lighthand_amd.topdown import surface_bytes
    model = _model()
    frames, L, _ = _inputs("p010", 3)
    step = InferStep(model, B, SIZE, SIZE, frames=FRAMES, frame_format="p010", frame_layout=L, surfaces=True)
    good = [_cuda(f) for f in frames]
    step.bind_surfaces(good)
    torch.cuda.synchronize()
    before, refs = step.plan.surface_table.cpu().tolist(), list(step._surface_refs)
    need = surface_bytes(L)
    wide = torch.zeros(need, 2, dtype=torch.uint8, device="cuda")
    odd = torch.zeros(need + 2, dtype=torch.uint8, device="cuda")[1:need + 1]
    for bad, word in ((torch.from_numpy(frames[0]), "cuda"), (good[0][:need - 1], "bytes"), (wide[:, 0], "contiguous"),
                      (torch.zeros(need, dtype=torch.int8, device="cuda"), "uint8"), (odd, "aligned"), (frames[0], "tensor")):
        with pytest.raises(ValueError, match=word):
            step.bind_surfaces([good[1], bad], start=1)             # the good one in front is not written either
    with pytest.raises(ValueError, match="fit"):
        step.bind_surfaces(good, start=1)
    with pytest.raises(ValueError, match="row by row"):              # ONE surface with two dimensions is taken for two short ones
        step.bind_surfaces(good[0].reshape(2, -1))
    with pytest.raises(ValueError, match="surfaces"):
        step(frames=_cuda(frames))
    torch.cuda.synchronize()
    assert step.plan.surface_table.cpu().tolist() == before and all(x is y for x, y in zip(step._surface_refs, refs))
    assert good[0][:need].numel() == need and step.bind_surfaces([good[0][:need]]) is None          # exactly enough bytes
    plain = InferStep(model, B, SIZE, SIZE, frames=FRAMES)
    with pytest.raises(ValueError, match="surfaces"):
        plain(surfaces=good)
    with pytest.raises(ValueError, match="surfaces"):
        plain.bind_surfaces(good)
    with pytest.raises(ValueError):
        InferStep(model, B, SIZE, SIZE)(surfaces=good)


# ------------------------------------------------------------------------------------------------ 6. nothing moved
def test_steps_without_the_new_arguments_keep_their_launch_list():
    """Steps built without surfaces= and with frame_format "rgb" / "nv12" enqueue what they always did -- lh_frames_crop_to_nhwc4 with
    its 15 bound arguments, lh_frames_crop_yuv_to_nhwc4 for NV12, lh_frames_crop_jitter_to_nhwc4 under crop_jitter -- and own the
    buffers they owned; the new options change that one launch."""
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    from lighthand_amd.runtime import InferStep, TrainStep
    model = _model()
    plain, off = InferStep(model, B, SIZE, SIZE, frames=FRAMES), InferStep(model, B, SIZE, SIZE, frames=FRAMES, frame_format="rgb", surfaces=False)
    rows = _calls(plain.plan)
    assert _calls(off.plan) == rows and tuple(plain.frames.shape) == (D.NF, D.HS, D.WS, 3)
    assert plain.plan.surface_table is None and plain.plan.frame_layout is None and not plain.surfaces
    names = [r[0] for r in rows]
    i = names.index("lh_frames_crop_to_nhwc4")
    assert names.count("lh_frames_crop_to_nhwc4") == 1 and not any("surfaces" in n or "yuv" in n or "area" in n for n in names)
    assert names[i - 1] == "lh_box_affine" and rows[i][1] == "frame crop input pipeline" and len(plain.plan.fwd[i].args) == 15
    assert rows[i][2][:8] == (B, D.NF, D.HS, D.WS, SIZE, SIZE, plain.plan.img_pad, plain.plan.img_wp)
    nv12 = _calls(InferStep(model, B, SIZE, SIZE, frames=FRAMES, frame_format="nv12").plan)
    swapped = list(rows)
    swapped[i] = ("lh_frames_crop_yuv_to_nhwc4", "NV12 frame crop input pipeline",
                  (B, D.NF, D.HS, D.WS, D.WS, D.HS * D.WS, D.HS * D.WS * 3 // 2, 0, SIZE, SIZE, plain.plan.img_pad, plain.plan.img_wp, 1) + rows[i][2][8:])
    assert nv12 == swapped
    for kw, what in ((dict(surfaces=True), "rgb frame crop input pipeline, surface table"), (dict(frame_format="yuv420p"), "yuv420p frame crop input pipeline"),
                     (dict(frame_format="nv12", surfaces=True, antialias=True), "nv12 frame crop input pipeline, surface table, antialiased")):
        new = _calls(InferStep(model, B, SIZE, SIZE, frames=FRAMES, **kw).plan)
        assert [r[0] for r in new] == [n.replace("lh_frames_crop_to_nhwc4", "lh_frames_crop_surfaces_to_nhwc4") for n in names] and new[i][1] == what
        assert new[:i] == rows[:i] and new[i + 1:] == rows[i + 1:]
    torch.manual_seed(1)
    train = get_pose_net(resnet_cfg(18), True).cuda().set_precision("bf16")
    step = TrainStep(train, B, SIZE, SIZE, lr=1e-3, frames=FRAMES, roi_aug=(30, 0.25, 0.1, 0.5), crop_jitter=(0.5,) * 4)
    t = [r[0] for r in _calls(step.plan)]
    assert t.count("lh_frames_crop_jitter_to_nhwc4") == 1 and not any("surfaces" in n for n in t) and tuple(step.frames.shape) == (D.NF, D.HS, D.WS, 3)
