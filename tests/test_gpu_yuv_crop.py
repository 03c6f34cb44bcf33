"""GPU: the frame crop on NV12 frames -- lh_frames_crop_yuv_to_nhwc4 against the RGB entries on grey frames (the same bits), a pitched
surface against the tight layout, the numpy restatement frames_crop_nv12_host of lighthand_amd.topdown (the rule: csrc/frames_crop_kernel.h,
above crop_sample_nv12), and InferStep / InferPipeline(frame_format="nv12") and the track_frames tool on top of it.  Shapes and slots are
tests/test_gpu_area_crop.py's: 3 frames of 150 x 210, crop 24 x 40, pad 3, 32 slots; so is the tolerance scheme (assert_close)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_area_crop import (B, FH, FW, H, HS, INDEX, LARGE, NF, PAD, SIZE, W, WS, _area, _border_is_zero, _calls, _dev, assert_close,
                                input_caps, slots)
from test_gpu_topdown import DT, MEAN, STD, _bits, _crop, _lib, _model, _stream

pytestmark = pytest.mark.gpu

SITING = {"left": 0, "center": 1}


def _yuv(frames_d, hs, ws, mat_d, src_d, h, w, pad, dtype, max_taps, yuv=("bt709", "limited"), siting="left", layout=None, wp=None):
    """lh_frames_crop_yuv_to_nhwc4 on a NaN-filled output; returns the padded NHWC4 buffer."""
    from lighthand_amd.topdown import nv12_layout, yuv_matrix
    L, lib = _lib()
    pitch, uv_offset, frame_stride, rows = layout or nv12_layout(hs, ws)
    assert tuple(frames_d.shape[1:]) == (rows, pitch) and frames_d.dtype == torch.uint8 and frames_d.is_contiguous()
    b = mat_d.shape[0]
    wp = wp or w + 2 * pad + 2
    code, tdt = DT[dtype]
    out = torch.full((b, h + 2 * pad, wp, 4), float("nan"), dtype=tdt, device="cuda")
    m3, s3, csc = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD), (C.c_float * 12)(*yuv_matrix(*yuv).tolist())
    L.check(lib.lh_frames_crop_yuv_to_nhwc4(frames_d.data_ptr(), out.data_ptr(), b, frames_d.shape[0], hs, ws, pitch, uv_offset, frame_stride,
                                            SITING[siting], csc, h, w, pad, wp, m3, s3, mat_d.data_ptr(), src_d.data_ptr(), max_taps, code,
                                            _stream()), "lh_frames_crop_yuv_to_nhwc4")
    torch.cuda.synchronize()
    return out


def _grey(n, hs, ws, seed):
    """Random luma, CbCr = 128, tight layout -> (NV12 frames [n][hs*3/2][ws], the same frames as grey RGB [n][hs][ws][3])."""
    luma = np.random.RandomState(seed).randint(0, 256, size=(n, hs, ws)).astype(np.uint8)
    nv = np.full((n, hs * 3 // 2, ws), 128, np.uint8)
    nv[:, :hs] = luma
    return nv, np.ascontiguousarray(np.repeat(luma[..., None], 3, 3))


def _noise(n, hs, ws, seed):
    """Random Y and CbCr, tight layout."""
    return np.random.RandomState(seed).randint(0, 256, size=(n, hs * 3 // 2, ws)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ 1. grey frames = the RGB entries
@pytest.mark.parametrize("oriented", [False, True], ids=["boxes", "rois"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_grey_frames_are_bit_equal_to_the_rgb_entries(dtype, oriented):
    """CbCr = 128 at full range: the whole buffer -- padding and channel 3 included -- has lh_frames_crop_to_nhwc4's bits at max_taps = 1
    and lh_frames_crop_area_to_nhwc4's at 8, on the 32 slots (up to 8 x minified, two empty, one naming a missing frame)."""
    nv, rgb = _grey(NF, HS, WS, 5)
    mat, src = slots(oriented)
    assert len(src) == 32 and (src < 0).sum() >= 2
    nv_d, rgb_d, mat_d, src_d = torch.from_numpy(nv).cuda(), torch.from_numpy(rgb).cuda(), _dev(mat, np.float32), _dev(src, np.int32)
    plain, area = _crop(rgb_d, mat_d, src_d, H, W, PAD, dtype), _area(rgb_d, mat_d, src_d, H, W, PAD, dtype, 8)
    assert not torch.equal(_bits(plain), _bits(area)) and _border_is_zero(plain, H, W, PAD)
    for standard, siting in (("bt601", "left"), ("bt709", "center")):
        one = _yuv(nv_d, HS, WS, mat_d, src_d, H, W, PAD, dtype, 1, (standard, "full"), siting)
        eight = _yuv(nv_d, HS, WS, mat_d, src_d, H, W, PAD, dtype, 8, (standard, "full"), siting)
        assert torch.equal(_bits(one), _bits(plain)), (standard, siting)
        assert torch.equal(_bits(eight), _bits(area)), (standard, siting)


# ------------------------------------------------------------------------------------------------ 2. a pitched surface
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_pitched_layout_is_bit_equal_to_the_tight_one(dtype):
    """pitch = ws + 22, luma_rows = hs + 6, every byte beside the planes 0xFF: the tight layout's bits, so nothing beside a plane is
    read (a read of a gap byte would change a value: the frames are noise, and so is the chroma)."""
    from lighthand_amd.topdown import nv12_layout
    tight = _noise(NF, HS, WS, 9)
    layout = nv12_layout(HS, WS, WS + 22, HS + 6)
    assert layout == (WS + 22, (WS + 22) * (HS + 6), (WS + 22) * (HS + 6 + HS // 2), HS + 6 + HS // 2)
    wide = np.full((NF, layout[3], layout[0]), 0xFF, np.uint8)
    wide[:, :HS, :WS], wide[:, HS + 6:, :WS] = tight[:, :HS], tight[:, HS:]
    mat, src = slots(True)
    mat_d, src_d = _dev(mat, np.float32), _dev(src, np.int32)
    for taps in (1, 8):
        a = _yuv(torch.from_numpy(tight).cuda(), HS, WS, mat_d, src_d, H, W, PAD, dtype, taps)
        b = _yuv(torch.from_numpy(wide).cuda(), HS, WS, mat_d, src_d, H, W, PAD, dtype, taps, layout=layout)
        assert not bool(torch.isnan(a.float()).any()) and torch.equal(_bits(a), _bits(b)), taps
        shifted = wide.copy()
        shifted[:, :HS, :WS] = 255 - shifted[:, :HS, :WS]           # ... and the comparison can fail: other luma, other bits
        assert not torch.equal(_bits(_yuv(torch.from_numpy(shifted).cuda(), HS, WS, mat_d, src_d, H, W, PAD, dtype, taps, layout=layout)), _bits(a))


# ------------------------------------------------------------------------------------------------ 3. against frames_crop_nv12_host
_REFERENCE = {}


def reference(siting, taps, oriented):
    """(frames, mat, src, want, dark) of one 32-slot set on noise frames, BT.709 limited, computed once.  The rule is continuous in the
    sample position except at the frame's edge (the chroma clamp and every floor are continuous), so the caps the tolerance rests on are
    input_caps' of the RGB comparison; they are asserted here, from numpy alone."""
    key = (siting, taps, oriented)
    if key not in _REFERENCE:
        from lighthand_amd.topdown import crop_taps_host, frames_crop_nv12_host
        frames = _noise(NF, HS, WS, 9)
        mat, src = slots(oriented)
        k = crop_taps_host(mat, taps)
        near, lit, dark = input_caps(mat, src, k, HS, WS, H, W, NF)
        print(f"slots (oriented={oriented}, max_taps={taps}): edge share {near:.2e}, inside share {lit:.3f}")
        assert len(src) == 32 and near <= 1e-3 and 0.2 < lit < 0.8
        assert dark[src < 0].all() and dark[31].all() and dark.sum() > 4 * H * W
        want = frames_crop_nv12_host(frames, (HS, WS), mat, src, (H, W), ("bt709", "limited"), siting, max_taps=taps)
        want.setflags(write=False)
        _REFERENCE[key] = (frames, mat, src, want, dark)
    return _REFERENCE[key]


CASES = [(d, s, t, False) for d in ("fp32", "bf16", "fp16") for s in ("left", "center") for t in (1, 8)] + \
        [("fp32", s, 8, True) for s in ("left", "center")]


@pytest.mark.parametrize("dtype,siting,taps,oriented", CASES, ids=[f"{d}-{s}-{t}-{'rois' if o else 'boxes'}" for d, s, t, o in CASES])
def test_nv12_crops_match_the_numpy_rule(dtype, siting, taps, oriented):
    frames, mat, src, want, dark = reference(siting, taps, oriented)
    frames_d, mat_d, src_d = torch.from_numpy(frames).cuda(), _dev(mat, np.float32), _dev(src, np.int32)
    out = _yuv(frames_d, HS, WS, mat_d, src_d, H, W, PAD, dtype, taps, siting=siting)
    got = np.transpose(out.float().cpu().numpy()[:, PAD:PAD + H, PAD:PAD + W, :3], (0, 3, 1, 2))
    print(f"NV12 crop {dtype} {siting} taps {taps}: max |d| {float(np.abs(got - want).max()):.3e}"
          + (f", bit-equal: {np.array_equal(got.view(np.int32), want.view(np.int32))}" if dtype == "fp32" else ""))
    assert_close(out, want, dark, dtype, H, W, PAD, f"NV12 crop {siting} taps {taps}")
    if dtype == "fp32" and not oriented:                           # the eager form is the same launch: no padding, wp = w
        from lighthand_amd.topdown import frames_crop
        eager = frames_crop(frames_d, mat_d, src_d, (H, W), max_taps=taps, frame_format="nv12", frame_size=(HS, WS), chroma_siting=siting)
        torch.cuda.synchronize()
        assert eager.shape == (32, H, W, 4) and eager.dtype == torch.float32
        assert torch.equal(_bits(eager), _bits(out[:, PAD:PAD + H, PAD:PAD + W].contiguous()))
        with pytest.raises(ValueError, match="frame_format"):
            frames_crop(frames_d, mat_d, src_d, (H, W), frame_format="i420", frame_size=(HS, WS))


# ------------------------------------------------------------------------------------------------ 4. InferStep(frame_format="nv12")
def _grey_inputs(boxes, seed=31):
    nv, rgb = _grey(NF, FH, FW, seed)
    common = dict(boxes=torch.tensor(boxes, dtype=torch.float32).cuda(), frame_index=torch.tensor(INDEX, dtype=torch.int32).cuda())
    return dict(frames=torch.from_numpy(nv).cuda(), **common), dict(frames=torch.from_numpy(rgb).cuda(), **common)


def _same_step(a, b):
    assert torch.equal(_bits(a.plan.img_nhwc4), _bits(b.plan.img_nhwc4))
    assert torch.equal(a.heatmaps, b.heatmaps) and torch.equal(a.preds, b.preds) and torch.equal(a.maxvals, b.maxvals)
    assert torch.equal(a.crop_preds, b.crop_preds) and torch.equal(a.valid, b.valid)


def test_infer_step_nv12_equals_the_rgb_step_on_grey_frames(monkeypatch):
    """InferStep(frame_format="nv12", yuv=("bt601", "full")) on grey NV12 frames against the RGB step on the same grey frames, one
    replay each: the image, heat-maps, preds, crop_preds and valid are bit-equal; with track + oriented + antialias so are next_boxes
    and next_rot."""
    from lighthand_amd.runtime import InferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    frames = (NF, FH, FW)
    nv_in, rgb_in = _grey_inputs(LARGE)
    nv12, rgb = InferStep(model, B, SIZE, SIZE, frames=frames, frame_format="nv12", yuv=("bt601", "full")), InferStep(model, B, SIZE, SIZE, frames=frames)
    assert (nv12.frame_format, rgb.frame_format) == ("nv12", "rgb") and InferStep(model, B, SIZE, SIZE).frame_format is None
    assert tuple(nv12.frames.shape) == (NF, FH * 3 // 2, FW) and nv12.frames.dtype == torch.uint8 and tuple(rgb.frames.shape) == (NF, FH, FW, 3)
    nv12(**nv_in)
    rgb(**rgb_in)
    torch.cuda.synchronize()
    assert nv12.valid.cpu().tolist() == [True] * B
    _same_step(nv12, rgb)

    options = dict(frames=frames, track=True, oriented=True, antialias=True, track_min_score=-1.0)
    nv12, rgb = InferStep(model, B, SIZE, SIZE, frame_format="nv12", yuv=("bt601", "full"), **options), InferStep(model, B, SIZE, SIZE, **options)
    rot = torch.tensor([[1.0, 0.0], [0.6, 0.8], [-3.0, 0.5], [0.0, -1.0]]).cuda()
    mirror = torch.tensor([0, 1, 0, 1], dtype=torch.int32).cuda()
    nv12(rot=rot, mirror=mirror, **nv_in)
    rgb(rot=rot, mirror=mirror, **rgb_in)
    torch.cuda.synchronize()
    _same_step(nv12, rgb)
    assert nv12.lost.cpu().tolist() == [0] * B
    assert torch.equal(nv12.next_boxes, rgb.next_boxes) and torch.equal(nv12.next_rot, rgb.next_rot) and torch.equal(nv12.lost, rgb.lost)


def test_infer_step_nv12_image_follows_the_rule_and_the_layout(monkeypatch):
    """Noise NV12 frames on a pitched surface, BT.709 limited, centre siting, antialias: plan.img_nhwc4 is frames_crop_nv12_host of
    plan.crop_mat, and the captured replay equals the eager launches bit for bit."""
    from lighthand_amd.runtime import InferStep
    from lighthand_amd.topdown import crop_taps_host, frames_crop_nv12_host, nv12_layout
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    layout = nv12_layout(FH, FW, FW + 32, FH + 8)
    options = dict(frames=(NF, FH, FW), frame_format="nv12", chroma_siting="center", frame_layout=layout, antialias=True)
    step = InferStep(model, B, SIZE, SIZE, **options)
    assert tuple(step.frames.shape) == (NF, layout[3], layout[0])
    frames = np.random.RandomState(17).randint(0, 256, size=(NF, layout[3], layout[0])).astype(np.uint8)
    inputs = dict(frames=torch.from_numpy(frames).cuda(), boxes=torch.tensor(LARGE, dtype=torch.float32).cuda(),
                  frame_index=torch.tensor(INDEX, dtype=torch.int32).cuda())
    step(**inputs)
    torch.cuda.synchronize()
    mat, src = step.plan.crop_mat.cpu().numpy(), step.plan.src_frame.cpu().numpy()
    taps = crop_taps_host(mat)
    assert taps.min() >= 2 and src.tolist() == INDEX
    want = frames_crop_nv12_host(frames, (FH, FW), mat, src, (SIZE, SIZE), ("bt709", "limited"), "center", max_taps=8, layout=layout)
    _, _, dark = input_caps(mat, src, taps, FH, FW, SIZE, SIZE, NF)
    assert_close(step.plan.img_nhwc4, want, dark, "bf16", SIZE, SIZE, step.plan.img_pad, "InferStep(frame_format='nv12') image")
    eager = InferStep(model, B, SIZE, SIZE, use_graph=False, **options)
    eager(**inputs)
    torch.cuda.synchronize()
    assert torch.equal(_bits(eager.plan.img_nhwc4), _bits(step.plan.img_nhwc4))
    assert torch.equal(eager.heatmaps, step.heatmaps) and torch.equal(eager.preds, step.preds) and torch.equal(eager.maxvals, step.maxvals)


# ------------------------------------------------------------------------------------------------ 5. InferPipeline and the tool
def test_infer_pipeline_nv12(monkeypatch):
    """InferPipeline(frame_format="nv12", depth=2): the two batches in flight return the single step's preds and maxvals bit for bit."""
    from lighthand_amd.runtime import InferPipeline, InferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    options = dict(frames=(NF, FH, FW), frame_format="nv12", yuv=("bt601", "limited"), antialias=True)
    batches = [dict(frames=torch.from_numpy(_noise(NF, FH, FW, seed)).cuda(), boxes=torch.tensor(LARGE, dtype=torch.float32).cuda(),
                    frame_index=torch.tensor(INDEX, dtype=torch.int32).cuda()) for seed in (40, 41, 42)]
    ref = InferStep(model, B, SIZE, SIZE, **options)
    want = []
    for kw in batches:
        ref(**kw)
        torch.cuda.synchronize()
        want.append((ref.preds.clone(), ref.maxvals.clone()))
    pipe = InferPipeline(model, B, SIZE, SIZE, depth=2, **options)
    assert [s.frame_format for s in pipe.steps] == ["nv12", "nv12"]
    got = list(pipe.map(batches))
    assert len(got) == 3 and all(torch.equal(g[0], w[0]) and torch.equal(g[1], w[1]) for g, w in zip(got, want))


def test_track_frames_cli_nv12(capsys):
    """The tool's closed loop on NV12 frames, 3 frames of 256 x 320 cropped to 32 x 32."""
    import json
    from lighthand_amd.tools import track_frames as T
    args = ["--synthetic", "3", "--frame_size", "256x320", "--hands", "2", "--depth", "18", "--size", "32"]
    result = T.main(args + ["--frame_format", "nv12"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == result
    assert (result["frame_format"], result["yuv_matrix"], result["yuv_range"], result["chroma_siting"]) == ("nv12", "bt709", "limited", "left")
    assert result["frames"] == 3 and result["slots"] == 6 and result["frames_per_s"] > 0
    other = T.main(args + ["--frame_format", "nv12", "--yuv_matrix", "bt601", "--yuv_range", "full", "--chroma_siting", "center", "--antialias",
                           "--oriented"])
    assert (other["yuv_matrix"], other["yuv_range"], other["chroma_siting"], other["antialias"]) == ("bt601", "full", "center", 8)


# ------------------------------------------------------------------------------------------------ 6. the launch list
def test_steps_without_the_new_arguments_keep_their_launch_list(monkeypatch):
    """A step built without frame_format= (or with "rgb") enqueues what it always did: lh_frames_crop_to_nhwc4 with its 15 bound
    arguments, or lh_frames_crop_area_to_nhwc4 under antialias; the NV12 step differs from it in that one launch."""
    from lighthand_amd.runtime import InferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    frames = (NF, FH, FW)
    plain, rgb, nv12 = InferStep(model, B, SIZE, SIZE, frames=frames), InferStep(model, B, SIZE, SIZE, frames=frames, frame_format="rgb"), \
        InferStep(model, B, SIZE, SIZE, frames=frames, frame_format="nv12")
    assert _calls(rgb.plan) == _calls(plain.plan)
    rows = _calls(plain.plan)
    names = [r[0] for r in rows]
    assert names.count("lh_frames_crop_to_nhwc4") == 1 and not any("yuv" in n or "area" in n for n in names)
    i = names.index("lh_frames_crop_to_nhwc4")
    assert names[i - 1] == "lh_box_affine" and rows[i][1] == "frame crop input pipeline" and len(plain.plan.fwd[i].args) == 15
    assert rows[i][2][:8] == (B, NF, FH, FW, SIZE, SIZE, plain.plan.img_pad, plain.plan.img_wp)
    swapped = list(rows)
    swapped[i] = ("lh_frames_crop_yuv_to_nhwc4", "NV12 frame crop input pipeline",
                  (B, NF, FH, FW, FW, FH * FW, FH * FW * 3 // 2, 0, SIZE, SIZE, plain.plan.img_pad, plain.plan.img_wp, 1) + rows[i][2][8:])
    assert _calls(nv12.plan) == swapped
    area = [r[0] for r in _calls(InferStep(model, B, SIZE, SIZE, frames=frames, antialias=True).plan)]
    assert area == [n.replace("lh_frames_crop_to_nhwc4", "lh_frames_crop_area_to_nhwc4") for n in names]
