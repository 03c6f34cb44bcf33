"""GPU: the antialiased frame crop -- lh_frames_crop_area_to_nhwc4 against lh_frames_crop_to_nhwc4 (one tap: the same bits), the
exact block mean, the numpy restatement frames_crop_host of lighthand_amd.topdown (the sampling rule: csrc/frames_crop_kernel.h,
above crop_taps), and InferStep / InferPipeline(antialias=) and the track_frames tool on top of it.  3 frames of 150 x 210, crop 24 x 40,
pad 3; 96 x 96 frames for the aligned cases; the tolerance scheme is tests/test_gpu_topdown.py::test_crops_match_the_numpy_sampling_rule's."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_area_crop_host import block_mean
from test_gpu_topdown import DT, MEAN, STD, ULP, _affine_np, _bits, _black, _close4, _crop, _frames, _lib, _model, _stream

pytestmark = pytest.mark.gpu

F = np.float32
HS, WS, H, W, PAD, NF = 150, 210, 24, 40, 3, 3


def _area(frames_d, mat_d, src_d, h, w, pad, dtype, max_taps, wp=None):
    """lh_frames_crop_area_to_nhwc4 on a NaN-filled output; returns the padded NHWC4 buffer."""
    L, lib = _lib()
    n, hs, ws = frames_d.shape[:3]
    b = mat_d.shape[0]
    wp = wp or w + 2 * pad + 2
    code, tdt = DT[dtype]
    out = torch.full((b, h + 2 * pad, wp, 4), float("nan"), dtype=tdt, device="cuda")
    m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    L.check(lib.lh_frames_crop_area_to_nhwc4(frames_d.data_ptr(), out.data_ptr(), b, n, hs, ws, h, w, pad, wp, m3, s3, mat_d.data_ptr(),
                                             src_d.data_ptr(), max_taps, code, _stream()), "lh_frames_crop_area_to_nhwc4")
    torch.cuda.synchronize()
    return out


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a, dtype)).cuda()


def _border_is_zero(out, h, w, pad):
    border = out.clone()
    border[:, pad:pad + h, pad:pad + w, :3] = 0
    return not bool(_bits(border).any())


# ------------------------------------------------------------------------------------------------ the 32 slots
# hand-written matrices (crop 24 x 40 -> frame 150 x 210): different scales on the two axes, a shear, and the tap counts 6 and 7
ANISO = [[3.3, 0.0, 20.0, 0.0, 0.9, 60.0],                          # (4, 1)
         [0.7, 0.0, 90.0, 0.0, 4.4, 25.0],                          # (1, 5)
         [2.5, 1.2, 30.0, 0.3, 1.7, 50.0],                          # a shear: (3, 3)
         [5.5, 0.0, 2.0, 0.0, 5.5, 10.0],                           # (6, 6)
         [3.9, -5.2, 150.0, 5.2, 3.9, -20.0],                       # the direction (0.6, 0.8) at scale 6.5: (7, 7)
         [-6.6, 0.0, 230.0, 0.0, 2.6, 40.0],                        # mirrored: (7, 3)
         [9.3, 0.0, -60.0, 0.0, 7.7, -15.0],                        # (8, 8), capped; most of it outside the frame
         [1.3, 0.0, 80.0, 0.0, 1.3, 70.0]]                          # (2, 2)
ANISO_SRC = [0, 1, 2, 0, 1, 2, 0, 5]                                # the last one names a frame that does not exist


def slots(oriented, seed=21, largest=220.0):
    """32 slots: 24 seeded boxes (half extents log-uniform over 8 px..largest, centres in and around the frame, two of them unusable)
    through box_affine_host or -- with seeded directions and mirrors -- roi_affine_host, and the 8 hand-written matrices."""
    from lighthand_amd.topdown import box_affine_host, roi_affine_host
    rng = np.random.RandomState(seed)
    n = 24
    c = np.stack([rng.uniform(-20, WS + 20, size=n), rng.uniform(-20, HS + 20, size=n)], 1)
    half = np.exp(rng.uniform(np.log(8), np.log(largest), size=(n, 2)))
    boxes = np.concatenate([c - half, c + half], 1).astype(np.float32)
    index = rng.randint(0, NF, size=n).astype(np.int32)
    rot = rng.normal(size=(n, 2)).astype(np.float32)
    mirror = rng.randint(0, 2, size=n).astype(np.int32)
    boxes[5, 0], index[11] = np.nan, -1                             # two empty slots
    if oriented:
        mat, src = roi_affine_host(boxes, rot, mirror, index, NF, (H, W), 1.25)
    else:
        mat, src = box_affine_host(boxes, index, NF, (H, W), 1.25)
    return np.concatenate([mat, np.asarray(ANISO, np.float32)]), np.concatenate([src, np.asarray(ANISO_SRC, np.int32)]).astype(np.int32)


def sample_positions(mat, taps, h, w):
    """Every sample position of one slot, in the kernel's fp32 order: (fx, fy), each [ky*kx][h][w]."""
    m0, m1, m2, m3, m4, m5 = np.asarray(mat, np.float32)
    kx, ky = int(taps[0]), int(taps[1])
    oy, ox = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    fx, fy = [], []
    with np.errstate(all="ignore"):
        for j in range(ky):
            uy = oy + F(2 * j + 1 - ky) / F(2 * ky)
            for i in range(kx):
                ux = ox + F(2 * i + 1 - kx) / F(2 * kx)
                fx.append((m0 * ux + m1 * uy) + m2)
                fy.append((m3 * ux + m4 * uy) + m5)
    return np.stack(fx), np.stack(fy)


def input_caps(mat, src, taps, hs, ws, h, w, n_frames):
    """What the tolerance of the comparison rests on, from numpy alone: (share of pixels with a sample within 1e-5 of a frame edge,
    share of pixels with a sample inside the frame, mask [b][h][w] of the pixels with no sample inside)."""
    near, lit, dark = 0, 0, []
    for i in range(len(src)):
        live = 0 <= src[i] < n_frames
        fx, fy = sample_positions(mat[i], taps[i] if live else (1, 1), h, w)
        with np.errstate(all="ignore"):
            inside = (fx >= F(-0.5)) & (fx <= F(ws) - F(0.5)) & (fy >= F(-0.5)) & (fy <= F(hs) - F(0.5)) & live
            edge = ((np.abs(fx + F(0.5)) < 1e-5) | (np.abs(fx - (ws - 0.5)) < 1e-5) | (np.abs(fy + F(0.5)) < 1e-5)
                    | (np.abs(fy - (hs - 0.5)) < 1e-5)) & live
        near += int(edge.any(0).sum())
        lit += int(inside.any(0).sum())
        dark.append(~inside.any(0))
    return near / float(len(src) * h * w), lit / float(len(src) * h * w), np.stack(dark)


def assert_close(out, want, dark, dtype, h, w, pad, what):
    """tests/test_gpu_topdown.py::test_crops_match_the_numpy_sampling_rule's scheme: the share of values off by more than 1e-4 (+ one
    unit in the last place of a 16-bit run dtype) stays below 1e-3, the fp32 median below 1e-6; pixels with no sample inside the
    frame are exactly black in the run dtype; padding and channel 3 are exactly 0."""
    got = np.transpose(out.float().cpu().numpy()[:, pad:pad + h, pad:pad + w, :3], (0, 3, 1, 2))
    d = np.abs(got - want)
    tol = 1e-4 + (ULP[dtype] * np.abs(want) if dtype != "fp32" else 0.0)
    print(f"{what} {dtype}: max |d| {float(d.max()):.3e}, median {float(np.median(d)):.3e}, share over tol {float((d > tol).mean()):.3e}")
    assert np.isfinite(got).all()
    assert (d > tol).mean() < 1e-3, float(d.max())
    if dtype == "fp32":
        assert float(np.median(d)) < 1e-6
    black = torch.from_numpy(_black()).to(DT[dtype][1]).float().numpy()
    outside = np.broadcast_to(dark[:, None], got.shape)
    assert (got[outside] == np.broadcast_to(black[None, :, None, None], got.shape)[outside]).all()
    assert _border_is_zero(out, h, w, pad)


# ------------------------------------------------------------------------------------------------ 1. one tap = the plain entry
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_one_tap_is_bit_equal_to_the_plain_entry(dtype):
    """max_taps = 1 through the new entry: the whole buffer -- padding and channel 3 included -- has lh_frames_crop_to_nhwc4's bits,
    on boxes and on oriented, mirrored ROIs of every size; and so has max_taps = 8 on every slot that is not minified."""
    from lighthand_amd.topdown import crop_taps_host
    frames = torch.from_numpy(_frames(NF, HS, WS, 5)).cuda()
    mb, sb = slots(False, largest=50.0)                             # scales 0.5 .. 5: both kinds of slot are well represented
    mr, sr = slots(True, largest=50.0)
    mat, src = np.concatenate([mb[:16], mr[:16]]), np.concatenate([sb[:16], sr[:16]])
    assert len(src) == 32 and (src < 0).sum() >= 2
    mat_d, src_d = _dev(mat, np.float32), _dev(src, np.int32)
    want = _crop(frames, mat_d, src_d, H, W, PAD, dtype)
    got = _area(frames, mat_d, src_d, H, W, PAD, dtype, 1)
    assert not bool(torch.isnan(want.float()).any()) and _border_is_zero(want, H, W, PAD)
    assert torch.equal(_bits(got), _bits(want))
    eight = _area(frames, mat_d, src_d, H, W, PAD, dtype, 8)
    single = torch.from_numpy((crop_taps_host(mat, 8) == 1).all(1) | (src < 0)).cuda()
    assert 4 < int(single.sum()) < 28
    assert torch.equal(_bits(eight)[single], _bits(want)[single])
    assert all(not torch.equal(_bits(eight)[i], _bits(want)[i]) for i in (~single).nonzero().flatten().tolist())
    assert _border_is_zero(eight, H, W, PAD)


# ------------------------------------------------------------------------------------------------ 2. aligned block means
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_aligned_minification_is_the_exact_block_mean(dtype):
    """Whole-frame boxes on 96 x 96 frames at padding 1, crop 96 / s: m = (s, 0, (s-1)/2, 0, s, (s-1)/2), the samples land on the
    integer pixels s*ox + i.  fp32: (block sum) * (1.f/(s*s)) * (1.f/255.f), Normalize, bit for bit; 16-bit runs: its rounding to the
    run dtype.  s = 16 at max_taps = 8: two frame pixels between the taps, every product still exact -- frames_crop_host's bits."""
    from lighthand_amd.topdown import box_affine_host, frames_crop_host
    frames = _frames(2, 96, 96, 13)
    frames_d = torch.from_numpy(frames).cuda()
    tdt = DT[dtype][1]
    for s in (2, 3, 4, 6, 8, 16):
        c = 96 // s
        mat, src = box_affine_host([[-0.5, -0.5, 95.5, 95.5]] * 3, [1, 0, 7], 2, (c, c), 1.0)
        assert mat[:2].tolist() == [[s, 0.0, (s - 1) / 2, 0.0, s, (s - 1) / 2]] * 2 and src.tolist() == [1, 0, -1]
        out = _area(frames_d, _dev(mat, np.float32), _dev(src, np.int32), c, c, PAD, dtype, 8)
        if s <= 8:
            want = np.stack([block_mean(frames[1], s, MEAN, STD), block_mean(frames[0], s, MEAN, STD)])
        else:
            want = frames_crop_host(frames, mat[:2], src[:2], (c, c), max_taps=8)       # 8 x 8 samples between the 16 x 16 pixels
        want = torch.from_numpy(np.transpose(want, (0, 2, 3, 1)).copy()).to(tdt).cuda()
        got = out[:2, PAD:PAD + c, PAD:PAD + c, :3]
        assert torch.equal(_bits(got.contiguous()), _bits(want.contiguous())), s
        black = torch.from_numpy(_black()).to(tdt).cuda()
        assert torch.equal(out[2, PAD:PAD + c, PAD:PAD + c, :3], black.expand(c, c, 3))  # the empty slot
        assert _border_is_zero(out, c, c, PAD)


# ------------------------------------------------------------------------------------------------ 3. against frames_crop_host
_REFERENCE = {}


def reference(oriented):
    """(frames, mat, src, taps, want, dark) of one 32-slot set, computed once; the caps its tolerance rests on are asserted here."""
    if oriented not in _REFERENCE:
        from lighthand_amd.topdown import crop_taps_host, frames_crop_host
        frames = _frames(NF, HS, WS, 5)
        mat, src = slots(oriented)
        taps = crop_taps_host(mat, 8)
        live = src >= 0
        assert len(src) == 32 and live.sum() >= 28
        near, lit, dark = input_caps(mat, src, taps, HS, WS, H, W, NF)
        print(f"slots (oriented={oriented}): edge share {near:.2e}, inside share {lit:.3f}, tap counts {sorted(set(taps[live].ravel().tolist()))}")
        assert near <= 1e-3
        assert 0.2 < lit < 0.8
        assert set(taps[live & (src < NF)].ravel().tolist()) == set(range(1, 9))
        with np.errstate(all="ignore"):
            scale = np.concatenate([np.sqrt(mat[live, 0] ** 2 + mat[live, 3] ** 2), np.sqrt(mat[live, 1] ** 2 + mat[live, 4] ** 2)])
        scale = scale[(scale > 1.0) & (scale < 8.5)]                # where a rounding of the scale could change a tap count
        assert (np.abs(scale - np.rint(scale)) > 1e-2).all() and (np.abs(scale - 1.015625) > 1e-2).all()
        want = frames_crop_host(frames, mat, src, (H, W), max_taps=8)
        want.setflags(write=False)
        _REFERENCE[oriented] = (frames, mat, src, taps, want, dark)
    return _REFERENCE[oriented]


@pytest.mark.parametrize("oriented", [False, True], ids=["boxes", "rois"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_area_crops_match_the_numpy_sampling_rule(dtype, oriented):
    frames, mat, src, taps, want, dark = reference(oriented)
    assert dark[src < 0].all() and dark[31].all() and dark.sum() > 4 * H * W
    out = _area(torch.from_numpy(frames).cuda(), _dev(mat, np.float32), _dev(src, np.int32), H, W, PAD, dtype, 8)
    assert_close(out, want, dark, dtype, H, W, PAD, "area crop")
    if dtype == "fp32" and not oriented:                           # the eager form is the same launch: no padding, wp = w
        from lighthand_amd.topdown import frames_crop
        eager = frames_crop(torch.from_numpy(frames).cuda(), _dev(mat, np.float32), _dev(src, np.int32), (H, W), max_taps=8)
        torch.cuda.synchronize()
        assert eager.shape == (32, H, W, 4) and eager.dtype == torch.float32
        assert torch.equal(_bits(eager), _bits(out[:, PAD:PAD + H, PAD:PAD + W].contiguous()))
        with pytest.raises(ValueError, match="max_taps"):
            frames_crop(torch.from_numpy(frames).cuda(), _dev(mat, np.float32), _dev(src, np.int32), (H, W), max_taps=9)


def test_fewer_taps_than_the_minification_follow_the_rule_too():
    """max_taps = 3: every count above 3 is capped, the taps are more than one frame pixel apart -- still frames_crop_host's values."""
    from lighthand_amd.topdown import crop_taps_host, frames_crop_host
    frames, mat, src, _, _, _ = reference(False)
    taps = crop_taps_host(mat, 3)
    assert taps.max() == 3
    _, _, dark = input_caps(mat, src, taps, HS, WS, H, W, NF)
    want = frames_crop_host(frames, mat, src, (H, W), max_taps=3)
    out = _area(torch.from_numpy(frames).cuda(), _dev(mat, np.float32), _dev(src, np.int32), H, W, PAD, "fp32", 3)
    assert_close(out, want, dark, "fp32", H, W, PAD, "area crop, 3 taps")


# ------------------------------------------------------------------------------------------------ 4. InferStep(antialias=)
B, SIZE, FH, FW = 4, 64, 96, 128
SMALL = [[20.0, 10.0, 60.0, 50.0], [60.5, 30.25, 100.0, 70.0], [90.0, 40.0, 120.5, 80.0], [40.0, 40.0, 56.0, 70.0]]    # <= 51 px: magnified
LARGE = [[-0.5, -0.5, FW - 0.5, FH - 0.5], [10.0, 5.0, 120.0, 90.0], [-40.0, -30.0, 150.0, 120.0], [30.0, 2.0, 110.0, 95.0]]
INDEX = [0, 1, 2, 0]


def _calls(plan):
    """The forward launch list without its addresses: (entry or marker, description, the arguments that are not pointers)."""
    rows = []
    for c in plan.fwd:
        if hasattr(c, "fn"):
            rows.append((c.fn.__name__, c.what, tuple(a for a in c.args if isinstance(a, (int, float)) and not isinstance(a, bool) and abs(a) < 1 << 20)))
        else:
            rows.append((type(c).__name__, c.kind))
    return rows


def _inputs(boxes, seed=31):
    return dict(frames=torch.from_numpy(_frames(NF, FH, FW, seed)).cuda(), boxes=torch.tensor(boxes, dtype=torch.float32).cuda(),
                frame_index=torch.tensor(INDEX, dtype=torch.int32).cuda())


def test_infer_step_antialias(monkeypatch):
    """antialias=False enqueues the calls of a step built without the argument; with magnifying boxes antialias=True returns the
    plain step's heat-maps and preds bit for bit; with minifying boxes plan.img_nhwc4 is frames_crop_host of plan.crop_mat; the
    captured graph's replay equals the eager launches bit for bit."""
    from lighthand_amd.runtime import InferStep
    from lighthand_amd.topdown import crop_taps_host, frames_crop_host
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    frames = (NF, FH, FW)
    plain, off, on = InferStep(model, B, SIZE, SIZE, frames=frames), InferStep(model, B, SIZE, SIZE, frames=frames, antialias=False), \
        InferStep(model, B, SIZE, SIZE, frames=frames, antialias=True)
    assert (plain.antialias, off.antialias, on.antialias) == (1, 1, 8)
    assert InferStep(model, B, SIZE, SIZE, frames=frames, antialias=3).antialias == 3
    assert _calls(off.plan) == _calls(plain.plan)
    names = [r[0] for r in _calls(plain.plan)]
    assert names.count("lh_frames_crop_to_nhwc4") == 1 and "lh_frames_crop_area_to_nhwc4" not in names
    swapped = [("lh_frames_crop_area_to_nhwc4", "antialiased frame crop input pipeline", r[2][:8] + (8,) + r[2][8:])
               if r[0] == "lh_frames_crop_to_nhwc4" else r for r in _calls(plain.plan)]
    assert _calls(on.plan) == swapped                               # one launch differs: the entry, and max_taps before dtype

    small = _inputs(SMALL)
    plain(**small)
    on(**small)
    torch.cuda.synchronize()
    assert crop_taps_host(on.plan.crop_mat.cpu().numpy()).tolist() == [[1, 1]] * B
    assert torch.equal(on.heatmaps, plain.heatmaps) and torch.equal(on.preds, plain.preds) and torch.equal(on.maxvals, plain.maxvals)
    assert torch.equal(_bits(on.plan.img_nhwc4), _bits(plain.plan.img_nhwc4))

    large = _inputs(LARGE)
    plain(**large)
    on(**large)
    torch.cuda.synchronize()
    mat, src = on.plan.crop_mat.cpu().numpy(), on.plan.src_frame.cpu().numpy()
    taps = crop_taps_host(mat)
    assert torch.equal(on.plan.crop_mat, plain.plan.crop_mat) and taps.min() >= 2 and taps.max() >= 4 and src.tolist() == INDEX
    assert not torch.equal(_bits(on.plan.img_nhwc4), _bits(plain.plan.img_nhwc4)) and not torch.equal(on.heatmaps, plain.heatmaps)
    want = frames_crop_host(large["frames"].cpu().numpy(), mat, src, (SIZE, SIZE), max_taps=8)
    _, _, dark = input_caps(mat, src, taps, FH, FW, SIZE, SIZE, NF)
    p = on.plan.img_pad
    assert on.plan.img_nhwc4.shape[2] == on.plan.img_wp
    assert_close(on.plan.img_nhwc4, want, dark, "bf16", SIZE, SIZE, p, "InferStep(antialias=True) image")

    eager = InferStep(model, B, SIZE, SIZE, frames=frames, antialias=True, use_graph=False)
    eager(**large)
    torch.cuda.synchronize()
    assert torch.equal(_bits(eager.plan.img_nhwc4), _bits(on.plan.img_nhwc4))
    assert torch.equal(eager.heatmaps, on.heatmaps) and torch.equal(eager.preds, on.preds) and torch.equal(eager.maxvals, on.maxvals)


def test_infer_step_antialias_composes_with_the_other_options(monkeypatch):
    """oriented + track + flip_test + antialias in one captured step: preds are crop_preds through crop_mat, the tracked ROI follows
    the raw keypoints, and the image differs from the same step without antialias."""
    from lighthand_amd.runtime import InferStep
    from lighthand_amd.topdown import crop_taps_host
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    options = dict(frames=(NF, FH, FW), oriented=True, track=True, flip_test=True, track_min_score=-1.0)
    step, plain = InferStep(model, B, SIZE, SIZE, antialias=True, **options), InferStep(model, B, SIZE, SIZE, **options)
    rot = torch.tensor([[1.0, 0.0], [0.6, 0.8], [-3.0, 0.5], [0.0, -1.0]]).cuda()
    mirror = torch.tensor([0, 1, 0, 1], dtype=torch.int32).cuda()
    for s in (step, plain):
        s(rot=rot, mirror=mirror, **_inputs(LARGE))
    torch.cuda.synchronize()
    assert crop_taps_host(step.plan.crop_mat.cpu().numpy()).min() >= 2 and step.valid.cpu().tolist() == [True] * B
    assert torch.equal(step.plan.crop_mat, plain.plan.crop_mat)
    assert not torch.equal(_bits(step.plan.img_nhwc4), _bits(plain.plan.img_nhwc4))
    want = _affine_np(step.plan.crop_mat.cpu().numpy(), step.crop_preds.cpu().numpy())
    assert _close4(step.preds.cpu().numpy(), want)
    assert step.lost.cpu().tolist() == [0] * B and bool(torch.isfinite(step.next_boxes).all()) and bool(torch.isfinite(step.next_rot).all())
    first_mat, next_boxes, next_rot = step.plan.crop_mat.clone(), step.next_boxes.clone(), step.next_rot.clone()
    step.advance()
    step()
    torch.cuda.synchronize()
    assert torch.equal(step.boxes, next_boxes) and torch.equal(step.rot, next_rot)      # the loop closes: the second replay crops there
    assert not torch.equal(step.plan.crop_mat, first_mat)
    assert _close4(step.preds.cpu().numpy(), _affine_np(step.plan.crop_mat.cpu().numpy(), step.crop_preds.cpu().numpy()))


# ------------------------------------------------------------------------------------------------ 5. InferPipeline and the tool
def test_infer_pipeline_antialias(monkeypatch):
    """InferPipeline(antialias=True, depth=2): the two batches in flight return the single step's preds and maxvals bit for bit."""
    from lighthand_amd.runtime import InferPipeline, InferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    batches = [_inputs(LARGE, seed=40), _inputs(SMALL, seed=41), _inputs(LARGE, seed=42)]
    ref = InferStep(model, B, SIZE, SIZE, frames=(NF, FH, FW), antialias=True)
    want = []
    for kw in batches:
        ref(**kw)
        torch.cuda.synchronize()
        want.append((ref.preds.clone(), ref.maxvals.clone()))
    pipe = InferPipeline(model, B, SIZE, SIZE, depth=2, frames=(NF, FH, FW), antialias=True)
    assert [s.antialias for s in pipe.steps] == [8, 8]
    got = list(pipe.map(batches))
    assert len(got) == 3 and all(torch.equal(g[0], w[0]) and torch.equal(g[1], w[1]) for g, w in zip(got, want))


def test_track_frames_cli_antialias(capsys):
    """The tool's closed loop with --antialias on a 3-frame sequence: hands a fifth of a 256 x 320 frame across, cropped to 32 x 32."""
    import json
    from lighthand_amd.tools import track_frames as T
    args = ["--synthetic", "3", "--frame_size", "256x320", "--hands", "2", "--depth", "18", "--size", "32"]
    result = T.main(args + ["--antialias"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == result
    assert result["antialias"] == 8 and result["frames"] == 3 and result["slots"] == 6 and result["frames_per_s"] > 0
    assert T.main(args + ["--antialias", "2", "--oriented"])["antialias"] == 2
    assert "antialias" not in T.main(args)
