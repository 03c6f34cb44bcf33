"""GPU: top-down inference on full frames -- lh_box_affine, lh_frames_crop_to_nhwc4 and lh_keypoints_to_boxes against the numpy
restatements of lighthand_amd.topdown and of the sampling rule, and InferStep / InferPipeline(frames=...) on top of them.

The sampling rule restated in numpy (fp32, the kernels are built with -ffp-contract=off): output pixel (ox, oy) of slot i samples
frame src_frame[i] at f = ((m0 ox + m1 oy) + m2, (m3 ox + m4 oy) + m5); inside [-0.5, ws-0.5] x [-0.5, hs-0.5] bilinearly with the
edge clamp of the warp kernel (tests/test_gpu_augment.py's warp_reference with the resize factor taken out), outside -- and in every
pixel of an empty slot -- black, 0 before Normalize."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import resnet_cfg

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DT = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}
ULP = {"fp32": 2.0 ** -23, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}           # one unit in the last place, relative
F = np.float32

# the ABI shapes: 3 frames of 37 x 53, crop 24 x 40, pad 3, 7 slots
HS, WS, H, W, PAD = 37, 53, 24, 40, 3
FRAME_INDEX = [0, 2, 2, 1, -1, 0, 5]
BOXES = [[10.3, 5.2, 40.7, 30.9],                  # inside the frame
         [-20.5, 10.0, 25.0, 45.5],                # half outside
         [-30.0, -20.0, 90.0, 70.0],               # larger than the frame
         [20.5, 12.5, 25.5, 15.5],                 # 5 px wide: x8 magnification at padding 1
         [10.0, 10.0, 10.0, 20.0],                 # degenerate
         [float("nan"), 4.0, 30.0, 30.0],          # NaN
         [4.0, 4.0, 30.0, 30.0]]                   # valid, but its frame index is out of range


def _lib():
    from lighthand_amd import _lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _frames(n, hs, ws, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, hs, ws, 3)).astype(np.uint8)


def _box_affine(boxes, index, n_frames, h, w, padding):
    """lh_box_affine on NaN-filled outputs; returns (mat, src_frame) device tensors."""
    L, lib = _lib()
    boxes_d = torch.as_tensor(np.asarray(boxes, np.float32)).cuda()
    index_d = torch.as_tensor(np.asarray(index, np.int32)).cuda()
    b = boxes_d.shape[0]
    mat = torch.full((b, 6), float("nan"), device="cuda")
    src = torch.full((b,), -77, dtype=torch.int32, device="cuda")
    L.check(lib.lh_box_affine(boxes_d.data_ptr(), index_d.data_ptr(), b, n_frames, h, w, padding, mat.data_ptr(), src.data_ptr(), _stream()),
            "lh_box_affine")
    torch.cuda.synchronize()
    return mat, src


def _crop(frames_d, mat_d, src_d, h, w, pad, dtype, wp=None):
    """lh_frames_crop_to_nhwc4 on a NaN-filled output; returns the padded NHWC4 buffer."""
    L, lib = _lib()
    n, hs, ws = frames_d.shape[:3]
    b = mat_d.shape[0]
    wp = wp or w + 2 * pad + 2
    code, tdt = DT[dtype]
    out = torch.full((b, h + 2 * pad, wp, 4), float("nan"), dtype=tdt, device="cuda")
    m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    L.check(lib.lh_frames_crop_to_nhwc4(frames_d.data_ptr(), out.data_ptr(), b, n, hs, ws, h, w, pad, wp, m3, s3, mat_d.data_ptr(),
                                        src_d.data_ptr(), code, _stream()), "lh_frames_crop_to_nhwc4")
    torch.cuda.synchronize()
    return out


def _black():
    return np.array([(F(0) - F(m)) * (F(1) / F(s)) for m, s in zip(MEAN, STD)], np.float32)


def crop_reference(frames, mat, src, h, w):
    """uint8 frames [n, hs, ws, 3], one slot's matrix and frame number -> (normalised float32 [3, h, w], inside mask, fx, fy)."""
    n, hs, ws = frames.shape[:3]
    m0, m1, m2, m3, m4, m5 = np.asarray(mat, np.float32)
    oy, ox = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    with np.errstate(all="ignore"):
        fx, fy = (m0 * ox + m1 * oy) + m2, (m3 * ox + m4 * oy) + m5
        inside = (fx >= F(-0.5)) & (fx <= F(ws) - F(0.5)) & (fy >= F(-0.5)) & (fy <= F(hs) - F(0.5)) & (0 <= src < n)
    cy, cx = np.where(inside, np.maximum(fy, F(0)), F(0)).astype(np.float32), np.where(inside, np.maximum(fx, F(0)), F(0)).astype(np.float32)
    y0, x0 = np.minimum(cy.astype(np.int32), hs - 1), np.minimum(cx.astype(np.int32), ws - 1)
    y1, x1 = np.minimum(y0 + 1, hs - 1), np.minimum(x0 + 1, ws - 1)
    wy, wx = cy - y0.astype(np.float32), cx - x0.astype(np.float32)
    img = np.transpose(frames[src if 0 <= src < n else 0].astype(np.float32), (2, 0, 1))
    a00, a01, a10, a11 = img[:, y0, x0], img[:, y0, x1], img[:, y1, x0], img[:, y1, x1]
    top, bot = a00 + (a01 - a00) * wx, a10 + (a11 - a10) * wx
    val = np.where(inside, (top + (bot - top) * wy) * (F(1) / F(255)), F(0)).astype(np.float32)
    m, s = np.asarray(MEAN, np.float32)[:, None, None], np.asarray(STD, np.float32)[:, None, None]
    return ((val - m) * (F(1) / s)).astype(np.float32), inside, fx, fy


def _close4(got, want):
    """Within 4 fp32 spacings of the expected value (tests/test_gpu_augment.py::test_affine_points_and_disc_consistency's bound)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return bool((np.abs(got - want) <= 4 * np.spacing(np.abs(want))).all())


# ------------------------------------------------------------------------------------------------ lh_box_affine
@pytest.mark.parametrize("padding", [1.0, 1.25])
def test_box_affine_matches_the_host_restatement(padding):
    from lighthand_amd.topdown import box_affine, box_affine_host
    want_mat, want_src = box_affine_host(BOXES, FRAME_INDEX, 3, (H, W), padding)
    assert want_src.tolist() == [0, 2, 2, 1, -1, -1, -1]
    mat, src = _box_affine(BOXES, FRAME_INDEX, 3, H, W, padding)
    assert src.cpu().numpy().tolist() == want_src.tolist()
    got = mat.cpu().numpy()
    print("box_affine max |got - want| in spacings:", float(np.nanmax(np.abs(got - want_mat) / np.spacing(np.maximum(np.abs(want_mat), F(1e-30))))))
    assert _close4(got, want_mat)
    assert (got[want_src < 0] == 0).all()
    if padding == 1.0:
        assert got[3, 0] == F(0.125) and got[3, 4] == F(0.125)                 # the 5 px box: 8 crop pixels per frame pixel
    # the eager wrapper is the same launch; more slots than one workgroup
    rng = np.random.RandomState(7)
    many = np.concatenate([rng.uniform(-100, 900, size=(200, 2)), rng.uniform(950, 2000, size=(200, 2))], 1).astype(np.float32)
    idx = rng.randint(-1, 5, size=200).astype(np.int32)
    m2, s2 = box_affine(torch.from_numpy(many).cuda(), torch.from_numpy(idx).cuda(), 4, (H, W), padding)
    wm, wsrc = box_affine_host(many, idx, 4, (H, W), padding)
    assert s2.cpu().numpy().tolist() == wsrc.tolist() and _close4(m2.cpu().numpy(), wm)


# ------------------------------------------------------------------------------------------------ lh_frames_crop_to_nhwc4
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_identity_crop_is_bit_equal_to_the_uint8_pipeline(dtype):
    """Crop size = frame size, whole-frame boxes, padding 1: the matrix is the exact identity and every slot reproduces
    lh_image_u8_to_nhwc4 on the frame it names, padding and channel 3 included."""
    L, lib = _lib()
    n_frames, index = 3, [0, 1, 2, 1, 0]
    frames = torch.from_numpy(_frames(n_frames, H, W, 11)).cuda()
    mat, src = _box_affine([[-0.5, -0.5, W - 0.5, H - 0.5]] * len(index), index, n_frames, H, W, 1.0)
    assert mat.cpu().tolist() == [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]] * len(index)
    got = _crop(frames, mat, src, H, W, PAD, dtype)
    code, tdt = DT[dtype]
    picked = frames[torch.tensor(index, device="cuda")].contiguous()
    want = torch.full_like(got, float("nan"))
    m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    L.check(lib.lh_image_u8_to_nhwc4(picked.data_ptr(), want.data_ptr(), len(index), H, W, H, W, PAD, got.shape[2], m3, s3, code, _stream()),
            "lh_image_u8_to_nhwc4")
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want))
    border = got.clone()
    border[:, PAD:PAD + H, PAD:PAD + W, :3] = 0
    assert not bool(_bits(border).any())                           # padding and channel 3: exactly +0


def _random_boxes(n, seed):
    """Boxes of many sizes around and across a HS x WS frame, and frame indices in 0..2."""
    rng = np.random.RandomState(seed)
    c = np.stack([rng.uniform(-5, WS + 5, size=n), rng.uniform(-5, HS + 5, size=n)], 1)
    half = np.stack([rng.uniform(1.5, 40, size=n), rng.uniform(1.5, 30, size=n)], 1)
    return np.concatenate([c - half, c + half], 1).astype(np.float32), rng.randint(0, 3, size=n).astype(np.int32)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_crops_match_the_numpy_sampling_rule(dtype):
    """The 7 ABI slots at padding 1 and 1.25 and 18 random boxes, 32 slots in one launch, against crop_reference.  fp32: the share of
    pixels off by more than 1e-4 stays below 1e-3 (a cap for pixels that sit on a clamp boundary; the boxes put at most that share
    of samples within 1e-5 of a frame edge, checked here) and the median error below 1e-6.  16-bit runs: within one unit in the
    last place of the run dtype on top of that.  Out-of-frame pixels and empty slots are exactly (0 - mean) * (1 / std) in the run
    dtype, padding and channel 3 exactly 0."""
    from lighthand_amd.topdown import box_affine_host
    frames = _frames(3, HS, WS, 5)
    rb, ri = _random_boxes(18, 21)
    mat = np.concatenate([box_affine_host(BOXES, FRAME_INDEX, 3, (H, W), 1.0)[0], box_affine_host(BOXES, FRAME_INDEX, 3, (H, W), 1.25)[0],
                          box_affine_host(rb, ri, 3, (H, W), 1.25)[0]])
    src = np.concatenate([box_affine_host(BOXES, FRAME_INDEX, 3, (H, W), 1.0)[1]] * 2 + [ri]).astype(np.int32)
    b = len(src)
    assert b == 32 and (src >= 0).sum() == 26
    want, inside, near_edge = [], [], 0
    for i in range(b):
        ref, ins, fx, fy = crop_reference(frames, mat[i], int(src[i]), H, W)
        want.append(ref)
        inside.append(ins)
        if src[i] >= 0:
            with np.errstate(all="ignore"):
                near_edge += int(((np.abs(fx + F(0.5)) < 1e-5) | (np.abs(fx - (WS - 0.5)) < 1e-5) | (np.abs(fy + F(0.5)) < 1e-5)
                                  | (np.abs(fy - (HS - 0.5)) < 1e-5)).sum())
    want, inside = np.stack(want), np.stack(inside)
    assert near_edge / float((src >= 0).sum() * H * W) <= 1e-3, near_edge
    assert 0.2 < inside.mean() < 0.8                               # both kinds of pixel are well represented
    out = _crop(torch.from_numpy(frames).cuda(), torch.from_numpy(mat).cuda(), torch.from_numpy(src).cuda(), H, W, PAD, dtype)
    full = out.float().cpu().numpy()
    got = np.transpose(full[:, PAD:PAD + H, PAD:PAD + W, :3], (0, 3, 1, 2))
    d = np.abs(got - want)
    tol = 1e-4 + (ULP[dtype] * np.abs(want) if dtype != "fp32" else 0.0)
    print(f"crop {dtype}: max |d| {float(d.max()):.3e}, median {float(np.median(d)):.3e}, share over tol {float((d > tol).mean()):.3e}")
    assert (d > tol).mean() < 1e-3, float(d.max())
    if dtype == "fp32":
        assert float(np.median(d)) < 1e-6
    black = torch.from_numpy(_black()).to(DT[dtype][1]).float().numpy()
    outside = np.broadcast_to(~inside[:, None], got.shape)
    assert (got[outside] == np.broadcast_to(black[None, :, None, None], got.shape)[outside]).all()
    assert (~inside[src < 0]).all() and (~inside).sum() > 6 * H * W
    border = out.clone()
    border[:, PAD:PAD + H, PAD:PAD + W, :3] = 0
    assert not bool(_bits(border).any())


def test_crop_indexes_a_frame_buffer_past_2_31_bytes():
    """41 frames of 3000 x 6000 x 3 bytes = 2.21 GB: the last frame starts past byte 2^31, and a 32-bit frame offset would read
    (or fault) elsewhere.  Only the last frame and the first carry data; the crop of the last must be the last's."""
    n_frames, hs, ws = 41, 3000, 6000
    assert (n_frames - 1) * hs * ws * 3 > 2 ** 31
    frames = torch.zeros((n_frames, hs, ws, 3), dtype=torch.uint8, device="cuda")
    corner = _frames(2, H, W, 3)
    frames[0, :H, :W], frames[-1, :H, :W] = torch.from_numpy(corner[0]).cuda(), torch.from_numpy(corner[1]).cuda()
    mat = torch.tensor([[1.0, 0, 0, 0, 1, 0]] * 2, device="cuda")
    src = torch.tensor([n_frames - 1, 0], dtype=torch.int32, device="cuda")
    got = _crop(frames, mat, src, H, W, PAD, "fp32").cpu().numpy()
    del frames
    for i, k in enumerate((1, 0)):
        want = ((corner[k].astype(np.float32) * (F(1) / F(255))) - np.asarray(MEAN, np.float32)) * (F(1) / np.asarray(STD, np.float32))
        assert np.array_equal(got[i, PAD:PAD + H, PAD:PAD + W, :3], want.astype(np.float32))


# ------------------------------------------------------------------------------------------------ lh_keypoints_to_boxes
def test_keypoints_to_boxes_is_bit_equal_to_the_host_restatement():
    from lighthand_amd.topdown import boxes_from_keypoints, boxes_from_keypoints_host
    j, min_joints, score = 21, 8, 0.25
    rng = np.random.RandomState(9)
    b = 70                                                          # more than one workgroup of 64 slots
    preds = rng.uniform(-50, 2000, size=(b, j, 2)).astype(np.float32)
    mv = rng.uniform(0, 0.5, size=(b, j, 1)).astype(np.float32)      # about half of the joints pass
    boxes = rng.uniform(0, 500, size=(b, 4)).astype(np.float32)
    src = rng.randint(0, 3, size=b).astype(np.int32)
    mv[0] = 0.9                                                     # every joint confident
    mv[1] = 0.01                                                    # none
    mv[2], mv[2, :min_joints - 1] = 0.01, 0.9                       # exactly min_joints - 1
    mv[3], mv[3, -min_joints:] = 0.01, score                        # exactly min_joints, each exactly at the threshold
    mv[4], src[4] = 0.9, -1                                         # an empty slot, every joint confident
    mv[5], preds[5] = 0.9, preds[5, :1] + rng.uniform(-3, 3, size=(j, 2)).astype(np.float32)      # a cluster narrower than min_side
    want_box, want_lost = boxes_from_keypoints_host(preds, mv, boxes, src, score, min_joints, 16.0)
    assert want_lost[:6].tolist() == [0, 1, 1, 0, 1, 0] and 5 < want_lost.sum() < b - 5
    nxt, lost = boxes_from_keypoints(torch.from_numpy(preds).cuda(), torch.from_numpy(mv).cuda(), torch.from_numpy(boxes).cuda(),
                                     torch.from_numpy(src).cuda(), score, min_joints, 16.0)
    torch.cuda.synchronize()
    assert lost.dtype == torch.int32 and lost.cpu().numpy().tolist() == want_lost.tolist()
    assert np.array_equal(nxt.cpu().numpy().view(np.int32), want_box.view(np.int32))


# ------------------------------------------------------------------------------------------------ InferStep / InferPipeline
B, SIZE, NF, FH, FW = 4, 64, 2, 96, 128
STEP_BOXES = [[20.0, 10.0, 90.0, 80.0], [60.5, 30.25, 140.0, 100.0], [-0.5, -0.5, FW - 0.5, FH - 0.5], [40.0, 40.0, 56.0, 70.0]]
STEP_INDEX = [0, 1, 1, 0]


def _model(seed=0):
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    torch.manual_seed(seed)
    return get_pose_net(resnet_cfg(18), True).cuda().set_precision("bf16").eval()


def _inputs(seed=31):
    return (torch.from_numpy(_frames(NF, FH, FW, seed)).cuda(), torch.tensor(STEP_BOXES, dtype=torch.float32).cuda(),
            torch.tensor(STEP_INDEX, dtype=torch.int32).cuda())


def _affine_np(mat, pts):
    m = mat[:, None, :]
    return np.stack([(m[..., 0] * pts[..., 0] + m[..., 1] * pts[..., 1]) + m[..., 2],
                     (m[..., 3] * pts[..., 0] + m[..., 4] * pts[..., 1]) + m[..., 5]], -1).astype(np.float32)


@pytest.mark.parametrize("options", [dict(), dict(flip_test=True, post_process="dark")], ids=["plain", "flip-dark"])
def test_infer_step_on_frames_end_to_end(options, monkeypatch):
    """Captured InferStep(frames=): after a replay plan.img_nhwc4 equals the stand-alone ABI calls on step.boxes bit for bit (mirrored
    once more under the flip test, whose second pass mirrors it in place); crop_preds, maxvals and the heat-maps equal a plain
    InferStep of the same options fed the fp32 crop as NCHW, bit for bit; preds are the fp32 affine of crop_preds."""
    from lighthand_amd.runtime import InferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    L, lib = _lib()
    model = _model()
    frames, boxes, index = _inputs()
    step = InferStep(model, B, SIZE, SIZE, frames=(NF, FH, FW), **options)
    assert step.images is None and step.next_boxes is None and step.lost is None
    assert step.boxes.cpu().tolist() == [[-0.5, -0.5, FW - 0.5, FH - 0.5]] * B and step.frame_index.cpu().tolist() == [0, 1, 0, 1]
    preds = step(frames=frames, boxes=boxes, frame_index=index)
    torch.cuda.synchronize()
    assert preds is step.preds and torch.equal(step.boxes, boxes) and step.valid.cpu().tolist() == [True] * B
    plan = step.plan
    mat, src = _box_affine(STEP_BOXES, STEP_INDEX, NF, SIZE, SIZE, 1.25)
    assert torch.equal(mat, plan.crop_mat) and torch.equal(src, plan.src_frame)
    ref_img = _crop(frames, mat, src, SIZE, SIZE, plan.img_pad, "bf16", wp=plan.img_wp)
    if options.get("flip_test"):
        L.check(lib.lh_nhwc4_mirror(ref_img.data_ptr(), B, SIZE, SIZE, plan.img_pad, plan.img_wp, plan.dt, _stream()), "lh_nhwc4_mirror")
        torch.cuda.synchronize()
    assert torch.equal(_bits(ref_img), _bits(plan.img_nhwc4))

    p = plan.img_pad
    crop32 = _crop(frames, mat, src, SIZE, SIZE, p, "fp32", wp=plan.img_wp)[:, p:p + SIZE, p:p + SIZE, :3].permute(0, 3, 1, 2).contiguous()
    plain = InferStep(model, B, SIZE, SIZE, **options)
    plain(crop32)
    torch.cuda.synchronize()
    assert torch.equal(step.heatmaps, plain.heatmaps)
    assert torch.equal(step.crop_preds, plain.preds) and torch.equal(step.maxvals, plain.maxvals)
    want = _affine_np(plan.crop_mat.cpu().numpy(), step.crop_preds.cpu().numpy())
    assert _close4(step.preds.cpu().numpy(), want)
    assert not torch.equal(step.preds, step.crop_preds)

    # an empty slot: black crop, preds (0, 0), valid False; the other slots do not move
    before = step.preds.clone()
    bad = boxes.clone()
    bad[1, 2] = float("nan")
    step(boxes=bad)
    torch.cuda.synchronize()
    assert step.valid.cpu().tolist() == [True, False, True, True]
    assert step.preds[1].abs().max().item() == 0
    if not options.get("flip_test"):                               # (batch statistics are off: slots are independent)
        assert torch.equal(step.preds[[0, 2, 3]], before[[0, 2, 3]])
    with pytest.raises(ValueError, match="frames"):
        step(torch.zeros(B, 3, SIZE, SIZE, device="cuda"))
    with pytest.raises(ValueError, match="frames"):
        plain(frames=frames)


def test_tracking_replay_reads_its_buffers(monkeypatch):
    """track=True with the threshold at the median confidence, so some joints pass and some do not: next_boxes / lost equal the host
    restatement of that replay's preds and maxvals; after advance() the second replay's crop_mat is the matrix of next_boxes and the
    image differs; the same inputs give the same bits again."""
    from lighthand_amd._lib import LightHandError
    from lighthand_amd.runtime import InferStep
    from lighthand_amd.topdown import box_affine_host, boxes_from_keypoints_host
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    frames, boxes, index = _inputs()
    probe = InferStep(model, B, SIZE, SIZE, frames=(NF, FH, FW))
    probe(frames=frames, boxes=boxes, frame_index=index)
    torch.cuda.synchronize()
    score = float(probe.maxvals.median())
    with pytest.raises(LightHandError, match="track=True"):
        probe.advance()
    step = InferStep(model, B, SIZE, SIZE, frames=(NF, FH, FW), track=True, track_min_score=score, track_min_joints=4, track_min_side=12.0)

    def run():
        step(frames=frames, boxes=boxes, frame_index=index)
        torch.cuda.synchronize()
        first = dict(preds=step.preds.clone(), maxvals=step.maxvals.clone(), next_boxes=step.next_boxes.clone(), lost=step.lost.clone(),
                     img=step.plan.img_nhwc4.clone(), mat=step.plan.crop_mat.clone())
        assert torch.equal(step.boxes, boxes)                       # the graph never writes the boxes
        step.advance()
        step()
        torch.cuda.synchronize()
        second = dict(preds=step.preds.clone(), next_boxes=step.next_boxes.clone(), lost=step.lost.clone(), img=step.plan.img_nhwc4.clone(),
                      mat=step.plan.crop_mat.clone(), boxes=step.boxes.clone())
        return first, second

    first, second = run()
    assert torch.equal(first["maxvals"], probe.maxvals) and torch.equal(first["preds"], probe.preds)
    passed = (first["maxvals"] >= score).sum().item()
    assert 0 < passed < B * 21
    want_box, want_lost = boxes_from_keypoints_host(first["preds"].cpu().numpy(), first["maxvals"].cpu().numpy(), boxes.cpu().numpy(),
                                                    np.asarray(STEP_INDEX, np.int32), score, 4, 12.0)
    assert first["lost"].cpu().numpy().tolist() == want_lost.tolist() and want_lost.sum() < B
    assert np.array_equal(first["next_boxes"].cpu().numpy().view(np.int32), want_box.view(np.int32))
    assert torch.equal(second["boxes"], first["next_boxes"])
    want_mat, want_src = box_affine_host(want_box, STEP_INDEX, NF, (SIZE, SIZE), 1.25)
    assert (want_src >= 0).all()
    # bit for bit: every operation of lh_box_affine is a correctly rounded fp32 one (the division too), in the host's order
    assert np.array_equal(second["mat"].cpu().numpy().view(np.int32), want_mat.view(np.int32))
    assert not torch.equal(second["mat"], first["mat"]) and not torch.equal(_bits(second["img"]), _bits(first["img"]))
    again_first, again_second = run()
    for a, b_ in ((first, again_first), (second, again_second)):
        for k in a:
            assert torch.equal(_bits(a[k]) if a[k].dtype == torch.bfloat16 else a[k], _bits(b_[k]) if b_[k].dtype == torch.bfloat16 else b_[k]), k


def test_infer_pipeline_on_frames(monkeypatch):
    """InferPipeline(frames=, depth=2): the two batches in flight return the single step's preds and maxvals bit for bit."""
    from lighthand_amd.runtime import InferPipeline, InferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    batches = []
    for k in range(2):
        frames, boxes, index = _inputs(seed=40 + k)
        batches.append(dict(frames=frames, boxes=boxes + 3.0 * k, frame_index=index.flip(0) if k else index))
    ref = InferStep(model, B, SIZE, SIZE, frames=(NF, FH, FW))
    want = []
    for kw in batches:
        ref(**kw)
        torch.cuda.synchronize()
        want.append((ref.preds.clone(), ref.maxvals.clone()))
    assert not torch.equal(want[0][0], want[1][0])
    pipe = InferPipeline(model, B, SIZE, SIZE, depth=2, frames=(NF, FH, FW))
    tickets = [pipe.submit(**kw) for kw in batches]
    for t, (p, m) in zip(tickets, want):
        gp, gm = pipe.result(t)
        torch.cuda.synchronize()
        assert torch.equal(gp, p) and torch.equal(gm, m)
    got = list(pipe.map(batches))
    assert len(got) == 2 and all(torch.equal(g[0], w[0]) and torch.equal(g[1], w[1]) for g, w in zip(got, want))


def test_track_frames_cli(capsys):
    """The closed loop of the tool on a tiny sequence: one JSON line with the rate, the lost slots and the options."""
    import json
    from lighthand_amd.tools import track_frames as T
    result = T.main(["--synthetic", "3", "--frame_size", "96x128", "--hands", "2", "--depth", "18", "--size", "64", "--flip_test", "--dark_decode"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == result
    assert result["frames"] == 3 and result["slots"] == 6 and 0 <= result["slots_lost"] <= 6 and result["frames_per_s"] > 0
    assert np.isfinite(result["track_min_score"])                    # the first frame's median confidence
    assert result["frame_size"] == [96, 128] and result["flip_test"] is True and result["dark_decode"] is True
