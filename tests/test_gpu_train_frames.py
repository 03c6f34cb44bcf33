"""GPU: training on hand ROIs cropped from full frames -- lh_roi_perturb / lh_affine_points_inv against their numpy restatements
(lighthand_amd.topdown, bit for bit), and runtime.TrainStep(frames=..., roi_aug=...) on top of them: the crop is InferStep's, the
whole-frame step is the uint8 step, image and joints move together under the augmentation, replays read the draw, empty slots
carry no loss."""
import numpy as np
import pytest
import torch

from conftest import resnet_cfg

pytestmark = pytest.mark.gpu

F = np.float32
SIZE = 64                      # the crop (and the smallest input the step tests use); heat-maps are 16 x 16
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _np_bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint16)


def _model(seed=0):
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    torch.manual_seed(seed)
    return get_pose_net(resnet_cfg(18), True).cuda().set_precision("bf16")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the kernels, bit for bit
def _slots(b=67):
    """b ROIs with a seeded draw each, and every special slot the entry documents."""
    from lighthand_amd.runtime import sample_roi_aug
    rng = np.random.RandomState(17)
    lo = rng.uniform(-10, 60, size=(b, 2))
    boxes = np.concatenate([lo, lo + rng.uniform(12, 60, size=(b, 2))], 1).astype(np.float32)
    ang = rng.uniform(-np.pi, np.pi, b)
    rot = (np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(0.4, 3.0, size=(b, 1))).astype(np.float32)
    mirror = (rng.randint(0, 2, b) * rng.randint(1, 4, b)).astype(np.int32)
    index = rng.randint(0, 3, b).astype(np.int32)
    aug = sample_roi_aug(b, 180.0, 0.3, 0.15, 0.5, generator=torch.Generator().manual_seed(2)).numpy()
    aug[[0, 1, 64, 66]] = (1, 0, 1, 0, 0, 0)                 # identity rows, one of them in the second block
    aug[2] = (1, 0, 1, 0, 0, 1)                              # a flip and nothing else
    aug[3, 5], mirror[3] = 1, 2                              # a flipped slot whose mirror is set
    rot[4] = 0                                               # rot = (0, 0)
    index[5] = -1                                            # frame_index = -1
    boxes[6, 2] = boxes[6, 0]                                # a zero-width box
    boxes[7, 1] = np.nan                                     # a NaN box
    aug[8, 2] = np.nan                                       # a NaN aug row
    aug[9, 0] = np.inf
    rot[10, 0] = np.nan
    return boxes, rot, mirror, index, aug


def test_roi_perturb_matches_the_restatement_bit_for_bit():
    from lighthand_amd import _lib as L
    from lighthand_amd.topdown import roi_perturb, roi_perturb_host
    boxes, rot, mirror, _, aug = _slots()
    for r, m in ((rot, mirror), (None, None)):               # rot_dev = mirror_dev = NULL: (1, 0) and 0
        want = roi_perturb_host(boxes, r, m, aug)
        got = roi_perturb(_cuda(boxes), None if r is None else _cuda(r), None if m is None else _cuda(m), _cuda(aug))
        torch.cuda.synchronize()
        for g, w, what in zip(got, want, ("boxes", "rot", "mirror")):
            assert np.array_equal(_np_bits(g.cpu().numpy()), _np_bits(w)), what
    assert np.array_equal(_np_bits(want[0][[0, 1, 64, 66, 7, 8, 9]]), _np_bits(boxes[[0, 1, 64, 66, 7, 8, 9]]))
    changed = np.abs(want[0] - boxes).max(1) > 0
    assert changed[11:64].all() and not changed[[0, 1, 64, 66]].any()          # (slot 2, the flip alone, is recomputed: an ulp may move)
    # aliased outputs are refused with an error text, before any launch
    lib = L.load()
    d = [_cuda(x) for x in (boxes, rot, mirror, aug)]
    ob, orot, om = torch.empty_like(d[0]), torch.empty_like(d[1]), torch.empty_like(d[2])
    for outs in ((d[0], orot, om), (ob, d[1], om), (ob, orot, d[2])):
        rc = lib.lh_roi_perturb(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 67, outs[0].data_ptr(), outs[1].data_ptr(),
                                outs[2].data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == -1 and b"lh_roi_perturb" in lib.lh_last_error() and b"alias" in lib.lh_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_np_bits(d[0].cpu().numpy()), _np_bits(boxes))          # nothing ran


def test_affine_points_inv_matches_the_restatement_bit_for_bit():
    from lighthand_amd.topdown import POINT_OFF, affine_points_inv, affine_points_inv_host, roi_affine_host, roi_perturb_host
    boxes, rot, mirror, index, aug = _slots()
    b, j = 67, 21
    mat, src = roi_affine_host(*roi_perturb_host(boxes, rot, mirror, aug), index, 3, (SIZE, SIZE), 1.25)
    assert (src[[4, 5, 6, 7, 10]] == -1).all() and (src[11:] >= 0).all()
    mat[12] = [1, 2, 0, 2, 4, 0]                             # live but singular
    mat[13, 4] = np.inf                                      # live, det not finite
    mat[14] = [1, 0, 0, 0, 1, 0]
    rng = np.random.RandomState(3)
    pts = rng.uniform(-40, 140, size=(b, j, 3)).astype(np.float32)          # pstride = 3; column 2 must never be read
    pts[..., 2] = np.nan
    want = affine_points_inv_host(pts, mat, src)
    got = affine_points_inv(_cuda(pts), _cuda(mat), _cuda(src))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == (b, j, 2) and np.array_equal(_np_bits(got), _np_bits(want))
    assert (got[[4, 5, 6, 7, 10, 12, 13]] == F(POINT_OFF)).all() and np.isfinite(got).all()
    assert np.array_equal(_np_bits(got[14]), _np_bits(pts[14, :, :2]))
    # ostride: the columns past the first two of the output are not written
    from lighthand_amd import _lib as L
    out = torch.full((b, j, 3), 5.0, device="cuda")
    d = [_cuda(pts), _cuda(mat), _cuda(src)]
    L.check(L.load().lh_affine_points_inv(d[0].data_ptr(), 3, d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), 3, b, j,
                                          torch.cuda.current_stream().cuda_stream), "lh_affine_points_inv")
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[..., 2] == 5).all() and np.array_equal(_np_bits(np.ascontiguousarray(out[..., :2])), _np_bits(want))


# ------------------------------------------------------------------------------------------------ 2. the crop is InferStep's
def _interior(plan):
    p = plan.img_pad
    return plan.img_nhwc4[:, p:p + plan.h, p:p + plan.w, :]


@pytest.mark.parametrize("case", ["rgb", "antialias", "nv12"])
def test_identity_roi_aug_crops_what_infer_step_crops(case, monkeypatch):
    """TrainStep(frames=..., roi_aug=(0, 0, 0)) and InferStep(frames=..., oriented=True) on the same frames, boxes, rot and mirror:
    the crops that reach the stem are equal bit for bit (the interiors: the two plans pad their input as their stems need)."""
    from lighthand_amd import topdown
    from lighthand_amd.runtime import InferStep, TrainStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    b, n, hs, ws = 4, 3, 96, 128
    rng = np.random.RandomState(5)
    rgb = rng.randint(0, 256, size=(n, hs, ws, 3)).astype(np.uint8)
    centre = rng.uniform(35, 60, size=(b, 2)) + [15, 0]
    half = rng.uniform(14, 24, size=(b, 2)) if case != "antialias" else rng.uniform(60, 90, size=(b, 2))      # minified: > 1 frame px per crop px
    boxes = np.concatenate([centre - half, centre + half], 1).astype(np.float32)
    rot = np.array([topdown.rot_from_angle(a) for a in (0.0, 0.7, -2.2, 3.0)], np.float32) * F(1.7)
    mirror = np.array([0, 1, 0, 1], np.int32)
    index = np.array([0, 2, 1, 2], np.int32)
    opts = dict(frames=(n, hs, ws), box_padding=1.25)
    frames = rgb
    if case == "antialias":
        opts["antialias"] = True
    if case == "nv12":
        opts["frame_format"] = "nv12"
        frames = topdown.rgb_to_nv12_host(rgb)
    args = dict(frames=_cuda(frames), boxes=_cuda(boxes), frame_index=_cuda(index), rot=_cuda(rot), mirror=_cuda(mirror))
    model = _model()
    inf = InferStep(model.eval(), b, SIZE, SIZE, oriented=True, **opts)
    inf(**args)
    torch.cuda.synchronize()
    want, want_mat = _interior(inf.plan).clone(), inf.plan.crop_mat.clone()
    if case == "antialias":
        assert (topdown.crop_taps_host(want_mat.cpu().numpy()) > 1).all()
    st = TrainStep(model, b, SIZE, SIZE, roi_aug=(0, 0, 0), **opts)
    joints = _cuda(rng.uniform(20, 80, size=(b, 21, 2)).astype(np.float32))
    st(joints=joints, **args)
    torch.cuda.synchronize()
    assert torch.equal(st.plan.roi_aug.cpu(), torch.tensor(topdown.ROI_AUG_IDENTITY).expand(b, 6))
    assert torch.equal(_bits(st.plan.crop_mat), _bits(want_mat)) and bool(st.valid.all())
    got = _interior(st.plan)
    assert got.dtype == want.dtype and torch.equal(_bits(got), _bits(want))
    assert float(got.float().abs().max()) > 1 and np.isfinite(float(st.loss))
    assert torch.equal(st.boxes, args["boxes"]) and torch.equal(st.rot, args["rot"]) and torch.equal(st.mirror, args["mirror"])


# ------------------------------------------------------------------------------------------------ 3. the whole-frame step is the uint8 step
def test_whole_frame_step_is_the_uint8_step(monkeypatch):
    """TrainStep(frames=(B, h, w), box_padding=1.0) with whole-frame boxes and frame_index = arange(B) (the plan's defaults) against
    TrainStep(input_u8=(h, w)) on the same images, joints and seeded init: the matrix is (1, 0, 0, 0, 1, 0), so the first step's
    target, loss, preds and maxvals are bit-equal and frame_preds == preds; the three-step loss trajectories agree within what two
    identical runs of the uint8 step differ by (measured here from the existing path; 0 expected)."""
    from lighthand_amd.runtime import TrainStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    b = 4
    rng = np.random.RandomState(8)
    images = _cuda(rng.randint(0, 256, size=(b, SIZE, SIZE, 3)).astype(np.uint8))
    joints = _cuda(rng.uniform(6, SIZE - 6, size=(b, 21, 2)).astype(np.float32))

    def run(frames):
        st = TrainStep(_model(), b, SIZE, SIZE, lr=1e-3, **(dict(frames=(b, SIZE, SIZE), box_padding=1.0) if frames else dict(input_u8=(SIZE, SIZE))))
        first = float(st(frames=images, joints=joints) if frames else st(images, joints))
        torch.cuda.synchronize()
        snap = {k: getattr(st, k).clone() for k in ("target", "preds", "maxvals")}
        losses = [first] + [float(st()) for _ in range(2)]
        torch.cuda.synchronize()
        return st, snap, losses

    _, snap_a, loss_a = run(False)
    _, snap_b, loss_b = run(False)
    noise = [abs(x - y) for x, y in zip(loss_a, loss_b)]
    st, snap, loss = run(True)
    print(f"uint8 step {loss_a}, again {loss_b} (differs by {noise}), frames step {loss}")
    assert all(np.isfinite(loss))
    assert torch.equal(st.plan.crop_mat.cpu(), torch.tensor([1.0, 0, 0, 0, 1, 0]).expand(b, 6)) and bool(st.valid.all())
    assert torch.equal(_bits(st.joints_crop), _bits(joints)) and torch.equal(st.joints, joints)
    for k in ("target", "preds", "maxvals"):
        assert torch.equal(_bits(snap[k]), _bits(snap_a[k])), k
    assert loss[0] == loss_a[0]
    for x, y, tol in zip(loss, loss_a, noise):
        assert abs(x - y) <= tol
    assert torch.equal(st.frame_preds, st.preds)


# ------------------------------------------------------------------------------------------------ 4. image and joints move together
def _constellation(b, hs, ws, seed, box=40):
    """b black frames with a 3 x 3 white square at each of 21 joints on a jittered 8-pixel grid inside a box x box region (blobs at
    least 6 frame pixels apart), the region's box per slot."""
    rng = np.random.RandomState(seed)
    frames = np.zeros((b, hs, ws, 3), np.uint8)
    joints = np.zeros((b, 21, 2), np.float32)
    boxes = np.zeros((b, 4), np.float32)
    for i in range(b):
        x0, y0 = rng.randint(20, ws - box - 20), rng.randint(20, hs - box - 20)
        cells = rng.permutation(25)[:21]
        for k, c in enumerate(cells):
            x, y = x0 + 4 + 8 * (c % 5) + rng.randint(-1, 2), y0 + 4 + 8 * (c // 5) + rng.randint(-1, 2)
            frames[i, y - 1:y + 2, x - 1:x + 2] = 255
            joints[i, k] = (x, y)
        boxes[i] = (x0 - 0.5, y0 - 0.5, x0 + box - 0.5, y0 + box - 0.5)
    return frames, joints, boxes


def test_image_and_joints_move_together(monkeypatch):
    """Black frames with a 3 x 3 white square at each joint, roi_aug=(180, 0.3, 0.15, 0.5) over 16 slots: wherever the draw puts the
    ROI, the blob of a joint is in the crop where joints_crop says -- for every joint of weight 1 whose 7 x 7 window lies inside the
    crop, the brightest pixels within 3 px of joints_crop (a magnified blob is a plateau of equal pixels: their centre) lie within
    1 px of it: half a pixel of rounding plus the bilinear spread of the blob.  The boxes are 40 px on a 64 px crop with padding 1: at
    most 40 * 1.3 / 64 = 0.81 frame pixels per crop pixel, magnified.  And frame_preds of a heat-map forced to the target returns the
    frame joints within one heat-map cell (4 crop px) times the ROI scale.  A rotation sign, the mirror or the shift axes that
    disagreed between lh_roi_perturb, lh_roi_affine and the inverse would fail here; the bit-equality tests cannot see that."""
    from lighthand_amd.runtime import TrainStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    b, hs, ws = 16, 96, 128
    frames, joints, boxes = _constellation(b, hs, ws, 31)
    spec = dict(rotation=180.0, scale=0.3, shift=0.15, mirror_prob=0.5, generator=torch.Generator().manual_seed(77))
    st = TrainStep(_model(), b, SIZE, SIZE, frames=(b, hs, ws), box_padding=1.0, roi_aug=spec, use_target_weight=True)
    st(frames=_cuda(frames), boxes=_cuda(boxes), frame_index=torch.arange(b, dtype=torch.int32).cuda(), joints=_cuda(joints))
    torch.cuda.synchronize()
    aug = st.plan.roi_aug.cpu().numpy()
    assert (aug[:, 5] == 1).any() and (aug[:, 5] == 0).any() and (aug[:, 1] < 0).any() and (aug[:, 1] > 0).any() and (aug[:, 0] < 0).any()
    mat = st.plan.crop_mat.cpu().numpy()
    scale = np.hypot(mat[:, 0], mat[:, 3])
    assert bool(st.valid.all()) and scale.max() <= 0.82 and scale.min() >= 0.43
    assert (np.sign(mat[:, 0] * mat[:, 4] - mat[:, 1] * mat[:, 3]) == np.where(aug[:, 5] == 1, -1, 1)).all()          # mirrored slots flip
    crop = _interior(st.plan)[..., 0].float().cpu().numpy() * STD[0] + MEAN[0]          # de-normalised red channel, [b][64][64]
    jc, weight = st.joints_crop.cpu().numpy(), st.target_weight.cpu().numpy()[..., 0]
    ys, xs = np.mgrid[0:SIZE, 0:SIZE]
    checked, worst = 0, 0.0
    for i in range(b):
        for k in range(21):
            x, y = jc[i, k]
            if weight[i, k] != 1 or not (3.5 <= x <= SIZE - 4.5 and 3.5 <= y <= SIZE - 4.5):
                continue
            near = (np.abs(xs - x) <= 3) & (np.abs(ys - y) <= 3)
            top = near & (crop[i] >= np.where(near, crop[i], -1).max() - 1e-6)
            assert np.where(near, crop[i], -1).max() > 0.9, (i, k, x, y)
            d = max(abs(xs[top].mean() - x), abs(ys[top].mean() - y))
            worst, checked = max(worst, d), checked + 1
            assert d <= 1.0, (i, k, x, y, d)
    print(f"{checked} of {b * 21} joints checked, the blob's centre at most {worst:.2f} px from joints_crop")
    assert checked > b * 21 // 2
    # the heat-map forced to the target: decode and map-back return the frame joints
    st.plan.out_nchw.copy_(st.target)
    st._fwd_loss_tail(torch.cuda.current_stream().cuda_stream, target_done=True)
    torch.cuda.synchronize()
    fp = st.frame_preds.cpu().numpy()
    inside = (weight == 1) & (jc[..., 0] >= 0) & (jc[..., 0] <= SIZE - 3) & (jc[..., 1] >= 0) & (jc[..., 1] <= SIZE - 3)      # the peak's cell is on the map
    dist = np.hypot(fp[..., 0] - joints[..., 0], fp[..., 1] - joints[..., 1])
    print(f"frame_preds: worst {np.max((dist / (4 * scale[:, None]))[inside]):.2f} of one heat-map cell times the ROI scale over {inside.sum()} joints")
    assert inside.sum() > b * 21 // 2 and (dist[inside] <= 4 * np.broadcast_to(scale[:, None], dist.shape)[inside]).all()


# ------------------------------------------------------------------------------------------------ 5. replays read the draw
def test_replays_read_the_draw(monkeypatch):
    from lighthand_amd.runtime import TrainStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    b, hs, ws = 4, 96, 128
    frames, joints, boxes = _constellation(b, hs, ws, 41)
    args = dict(frames=_cuda(frames), boxes=_cuda(boxes), frame_index=torch.arange(b, dtype=torch.int32).cuda(), joints=_cuda(joints))

    def step(use_graph):
        return TrainStep(_model(), b, SIZE, SIZE, lr=1e-3, frames=(b, hs, ws), roi_aug=dict(rotation=40.0, scale=0.2, shift=0.1, mirror_prob=0.5),
                         use_graph=use_graph)

    def call(st, seed, first=False):
        st.roi_aug["generator"] = torch.Generator().manual_seed(seed)
        loss = float(st(**args) if first else st())
        torch.cuda.synchronize()
        return st.plan.crop_mat.clone(), st.joints_crop.clone(), st.target.clone(), loss

    st = step(True)
    one = call(st, 1, first=True)
    two = call(st, 2)
    again = call(st, 1)
    assert st.graphs is not None
    assert not torch.equal(one[0], two[0]) and not torch.equal(one[1], two[1]) and not torch.equal(one[2], two[2])
    for x, y in zip(one[:3], again[:3]):
        assert torch.equal(_bits(x), _bits(y))
    assert torch.equal(st.boxes, args["boxes"])                                # the caller's ROI is never written
    eager = call(step(False), 1, first=True)
    for x, y in zip(one[:3], eager[:3]):
        assert torch.equal(_bits(x), _bits(y))
    assert eager[3] == one[3] and np.isfinite(one[3])


# ------------------------------------------------------------------------------------------------ 6. empty slots
@pytest.mark.parametrize("encoding", ["quantised", "unbiased"])
def test_empty_slots_carry_no_loss(encoding, monkeypatch):
    from lighthand_amd.runtime import TrainStep
    from lighthand_amd.topdown import POINT_OFF
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    b, hs, ws = 6, 96, 128
    frames, joints, boxes = _constellation(b, hs, ws, 51)
    index = np.arange(b, dtype=np.int32)
    index[[1, 4]] = -1
    st = TrainStep(_model(), b, SIZE, SIZE, lr=1e-3, frames=(b, hs, ws), box_padding=1.0, use_target_weight=True, target_encoding=encoding,
                   coord_loss_weight=0.1)
    loss = float(st(frames=_cuda(frames), boxes=_cuda(boxes), frame_index=_cuda(index), joints=_cuda(joints)))
    torch.cuda.synchronize()
    assert np.isfinite(loss) and loss > 0 and np.isfinite(float(st.coord_loss))
    assert st.valid.cpu().tolist() == [True, False, True, True, False, True]
    weight = st.target_weight.cpu().numpy()[..., 0]
    assert not weight[[1, 4]].any() and weight[[0, 2, 3, 5]].all()
    assert not st.target[[1, 4]].any() and bool((st.target[[0, 2, 3, 5]].amax((2, 3)) > 0.5).all())
    assert bool((st.joints_crop[[1, 4]] == POINT_OFF).all()) and not st.coord_joint_loss[[1, 4]].any()
    black = _interior(st.plan)[[1, 4]][..., :3].float()
    assert torch.equal(black, black[:, :1, :1].expand_as(black)) and bool((black < 0).all())          # an empty slot's crop is black
    assert np.isfinite(float(st())) and torch.isfinite(st.model.arena().flat).all()


# ------------------------------------------------------------------------------------------------ 7. the training tool
def test_train_cli_on_frames(tmp_path, monkeypatch):
    """main() with --frame_size and all four ROI factors: one epoch on 12 synthetic frames (a short last batch included) trains with
    finite losses through TrainStep(frames=, roi_aug=), validates through InferStep(frames=) and writes the checkpoint."""
    import os
    from lighthand_amd import runtime
    from lighthand_amd.tools import train as T
    made = []
    real_init = runtime.TrainStep.__init__

    def spy(self, *a, **k):
        real_init(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(runtime.TrainStep, "__init__", spy)
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    args = T.parse_args(["--root_path", str(tmp_path), "--batch_size", "8", "--epoch", "1", "--depth", "18", "--size", "64", "--precision", "bf16",
                         "--reset", "--name", "frames", "--synthetic", "12", "--val_synthetic", "8", "--frame_size", "96x128", "--roi_rot", "30",
                         "--roi_scale", "0.25", "--roi_shift", "0.1", "--roi_mirror", "0.5", "--use_target_weight"])
    args.num_workers = 0
    best = T.main(args)
    assert np.isfinite(best)
    assert sorted(st.joints.shape[0] for st in made) == [4, 8]
    for st in made:
        assert st.roi_aug["rotation"] == 30.0 and st.joints_crop is not None and tuple(st.frames.shape) == (st.joints.shape[0], 96, 128, 3)
        assert np.isfinite(float(st.loss)) and bool(st.valid.all())
        assert not torch.equal(st.plan.roi_aug.cpu(), torch.tensor([1.0, 0, 1, 0, 0, 0]).repeat(st.joints.shape[0], 1))
    assert os.path.isfile(os.path.join(args.output_dir, "checkpoint-good", "state_dict.bin"))
