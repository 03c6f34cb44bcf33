"""GPU: online geometric augmentation -- lh_image_u8_warp_to_nhwc4 (per-image affine warp in front of the fused uint8 input
pipeline, with and without ColorJitter), lh_affine_points, and TrainStep(geometric_aug=) / the training CLI on top of them.

The warp rule restated in numpy (fp32, the kernels are built with -ffp-contract=off): output pixel (ox, oy) samples the resized
frame at u = (a ox + b oy + c, d ox + e oy + f); inside [-0.5, w-0.5] x [-0.5, h-0.5] with the resize rule of
oracle/color.py's resize_bilinear at u, outside as black (0 before ColorJitter and Normalize)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

from conftest import resnet_cfg

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DT = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}
F = np.float32


def warp_reference(u8, h, w, inv, factors=None, order=None):
    """uint8 [hs, ws, 3] -> warped, resized [ColorJitter] normalised float32 [3, h, w]."""
    from oracle import color as oc
    hs, ws = u8.shape[:2]
    a, b, c, d, e, f = np.asarray(inv, np.float32)
    oy, ox = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    ux, uy = (a * ox + b * oy) + c, (d * ox + e * oy) + f
    inside = (ux >= F(-0.5)) & (ux <= F(w) - F(0.5)) & (uy >= F(-0.5)) & (uy <= F(h) - F(0.5))
    sy, sx = F(hs) / F(h), F(ws) / F(w)
    fy = np.maximum((uy + F(0.5)) * sy - F(0.5), F(0)).astype(np.float32)
    fx = np.maximum((ux + F(0.5)) * sx - F(0.5), F(0)).astype(np.float32)
    fy, fx = np.where(inside, fy, F(0)), np.where(inside, fx, F(0))
    y0, x0 = np.minimum(fy.astype(np.int32), hs - 1), np.minimum(fx.astype(np.int32), ws - 1)
    y1, x1 = np.minimum(y0 + 1, hs - 1), np.minimum(x0 + 1, ws - 1)
    wy, wx = fy - y0.astype(np.float32), fx - x0.astype(np.float32)
    src = np.transpose(u8.astype(np.float32), (2, 0, 1))
    a00, a01, a10, a11 = src[:, y0, x0], src[:, y0, x1], src[:, y1, x0], src[:, y1, x1]
    top, bot = a00 + (a01 - a00) * wx, a10 + (a11 - a10) * wx
    img = np.where(inside, (top + (bot - top) * wy) * (F(1) / F(255)), F(0)).astype(np.float32)
    if order is not None:
        img = oc.color_jitter(img, factors, order)
    m, s = np.asarray(MEAN, np.float32)[:, None, None], np.asarray(STD, np.float32)[:, None, None]
    return ((img - m) * (F(1) / s)).astype(np.float32)


def _lib():
    from lighthand_amd import _lib as L
    return L, L.load()


def _run(u8, h, w, pad, dtype, inv=None, factors=None, order=None):
    """One call of the warp entry (inv given) or of the plain / jitter entries; returns the padded NHWC4 output."""
    L, lib = _lib()
    n, hs, ws = u8.shape[:3]
    wp = w + 2 * pad + 2
    code, tdt = DT[dtype]
    out = torch.full((n, h + 2 * pad, wp, 4), float("nan"), dtype=tdt, device="cuda")
    m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    ws_j = torch.empty(lib.lh_image_jitter_workspace_bytes(n), dtype=torch.uint8, device="cuda") if factors is not None else None
    f_keep = (factors.cuda() if factors is not None else None, order.cuda() if order is not None else None)
    fp, fo = (f_keep[0].data_ptr(), f_keep[1].data_ptr()) if factors is not None else (None, None)
    s = torch.cuda.current_stream().cuda_stream
    if inv is not None:
        inv_d = inv.cuda()
        L.check(lib.lh_image_u8_warp_to_nhwc4(u8.data_ptr(), out.data_ptr(), n, hs, ws, h, w, pad, wp, m3, s3, inv_d.data_ptr(), fp, fo,
                                              ws_j.data_ptr() if ws_j is not None else None, code, s), "lh_image_u8_warp_to_nhwc4")
    elif factors is not None:
        L.check(lib.lh_image_u8_jitter_to_nhwc4(u8.data_ptr(), out.data_ptr(), n, hs, ws, h, w, pad, wp, m3, s3, fp, fo, ws_j.data_ptr(),
                                                code, s), "lh_image_u8_jitter_to_nhwc4")
    else:
        L.check(lib.lh_image_u8_to_nhwc4(u8.data_ptr(), out.data_ptr(), n, hs, ws, h, w, pad, wp, m3, s3, code, s), "lh_image_u8_to_nhwc4")
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _jitter_draw(n, seed):
    from lighthand_amd.runtime import sample_color_jitter
    perms = list(itertools.permutations(range(4)))
    factors, order = sample_color_jitter(n, generator=torch.Generator().manual_seed(seed))
    for i in range(n):
        order[i] = torch.tensor(perms[i % len(perms)], dtype=torch.int32)
    return factors, order


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("src", [(224, 224), (256, 256), (300, 200)])
def test_identity_warp_is_bit_equal_to_the_plain_pipelines(dtype, src):
    """Identity matrices reproduce lh_image_u8_to_nhwc4 and (all 24 op orders) lh_image_u8_jitter_to_nhwc4 bit for bit."""
    n, (hs, ws) = 24, src
    g = torch.Generator().manual_seed(hs + ws)
    u8 = torch.randint(0, 256, (n, hs, ws, 3), dtype=torch.uint8, generator=g).cuda()
    eye = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]).repeat(n, 1)
    plain, warped = _run(u8, 256, 256, 3, dtype), _run(u8, 256, 256, 3, dtype, inv=eye)
    assert torch.equal(_bits(plain), _bits(warped))
    factors, order = _jitter_draw(n, 11)
    plain, warped = _run(u8, 256, 256, 3, dtype, factors=factors, order=order), _run(u8, 256, 256, 3, dtype, inv=eye, factors=factors, order=order)
    assert torch.equal(_bits(plain), _bits(warped))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_exact_matrices_rotate_flip_and_shift(dtype):
    """90 and 180 degree rotations about the centre and an integer shift sample the identity output at integer positions: the
    result is rot90 / flip / shift of it bit for bit, and the exposed band is exactly (0 - mean) / std in the run dtype."""
    n, h, w, pad = 3, 256, 256, 3
    u8 = torch.randint(0, 256, (n, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).cuda()
    ident = _run(u8, h, w, pad, dtype)[:, pad:pad + h, pad:pad + w, :3].float().cpu()
    tx, ty = 17, -9
    inv = torch.tensor([[0.0, 1.0, 0.0, -1.0, 0.0, w - 1.0],             # u = (oy, w-1-ox): a quarter turn about the centre
                        [-1.0, 0.0, w - 1.0, 0.0, -1.0, h - 1.0],        # half turn
                        [1.0, 0.0, -tx, 0.0, 1.0, -ty]])                  # content moves by (+17, -9)
    got_full = _run(u8, h, w, pad, dtype, inv=inv)
    got = got_full[:, pad:pad + h, pad:pad + w, :3].float().cpu()
    OY, OX = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    assert torch.equal(got[0], ident[0][(w - 1) - OX, OY])
    assert torch.equal(got[0], torch.rot90(ident[0], k=-1, dims=(0, 1)))
    assert torch.equal(got[1], torch.flip(ident[1], dims=(0, 1)))
    band = (torch.tensor([(F(0) - F(m)) * (F(1) / F(s)) for m, s in zip(MEAN, STD)], dtype=torch.float32)).to(DT[dtype][1]).float()
    inside = ((OX - tx) >= 0) & ((OY - ty) < h)
    want = torch.empty_like(ident[2])
    want[:] = band
    sy, sx = OY[inside] - ty, OX[inside] - tx
    want[inside] = ident[2][sy, sx]
    assert torch.equal(got[2], want)
    assert int((~inside).sum()) == tx * h + (-ty) * w - tx * (-ty)
    assert float(got_full[:, :pad].float().abs().max()) == 0 and float(got_full[..., 3].float().abs().max()) == 0


@pytest.mark.parametrize("jitter", [False, True])
def test_random_matrices_match_the_numpy_rule(jitter):
    """Rotation +-45 degrees, scale 0.7-1.3, shift +-15 %: the kernel against warp_reference.  As in the jitter test, a handful of
    pixels may take the other branch of a hue-sector / clamp boundary after fp32 reassociation of the strip-summed grey mean."""
    from lighthand_amd.runtime import sample_affine
    n, h, w, pad = 12, 256, 256, 3
    u8n = np.random.RandomState(5).randint(0, 256, size=(n, 224, 224, 3)).astype(np.uint8)
    u8n[1] = u8n[1][..., :1]                                          # a grey image (hue no-op)
    inv, _ = sample_affine(n, 45.0, 0.3, 0.15, generator=torch.Generator().manual_seed(6), size=(h, w))
    factors, order = _jitter_draw(n, 13) if jitter else (None, None)
    got = _run(torch.from_numpy(u8n).cuda(), h, w, pad, "fp32", inv=inv, factors=factors, order=order).cpu().numpy()
    worst = 0.0
    for i in range(n):
        want = warp_reference(u8n[i], h, w, inv[i].numpy(), factors[i].numpy() if jitter else None,
                              [int(v) for v in order[i]] if jitter else None)
        g = np.transpose(got[i, pad:pad + h, pad:pad + w, :3], (2, 0, 1))
        d = np.abs(g - want)
        assert (d > 1e-4).mean() < 1e-3, (i, float(d.max()))
        worst = max(worst, float(np.median(d)))
    assert worst < 1e-6


def test_affine_points_and_disc_consistency():
    """lh_affine_points against numpy (a few fp32 ulps); then 21 bright discs drawn at the joints of a synthetic frame, warped:
    each disc's arg-max lands within 1 px of its transformed joint, and the target rendered from the transformed joints peaks
    within one heat-map pixel of it."""
    from lighthand_amd.heatmap import render_targets
    from lighthand_amd.runtime import sample_affine
    L, lib = _lib()
    s = torch.cuda.current_stream().cuda_stream
    b, j = 37, 21
    pts = torch.from_numpy(np.random.RandomState(1).uniform(-40, 300, size=(b, j, 3)).astype(np.float32))
    inv, fwd = sample_affine(b, 45.0, 0.3, 0.15, generator=torch.Generator().manual_seed(2), size=(256, 256))
    out = torch.full((b, j, 2), float("nan"), device="cuda")
    pts_d, fwd_d = pts.cuda(), fwd.cuda()                            # held: a bare .cuda().data_ptr() frees the block at once
    L.check(lib.lh_affine_points(pts_d.data_ptr(), 3, fwd_d.data_ptr(), out.data_ptr(), 2, b, j, s), "lh_affine_points")
    got = out.cpu().numpy()
    p, m = pts.numpy(), fwd.numpy()[:, None, :]
    want = np.stack([(m[..., 0] * p[..., 0] + m[..., 1] * p[..., 1]) + m[..., 2], (m[..., 3] * p[..., 0] + m[..., 4] * p[..., 1]) + m[..., 5]], -1)
    assert (np.abs(got - want) <= 4 * np.spacing(np.abs(want).astype(np.float32))).all()

    n, size = 4, 256
    gy, gx = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
    grid = np.stack([gx.ravel(), gy.ravel()], 1)[:j].astype(np.float32) * 24 + 80     # joints 24 px apart around the centre
    joints = np.stack([grid + np.random.RandomState(k).uniform(-1, 1, size=grid.shape).astype(np.float32) for k in range(n)])
    yy, xx = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    frames = np.zeros((n, size, size, 3), np.uint8)
    for k in range(n):
        cone = np.zeros((size, size), np.float32)
        for x, y in joints[k]:
            cone = np.maximum(cone, 255 * np.clip(1 - np.hypot(xx - x, yy - y) / 6, 0, 1))
        frames[k] = np.round(cone)[..., None]
    inv, fwd = sample_affine(n, 30.0, 0.15, 0.05, generator=torch.Generator().manual_seed(3), size=(size, size))
    img = _run(torch.from_numpy(frames).cuda(), size, size, 0, "fp32", inv=inv)[..., 0].cpu().numpy()
    ja = torch.zeros(n, j, 2, device="cuda")
    joints_d, fwd_d = torch.from_numpy(joints).cuda(), fwd.cuda()
    L.check(lib.lh_affine_points(joints_d.data_ptr(), 2, fwd_d.data_ptr(), ja.data_ptr(), 2, n, j, s), "lh_affine_points")
    torch.cuda.synchronize()
    jan = ja.cpu().numpy()
    for k in range(n):
        for x, y in jan[k]:
            cx, cy = int(round(float(x))), int(round(float(y)))
            assert 10 <= cx < size - 10 and 10 <= cy < size - 10
            win = img[k, cy - 5:cy + 6, cx - 5:cx + 6]                  # discs >= 18 px apart after the warp: one per window
            py, px = np.unravel_index(np.argmax(win), win.shape)
            assert max(abs(px - 5 + cx - x), abs(py - 5 + cy - y)) <= 1.0, (k, x, y, px, py)
    tgt = render_targets(ja).cpu().numpy()
    hm = tgt.shape[-1]
    for k in range(n):
        for jj in range(j):
            py, px = np.unravel_index(np.argmax(tgt[k, jj]), (hm, hm))
            assert abs(px - jan[k, jj, 0] / 4) <= 1.0 and abs(py - jan[k, jj, 1] / 4) <= 1.0


def _model(kind, seed=0):
    from lighthand_amd.modeling.hrnet.pose_hrnet import get_hrnet, hrnet_cfg
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    torch.manual_seed(seed)
    if kind == "r18":
        return get_pose_net(resnet_cfg(18), True).cuda().set_precision("bf16")
    return get_hrnet(hrnet_cfg(32), True).cuda().set_precision("fp16")


def _data(b, k, hs=48, ws=56, size=64):
    rng = np.random.RandomState(100 + k)
    x = torch.from_numpy(rng.randint(0, 256, size=(b, hs, ws, 3)).astype(np.uint8)).cuda()
    jt = torch.from_numpy(rng.uniform(8, size - 8, size=(b, 21, 2)).astype(np.float32)).cuda()
    return x, jt


@pytest.mark.parametrize("kind", ["r18", "hrnet"])
def test_train_step_geometric_aug(kind, monkeypatch):
    """Captured TrainStep(input_u8=, geometric_aug=): prob=0 is the step without the argument bit for bit (loss and the whole
    parameter arena, 3 steps); with draws, plan.img_nhwc4 / target after a replay equal the standalone ABI calls on the matrices
    that step drew; two draws give two inputs; a seeded generator gives the eager and the captured step the same losses."""
    from lighthand_amd import _lib as L
    from lighthand_amd.heatmap import RADIUS, _patch_on
    from lighthand_amd.runtime import TrainStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    lib = L.load()
    b, size, hs, ws = 4, 64, 48, 56
    data = [_data(b, k) for k in range(3)]
    arenas, losses = [], []
    for geo in (None, {"rotation": 30.0, "scale": 0.2, "shift": 0.1, "prob": 0.0}):
        m = _model(kind)
        st = TrainStep(m, b, size, size, lr=1e-3, input_u8=(hs, ws), geometric_aug=geo)
        losses.append([float(st(x, jt)) for x, jt in data])
        torch.cuda.synchronize()
        arenas.append(m.arena().flat.clone())
    assert losses[0] == losses[1] and all(np.isfinite(losses[0]))
    assert torch.equal(arenas[0], arenas[1])

    m = _model(kind)
    st = TrainStep(m, b, size, size, lr=1e-3, input_u8=(hs, ws), geometric_aug=(30.0, 0.2, 0.1))
    plan = st.plan
    imgs = []
    for x, jt in data[:2]:
        st(x, jt)
        torch.cuda.synchronize()
        assert not torch.equal(plan.warp_inv.cpu(), torch.tensor([1.0, 0, 0, 0, 1, 0]).repeat(b, 1))
        s = torch.cuda.current_stream().cuda_stream
        ref_img = torch.full_like(plan.img_nhwc4, float("nan"))
        m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
        L.check(lib.lh_image_u8_warp_to_nhwc4(st.images_u8.data_ptr(), ref_img.data_ptr(), b, hs, ws, size, size, plan.img_pad, plan.img_wp,
                                              m3, s3, plan.warp_inv.data_ptr(), None, None, None, plan.dt, s), "warp")
        ja = torch.full_like(st.joints, float("nan"))
        L.check(lib.lh_affine_points(st.joints.data_ptr(), 2, plan.warp_fwd.data_ptr(), ja.data_ptr(), 2, b, 21, s), "points")
        tgt = torch.full_like(st.target, float("nan"))
        L.check(lib.lh_gaussian_target(ja.data_ptr(), 2, _patch_on(ja.device).data_ptr(), RADIUS, tgt.data_ptr(), b, 21, tgt.shape[2], s),
                "target")
        torch.cuda.synchronize()
        assert torch.equal(_bits(ref_img), _bits(plan.img_nhwc4))
        assert torch.equal(ja, st.joints_aug) and torch.equal(tgt, st.target)
        assert torch.equal(st.joints, jt)                                 # the caller's joints are kept
        imgs.append(plan.img_nhwc4.clone())
    assert not torch.equal(imgs[0], imgs[1])
    st(*data[1])                                                           # the same batch again: a new draw, a new input
    torch.cuda.synchronize()
    assert not torch.equal(imgs[1], plan.img_nhwc4)

    runs = []
    for use_graph in (True, False):
        m = _model(kind)
        geo = {"rotation": 30.0, "scale": 0.2, "shift": 0.1, "generator": torch.Generator().manual_seed(21)}
        st = TrainStep(m, b, size, size, lr=1e-3, input_u8=(hs, ws), geometric_aug=geo, use_graph=use_graph)
        runs.append([float(st(x, jt)) for x, jt in data])
    assert runs[0] == runs[1] and all(np.isfinite(runs[0]))


def test_train_cli_with_geometric_factors(tmp_path, monkeypatch):
    """main(args, train_set=, val_set=) on raw uint8 frames with all three factors: two epochs (a short last batch included) train
    with finite losses and write the checkpoint; both the full-size and the short-batch step carry the warp."""
    from lighthand_amd import runtime
    from lighthand_amd.tools import train as T

    class RawFrames(torch.utils.data.Dataset):
        def __init__(self, n, seed):
            rng = np.random.RandomState(seed)
            self.x = rng.randint(0, 256, size=(n, 48, 80, 3)).astype(np.uint8)
            self.j = rng.uniform(8, 56, size=(n, 21, 2)).astype(np.float32)

        def __len__(self):
            return len(self.x)

        def __getitem__(self, i):
            return self.x[i], self.j[i]

    made = []
    real_init = runtime.TrainStep.__init__

    def spy(self, *a, **k):
        real_init(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(runtime.TrainStep, "__init__", spy)
    args = T.parse_args(["--root_path", str(tmp_path), "--batch_size", "8", "--epoch", "2", "--depth", "18", "--size", "64",
                         "--precision", "bf16", "--reset", "--name", "geo", "--rot_factor", "20", "--scale_factor", "0.2",
                         "--shift_factor", "0.1"])
    args.num_workers = 0
    best = T.main(args, train_set=RawFrames(28, 3), val_set=RawFrames(8, 4))
    assert np.isfinite(best)
    assert sorted(st.joints.shape[0] for st in made) == [4, 8]          # 28 = 3 x 8 + a short batch of 4
    for st in made:
        assert st.geometric_aug["rotation"] == 20.0 and st.joints_aug is not None
        assert np.isfinite(float(st.loss))
        assert not torch.equal(st.plan.warp_fwd.cpu(), torch.tensor([1.0, 0, 0, 0, 1, 0]).repeat(st.joints.shape[0], 1))
    assert os.path.isfile(os.path.join(args.output_dir, "checkpoint-good", "state_dict.bin"))
