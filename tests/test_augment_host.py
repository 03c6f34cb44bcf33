"""CPU: the host side of the online geometric augmentation -- runtime.sample_affine (the per-image draw), argument validation
of lh_image_u8_warp_to_nhwc4 / lh_affine_points without a GPU, TrainStep's and the training CLI's refusals and flags."""
import ctypes as C

import numpy as np
import pytest
import torch


def _m3(t):
    a = t.double().numpy().reshape(-1, 2, 3)
    return np.concatenate([a, np.tile([[[0.0, 0.0, 1.0]]], (len(a), 1, 1))], 1)


def test_sample_affine_is_seeded_and_in_range():
    from lighthand_amd.runtime import sample_affine
    h, w = 256, 192
    kw = dict(rotation=30.0, scale=0.25, shift=0.1, size=(h, w))
    inv0, fwd0 = sample_affine(500, generator=torch.Generator().manual_seed(7), **kw)
    inv1, fwd1 = sample_affine(500, generator=torch.Generator().manual_seed(7), **kw)
    assert inv0.dtype == fwd0.dtype == torch.float32 and inv0.shape == fwd0.shape == (500, 6)
    assert torch.equal(inv0, inv1) and torch.equal(fwd0, fwd1)
    inv2, _ = sample_affine(500, generator=torch.Generator().manual_seed(8), **kw)
    assert not torch.equal(inv0, inv2)
    f = fwd0.double().numpy()
    s = np.hypot(f[:, 0], f[:, 1])                                   # isotropic scale
    ang = np.degrees(np.arctan2(f[:, 1], f[:, 0]))                   # cv2.getRotationMatrix2D's sign: [[cos, sin], [-sin, cos]]
    assert np.allclose(f[:, 3], -f[:, 1]) and np.allclose(f[:, 4], f[:, 0])
    assert (s >= 0.75 - 1e-6).all() and (s <= 1.25 + 1e-6).all() and s.min() < 0.8 and s.max() > 1.2
    assert (np.abs(ang) <= 30 + 1e-4).all() and ang.min() < -25 and ang.max() > 25
    # the shift is what the centre of the frame moves by
    c = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
    moved = np.stack([f[:, 0] * c[0] + f[:, 1] * c[1] + f[:, 2], f[:, 3] * c[0] + f[:, 4] * c[1] + f[:, 5]], 1) - c
    assert (np.abs(moved[:, 0]) <= 0.1 * w + 1e-3).all() and (np.abs(moved[:, 1]) <= 0.1 * h + 1e-3).all()
    assert np.abs(moved[:, 0]).max() > 0.08 * w and np.abs(moved[:, 1]).max() > 0.08 * h


def test_sample_affine_inverse_and_identity():
    from lighthand_amd.runtime import sample_affine
    h, w = 256, 256
    inv, fwd = sample_affine(300, 45.0, 0.3, 0.15, generator=torch.Generator().manual_seed(1), size=(h, w))
    prod = _m3(inv) @ _m3(fwd)
    assert np.abs(prod[:, :2, :2] - np.eye(2)).max() < 1e-6
    assert np.abs(prod[:, :2, 2]).max() < 1e-6 * max(h, w)             # translations of ~100 px carry fp32's 1e-7 relative
    eye = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]).expand(300, 6)
    bits = lambda t: t.view(torch.int32)
    for inv, fwd in (sample_affine(300, 45.0, 0.3, 0.15, prob=0.0, generator=torch.Generator().manual_seed(1), size=(h, w)),
                     sample_affine(300, 0.0, 0.0, 0.0, generator=torch.Generator().manual_seed(1), size=(h, w)),
                     sample_affine(300, 45.0, 0.3, 0.15, mask=torch.zeros(300, dtype=torch.bool), size=(h, w))):
        assert torch.equal(bits(inv), bits(eye.contiguous())) and torch.equal(bits(fwd), bits(eye.contiguous()))
    mask = torch.arange(300) % 3 == 0
    inv, fwd = sample_affine(300, 45.0, 0.3, 0.15, prob=0.5, mask=mask, generator=torch.Generator().manual_seed(2), size=(h, w))
    ident = (fwd == eye).all(1)
    assert ident[~mask].all()
    assert 0.3 < float((~ident[mask]).float().mean()) < 0.7            # prob=0.5 of the masked samples


def test_warp_entries_validate_arguments_without_gpu():
    from lighthand_amd import _lib
    lib = _lib.load()
    m3, s3 = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25)
    fake = C.c_void_p(0x1000)                                     # never dereferenced: validation fails before any launch
    good = dict(n=2, hs=8, ws=8, h=8, w=8, pad=3, wp=16)

    def warp(hwc=fake, out=fake, inv=fake, factors=None, order=None, ws=None, **kw):
        a = dict(good, **kw)
        return lib.lh_image_u8_warp_to_nhwc4(hwc, out, a["n"], a["hs"], a["ws"], a["h"], a["w"], a["pad"], a["wp"], m3, s3, inv,
                                             factors, order, ws, _lib.LH_BF16, None)
    for rc in (warp(hwc=None), warp(out=None), warp(inv=None), warp(n=0), warp(n=-1), warp(wp=8 + 2 * 3 - 1), warp(hs=0),
               warp(factors=fake), warp(factors=fake, order=fake)):
        assert rc == -1 and b"lh_image_u8_warp_to_nhwc4" in lib.lh_last_error()
    assert lib.lh_image_u8_warp_to_nhwc4(fake, fake, 2, 8, 8, 8, 8, 3, 16, None, s3, fake, None, None, None, _lib.LH_BF16, None) == -1
    for rc in (lib.lh_affine_points(None, 2, fake, fake, 2, 2, 21, None), lib.lh_affine_points(fake, 2, None, fake, 2, 2, 21, None),
               lib.lh_affine_points(fake, 2, fake, None, 2, 2, 21, None), lib.lh_affine_points(fake, 1, fake, fake, 2, 2, 21, None),
               lib.lh_affine_points(fake, 2, fake, fake, 1, 2, 21, None), lib.lh_affine_points(fake, 2, fake, fake, 2, 0, 21, None),
               lib.lh_affine_points(fake, 2, fake, fake, 2, 2, 0, None)):
        assert rc == -1 and b"lh_affine_points" in lib.lh_last_error()


def test_train_step_refuses_geometric_aug_without_uint8_input():
    from lighthand_amd._lib import LightHandError
    from lighthand_amd.runtime import TrainStep
    with pytest.raises(LightHandError, match="input_u8"):
        TrainStep(object(), 2, 64, 64, geometric_aug=(10.0, 0.1, 0.1))
    with pytest.raises(LightHandError, match="targets_from_joints"):
        TrainStep(object(), 2, 64, 64, input_u8=(48, 48), targets_from_joints=False, geometric_aug=(10.0, 0.1, 0.1))
    with pytest.raises(LightHandError, match="unknown keys"):
        TrainStep(object(), 2, 64, 64, input_u8=(48, 48), geometric_aug={"rotation": 10.0, "flip": True})


def test_train_cli_geometric_flags():
    from lighthand_amd.tools import train as T
    args = T.parse_args([])
    assert (args.rot_factor, args.scale_factor, args.shift_factor) == (0.0, 0.0, 0.0)
    assert T.geometric_aug(args, "u8") is None and T.geometric_aug(args, "f32") is None
    args = T.parse_args(["--rot"])                                # the reference's dead flag stays a no-op
    assert args.rot and T.geometric_aug(args, "u8") is None and T.geometric_aug(args, "f32") is None
    args = T.parse_args(["--rot_factor", "20", "--scale_factor", "0.25", "--shift_factor", "0.1"])
    assert T.geometric_aug(args, "u8") == (20.0, 0.25, 0.1)
    assert T.geometric_aug(T.parse_args(["--shift_factor", "0.05"]), "u8") == (0.0, 0.0, 0.05)


def test_train_cli_refuses_geometric_factor_with_float_dataset(tmp_path):
    from lighthand_amd.tools import train as T

    class Floats(torch.utils.data.Dataset):
        def __len__(self):
            return 4

        def __getitem__(self, i):
            return torch.zeros(3, 64, 64), torch.full((21, 2), 32.0)
    args = T.parse_args(["--root_path", str(tmp_path), "--size", "64", "--rot_factor", "15"])
    with pytest.raises(SystemExit, match="uint8"):
        T.main(args, train_set=Floats(), val_set=Floats())
    with pytest.raises(SystemExit, match="uint8"):
        T.main(T.parse_args(["--root_path", str(tmp_path), "--synthetic", "8", "--scale_factor", "0.2"]))
