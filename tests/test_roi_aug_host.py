"""CPU: training on hand ROIs cropped from full frames, the host side -- runtime.sample_roi_aug, the numpy restatements of
lh_roi_perturb / lh_affine_points_inv (lighthand_amd.topdown: the geometry is checked here, the kernels against them in
tests/test_gpu_train_frames.py), the two C-ABI entries (exported, declared, arguments validated without a GPU), what the target
renderers make of LH_POINT_OFF, and TrainStep's refusals through the device-free validation function."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

F = np.float32
NEW = ("lh_roi_perturb", "lh_affine_points_inv")
EYE = (1.0, 0.0, 1.0, 0.0, 0.0, 0.0)
EPS = float(np.finfo(np.float32).eps)          # 2^-23: one fp32 ulp of a value in [1, 2)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the draw
def test_sample_roi_aug_is_seeded_and_respects_its_ranges():
    from lighthand_amd.runtime import sample_roi_aug
    g = lambda: torch.Generator().manual_seed(11)
    a = sample_roi_aug(512, 40.0, 0.3, 0.15, 0.5, generator=g())
    b = sample_roi_aug(512, 40.0, 0.3, 0.15, 0.5, generator=g())
    assert a.dtype == torch.float32 and tuple(a.shape) == (512, 6) and not a.is_cuda and torch.equal(a, b)
    assert not torch.equal(a, sample_roi_aug(512, 40.0, 0.3, 0.15, 0.5, generator=torch.Generator().manual_seed(12)))
    a = a.numpy().astype(np.float64)
    c, s, k, tx, ty, flip = a.T
    # (c, s) are cos / sin formed in fp64 and rounded once: c*c + s*s misses 1 by at most 2 * 2^-24 (|c| dc + |s| ds, each d <= 2^-25
    # relative, |c| + |s| <= sqrt 2) plus second-order terms: 3 * 2^-24 holds with room
    assert np.abs(c * c + s * s - 1).max() <= 3 * 2.0 ** -24
    ang = np.degrees(np.arctan2(s, c))
    assert np.abs(ang).max() <= 40.0 + 1e-4 and np.abs(ang).max() > 30 and ang.min() < -30
    assert k.min() >= F(0.7) and k.max() <= F(1.3) and k.min() < 0.75 and k.max() > 1.25
    for t in (tx, ty):
        assert np.abs(t).max() <= F(0.15) and t.min() < -0.1 and t.max() > 0.1
    assert set(flip.tolist()) == {0.0, 1.0} and 0.35 < flip.mean() < 0.65
    assert not np.signbit(a).all(0)[[1, 3, 4]].any()


def test_sample_roi_aug_identity_rows_are_exact():
    from lighthand_amd.runtime import sample_roi_aug
    eye = torch.tensor(EYE).expand(64, 6)
    assert torch.equal(sample_roi_aug(64, 0, 0, 0, 0), eye)                                     # every factor 0
    assert torch.equal(sample_roi_aug(64, 180.0, 0.3, 0.2, 0.5, prob=0.0), eye)                 # never drawn
    mask = torch.arange(64) % 3 == 0
    a = sample_roi_aug(64, 180.0, 0.3, 0.2, 0.5, mask=mask, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a[~mask], eye[~mask]) and not (a[mask] == eye[mask]).all(1).any()
    half = sample_roi_aug(4096, 30.0, 0.0, 0.0, 0.0, prob=0.25, generator=torch.Generator().manual_seed(6))
    drawn = ~(half == torch.tensor(EYE)).all(1)
    assert 0.2 < drawn.float().mean() < 0.3
    assert torch.equal(half[:, 2:], torch.tensor(EYE[2:]).expand(4096, 4))                      # rotation alone: k, tx, ty, flip untouched
    only_flip = sample_roi_aug(256, 0, 0, 0, 1.0)
    assert torch.equal(only_flip, torch.tensor((1.0, 0.0, 1.0, 0.0, 0.0, 1.0)).expand(256, 6))


# ------------------------------------------------------------------------------------------------ 2. roi_perturb_host
def _rois(n, seed):
    rng = np.random.RandomState(seed)
    lo = rng.uniform(-20, 60, size=(n, 2))
    boxes = np.concatenate([lo, lo + rng.uniform(8, 70, size=(n, 2))], 1).astype(np.float32)
    ang = rng.uniform(-np.pi, np.pi, n)
    rot = (np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(0.3, 4.0, size=(n, 1))).astype(np.float32)         # any length
    return boxes, rot, rng.randint(0, 2, n).astype(np.int32) * rng.randint(1, 5, n).astype(np.int32), rng


def test_roi_perturb_identity_rows_return_the_input_bits():
    from lighthand_amd.topdown import roi_perturb_host
    boxes, rot, mirror, _ = _rois(40, 1)
    nb, nr, nm = roi_perturb_host(boxes, rot, mirror, np.tile(F(EYE), (40, 1)))
    assert nb.dtype == np.float32 and nr.dtype == np.float32 and nm.dtype == np.int32
    assert np.array_equal(_bits(nb), _bits(boxes)) and np.array_equal(_bits(nr), _bits(rot)) and np.array_equal(nm, mirror)
    assert not np.allclose(np.hypot(rot[:, 0], rot[:, 1]), 1, atol=1e-2)                        # the directions were not unit: kept so
    nb, nr, nm = roi_perturb_host(boxes, None, None, np.tile(F(EYE), (40, 1)))                  # NULL rot / mirror = (1, 0) / 0
    assert np.array_equal(nr, np.tile(F([1, 0]), (40, 1))) and not nm.any() and np.array_equal(_bits(nb), _bits(boxes))


def test_roi_perturb_rotation_scale_shift_and_flip():
    from lighthand_amd.topdown import roi_perturb_host, rot_from_angle
    # box coordinates on a 1/4 grid and dyadic scales: every product and sum below is exact in fp32
    boxes = F([[10.25, 20.5, 50.75, 84.5], [-8.0, 3.25, 24.0, 19.75], [100.5, 7.0, 164.5, 39.0]])
    up = np.tile(F([1, 0]), (3, 1))
    cx, cy = (boxes[:, 0] + boxes[:, 2]) * F(0.5), (boxes[:, 1] + boxes[:, 3]) * F(0.5)
    bw, bh = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]

    def centre_extent(b):
        return (b[:, 0] + b[:, 2]) * F(0.5), (b[:, 1] + b[:, 3]) * F(0.5), b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]

    # a pure rotation leaves centre and extents alone and turns the direction by the angle
    c, s = rot_from_angle(np.radians(35.0))
    nb, nr, nm = roi_perturb_host(boxes, up, None, np.tile(F([c, s, 1, 0, 0, 0]), (3, 1)))
    assert np.array_equal(_bits(nb), _bits(boxes)) and not nm.any()
    assert np.array_equal(nr, np.tile(F([c, s]), (3, 1)))
    nr = roi_perturb_host(boxes, np.tile(F([0, 2]), (3, 1)), None, np.tile(F([0, 1, 1, 0, 0, 0]), (3, 1)))[1]
    assert np.array_equal(nr, np.tile(F([-1, 0]), (3, 1)))                                      # (0, 2) turned by 90 degrees, normalised
    # a pure scale keeps the centre bit for bit (tx = ty = 0) and multiplies the extents
    for k in (0.75, 1.25, 1.5):
        nb, nr, _ = roi_perturb_host(boxes, up, None, np.tile(F([1, 0, k, 0, 0, 0]), (3, 1)))
        ncx, ncy, nbw, nbh = centre_extent(nb)
        assert np.array_equal(_bits(ncx), _bits(cx)) and np.array_equal(_bits(ncy), _bits(cy))
        assert np.array_equal(nbw, bw * F(k)) and np.array_equal(nbh, bh * F(k)) and np.array_equal(nr, up)
    # tx = 1 on a ROI turned by 90 degrees (its +x axis is the frame's +y): the centre moves by bw along frame y
    nb, _, _ = roi_perturb_host(boxes, np.tile(F([0, 1]), (3, 1)), None, np.tile(F([1, 0, 1, 1, 0, 0]), (3, 1)))
    ncx, ncy, nbw, nbh = centre_extent(nb)
    assert np.array_equal(ncx, cx) and np.array_equal(ncy, cy + bw) and np.array_equal(nbw, bw) and np.array_equal(nbh, bh)
    # ty = 0.5 on an upright ROI: half its height down
    nb, _, _ = roi_perturb_host(boxes, up, None, np.tile(F([1, 0, 1, 0, 0.5, 0]), (3, 1)))
    assert np.array_equal(centre_extent(nb)[1], cy + bh * F(0.5)) and np.array_equal(centre_extent(nb)[0], cx)
    # a flip toggles the mirror (any non-zero mirror counts as set) and nothing else
    nb, nr, nm = roi_perturb_host(boxes, up, [0, 1, 3], np.tile(F([1, 0, 1, 0, 0, 1]), (3, 1)))
    assert nm.tolist() == [1, 0, 0] and np.array_equal(_bits(nb), _bits(boxes)) and np.array_equal(nr, up)


def test_roi_perturb_passes_what_is_not_finite_through():
    from lighthand_amd.topdown import roi_affine_host, roi_perturb_host
    good, row = [4.0, 4.0, 30.0, 30.0], [0.8, 0.6, 1.25, 0.1, -0.1, 1.0]
    boxes = F([good, [np.nan, 4, 30, 30], [4, 4, np.inf, 30], good, good, good, good, [30, 4, 30, 30]])
    rot = F([[1, 0], [1, 0], [1, 0], [np.nan, 1], [0, 0], [1, 0], [1, 0], [0, 3]])
    aug = F([row, row, row, row, row, [np.nan] + row[1:], row[:3] + [np.inf] + row[4:], row])
    mirror = np.array([0, 1, 0, 2, 0, 1, 0, 0], np.int32)
    nb, nr, nm = roi_perturb_host(boxes, rot, mirror, aug)
    for i in range(1, 7):
        assert np.array_equal(_bits(nb[i]), _bits(boxes[i])) and np.array_equal(_bits(nr[i]), _bits(rot[i])) and nm[i] == mirror[i], i
    assert not np.array_equal(nb[0], boxes[0]) and nm[0] == 1 and np.isfinite(nb[0]).all()
    assert np.isfinite(nb[7]).all() and nb[7, 2] - nb[7, 0] == 0          # a zero-width box stays zero-width: lh_roi_affine empties it
    _, src = roi_affine_host(nb, nr, nm, np.zeros(8, np.int32), 1, (64, 64), 1.25)
    assert src.tolist() == [0, -1, -1, -1, -1, 0, 0, -1]                  # the NaN aug rows crop the caller's ROI


def test_roi_perturb_fp64_yardstick():
    """dtype=np.float64 runs the same operations on the same fp32 inputs; the fp32 order stays within a few ulp of the largest
    intermediate: a centre coordinate of the box' is cx + d - hw, three roundings on top of those of cx (1), d (3) and hw (2), each
    at most 2^-24 of a magnitude <= |cx| + |d| + |hw| =: m, so 9 * 2^-24 * m; a direction component has 2 (ux, uy: sqrt and divide on
    top of n's 2) + 3 roundings of magnitudes <= 1."""
    from lighthand_amd.topdown import roi_perturb_host
    from lighthand_amd.runtime import sample_roi_aug
    boxes, rot, mirror, _ = _rois(256, 2)
    aug = sample_roi_aug(256, 180.0, 0.3, 0.2, 0.5, generator=torch.Generator().manual_seed(3)).numpy()
    got, want = roi_perturb_host(boxes, rot, mirror, aug), roi_perturb_host(boxes, rot, mirror, aug, dtype=np.float64)
    assert want[0].dtype == np.float64 and np.array_equal(got[2], want[2])
    bw, bh = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    m = np.abs(boxes).max(1).astype(np.float64) + (np.abs(aug[:, 3]) * bw + np.abs(aug[:, 4]) * bh) + np.maximum(bw, bh) * aug[:, 2]
    err = np.abs(got[0] - want[0]).max(1)
    print(f"roi_perturb fp32 vs fp64: box {np.max(err / (2.0 ** -24 * m)):.2f} x 2^-24 m (bound 9), rot {np.abs(got[1] - want[1]).max() / 2.0 ** -24:.2f} x 2^-24 (bound 8)")
    assert (err <= 9 * 2.0 ** -24 * m).all()
    assert np.abs(got[1] - want[1]).max() <= 8 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ 3. affine_points_inv_host
def test_affine_points_inv_identity_and_empty_slots():
    from lighthand_amd.topdown import POINT_OFF, affine_points_inv_host, box_affine_host
    rng = np.random.RandomState(4)
    pts = rng.uniform(-300, 900, size=(5, 21, 3)).astype(np.float32)
    eye = np.tile(F([1, 0, 0, 0, 1, 0]), (5, 1))
    out = affine_points_inv_host(pts, eye, np.zeros(5, np.int32))
    assert out.dtype == np.float32 and out.shape == (5, 21, 2) and np.array_equal(_bits(out), _bits(pts[..., :2]))
    # the matrix of a whole-frame box with padding 1 and a crop of the frame's size IS that identity
    mat, src = box_affine_host(np.tile(F([-0.5, -0.5, 127.5, 95.5]), (5, 1)), np.arange(5), 5, (96, 128), 1.0)
    assert np.array_equal(mat, eye) and (src >= 0).all()
    mats = np.tile(F([2, 0, 5, 0, 2, 7]), (5, 1))
    mats[1] = 0                                              # an empty slot's matrix
    mats[2] = [1, 2, 0, 2, 4, 0]                             # singular
    mats[3] = [np.inf, 0, 0, 0, 1, 0]                        # det not finite
    out = affine_points_inv_host(pts, mats, np.array([0, -1, 0, 0, -1], np.int32))
    assert POINT_OFF == -65536.0 and (out[[1, 2, 3, 4]] == F(POINT_OFF)).all()
    assert np.array_equal(out[0], (pts[0, :, :2] - F([5, 7])) * F(0.5))


def _seeded_rois(n=64, size=(64, 64)):
    """n ROIs over the full circle, 0.25 .. 8 frame pixels per crop pixel, every second one mirrored, with 21 joints each inside them."""
    from lighthand_amd.topdown import roi_affine_host
    rng = np.random.RandomState(9)
    scale = np.exp(rng.uniform(np.log(0.25), np.log(8.0), n))
    ang = rng.uniform(-np.pi, np.pi, n)
    ang[:4] = [0.0, np.pi / 2, np.pi, -np.pi / 2]
    centre = rng.uniform(100, 1800, size=(n, 2))
    half = scale[:, None] * size[1] / 2 * rng.uniform(0.6, 1.0, size=(n, 2))
    boxes = np.concatenate([centre - half, centre + half], 1).astype(np.float32)
    rot = np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)
    mirror = (np.arange(n) % 2).astype(np.int32)
    mat, src = roi_affine_host(boxes, rot, mirror, np.zeros(n, np.int32), 1, size, 1.0)
    assert (src == 0).all()
    got_scale = np.hypot(mat[:, 0], mat[:, 3])
    assert got_scale.min() < 0.4 and got_scale.max() > 5 and got_scale.min() >= 0.14 and got_scale.max() <= 8.01
    joints = (centre[:, None, :] + rng.uniform(-1, 1, size=(n, 21, 2)) * half.max(1)[:, None, None]).astype(np.float32)
    return mat, src, joints


def _inverse_bound(mat, pts):
    """The bound of test_affine_points_inv_against_fp64, per point: fp64 [b][j]."""
    m = mat.astype(np.float64)
    q = np.maximum(np.abs(pts[..., 0].astype(np.float64) - m[:, None, 2]), np.abs(pts[..., 1].astype(np.float64) - m[:, None, 5]))
    det = np.abs(m[:, 0] * m[:, 4] - m[:, 1] * m[:, 3])
    kappa = (np.abs(m[:, 0] * m[:, 4]) + np.abs(m[:, 1] * m[:, 3])) / det
    big = q * np.abs(m[:, [0, 1, 3, 4]]).max(1)[:, None]
    return 1.01 * (4 + 2 * kappa)[:, None] * EPS * big / det[:, None]


def test_affine_points_inv_against_fp64():
    """fp32 order against the same operations in fp64, on 64 seeded ROIs.  With u = 2^-24 and M = max(|q|) * max(|m|):
    qx, qy carry one rounding each (u), every product one more, the difference of the two products one more: the numerator
    N = m4*qx - m1*qy is off by at most 3u * (|m4 qx| + |m1 qy|) <= 3u * 2M.  det = m0*m4 - m1*m3 is off by 2u * (|m0 m4| + |m1 m3|) =
    2u * kappa * |det|, which moves the quotient by 2u * kappa * |N| / |det| <= 2u * kappa * 2M / |det|; the division adds u * |N| / |det|
    <= u * 2M / |det|.  Sum: (3 + 2 kappa + 1) * 2u * M / |det| = (4 + 2 kappa) ulp(1) * M / |det| -- for a rotation with uniform scale
    kappa = 1: six ulp of M / |det|.  1 % covers the second-order terms."""
    from lighthand_amd.topdown import affine_points_inv_host
    mat, src, joints = _seeded_rois()
    got, want = affine_points_inv_host(joints, mat, src), affine_points_inv_host(joints, mat, src, dtype=np.float64)
    assert got.dtype == np.float32 and want.dtype == np.float64
    err, bound = np.abs(got - want).max(-1), _inverse_bound(mat, joints)
    print(f"affine_points_inv fp32 vs fp64: worst {np.max(err / bound):.3f} of the bound, {err.max():.2e} crop px")
    assert (err <= bound).all()
    assert np.abs(want).max() < 200          # the joints do land in and around the 64 x 64 crop


def test_roi_round_trip_returns_the_joints():
    """roi_affine_host -> affine_points_inv_host -> the forward matrix (lh_affine_points' (m0*x + m1*y) + m2 in fp32) returns the frame
    joints: the inverse's error e (the bound above, crop pixels) reaches the frame through |m0| + |m1| <= 2 max|m|, and the forward
    map adds three roundings of magnitudes <= |m0 ox| + |m1 oy| + |m2| =: f, so 2 max|m| * e + 3 * 2^-24 * f frame pixels."""
    from lighthand_amd.topdown import affine_points_inv_host
    mat, src, joints = _seeded_rois()
    crop = affine_points_inv_host(joints, mat, src)
    m = mat[:, None, :]
    back = np.stack([(m[..., 0] * crop[..., 0] + m[..., 1] * crop[..., 1]) + m[..., 2],
                     (m[..., 3] * crop[..., 0] + m[..., 4] * crop[..., 1]) + m[..., 5]], -1)
    assert back.dtype == np.float32
    c64, m64 = np.abs(crop.astype(np.float64)), np.abs(mat.astype(np.float64))[:, None, :]
    f = np.maximum(m64[..., 0] * c64[..., 0] + m64[..., 1] * c64[..., 1] + m64[..., 2], m64[..., 3] * c64[..., 0] + m64[..., 4] * c64[..., 1] + m64[..., 5])
    bound = 2 * m64[..., [0, 1, 3, 4]].max(-1) * _inverse_bound(mat, joints) + 3 * 2.0 ** -24 * f
    err = np.abs(back.astype(np.float64) - joints).max(-1)
    print(f"ROI round trip: worst {np.max(err / bound):.3f} of the bound, {err.max():.2e} frame px")
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ 4. renderers, C ABI, refusals
@pytest.mark.parametrize("weighted,unbiased", [(False, False), (True, False), (False, True), (True, True)])
def test_point_off_renders_a_zero_map_and_weight_zero(weighted, unbiased):
    from lighthand_amd.heatmap import render_targets_host
    from lighthand_amd.topdown import POINT_OFF
    joints = np.full((2, 5, 3), POINT_OFF, np.float32)
    joints[..., 2] = 1.0                                     # visible: the weight can only come from the position
    joints[1, 2, :2] = [20.0, 30.0]                          # one joint on the map, so the test is not vacuous
    target, weight = render_targets_host(joints, 16, weighted=weighted, unbiased=unbiased)
    on = np.zeros((2, 5), bool)
    on[1, 2] = True
    assert not target[~on].any() and target[1, 2].max() > 0.9
    if weighted:
        assert not weight[~on].any() and weight[1, 2, 0] == 1
    if not unbiased:                                         # the quantised renderers against the oracle's generate_target
        from oracle.heatmap import generate_target
        want = np.stack([generate_target(j, num_joints=5, size=16) for j in joints])
        assert np.array_equal(target, want)


def test_entries_are_exported_declared_and_validate_arguments_without_gpu():
    from lighthand_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lighthand_hip.h")).read()
    assert re.search(r"#define\s+LH_POINT_OFF\s+\(-65536\.f\)", header)
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    a, b, c, d, e, f, g = (C.c_void_p(0x1000 * i) for i in range(1, 8))          # never dereferenced: validation fails before any launch

    def perturb(boxes=a, rot=b, mirror=c, aug=d, n=4, ob=e, orot=f, om=g):
        return lib.lh_roi_perturb(boxes, rot, mirror, aug, n, ob, orot, om, None)
    for rc in (perturb(boxes=None), perturb(aug=None), perturb(ob=None), perturb(orot=None), perturb(om=None), perturb(n=0)):
        assert rc == -1 and b"lh_roi_perturb" in lib.lh_last_error()
    for rc in (perturb(ob=a), perturb(orot=b), perturb(om=c), perturb(ob=d), perturb(orot=d), perturb(orot=a), perturb(ob=b)):
        assert rc == -1 and b"lh_roi_perturb" in lib.lh_last_error() and b"alias" in lib.lh_last_error()

    def inv(pts=a, ps=2, mat=b, src=c, out=d, os_=2, n=4, j=21):
        return lib.lh_affine_points_inv(pts, ps, mat, src, out, os_, n, j, None)
    for rc in (inv(pts=None), inv(mat=None), inv(src=None), inv(out=None), inv(ps=1), inv(os_=1), inv(n=0), inv(j=0), inv(n=1 << 20, j=1 << 12)):
        assert rc == -1 and b"lh_affine_points_inv" in lib.lh_last_error()


def test_the_two_entries_add_no_kernel_symbol():
    """lh_roi_perturb and lh_affine_points_inv run as modes of frames_crop_kernel's fp32 instantiation (csrc/frames_crop_kernel.h: CropArgs.op):
    the library's kernel symbols are those of the resource table in force, which tests/test_kernel_resources.py holds to [0, 0] scratch
    and spills for that kernel -- the table and tools/kernel_resources.py stay as they are."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    assert os.path.basename(kr.GOLDEN) == "kernel_ceilings_roi.json"
    with open(kr.GOLDEN) as f:
        table = json.load(f)
    assert not [k for k in table if "roi_perturb" in k or "points_inv" in k]
    assert table["_Z18frames_crop_kernelIfEv8CropArgs"] == [0, 0]
    if not os.path.exists(kr.LIB) or not kr.tools_present():
        return
    built = kr.read_resources()
    assert not [k for k in built if k not in table] and built["_Z18frames_crop_kernelIfEv8CropArgs"] == [0, 0]


def test_train_step_refusals_before_any_device_work():
    """One assertion per rule, through the validation function TrainStep calls first (no model, no device)."""
    from lighthand_amd.runtime import TrainStep, _check_train_frames as check
    fr = (4, 96, 128)
    assert check(None, None) == (None, None, None)
    got, spec, jitter = check(None, fr, roi_aug=(30, 0.2, 0.1))
    assert got == fr and jitter is None and spec["rotation"] == 30 and spec["mirror_prob"] == 0.0 and spec["prob"] == 1.0 and spec["generator"] is None
    assert check(None, fr, roi_aug=(30, 0.2, 0.1, 0.5))[1]["mirror_prob"] == 0.5
    assert check(None, fr, roi_aug=dict(rotation=10, prob=0.5))[1]["prob"] == 0.5
    with pytest.raises(ValueError, match="input_u8"):
        check(None, fr, input_u8=(96, 128))
    with pytest.raises(ValueError, match="geometric_aug"):
        check(None, fr, geometric_aug=(30, 0.2, 0.1))
    with pytest.raises(ValueError, match="color_jitter"):
        check(None, fr, color_jitter=(0.5, 0.5, 0.5, 0.5))
    with pytest.raises(ValueError, match="targets_from_joints"):
        check(None, fr, targets_from_joints=False)
    with pytest.raises(ValueError, match="roi_aug"):
        check(None, None, roi_aug=(30, 0.2, 0.1))
    with pytest.raises(ValueError, match="use_target_weight"):
        check(None, fr, coord_loss_weight=0.5)
    assert check(None, fr, coord_loss_weight=0.5, use_target_weight=True)[0] == fr
    # the options shared with InferStep keep its rules
    with pytest.raises(ValueError, match="box_padding"):
        check(None, fr, box_padding=0)
    with pytest.raises(ValueError, match="frames must be"):
        check(None, (4, 96))
    with pytest.raises(ValueError, match="oriented"):
        check(None, None, oriented=True)
    with pytest.raises(ValueError, match="antialias"):
        check(None, None, antialias=True)
    with pytest.raises(ValueError, match="antialias"):
        check(None, fr, antialias=9)
    with pytest.raises(ValueError, match="nv12"):
        check(None, fr, chroma_siting="center")
    with pytest.raises(ValueError, match="NV12"):
        check(None, (4, 95, 128), frame_format="nv12")
    for bad in ((30, 0.2), (30, 0.2, 0.1, 0.5, 1), "30", (30, -0.2, 0.1), (30, 1.0, 0.1), (30, 0.2, 0.1, 1.5), (float("nan"), 0, 0),
                dict(rotation=3, angle=2), dict(prob=2)):
        with pytest.raises(ValueError, match="roi_aug"):
            check(None, fr, roi_aug=bad)
    # and TrainStep itself refuses before it looks at the model
    with pytest.raises(ValueError, match="roi_aug"):
        TrainStep(object(), 2, 64, 64, roi_aug=(30, 0.2, 0.1))
    with pytest.raises(ValueError, match="geometric_aug"):
        TrainStep(object(), 2, 64, 64, frames=fr, geometric_aug=(30, 0.2, 0.1))


# ------------------------------------------------------------------------------------------------ 5. the training tool's flags
def test_train_cli_frame_flags(capsys):
    from lighthand_amd.tools import train as T
    from lighthand_amd.tools import track_frames
    from lighthand_amd.tools.synthetic_frames import synthetic_sequence
    assert track_frames.synthetic_sequence is synthetic_sequence                   # one renderer, shared
    frames, boxes = synthetic_sequence(3, 96, 128, 2, seed=1)
    same, same_boxes, joints = synthetic_sequence(3, 96, 128, 2, seed=1, return_joints=True)
    assert np.array_equal(frames, same) and np.array_equal(boxes, same_boxes) and joints.shape == (3, 2, 21, 2)
    assert np.array_equal(boxes[:, :2], joints[0].min(1)) and np.array_equal(boxes[:, 2:], joints[0].max(1))
    base = ["--synthetic", "8", "--batch_size", "4"]
    off = T.parse_args(base)
    assert off.frame_size is None and T.roi_aug(off) is None and not off.oriented and off.antialias is None and off.frame_format == "rgb"
    on = T.parse_args(base + ["--frame_size", "96x128", "--roi_rot", "30", "--roi_scale", "0.25", "--roi_shift", "0.1", "--roi_mirror", "0.5",
                              "--oriented", "--antialias", "--frame_format", "nv12", "--yuv_matrix", "bt601", "--chroma_siting", "center"])
    assert on.frame_size == (96, 128) and T.roi_aug(on) == (30.0, 0.25, 0.1, 0.5)
    assert T.frame_options(on) == dict(oriented=True, antialias=8, frame_format="nv12", yuv=("bt601", "limited"), chroma_siting="center")
    assert T.frame_options(T.parse_args(base + ["--frame_size", "96x128"])) == dict(oriented=False)
    for bad in (["--roi_rot", "30"], ["--oriented"], ["--antialias", "4"], ["--frame_format", "nv12"], ["--frame_size", "96"],
                ["--frame_size", "96x128", "--rot_factor", "10"], ["--frame_size", "96x128", "--antialias", "9"],
                ["--frame_size", "95x128", "--frame_format", "nv12"], ["--frame_size", "96x128", "--roi_scale", "1.0"],
                ["--frame_size", "96x128", "--roi_mirror", "1.5"], ["--frame_size", "96x128", "--coord_loss_weight", "0.5"],
                ["--frame_size", "96x128", "--yuv_range", "full"]):
        with pytest.raises(SystemExit):
            T.parse_args(base + bad)
    with pytest.raises(SystemExit):
        T.parse_args(["--frame_size", "96x128"])                                   # no --synthetic
    capsys.readouterr()
    ds = T.SyntheticFrames(5, (96, 128), 3)
    frame, jt, box = ds[2]
    assert len(ds) == 5 and frame.dtype == torch.uint8 and tuple(frame.shape) == (96, 128, 3) and tuple(jt.shape) == (21, 2)
    assert torch.equal(box, torch.cat([jt.min(0).values, jt.max(0).values]))
    assert int(frame[int(jt[0, 1].round()), int(jt[0, 0].round()), 0]) == 255      # a disc sits on the joint
    nv = T.SyntheticFrames(2, (96, 128), 3, invisible=0.5, nv12=("bt709", "limited"))
    assert tuple(nv[0][0].shape) == (144, 128) and tuple(nv[0][1].shape) == (21, 3) and set(nv.joints[..., 2].unique().tolist()) <= {0.0, 1.0}
