"""CPU: oriented, mirrored hand ROIs and the One-Euro filter on the host -- the numpy restatements of lh_roi_affine /
lh_keypoints_to_rois / lh_one_euro (lighthand_amd.topdown: the geometry and the filter are checked here, the kernels against them in
tests/test_gpu_roi.py), the three C-ABI entries (exported, declared, arguments validated without a GPU), InferStep's /
InferPipeline's refusals and the resource table."""
import ctypes as C
import importlib.util
import json
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT

F = np.float32
NEW = ("lh_roi_affine", "lh_keypoints_to_rois", "lh_one_euro")
KERNELS = ("roi_affine_kernel", "keypoints_to_rois_kernel", "one_euro_kernel")
ANGLES = (0.0, 37.0, 90.0, 171.0, -120.0)


def _spacings(got, want, scale):
    """max |got - want| in fp32 spacings of ``scale``."""
    return float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / np.spacing(np.asarray(scale, np.float32))))


# ------------------------------------------------------------------------------------------------ 1. upright ROI = plain box
@pytest.mark.parametrize("size", [(64, 64), (24, 40)])
def test_upright_roi_is_the_plain_box(size):
    """rot = (1, 0), mirror = 0: m0 / m4 / src_frame equal lh_box_affine's, m1 / m3 are +-0, and m2 / m5 -- the same point reached
    through another order of operations -- lie within 2 fp32 spacings of |box coordinate| + sw (measured: 0.5)."""
    from lighthand_amd.topdown import box_affine_host, roi_affine_host
    h, w = size
    rng = np.random.RandomState(3 + h)
    n = 300
    boxes = np.concatenate([rng.uniform(-50, 900, size=(n, 2)), rng.uniform(950, 1900, size=(n, 2))], 1).astype(np.float32)
    index = rng.randint(0, 3, size=n).astype(np.int32)
    want, want_src = box_affine_host(boxes, index, 3, size, 1.25)
    got, src = roi_affine_host(boxes, np.tile(F([1, 0]), (n, 1)), np.zeros(n, np.int32), index, 3, size, 1.25)
    assert got.dtype == np.float32 and src.dtype == np.int32 and src.tolist() == want_src.tolist() and (src >= 0).all()
    assert np.array_equal(got[:, [0, 4]], want[:, [0, 4]])
    assert (got[:, [1, 3]] == 0).all()
    sw = F(1.25) * np.maximum(boxes[:, 2] - boxes[:, 0], (boxes[:, 3] - boxes[:, 1]) * F(w) / F(h))
    scale = np.abs(boxes).max(1) + sw
    worst = max(_spacings(got[:, 2], want[:, 2], scale), _spacings(got[:, 5], want[:, 5], scale))
    print(f"upright ROI {size}: m2 / m5 differ from lh_box_affine's by at most {worst:.2f} spacings of |coordinate| + sw")
    assert worst <= 2
    # a direction of any length is the same direction
    longer, _ = roi_affine_host(boxes, np.tile(F([4, 0]), (n, 1)), np.zeros(n, np.int32), index, 3, size, 1.25)
    assert np.array_equal(longer, got)


def test_roi_empty_slots():
    from lighthand_amd.topdown import roi_affine_host
    good, up = [4.0, 4.0, 30.0, 30.0], [1.0, 0.0]
    boxes = np.array([good, good, good, [np.nan, 4, 30, 30], [30, 4, 30, 30], good, good, good, good], np.float32)
    index = np.array([0, 3, -1, 0, 0, 0, 0, 0, 2], np.int32)
    rot = np.array([up, up, up, up, up, [0, 0], [np.nan, 1], [np.inf, 0], [0, -2]], np.float32)
    mat, src = roi_affine_host(boxes, rot, np.array([0, 1, 0, 1, 0, 1, 0, 1, 1]), index, 3, (64, 64), 1.25)
    assert src.tolist() == [0, -1, -1, -1, -1, -1, -1, -1, 2]
    assert (mat[src < 0] == 0).all() and np.isfinite(mat).all()
    a = mat[0, 0]
    assert a > 0 and mat[8].tolist()[:2] == [0.0, a] and mat[8].tolist()[3:5] == [a, 0.0]       # rot (0, -2), mirrored: c = 0, s = -1, g = -1


def test_mirror_flips_the_crops_x_axis_about_its_centre():
    from lighthand_amd.topdown import roi_affine_host, rot_from_angle
    box, rot = [[100.0, 50.0, 300.0, 250.0]] * 2, [rot_from_angle(0.6)] * 2
    mat, _ = roi_affine_host(box, rot, [0, 1], [0, 0], 1, (64, 48), 1.25)
    m = mat.astype(np.float64)
    for x, y in ((0.0, 0.0), (10.0, 50.0), (47.0, 63.0)):
        plain = (m[0, 0] * x + m[0, 1] * y + m[0, 2], m[0, 3] * x + m[0, 4] * y + m[0, 5])
        xm = 47.0 - x
        flipped = (m[1, 0] * xm + m[1, 1] * y + m[1, 2], m[1, 3] * xm + m[1, 4] * y + m[1, 5])
        assert np.allclose(plain, flipped, atol=1e-3)
    assert np.allclose(rot_from_angle(0.0), (1.0, 0.0)) and np.allclose(rot_from_angle(np.pi / 2), (0.0, 1.0), atol=1e-15)


# ------------------------------------------------------------------------------------------------ 2. canonicalisation
def hand(seed=5, span=220.0):
    """A fixed 21-joint constellation about (0, 0), fp64: the wrist (joint 0) at the bottom, joint 9 above it (y points down)."""
    pts = np.random.RandomState(seed).uniform(-0.5, 0.5, size=(21, 2)) * span
    pts[0], pts[9] = (6.0, 0.45 * span), (-4.0, -0.1 * span)
    return pts


def turned(pts, degrees, mirrored, centre):
    """The constellation mirrored in x (a left hand), turned about its centre, and placed in the frame; fp32 frame coordinates."""
    p = pts * np.array([-1.0, 1.0]) if mirrored else pts
    t = np.deg2rad(degrees)
    r = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    return (p @ r.T + np.asarray(centre)).astype(np.float32)


def crop_coordinates(mat, pts):
    """Frame points -> crop pixel indices through the inverse of a crop matrix, in fp64."""
    m = np.asarray(mat, np.float64)
    inv = np.linalg.inv(np.array([[m[0], m[1]], [m[3], m[4]]]))
    return (np.asarray(pts, np.float64) - np.array([m[2], m[5]])) @ inv.T


def canonicalisation_cases(size=(256, 256), centre=(1000.25, 500.75)):
    """[(frame joints fp32 [21][2], mirrored)] for every angle, plain and mirrored, in a 1080 x 1920 frame."""
    cases = [(turned(hand(), deg, mir, centre), mir) for mir in (0, 1) for deg in ANGLES]
    assert all(0 <= j[:, 0].min() and j[:, 0].max() < 1920 and 0 <= j[:, 1].min() and j[:, 1].max() < 1080 for j, _ in cases)
    return cases


def check_canonical(crops, mats, joints):
    """The shared assertions of the host test and the GPU one: ``crops`` [10][21][2] agree with the first within 8 fp32 spacings of the
    frame coordinates divided by the scale a, and wrist -> joint 9 points along -y.  Returns the bound (crop pixels)."""
    a = min(float(np.hypot(m[0], m[3])) for m in mats)
    bound = 8 * float(np.spacing(F(np.abs(joints).max()))) / a
    worst = max(float(np.abs(c - crops[0]).max()) for c in crops)
    print(f"canonicalisation: crops differ by at most {worst:.3e} px, bound {bound:.3e} px (scale a = {a:.4f})")
    assert worst <= bound
    for c in crops:
        up = c[9] - c[0]
        assert up[1] < 0 and abs(up[0]) <= 2 * bound
    return bound


def test_canonicalisation():
    """The property the feature exists for: however the hand is turned in the frame, and whether it is a left or a right one, the
    network sees the same crop."""
    from lighthand_amd.topdown import (box_affine_host, boxes_from_keypoints_host, roi_affine_host, rois_from_keypoints_host)
    size = (256, 256)
    cases = canonicalisation_cases(size)
    joints = np.stack([j for j, _ in cases])
    mirror = np.array([m for _, m in cases], np.int32)
    b = len(cases)
    assert b == 10
    mv, src = np.ones((b, 21), np.float32), np.zeros(b, np.int32)
    start = np.tile(F([800, 300, 1200, 700]), (b, 1))
    upright = np.tile(F([1, 0]), (b, 1))
    boxes, rot, lost = rois_from_keypoints_host(joints, mv, start, upright, src)
    assert lost.tolist() == [0] * b
    assert np.allclose(np.hypot(rot[:, 0], rot[:, 1]), 1.0, atol=1e-6)
    mats, msrc = roi_affine_host(boxes, rot, mirror, src, 1, size, 1.25)
    assert (msrc == 0).all()
    crops = [crop_coordinates(m, j) for m, j in zip(mats, joints)]
    bound = check_canonical(crops, mats, joints)
    assert all(-0.5 <= c.min() and c.max() <= 255.5 for c in crops)          # the padded ROI holds every joint
    # the upright path does not have the property (so the test cannot pass vacuously)
    plain_boxes, plain_lost = boxes_from_keypoints_host(joints, mv, start, src)
    plain_mats, _ = box_affine_host(plain_boxes, src, 1, size, 1.25)
    plain = [crop_coordinates(m, j) for m, j in zip(plain_mats, joints)]
    assert max(float(np.abs(c - plain[0]).max()) for c in plain) > 10 * bound


# ------------------------------------------------------------------------------------------------ 3. rotated bounds
def test_rois_from_keypoints_host():
    from lighthand_amd.topdown import rois_from_keypoints_host
    j = 21
    rng = np.random.RandomState(0)
    preds = rng.uniform(100, 400, size=(7, j, 2)).astype(np.float32)
    mv = np.full((7, j, 1), 0.9, np.float32)
    old = rng.uniform(0, 50, size=(7, 4)).astype(np.float32)
    rot = np.array([[0.6, 0.8]] * 7, np.float32)
    rot[2] = (3.0, -4.0)                                         # not a unit vector
    src = np.array([0, 0, 0, 0, 0, -1, 0], np.int32)
    preds[1] = preds[1, :1] + rng.uniform(-2, 2, size=(j, 2)).astype(np.float32)       # slot 1: a 4 px cluster -> min_side, anchors too close
    mv[2, 9] = 0.05                                              # slot 2: an anchor below min_score -> keeps rot / |rot|
    mv[3, 5:] = 0.05                                             # slot 3: five joints (anchor 9 is not among them), the others far away
    preds[3, 5:] += 1000
    mv[4, 7:] = 0.0                                              # slot 4: seven joints, one short of min_joints
    rot[6] = (0.0, 0.0)                                          # slot 6: no incoming direction, but the anchors give one
    nxt, nrot, lost = rois_from_keypoints_host(preds, mv, old, rot, src, axis=(0, 9), min_score=0.1, min_joints=5, min_side=16.0, min_axis=4.0)
    assert nxt.dtype == np.float32 and nrot.dtype == np.float32 and lost.dtype == np.int32
    assert lost.tolist() == [0, 0, 0, 0, 0, 1, 0]
    # slot 0: the direction of the anchors, and a tight box of the projected joints
    d = (preds[0, 9] - preds[0, 0]).astype(np.float64)
    u = d / np.hypot(*d)
    assert np.allclose(nrot[0], (-u[1], u[0]), atol=1e-6)
    for i in (0, 3, 6):
        c, s = nrot[i].astype(np.float64)
        pts = preds[i][mv[i, :, 0] >= 0.1].astype(np.float64)
        p, q = pts[:, 0] * c + pts[:, 1] * s, pts[:, 1] * c - pts[:, 0] * s
        cp, cq = (p.min() + p.max()) / 2, (q.min() + q.max()) / 2
        want = np.array([cp * c - cq * s - (p.max() - p.min()) / 2, cp * s + cq * c - (q.max() - q.min()) / 2,
                         cp * c - cq * s + (p.max() - p.min()) / 2, cp * s + cq * c + (q.max() - q.min()) / 2])
        assert np.abs(nxt[i] - want).max() <= 8 * np.spacing(F(np.abs(want).max()))
    assert np.allclose(nrot[3], (0.6, 0.8), atol=1e-6) and np.allclose(nrot[6, 0] ** 2 + nrot[6, 1] ** 2, 1.0, atol=1e-6)
    # slot 1: widened about its centre to min_side, orientation kept (the anchors are closer than min_axis)
    assert np.allclose(nrot[1], (0.6, 0.8), atol=1e-6)
    assert abs((nxt[1, 2] - nxt[1, 0]) - 16.0) <= 1e-3 and abs((nxt[1, 3] - nxt[1, 1]) - 16.0) <= 1e-3
    assert np.abs((nxt[1, :2] + nxt[1, 2:]) / 2 - preds[1].mean(0)).max() < 4.0
    # slot 2: the incoming direction, normalised
    assert np.allclose(nrot[2], (0.6, -0.8), atol=1e-6)
    # slot 5: empty -> keeps box and rot, bit for bit
    assert nxt[5].tolist() == old[5].tolist() and nrot[5].tolist() == rot[5].tolist()
    nxt, nrot, lost = rois_from_keypoints_host(preds, mv, old, rot, src, axis=(0, 9), min_score=0.1, min_joints=8, min_side=16.0, min_axis=4.0)
    assert lost.tolist() == [0, 0, 0, 1, 1, 1, 0]                # 5 and 7 joints < 8
    assert nxt[3].tolist() == old[3].tolist() and nrot[4].tolist() == rot[4].tolist()
    # no direction at all (zero rot and an anchor below the threshold): lost, never NaN
    mv[6, 0] = 0.0
    nxt, nrot, lost = rois_from_keypoints_host(preds, mv, old, rot, src, axis=(0, 9), min_score=0.1, min_joints=5)
    assert lost[6] == 1 and nxt[6].tolist() == old[6].tolist() and nrot[6].tolist() == [0.0, 0.0]
    assert np.isfinite(nxt).all() and np.isfinite(nrot).all()


# ------------------------------------------------------------------------------------------------ 4. the filter
def sine_sequence(frames=300, seed=11):
    """[frames][1][1][2]: a 400 px sine plus sigma = 2 px noise around x ~ 960 (y: the same around 540), fp32."""
    rng = np.random.RandomState(seed)
    t = np.arange(frames) / 30.0
    x = 960.0 + 400.0 * np.sin(2 * np.pi * 0.5 * t) + rng.normal(0, 2, size=frames)
    y = 540.0 + 400.0 * np.cos(2 * np.pi * 0.3 * t) + rng.normal(0, 2, size=frames)
    return np.stack([x, y], 1).astype(np.float32).reshape(frames, 1, 1, 2)


def run_filter(fn, seq, dt=1.0 / 30.0, **kw):
    state, out = None, []
    for x in seq:
        y, state = fn(x, dt, state, **kw)
        out.append(y)
    return np.stack(out)


def test_one_euro_restatement_against_fp64():
    from lighthand_amd.topdown import one_euro_host, one_euro_host64
    seq = sine_sequence()
    got = run_filter(one_euro_host, seq, min_cutoff=1.0, beta=0.007)
    want = run_filter(one_euro_host64, seq, min_cutoff=1.0, beta=0.007)
    assert got.dtype == np.float32 and want.dtype == np.float64
    bound = 16 * float(np.spacing(F(np.abs(seq).max())))
    worst = float(np.abs(got - want).max())
    print(f"one_euro_host against fp64 over 300 frames: max |d| {worst:.3e} px, bound {bound:.3e} px")
    assert worst < bound
    assert float(np.abs(want[30:] - seq[30:]).max()) > 1.0         # the filter does filter: it lags the 400 px sine
    # beta = 0 and a huge cut-off: alpha -> 1, the input comes back
    through = run_filter(one_euro_host, seq, min_cutoff=1e9, beta=0.0)
    assert float(np.abs(through - seq).max()) < bound


def test_one_euro_resets():
    from lighthand_amd.topdown import one_euro_host
    rng = np.random.RandomState(2)
    x = rng.uniform(0, 1000, size=(4, 5, 3, 2)).astype(np.float32)     # 4 frames, 5 slots, 3 joints
    kw = dict(min_cutoff=1.0, beta=0.007)
    y0, st = one_euro_host(x[0], 1 / 30, None, **kw)
    assert np.array_equal(y0, x[0]) and st[2].tolist() == [1] * 5 and np.array_equal(st[0], x[0]) and not st[1].any()      # first frame
    dt = np.array([1 / 30, 0.0, np.nan, 1 / 30, -1.0], np.float32)
    y1, st1 = one_euro_host(x[1], dt, st, src_frame=[0, 0, 0, 0, 0], lost=[0, 0, 0, 1, 0], **kw)
    assert not np.array_equal(y1[0], x[1, 0]) and np.isfinite(y1).all()
    lo, hi = np.minimum(x[0, 0], x[1, 0]), np.maximum(x[0, 0], x[1, 0])
    assert (y1[0] >= lo).all() and (y1[0] <= hi).all()                                      # a convex mix of old and new
    for slot in (1, 2, 4):                                                                  # dt <= 0, NaN: the filter starts again
        assert np.array_equal(y1[slot], x[1, slot]) and np.array_equal(st1[0][slot], x[1, slot]) and not st1[1][slot].any()
    assert st1[2].tolist() == [1, 1, 1, 0, 1]
    assert np.array_equal(y1[3], x[1, 3]) and np.array_equal(st1[0][3], st[0][3])           # lost: passed through, state untouched
    y2, st2 = one_euro_host(x[2], 1 / 30, st1, src_frame=[0, -1, 0, 0, 0], lost=[0, 0, 0, 0, 0], **kw)
    assert np.array_equal(y2[3], x[2, 3]) and st2[2].tolist() == [1, 0, 1, 1, 1]            # found again: starts fresh; slot 1 empty
    assert np.array_equal(y2[1], x[2, 1])
    y3, st3 = one_euro_host(x[3], 1 / 30, st2, **kw)
    assert not np.array_equal(y3[3], x[3, 3]) and np.array_equal(y3[1], x[3, 1]) and st3[2].tolist() == [1] * 5
    assert np.array_equal(st[0], x[0])                                                      # the inputs are not modified


def test_one_euro_halves_the_jitter_of_a_still_point():
    from lighthand_amd.topdown import one_euro_host
    rng = np.random.RandomState(4)
    seq = (np.array([960.0, 540.0]) + rng.normal(0, 2, size=(300, 2))).astype(np.float32).reshape(300, 1, 1, 2)
    out = run_filter(one_euro_host, seq, min_cutoff=1.0, beta=0.007)
    raw, smooth = float(seq[30:].std(0).mean()), float(out[30:].std(0).mean())
    print(f"still point, sigma = 2 px: standard deviation {raw:.2f} px raw, {smooth:.2f} px filtered")
    assert smooth < 0.5 * raw


# ------------------------------------------------------------------------------------------------ C ABI
def test_roi_entries_are_exported_and_declared():
    from lighthand_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lighthand_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_roi_entries_validate_arguments_without_gpu():
    from lighthand_amd import _lib
    lib = _lib.load()
    fake, fake2, fake3 = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)      # never dereferenced

    def affine(boxes=fake, rot=fake, mirror=fake, index=fake, b=4, n=2, h=64, w=64, padding=1.25, mat=fake, src=fake):
        return lib.lh_roi_affine(boxes, rot, mirror, index, b, n, h, w, padding, mat, src, None)
    for rc in (affine(boxes=None), affine(rot=None), affine(mirror=None), affine(index=None), affine(mat=None), affine(src=None), affine(b=0),
               affine(n=0), affine(h=0), affine(w=-1), affine(padding=0.0), affine(padding=float("nan")), affine(padding=float("inf"))):
        assert rc == -1 and b"lh_roi_affine" in lib.lh_last_error()

    def k2r(preds=fake, mv=fake, boxes=fake, rot=fake, src=fake, b=4, j=21, k0=0, k1=9, score=0.1, joints=8, side=16.0, axis=4.0, nxt=fake2,
            nrot=fake3, lost=fake):
        return lib.lh_keypoints_to_rois(preds, mv, boxes, rot, src, b, j, k0, k1, score, joints, side, axis, nxt, nrot, lost, None)
    for rc in (k2r(preds=None), k2r(mv=None), k2r(boxes=None), k2r(rot=None), k2r(src=None), k2r(nxt=None), k2r(nrot=None), k2r(lost=None),
               k2r(b=0), k2r(j=0), k2r(joints=0), k2r(side=-1.0), k2r(side=float("inf")), k2r(score=float("nan")), k2r(axis=0.0),
               k2r(axis=float("nan")), k2r(k0=-1), k2r(k1=21), k2r(k0=9), k2r(nxt=fake), k2r(nrot=fake)):
        assert rc == -1 and b"lh_keypoints_to_rois" in lib.lh_last_error()

    def euro(x=fake, src=fake, lost=None, dt=fake, b=4, j=21, fc=1.0, beta=0.007, dc=1.0, xhat=fake2, dxhat=fake3, init=fake, out=fake):
        return lib.lh_one_euro(x, src, lost, dt, b, j, fc, beta, dc, xhat, dxhat, init, out, None)
    for rc in (euro(x=None), euro(src=None), euro(dt=None), euro(xhat=None), euro(dxhat=None), euro(init=None), euro(out=None), euro(b=0),
               euro(j=0), euro(fc=0.0), euro(fc=-1.0), euro(fc=float("nan")), euro(beta=-0.1), euro(beta=float("inf")), euro(dc=0.0),
               euro(dc=float("nan")), euro(xhat=fake), euro(dxhat=fake), euro(dxhat=fake2), euro(out=fake2), euro(out=fake3)):
        assert rc == -1 and b"lh_one_euro" in lib.lh_last_error()


# ------------------------------------------------------------------------------------------------ 5. argument errors
def test_infer_step_refuses_bad_roi_arguments():
    """Refused with ValueError before the model is looked at (and so before any device work)."""
    from lighthand_amd.runtime import InferPipeline, InferStep
    fr = dict(frames=(2, 96, 128))
    for cls in (InferStep, InferPipeline):
        with pytest.raises(ValueError, match="frames"):
            cls(object(), 2, 64, 64, oriented=True)
        with pytest.raises(ValueError, match="frames"):
            cls(object(), 2, 64, 64, smooth=(1.0, 0.007))
        for bad in ((0, 0), (9, 9), (-1, 9), (0,), (0, 9, 3), (0.0, 9), (True, 9), "09", 9, None):
            with pytest.raises(ValueError, match="track_axis"):
                cls(object(), 2, 64, 64, oriented=True, track=True, track_axis=bad, **fr)
        for bad in (0, -4.0, float("nan"), float("inf"), "4", None):
            with pytest.raises(ValueError, match="track_min_axis"):
                cls(object(), 2, 64, 64, oriented=True, track=True, track_min_axis=bad, **fr)
        for bad in ((-1.0, 0.007), (0.0, 0.007), (1.0, -0.007), (1.0, 0.007, -1.0), (1.0, 0.007, 0.0), (1.0,), (1.0, 0.007, 1.0, 2.0),
                    (float("nan"), 0.007), (1.0, float("inf")), (1.0, 0.007, float("nan")), ("1", 0.007), 1.0, True):
            with pytest.raises(ValueError, match="smooth"):
                cls(object(), 2, 64, 64, smooth=bad, **fr)
        with pytest.raises(ValueError, match="input_u8"):                     # the earlier checks still come first
            cls(object(), 2, 64, 64, oriented=True, input_u8=(96, 128), **fr)
        # anchors past the model's joints: the count is the output channels of its last convolution, read before any plan is built
        # (the stand-in has nothing else a plan could be built from)
        model = types.SimpleNamespace(final_layer=types.SimpleNamespace(out_channels=21))
        for bad in ((0, 21), (21, 0), (5, 400)):
            with pytest.raises(ValueError, match="track_axis.*21 joints"):
                cls(model, 2, 64, 64, oriented=True, track=True, track_axis=bad, **fr)


def test_track_frames_cli_flags_for_rois():
    from lighthand_amd.tools import track_frames as T
    args = T.build_parser().parse_args(["--synthetic", "8", "--frame_size", "96x128"])
    assert (args.oriented, args.mirror, args.one_euro, args.spin) == (False, False, None, 0.0)
    args = T.build_parser().parse_args(["--synthetic", "4", "--oriented", "--mirror", "--one_euro", "1.0", "0.007", "--spin", "10"])
    assert (args.oriented, args.mirror, args.one_euro, args.spin) == (True, True, [1.0, 0.007], 10.0)
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--synthetic", "4", "--one_euro", "1.0"])
    still, boxes = T.synthetic_sequence(3, 96, 128, 2, seed=1)
    same, same_boxes = T.synthetic_sequence(3, 96, 128, 2, seed=1, spin=0.0)
    spun, spun_boxes = T.synthetic_sequence(3, 96, 128, 2, seed=1, spin=10.0)
    assert (still == same).all() and (boxes == same_boxes).all()
    assert (spun[0] == still[0]).all() and (spun_boxes == boxes).all() and not (spun[2] == still[2]).all()


# ------------------------------------------------------------------------------------------------ 6. resource table
def test_roi_kernels_are_listed_without_scratch_or_spills():
    """The three kernels are listed with [0, 0] in the table that tests/test_kernel_resources.py holds every built kernel to
    (tools/kernel_resources.py: GOLDEN), none of them is in kernel_resources.json or kernel_ceilings.json, and every other entry of
    the table in force is kernel_ceilings.json's, unchanged.  Reads the JSON files only."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    with open(kr.GOLDEN) as f:
        table = json.load(f)
    with open(kr.FROZEN) as f:
        frozen = json.load(f)
    with open(os.path.join(ROOT, "tests", "golden", "kernel_ceilings.json")) as f:
        ceilings = json.load(f)
    new = {}
    for name in KERNELS:
        hits = {k: v for k, v in table.items() if name in k}
        assert len(hits) == 1 and not any(k in frozen or k in ceilings for k in hits), name
        assert all(v == [0, 0] for v in hits.values()), hits
        new.update(hits)
    assert {k: v for k, v in table.items() if k not in new} == ceilings
