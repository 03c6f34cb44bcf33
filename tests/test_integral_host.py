"""CPU: the host side of integral regression (lh_integral_l1, heatmap.IntegralL1Loss, post_process="soft", TrainStep(coord_loss_weight=),
the CLI flags) and the float64 NumPy restatement of the kernel's formulas, which tests/test_gpu_integral.py measures the kernel against.

The restatement is checked here against torch float64 autograd through softmax -> expectation -> weighted L1 on the four shapes of
the GPU test: loss and gradient agree to 1e-12 (the gradient relative to its plane's largest magnitude; measured 4e-15 to 4e-14)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

F32, F64 = np.float32, np.float64

# (b, j, h, w, beta): fewer cells than a wave and not square; not a multiple of 256; the product shape; the largest plane
SHAPES = [(2, 3, 6, 10, 10.0), (3, 5, 24, 40, 30.0), (1, 21, 64, 64, 100.0), (1, 2, 96, 96, 100.0)]
SCALE = 4.0


def make_case(b, j, h, w, beta, seed):
    """Seeded inputs: maps = A * (a sigma-2 Gaussian around an interior cell + noise of 1/20) with A = 20 / beta, so that beta * map
    spans 20 whatever beta is: the softmax keeps a few percent of its mass on the peak's neighbours (a one-hot softmax would leave
    the gradient's largest entry a rounding residue of x_peak - ex, and no two float64 evaluations would agree on it) and none in
    the far field; joints (input pixels, scale 4) offset from the peak by 0.3 to 2 cells per axis with a random sign; weights from
    {0, 0.7, 1} with a 0 and a non-zero one in every case.
    Returns (maps f32 [b][j][h][w], joints f32 [b][j][2], weight f32 [b][j])."""
    rng = np.random.RandomState(seed)
    px, py = rng.randint(2, w - 2, size=(b, j)), rng.randint(2, h - 2, size=(b, j))
    ys, xs = np.mgrid[0:h, 0:w]
    maps = np.exp(-((xs - px[..., None, None]) ** 2 + (ys - py[..., None, None]) ** 2) / 8.0) + rng.randn(b, j, h, w) / 20.0
    maps *= 20.0 / beta
    off = rng.uniform(0.3, 2.0, size=(b, j, 2)) * rng.choice([-1.0, 1.0], size=(b, j, 2))
    joints = (np.stack([px, py], -1) + off) * SCALE
    weight = rng.choice([0.0, 0.7, 1.0], size=(b, j))
    weight.reshape(-1)[:2] = (0.0, 0.7)
    return maps.astype(F32), joints.astype(F32), weight.astype(F32)


def restate(maps, joints, weight, beta, scale, lam, gs=1.0, recipe=False):
    """The formulas of lh_integral_l1 from the fp32 inputs.  recipe=False: everything in float64.  recipe=True: the kernel's
    precision recipe -- fp32 exp argument and exp, fp64 sums, preds / residual / joint_loss in fp32, k_n rounded to fp32, the
    bracket in fp64 rounded once, two fp32 products.  Returns (preds [b][j][2], joint_loss [b][j], loss, grad [b][j][h][w])."""
    b, j, h, w = maps.shape
    wgt = np.ones((b, j), F32) if weight is None else np.asarray(weight, F32).reshape(b, j)
    m = np.asarray(maps, F32).reshape(b, j, -1)
    x, y = (np.arange(h * w) % w).astype(F64), (np.arange(h * w) // w).astype(F64)
    if recipe:
        e32 = np.exp((F32(beta) * (m - m.max(2, keepdims=True))).astype(F32)).astype(F32)
        e = e32.astype(F64)
    else:
        e = np.exp(F64(beta) * (m.astype(F64) - m.max(2, keepdims=True).astype(F64)))
    s0 = e.sum(2)
    ex, ey = (e * x).sum(2) / s0, (e * y).sum(2) / s0
    jt = np.asarray(joints, F32)[..., :2]
    if recipe:
        preds = np.stack([ex.astype(F32) * F32(scale), ey.astype(F32) * F32(scale)], -1).astype(F32)
        r = (preds - jt).astype(F32)
        jl = (wgt * (np.abs(r[..., 0]) + np.abs(r[..., 1])).astype(F32)).astype(F32)
    else:
        preds = np.stack([ex, ey], -1) * F64(scale)
        r = preds - jt.astype(F64)
        jl = wgt.astype(F64) * (np.abs(r[..., 0]) + np.abs(r[..., 1]))
    sg = np.sign(r).astype(F64)
    loss = F64(lam) * jl.astype(F64).sum() / (2 * b * j)
    k = F64(gs) * F64(lam) * wgt.astype(F64) * F64(scale) * F64(beta) / (2 * b * j) / s0
    bracket = (x - ex[..., None]) * sg[..., 0:1] + (y - ey[..., None]) * sg[..., 1:2]
    if recipe:
        grad = ((e32 * k.astype(F32)[..., None]).astype(F32) * bracket.astype(F32)).astype(F32)
        loss = F32(loss)
    else:
        grad = e * k[..., None] * bracket
    return preds, jl, loss, grad.reshape(b, j, h, w)


def plane_rel_err(got, want):
    """max |got - want| per plane, relative to the plane's max |want|; planes whose `want` is all zero give 0 when got is zero too."""
    b, j = want.shape[:2]
    d = np.abs(np.asarray(got, F64) - want).reshape(b, j, -1).max(2)
    ref = np.abs(want).reshape(b, j, -1).max(2)
    return np.where(ref > 0, d / np.where(ref > 0, ref, 1.0), np.where(d > 0, np.inf, 0.0))


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_equals_torch_float64_autograd(shape):
    b, j, h, w, beta = shape
    maps, joints, weight = make_case(b, j, h, w, beta, seed=h * w)
    lam, gs = 0.37, 3.0
    preds, jl, loss, grad = restate(maps, joints, weight, beta, SCALE, lam, gs)
    # no residual near the sign change: 0.04 px is a thousand times the fp32 rounding of a coordinate of 384 px (2.3e-5 px)
    assert np.abs(preds - joints).min() > 0.01 * SCALE

    hm = torch.from_numpy(maps.astype(F64)).requires_grad_(True)
    p = torch.softmax(beta * hm.flatten(2), dim=2)
    # coordinates relative to each plane's arg-max cell (added back after the sum: the same expectation), so that autograd's own
    # p * (v - sum p v) does not cancel two numbers of the size of the map where p is large
    idx, top = torch.arange(h * w, dtype=torch.float64), torch.from_numpy(maps.reshape(b, j, -1).argmax(2))
    cx, cy = (top % w).double()[..., None], torch.div(top, w, rounding_mode="floor").double()[..., None]
    tx = (p * (idx % w - cx)).sum(2) + cx[..., 0]
    ty = (p * (torch.div(idx, w, rounding_mode="floor") - cy)).sum(2) + cy[..., 0]
    tp = torch.stack([tx, ty], -1) * SCALE
    tjl = torch.from_numpy(weight.astype(F64)) * (tp - torch.from_numpy(joints.astype(F64))).abs().sum(2)
    tloss = lam * tjl.sum() / (2 * b * j)
    (gs * tloss).backward()
    assert np.abs(preds - tp.detach().numpy()).max() <= 1e-12 * np.abs(preds).max()
    assert np.abs(jl - tjl.detach().numpy()).max() <= 1e-12 * np.abs(jl).max()
    assert abs(loss - tloss.item()) <= 1e-12 * abs(loss) and loss > 0
    err = plane_rel_err(hm.grad.numpy(), grad)
    print(f"{shape}: restatement vs autograd, gradient {err.max():.2e}")
    assert err.max() <= 1e-12
    assert not grad[weight == 0].any() and grad[weight != 0].any()


def test_recipe_restatement_is_close_to_the_float64_one():
    """The yardstick of the GPU test, on the CPU: the kernel's precision recipe against all-float64, per plane relative to max |g|
    (prints the figures; they are fp32 rounding of the exp argument, so anything near 1e-5 would be a wrong recipe)."""
    for b, j, h, w, beta in SHAPES:
        maps, joints, weight = make_case(b, j, h, w, beta, seed=h * w)
        want = restate(maps, joints, weight, beta, SCALE, 0.01)
        got = restate(maps, joints, weight, beta, SCALE, 0.01, recipe=True)
        err = plane_rel_err(got[3], want[3]).max()
        print(f"({b}, {j}, {h}, {w}, {beta}): recipe vs float64, gradient {err:.2e}")
        assert 0 < err < 2e-6
        assert np.abs(got[0] - want[0]).max() <= 2 * np.spacing(F32(np.abs(want[0]).max()))


def test_entries_are_exported_declared_and_bound_with_the_header_arity():
    from lighthand_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lighthand_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(lh_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S))
    for name, arity in (("lh_integral_l1_workspace_bytes", 2), ("lh_integral_l1", 20), ("lh_heatmap_soft_argmax", 8)):
        assert name in protos, f"{name} is not declared in the header"
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert len(protos[name].split(",")) == len(_lib.SIGNATURES[name][1]) == arity, name
    assert lib.lh_integral_l1_workspace_bytes(64, 21) >= 64 * 21 * 8 + 4 and lib.lh_integral_l1_workspace_bytes(0, 21) == 0


def test_integral_l1_validates_arguments_without_gpu():
    from lighthand_amd import _lib
    lib = _lib.load()
    hm, jt, pr, ls, gr, ws = (C.c_void_p(a) for a in (0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000))   # never dereferenced

    def call(hm=hm, jt=jt, jstride=2, b=2, j=21, h=64, w=64, beta=100.0, scale=4.0, lam=1.0, pr=pr, ls=ls, gr=gr, ws=ws):
        return lib.lh_integral_l1(hm, jt, jstride, None, b, j, h, w, beta, scale, lam, pr, None, ls, 0, gr, 0, None, ws, None)
    nan, inf = float("nan"), float("inf")
    bad = [call(hm=None), call(jt=None), call(pr=None), call(ls=None), call(ws=None), call(jstride=1), call(b=0), call(j=-1), call(h=0),
           call(w=0), call(beta=0.0), call(beta=-1.0), call(beta=nan), call(beta=inf), call(lam=nan), call(lam=inf), call(scale=nan),
           call(h=5, w=5), call(h=3, w=6), call(h=96, w=97), call(h=128, w=128), call(h=1 << 16, w=1 << 16),
           call(hm=C.c_void_p(0x100004)), call(gr=C.c_void_p(0x500008)), call(ws=C.c_void_p(0x600004))]
    for k, rc in enumerate(bad):
        assert rc == -1, k
    assert call(beta=0.0) == -1 and b"lh_integral_l1" in lib.lh_last_error() and b"beta" in lib.lh_last_error()
    assert call(h=5, w=5) == -1 and b"multiple of 4" in lib.lh_last_error()
    assert call(h=96, w=97) == -1 and b"exceeds" in lib.lh_last_error()
    assert call(hm=None) == -1 and b"lh_integral_l1" in lib.lh_last_error()


def test_soft_is_a_decode_mode_and_the_others_stay():
    from lighthand_amd import heatmap
    assert heatmap.decode_mode("soft") == "soft"
    assert [heatmap.decode_mode(v) for v in (False, None, True, "quarter", "dark")] == [None, None, "quarter", "quarter", "dark"]
    for bad in ("Soft", "softmax", "integral", ""):
        with pytest.raises(ValueError, match="post_process"):
            heatmap.decode_mode(bad)


def test_defaults_are_off():
    from lighthand_amd import heatmap
    from lighthand_amd.runtime import InferPipeline, InferStep, TrainStep
    from lighthand_amd.tools import wearable_eval_2d as E
    p = inspect.signature(TrainStep.__init__).parameters
    assert p["coord_loss_weight"].default == 0.0 and p["soft_argmax_beta"].default == 100.0
    for fn in (heatmap.max_preds_device, heatmap.get_max_preds, InferStep.__init__, InferPipeline.__init__, E._Steps.__init__,
               E.pred_store, E.pred_store_test, E.device_eval):
        p = inspect.signature(fn).parameters
        assert p["post_process"].default is False and p["soft_argmax_beta"].default == 100.0, fn
    p = inspect.signature(heatmap.IntegralL1Loss.__init__).parameters
    assert p["beta"].default == 100.0 and p["scale"].default == 1.0
    assert list(inspect.signature(heatmap.IntegralL1Loss.forward).parameters)[1:] == ["output", "joints", "target_weight"]


def test_bad_options_raise_at_construction():
    from lighthand_amd import heatmap
    from lighthand_amd._lib import LightHandError
    from lighthand_amd.runtime import InferPipeline, InferStep, TrainStep
    for bad in (-0.01, float("nan"), float("inf"), "0.1", None, True):
        with pytest.raises(ValueError, match="coord_loss_weight"):
            TrainStep(object(), 2, 64, 64, coord_loss_weight=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "100", None):
        with pytest.raises(ValueError, match="soft_argmax_beta"):
            TrainStep(object(), 2, 64, 64, coord_loss_weight=0.1, soft_argmax_beta=bad)
        with pytest.raises(ValueError, match="soft_argmax_beta"):
            InferStep(object(), 2, 64, 64, post_process="soft", soft_argmax_beta=bad)
        with pytest.raises(ValueError, match="soft_argmax_beta"):
            InferPipeline(object(), 2, 64, 64, post_process="soft", soft_argmax_beta=bad)
    with pytest.raises(LightHandError, match="targets_from_joints"):
        TrainStep(object(), 2, 64, 64, coord_loss_weight=0.1, targets_from_joints=False)
    for bad in (0.0, -3.0, float("nan")):
        with pytest.raises(ValueError, match="beta"):
            heatmap.IntegralL1Loss(beta=bad)
    with pytest.raises(LightHandError, match="HIP device"):
        heatmap.IntegralL1Loss()(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 2))


def test_cli_flags():
    from lighthand_amd.tools import train as T
    from lighthand_amd.tools import wearable_eval_2d as E
    a = T.parse_args([])
    assert (a.coord_loss_weight, a.soft_argmax_beta, a.soft_decode) == (0.0, 100.0, False)
    a = T.parse_args(["--coord_loss_weight", "0.01", "--soft_argmax_beta", "50", "--soft_decode"])
    assert (a.coord_loss_weight, a.soft_argmax_beta, a.soft_decode) == (0.01, 50.0, True)
    for argv in (["--soft_decode", "--dark_decode"], ["--coord_loss_weight", "-1"], ["--soft_argmax_beta", "0"],
                 ["--coord_loss_weight", "much"]):
        with pytest.raises(SystemExit) as err:
            T.parse_args(argv)
        assert err.value.code == 2, argv
    e = E.build_parser().parse_args([])
    assert (e.soft_decode, e.soft_argmax_beta) == (False, 100.0)
    e = E.build_parser().parse_args(["--soft_decode", "--soft_argmax_beta", "25"])
    assert (e.soft_decode, e.soft_argmax_beta, e.post_process, e.dark_decode) == (True, 25.0, False, False)
    for other in ("--post_process", "--dark_decode"):
        with pytest.raises(SystemExit) as err:
            E.main(["--synthetic", "4", "--soft_decode", other])
        assert err.value.code == 2                                   # argparse's error exit, before any model is built
    with pytest.raises(SystemExit) as err:
        E.main(["--synthetic", "4", "--soft_decode", "--soft_argmax_beta", "0"])
    assert err.value.code == 2
