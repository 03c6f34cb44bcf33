"""GPU: integral regression -- lh_integral_l1, heatmap.IntegralL1Loss, TrainStep(coord_loss_weight=), post_process="soft".

No reference oracle exists (the reference has neither a soft-arg-max nor a coordinate loss): the kernel is measured against the
float64 NumPy restatement of tests/test_integral_host.py, which that file checks against torch float64 autograd.

The gradient yardstick is a host restatement, never the code under test: the restatement evaluated with the kernel's precision recipe
(fp32 exp argument and exp, fp64 sums, fp64 bracket) against the all-float64 one, per plane relative to the plane's max |g|.  On the
CPU that measures 1.75e-7, 1.44e-7, 2.03e-7 and 1.01e-7 on the four shapes below; the device bound is FACTOR = 8 times the value the
test measures for its own inputs (8 for the device expf's 1-2 ulp and another summation order).  The test prints the device figures next to
the yardsticks before it asserts; on an MI355X the gradient measured 1.03e-7, 1.44e-7, 1.55e-7 and 0.81e-7 (0.6 to 1.0 of the yardstick,
the same with and without grad_scale).  joint_loss follows the same rule, FACTOR times its own host yardstick (5.4e-8, 1.6e-7,
7.8e-7 and 1.5e-6 on the CPU), plus ONE additive allowance from the number format that FACTOR does not multiply: a residual is the
difference of two fp32 coordinates, so one plane's loss carries up to one ulp of the largest coordinate, relative to the smallest
plane loss.  loss is a positive combination of the plane losses, so it keeps their relative bound (allowance included), plus 2^-24
for its own rounding to fp32.  In accumulate mode grad = fp32(prefill + g): one more rounding, 2^-24 of the largest |prefill + g| of the plane."""
import os

import numpy as np
import pytest
import torch

from conftest import resnet_cfg
from test_integral_host import SCALE, SHAPES, make_case, plane_rel_err, restate

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
FACTOR = 8.0
EPS = 2.0 ** -24


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def _integral(maps, joints, weight, beta, lam, gs=None, grad=None, add_grad=False, loss0=None, with_grad=True, scale=SCALE):
    """lh_integral_l1 on device tensors -> dict of NumPy outputs.  ``grad``: the pre-filled gradient buffer (NaN when absent)."""
    from lighthand_amd import _lib
    lib = _lib.load()
    b, j, h, w = maps.shape
    preds = torch.full((b, j, 2), float("nan"), device="cuda")
    jl = torch.full((b, j), float("nan"), device="cuda")
    loss = torch.full((), float("nan") if loss0 is None else float(loss0), device="cuda")
    if with_grad and grad is None:
        grad = torch.full_like(maps, float("nan"))
    g = grad.clone() if with_grad else None
    ws = torch.zeros(lib.lh_integral_l1_workspace_bytes(b, j), dtype=torch.uint8, device="cuda")
    gsd = None if gs is None else torch.tensor([gs], dtype=torch.float32, device="cuda")
    _lib.check(lib.lh_integral_l1(maps.data_ptr(), joints.data_ptr(), joints.shape[2], None if weight is None else weight.data_ptr(), b, j,
                                  h, w, float(beta), float(scale), float(lam), preds.data_ptr(), jl.data_ptr(), loss.data_ptr(),
                                  int(loss0 is not None), None if g is None else g.data_ptr(), int(add_grad),
                                  None if gsd is None else gsd.data_ptr(), ws.data_ptr(), _stream()), "lh_integral_l1")
    torch.cuda.synchronize()
    return dict(preds=preds.cpu().numpy(), jl=jl.cpu().numpy(), loss=F32(loss.item()), grad=None if g is None else g.cpu().numpy(),
                coord=F32(ws[:4].view(torch.float32)[0].item()))


def _yardsticks(maps, joints, weight, beta, lam, gs=1.0, scale=SCALE):
    """(all-float64 restatement, gradient yardstick, joint_loss yardstick, format allowance): the recipe restatement against the
    float64 one; the allowance (one ulp of the largest coordinate over the smallest plane loss) is added once, outside FACTOR."""
    want = restate(maps, joints, weight, beta, scale, lam, gs)
    rec = restate(maps, joints, weight, beta, scale, lam, gs, recipe=True)
    y_grad = plane_rel_err(rec[3], want[3]).max()
    pos = want[1] > 0
    y_jl = (np.abs(rec[1].astype(F64) - want[1])[pos] / want[1][pos]).max()
    wgt = np.ones_like(want[1]) if weight is None else np.asarray(weight, F64).reshape(want[1].shape)
    fmt = np.spacing(F32(np.abs(want[0]).max())) * wgt[pos].max() / want[1][pos].min()
    return want, y_grad, y_jl, F64(fmt)


def _case(shape, seed=None):
    b, j, h, w, beta = shape
    maps, joints, weight = make_case(b, j, h, w, beta, seed=h * w if seed is None else seed)
    return maps, joints, weight, tuple(torch.from_numpy(a).cuda() for a in (maps, joints, weight))


@pytest.mark.parametrize("gs", [None, 1024.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_matches_the_restatement(shape, gs):
    """1. preds bit-equal to soft_argmax_device; gradient, joint_loss and loss within FACTOR x the host yardstick of the float64
    restatement (module docstring), in write mode and in accumulate mode on a pre-filled gradient; planes of weight 0 are exactly
    zero (write) or bit-untouched (accumulate)."""
    from lighthand_amd.heatmap import soft_argmax_device
    beta, lam = shape[4], 0.01
    maps, joints, weight, (dm, dj, dw) = _case(shape)
    want, y_grad, y_jl, fmt = _yardsticks(maps, joints, weight, beta, lam, 1.0 if gs is None else gs)
    wp, wjl, wloss, wgrad = want
    assert np.abs(wp - joints).min() > 0.01 * SCALE and (weight == 0).any() and (weight > 0).any()

    out = _integral(dm, dj, dw, beta, lam, gs)
    soft = soft_argmax_device(dm, beta=beta, scale=SCALE)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out["preds"]), _bits(soft))
    e_grad = plane_rel_err(out["grad"], wgrad).max()
    pos = wjl > 0
    e_jl = (np.abs(out["jl"].astype(F64) - wjl)[pos] / wjl[pos]).max()
    e_loss = abs(F64(out["loss"]) - wloss) / wloss
    print(f"{shape} gs={gs}: gradient {e_grad:.2e} (yardstick {y_grad:.2e}), joint_loss {e_jl:.2e} (yardstick {y_jl:.2e}, format {fmt:.2e}), "
          f"loss {e_loss:.2e}")
    assert e_grad <= FACTOR * y_grad
    assert e_jl <= FACTOR * y_jl + fmt and (out["jl"][~pos] == 0).all()
    assert e_loss <= FACTOR * y_jl + fmt + EPS and out["coord"] == out["loss"]
    assert not _bits(out["grad"])[weight == 0].any()                       # exactly +0.f

    # accumulate: a pre-filled gradient of the size of the plane's own gradient, and a loss that is added to
    rng = np.random.RandomState(5)
    gmax = np.abs(wgrad).reshape(*wgrad.shape[:2], -1).max(2)
    fill = (rng.randn(*wgrad.shape) * np.where(gmax > 0, gmax, 1.0)[..., None, None]).astype(F32)
    acc = _integral(dm, dj, dw, beta, lam, gs, grad=torch.from_numpy(fill).cuda(), add_grad=True, loss0=0.75)
    total = fill.astype(F64) + wgrad
    d = np.abs(acc["grad"].astype(F64) - total).reshape(*gmax.shape, -1).max(2)
    bound = FACTOR * y_grad * gmax + EPS * np.abs(total).reshape(*gmax.shape, -1).max(2)
    print(f"{shape} gs={gs}: accumulate, worst plane at {np.max(d / bound):.2f} of its bound")
    assert (d <= bound).all()
    assert np.array_equal(_bits(acc["grad"])[weight == 0], _bits(fill)[weight == 0])
    assert np.array_equal(_bits(acc["preds"]), _bits(out["preds"])) and np.array_equal(_bits(acc["jl"]), _bits(out["jl"]))
    assert acc["coord"] == out["loss"] and acc["loss"] == F32(F32(0.75) + out["loss"])
    # no gradient buffer: the same loss; no weights: ones
    ng = _integral(dm, dj, dw, beta, lam, gs, with_grad=False)
    assert ng["loss"] == out["loss"] and np.array_equal(_bits(ng["jl"]), _bits(out["jl"]))
    ones = _integral(dm, dj, torch.ones_like(dw), beta, lam, gs)
    none = _integral(dm, dj, None, beta, lam, gs)
    assert none["loss"] == ones["loss"] and np.array_equal(_bits(none["grad"]), _bits(ones["grad"]))


def test_two_calls_give_the_same_bits():
    """2. No atomics, fixed reduction order."""
    shape = SHAPES[2]
    _, _, _, (dm, dj, dw) = _case(shape)
    a = _integral(dm, dj, dw, shape[4], 0.01, 1024.0)
    junk = torch.randn(1 << 22, device="cuda")                   # other work in between
    junk.mul_(2.0)
    b = _integral(dm, dj, dw, shape[4], 0.01, 1024.0)
    assert a["loss"] == b["loss"] and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("grad", "jl", "preds"))


def test_bad_arguments_launch_nothing():
    """3. LH_ERR_ARG with the error text set, and every output buffer keeps its bits."""
    from lighthand_amd import _lib
    lib = _lib.load()
    maps = torch.randn(2, 3, 6, 10, device="cuda")
    odd = torch.randn(2, 3, 5, 5, device="cuda")
    big = torch.randn(1, 1, 96, 97, device="cuda")
    joints = torch.rand(2, 3, 2, device="cuda") * 20
    preds, jl, loss = torch.full((2, 3, 2), 7.0, device="cuda"), torch.full((2, 3), 7.0, device="cuda"), torch.full((), 7.0, device="cuda")
    grad = torch.full((1, 1, 96, 97), 7.0, device="cuda")
    ws = torch.full((lib.lh_integral_l1_workspace_bytes(2, 3),), 7, dtype=torch.uint8, device="cuda")

    def call(m=maps, jt=joints.data_ptr(), b=2, j=3, beta=10.0, pr=preds.data_ptr(), ls=loss.data_ptr(), w=ws.data_ptr()):
        return lib.lh_integral_l1(m.data_ptr(), jt, 2, None, b, j, m.shape[2], m.shape[3], beta, 4.0, 1.0, pr, jl.data_ptr(), ls, 0,
                                  grad.data_ptr(), 0, None, w, _stream())
    for rc in (call(m=odd), call(m=big, b=1, j=1), call(beta=0.0), call(beta=-2.0), call(jt=None), call(pr=None), call(ls=None),
               call(w=None)):
        assert rc == -1 and b"lh_integral_l1" in lib.lh_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (preds, jl, loss, grad, ws))
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((preds == 7).any()) and float(loss) != 7.0


def test_loss_module_delivers_the_gradient_through_autograd():
    """4. IntegralL1Loss: loss, .preds and .joint_loss are the kernel's (lambda = 1), the heat-maps receive the kernel's gradient times
    the upstream gradient; weights of shape [B, J, 1], [B, J] and None; joints with a third column."""
    from lighthand_amd.heatmap import IntegralL1Loss
    shape = SHAPES[1]
    _, _, _, (dm, dj, dw) = _case(shape)
    for weight in (dw[..., None], dw, None):
        ref = _integral(dm, dj, weight if weight is None else dw, shape[4], 1.0)
        crit = IntegralL1Loss(beta=shape[4], scale=SCALE)
        x = dm.clone().requires_grad_(True)
        loss = crit(x, torch.cat([dj, torch.ones_like(dj[..., :1])], -1), weight)
        (loss * 3.0).backward()
        assert F32(loss.item()) == ref["loss"]
        assert np.array_equal(_bits(x.grad), _bits(ref["grad"] * F32(3.0)))
        assert np.array_equal(_bits(crit.preds), _bits(ref["preds"])) and np.array_equal(_bits(crit.joint_loss), _bits(ref["jl"]))
        assert not crit.joint_loss.requires_grad and not crit.preds.requires_grad
    # no gradient wanted (validation): the same loss and outputs, nothing kept for a backward
    with torch.no_grad():
        quiet = IntegralL1Loss(beta=shape[4], scale=SCALE)
        ql = quiet(dm, dj, None)
    assert F32(ql.item()) == ref["loss"] and not ql.requires_grad
    assert np.array_equal(_bits(quiet.preds), _bits(ref["preds"])) and np.array_equal(_bits(quiet.joint_loss), _bits(ref["jl"]))
    with pytest.raises(ValueError):
        IntegralL1Loss()(dm, dj, dw[:, :2])
    with pytest.raises(ValueError):
        IntegralL1Loss()(dm, dj[:, :2])


# ------------------------------------------------------------------------------------------------ step level
def _model(precision="fp32", seed=9001):
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    torch.manual_seed(seed)
    return get_pose_net(resnet_cfg(18), True).cuda().set_precision(precision)


def _batch(b, size, seed):
    rng = np.random.RandomState(seed)
    return (torch.from_numpy(rng.randn(b, 3, size, size).astype(F32)).cuda(),
            torch.from_numpy(rng.uniform(8, size - 8, size=(b, 21, 2)).astype(F32)).cuda())


def _train(steps, data, after=None, **kw):
    from lighthand_amd.runtime import TrainStep
    m = _model()
    st = TrainStep(m, 4, 64, 64, lr=1e-3, **kw)
    trace = []
    for k, (x, j) in enumerate(data[:steps]):
        loss = st(x, j)
        torch.cuda.synchronize()
        trace.append((loss.clone(), m.arena().flat.clone(), after(st, k) if after else None))
    return st, trace


def test_default_step_is_the_plain_step(monkeypatch):
    """5. R18 fp32 64^2 batch 4, 3 steps: coord_loss_weight=0.0 is the plain step bit for bit (loss and parameters after every
    step) and owns none of the new buffers."""
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    data = [_batch(4, 64, 30 + k) for k in range(3)]
    _, plain = _train(3, data)
    st, zero = _train(3, data, coord_loss_weight=0.0, soft_argmax_beta=50.0)
    for (la, wa, _), (lb, wb, _) in zip(plain, zero):
        assert np.array_equal(_bits(la), _bits(lb)) and torch.equal(wa, wb)
    assert st.coord_loss is None and st.soft_preds is None and st._integral_ws is None and st.coord_joint_loss is None


def _mse_reference(st):
    """lh_mse_heatmap (the plain step's loss kernel) on the step's own heat-maps and target -> (loss f32, grad f32 NumPy)."""
    from lighthand_amd import _lib
    lib = _lib.load()
    out = st.plan.out_nchw
    loss, grad = torch.zeros((), device="cuda"), torch.empty_like(out)
    ws = torch.empty(lib.lh_mse_workspace_bytes(out.numel()), dtype=torch.uint8, device="cuda")
    _lib.check(lib.lh_mse_heatmap(out.data_ptr(), st.target.data_ptr(), out.numel(), loss.data_ptr(), grad.data_ptr(),
                                  None if st._loss_scale_dev is None else st._loss_scale_dev.data_ptr(), ws.data_ptr(), _stream()),
               "lh_mse_heatmap")
    torch.cuda.synchronize()
    return F32(loss.item()), grad.cpu().numpy()


def _check_step_against_restatement(st, lam, beta, joints, weight, gs=1.0, mse=None):
    """step.loss = plain MSE loss + restated coordinate loss, plan.dout_nchw = MSE gradient + restated coordinate gradient, within
    test 1's tolerance (the restatement and its yardsticks are evaluated on the step's own plan.out_nchw)."""
    out = st.plan.out_nchw.cpu().numpy()
    mse_loss, mse_grad = mse if mse is not None else _mse_reference(st)
    want, y_grad, y_jl, fmt = _yardsticks(out, joints, weight, beta, lam, gs)
    wp, wjl, wloss, wgrad = want
    assert np.abs(wp - joints)[np.broadcast_to((np.ones_like(wjl) if weight is None else weight)[..., None] > 0, wp.shape)].min() > 1e-3
    from lighthand_amd.heatmap import soft_argmax_device
    assert np.array_equal(_bits(st.soft_preds), _bits(soft_argmax_device(st.plan.out_nchw, beta=beta, scale=SCALE)))
    coord = F64(st.coord_loss.item())
    print(f"coordinate loss {coord:.6f} (restated {wloss:.6f}), mse loss {mse_loss:.6f}, step loss {float(st.loss):.6f}")
    assert abs(coord - wloss) <= (FACTOR * y_jl + fmt + EPS) * wloss
    total = F64(mse_loss) + wloss
    assert abs(F64(st.loss.item()) - total) <= (FACTOR * y_jl + fmt + EPS) * wloss + EPS * total
    gmax = np.abs(wgrad).reshape(*wgrad.shape[:2], -1).max(2)
    sum_ = mse_grad.astype(F64) + wgrad
    d = np.abs(st.plan.dout_nchw.cpu().numpy().astype(F64) - sum_).reshape(*gmax.shape, -1).max(2)
    bound = FACTOR * y_grad * gmax + EPS * np.abs(sum_).reshape(*gmax.shape, -1).max(2)
    print(f"dout: worst plane at {np.max(d[bound > 0] / bound[bound > 0]):.2f} of its bound")
    assert (d <= bound).all() and gmax.max() > 0
    return mse_grad


def test_captured_step_matches_the_eager_step_and_the_restatement(monkeypatch):
    """6. coord_loss_weight = 0.01: captured and eager steps agree bit for bit over 3 steps (loss, coordinate loss, parameters), and
    after the first step loss and plan.dout_nchw are the plain MSE kernel's plus the restated coordinate term."""
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    data = [_batch(4, 64, 30 + k) for k in range(3)]

    def checked(st, k):
        if k == 0:
            _check_step_against_restatement(st, 0.01, 100.0, data[0][1].cpu().numpy(), None)
        return st.coord_loss.clone()
    st, graph = _train(3, data, after=checked, coord_loss_weight=0.01)
    _, eager = _train(3, data, after=lambda st, k: st.coord_loss.clone(), coord_loss_weight=0.01, use_graph=False)
    for k, ((la, wa, ca), (lb, wb, cb)) in enumerate(zip(graph, eager)):
        print(f"step {k}: loss {float(la):.8f} / {float(lb):.8f}, coordinate loss {float(ca):.6f} / {float(cb):.6f}, "
              f"parameters differ in {int((wa != wb).sum())} places")
    for (la, wa, ca), (lb, wb, cb) in zip(graph, eager):
        assert np.array_equal(_bits(la), _bits(lb)) and np.array_equal(_bits(ca), _bits(cb)) and torch.equal(wa, wb)
    assert tuple(st.soft_preds.shape) == (4, 21, 2) and st.coord_loss.dim() == 0
    _, plain = _train(1, data)
    assert float(graph[0][0]) > float(plain[0][0])                       # the coordinate term is in the loss


def test_invisible_joint_keeps_the_gradient_of_the_run_without_the_term(monkeypatch):
    """7a. use_target_weight with joints marked invisible: those planes of dout are bit-equal to the run without the coordinate
    term (zero from the weighted MSE, untouched by lh_integral_l1).  A visible plane differs wherever its coordinate gradient is
    large enough to survive the fp32 addition to the MSE gradient: an untrained R18's maps span +-1.8, so at beta = 100 the softmax
    of a plane whose two largest cells lie 0.3 apart is one-hot to 1e-13, its coordinate gradient vanishes (e_p is ~0 off the
    peak, x_p - ex is ~0 on it) and fp32(mse + g) keeps the bits of mse.  The planes that must differ are therefore chosen from
    the float64 restatement: some cell with |g| > 2^-20 |mse|, 16 times the largest half-ulp an fp32 sum can absorb."""
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    x, j = _batch(4, 64, 44)
    vis = torch.ones(4, 21, 1, device="cuda")
    vis[0, 3], vis[2, 20], vis[3, 0] = 0, 0, 0
    data = [(x, torch.cat([j, vis], -1))]
    grab = lambda st, k: st.plan.dout_nchw.clone()
    st, with_term = _train(1, data, after=grab, use_target_weight=True, coord_loss_weight=0.01)
    _, without = _train(1, data, after=grab, use_target_weight=True)
    a, b, off = with_term[0][2], without[0][2], vis[..., 0] == 0
    assert torch.equal(a[off].view(torch.int32), b[off].view(torch.int32)) and not a[off].any()
    weight = vis[..., 0].cpu().numpy()
    wgrad = restate(st.plan.out_nchw.cpu().numpy(), j.cpu().numpy(), weight, 100.0, SCALE, 0.01)[3]
    clear = (np.abs(wgrad) > 2.0 ** -20 * np.abs(b.cpu().numpy())).reshape(4, 21, -1).any(2)
    print(f"{int(clear.sum())} of {int((weight > 0).sum())} visible planes carry a coordinate gradient above the MSE gradient's rounding")
    assert clear.any() and not clear[weight == 0].any()
    assert all(not torch.equal(a[n, k], b[n, k]) for n, k in zip(*np.nonzero(clear)))
    assert not st.coord_joint_loss[off].any() and bool((st.coord_joint_loss[~off] > 0).all())
    _check_step_against_restatement(st, 0.01, 100.0, j.cpu().numpy(), vis[..., 0].cpu().numpy(), mse=(F32(without[0][0].item()), b.cpu().numpy()))


def test_residual_is_taken_against_the_warped_joints(monkeypatch):
    """7b. geometric_aug: coord_joint_loss is |soft_preds - joints_aug| summed over the axes, not the distance to the caller's joints."""
    from lighthand_amd.runtime import TrainStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    geo = {"rotation": 30.0, "scale": 0.3, "shift": 0.2, "generator": torch.Generator().manual_seed(21)}
    st = TrainStep(_model("bf16"), 4, 64, 64, lr=1e-3, input_u8=(48, 56), geometric_aug=geo, coord_loss_weight=0.01)
    rng = np.random.RandomState(100)
    x = torch.from_numpy(rng.randint(0, 256, size=(4, 48, 56, 3)).astype(np.uint8)).cuda()
    j = torch.from_numpy(rng.uniform(8, 56, size=(4, 21, 2)).astype(F32)).cuda()
    st(x, j)
    torch.cuda.synchronize()
    assert not torch.equal(st.joints_aug, st.joints)
    want = (st.soft_preds - st.joints_aug).abs().sum(2)
    other = (st.soft_preds - st.joints).abs().sum(2)
    assert np.array_equal(_bits(st.coord_joint_loss), _bits(want)) and not torch.equal(want, other)
    assert abs(float(st.coord_loss) - 0.01 * float(want.double().mean()) / 2) <= 1e-6 * float(st.coord_loss)


def test_fp16_dynamic_loss_scale_scales_the_coordinate_gradient(monkeypatch):
    """7c. R18 fp16, loss_scale="dynamic" from 2**40: the overflowing first steps are skipped and halve the scale; every replay's
    plan.dout_nchw is the MSE gradient plus the restated coordinate gradient AT THE SCALE THAT REPLAY READ from the device -- the
    captured graph is never re-captured."""
    from lighthand_amd.amp import DynamicLossScale
    from lighthand_amd.runtime import TrainStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    x, j = _batch(4, 64, 70)
    m = _model("fp16")
    st = TrainStep(m, 4, 64, 64, lr=1e-3, loss_scale=DynamicLossScale(init_scale=2.0 ** 40), coord_loss_weight=0.01)
    prev, found, graphs = m.arena().flat.clone(), [], None
    for _ in range(60):
        scale_read = st.scaler.scale
        st(x, j)
        torch.cuda.synchronize()
        graphs = graphs or st.graphs
        assert st.graphs is graphs
        f = int(st.scaler.found_inf)
        found.append(f)
        if f:
            assert torch.equal(m.arena().flat, prev) and st.scaler.scale == scale_read * 0.5
        elif found.count(0) in (1, 3):
            _check_step_against_restatement(st, 0.01, 100.0, j.cpu().numpy(), None, gs=scale_read)
        prev = m.arena().flat.clone()
        if found.count(0) == 3:
            break
    assert found[0] == 1 and found.count(0) == 3 and torch.isfinite(m.arena().flat).all()


def test_training_lowers_the_coordinate_loss(monkeypatch):
    """8. 30 steps on one fixed batch with coord_loss_weight = 0.05: the coordinate loss of step 30 is below that of step 1 (a sanity
    check, no accuracy threshold)."""
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    from lighthand_amd.runtime import TrainStep
    x, j = _batch(4, 64, 80)
    st = TrainStep(_model(), 4, 64, 64, lr=1e-3, coord_loss_weight=0.05)
    st(x, j)
    first = float(st.coord_loss)
    for _ in range(29):
        st(x, j)
    last = float(st.coord_loss)
    print(f"coordinate loss: step 1 {first:.5f}, step 30 {last:.5f}")
    assert np.isfinite(first) and np.isfinite(last) and 0 < last < first


def test_soft_decode_of_the_inference_steps(monkeypatch):
    """9. InferStep(post_process="soft"): preds is soft_argmax_device on step.heatmaps bit for bit, captured and eager, with and
    without the flip test (then on the merged maps); maxvals stays the arg-max's; max_preds_device("soft") gives the same."""
    from lighthand_amd.heatmap import get_max_preds, max_preds_device, soft_argmax_device
    from lighthand_amd.runtime import InferPipeline, InferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model(seed=5).eval()
    x = torch.from_numpy(np.random.RandomState(5).randn(2, 3, 64, 64).astype(F32)).cuda()
    for flip in (False, True):
        for graph in (True, False):
            st = InferStep(model, 2, 64, 64, post_process="soft", soft_argmax_beta=40.0, flip_test=flip, use_graph=graph)
            st(x)
            torch.cuda.synchronize()
            want = soft_argmax_device(st.heatmaps, beta=40.0, scale=4.0)
            hard, mv, idx = max_preds_device(st.heatmaps, scale=4.0)
            p, m2, i2 = max_preds_device(st.heatmaps, scale=4.0, post_process="soft", soft_argmax_beta=40.0)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(st.preds), _bits(want)) and np.array_equal(_bits(p), _bits(want)), (flip, graph)
            assert np.array_equal(_bits(st.maxvals), _bits(mv)) and torch.equal(m2, mv) and torch.equal(i2, idx)
            assert not torch.equal(want, hard)
        if flip:
            plain = InferStep(model, 2, 64, 64)
            plain(x)
            torch.cuda.synchronize()
            assert not torch.equal(plain.heatmaps, st.heatmaps)          # the decode read the merged maps
    gp, gm = get_max_preds(st.heatmaps, post_process="soft", soft_argmax_beta=40.0)
    # get_max_preds keeps the reference's signature: heat-map cells, no scale
    assert np.array_equal(_bits(gp), _bits(soft_argmax_device(st.heatmaps, beta=40.0, scale=1.0)))
    assert torch.equal(gm, max_preds_device(st.heatmaps)[1])
    pipe = InferPipeline(model, 2, 64, 64, depth=1, post_process="soft", soft_argmax_beta=40.0)
    pp, _ = pipe.result(pipe.submit(x))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(pp), _bits(soft_argmax_device(pipe.steps[0].heatmaps, beta=40.0, scale=4.0)))


def test_eval_cli_with_soft_decode(tmp_path, capsys):
    """10. wearable_eval_2d --synthetic 8 --soft_decode runs to its metrics line."""
    from lighthand_amd.tools import wearable_eval_2d as E
    from lighthand_amd.tools.train import build_model
    args = E.build_parser().parse_args(["--depth", "18"])
    args.model = "simplebaseline"
    torch.manual_seed(12)
    run = tmp_path / "simplebaseline" / "frei" / "run1" / "checkpoint-good"
    run.mkdir(parents=True)
    torch.save({"model_state_dict": build_model(args).state_dict()}, str(run / "state_dict.bin"))
    files = E.main(["--root_path", str(tmp_path), "--model_path", "simplebaseline/frei", "--batch_size", "4", "--depth", "18",
                    "--size", "64", "--synthetic", "8", "--soft_decode"])
    assert len(files) == 3 and all(os.path.isfile(f) for f in files)
    assert "Writting ===>" in capsys.readouterr().out
    assert all(line.count(";") > 4 for f in files for line in open(f))
