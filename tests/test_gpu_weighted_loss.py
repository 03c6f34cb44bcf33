"""GPU: the visibility-weighted heat-map loss and online hard-keypoint mining (lh_gaussian_target_w, lh_joints_mse,
heatmap.WeightedJointsMSELoss, TrainStep(use_target_weight=, ohkm_topk=)).

Neither piece has a reference oracle (the reference computes target_weight and never applies it, and has no mining): the formulas
are those of the SimpleBaseline / HRNet code line, restated here in NumPy / torch on the CPU.  No tolerance below is measured:
gradients and targets are compared bit for bit with an fp32 restatement that forms every product in the kernel's order; the loss
values are fp64 sums rounded once to fp32 on both sides, so 1e-6 relative is ~16 fp32 half-ulps of head-room over the 2^-24 of
that rounding plus the fp64 summation-order difference (~1e-13)."""
import numpy as np
import pytest
import torch

from conftest import resnet_cfg
from oracle import heatmap as oh

pytestmark = pytest.mark.gpu

F32 = np.float32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def _in_frame(joints, size):
    """oracle.heatmap.generate_target's skip condition (src/tools/dataset.py:171-186), negated: [..., >=2] -> bool [...]."""
    j = np.asarray(joints)
    out = np.zeros(j.shape[:-1], bool)
    for idx in np.ndindex(*out.shape):
        mx, my = oh._trunc_center(j[idx][0]), oh._trunc_center(j[idx][1])
        x0, y0, x1, y1 = mx - oh.RADIUS, my - oh.RADIUS, mx + oh.RADIUS + 1, my + oh.RADIUS + 1
        out[idx] = not (x0 >= size or y0 >= size or x1 < 0 or y1 < 0)
    return out


def _weight_restated(joints, vis, size):
    v = np.ones(joints.shape[:-1], F32) if vis is None else np.asarray(vis, F32)
    return np.where(v > 0.5, v, F32(0)) * _in_frame(joints, size).astype(F32)


def _edge_joints(b, nj, seed, frame=256.0, margin=40.0):
    """Coordinates inside the frame, up to 10 heat-map pixels outside each of its four edges (both sides of the skip decision,
    which falls 6 to 8 heat-map pixels outside: the patch radius is 6), and far outside."""
    rng = np.random.RandomState(seed)
    j = rng.uniform(0, frame, size=(b, nj, 2)).astype(F32)
    kind = rng.randint(0, 6, size=(b, nj))
    j[..., 0] = np.where(kind == 1, rng.uniform(-margin, 0, size=(b, nj)), j[..., 0])
    j[..., 0] = np.where(kind == 2, rng.uniform(frame, frame + margin, size=(b, nj)), j[..., 0])
    j[..., 1] = np.where(kind == 3, rng.uniform(-margin, 0, size=(b, nj)), j[..., 1])
    j[..., 1] = np.where(kind == 4, rng.uniform(frame, frame + margin, size=(b, nj)), j[..., 1])
    far = rng.choice([-1000.0, 1000.0, 5e4], size=(b, nj, 2)).astype(F32)
    j = np.where((kind == 5)[..., None], far, j).astype(F32)
    return j, kind


def test_weighted_render_matches_the_restatement_bit_for_bit():
    """1. 64 x 21 joints inside the frame, just outside each edge and far outside, random 0/1 visibility: the weight is the
    restatement exactly; the target is oracle.heatmap.generate_target bit for bit where the weight is 1 and exactly zero elsewhere;
    without a visibility column the target is today's render_targets bit for bit."""
    from lighthand_amd.heatmap import generate_target, render_targets
    j, kind = _edge_joints(64, 21, 3)
    vis = (np.random.RandomState(4).uniform(size=(64, 21)) < 0.7).astype(F32)
    want_w = _weight_restated(j, vis, 64)
    frame = _in_frame(j, 64)
    assert set(np.unique(kind)) == set(range(6))
    for k in range(1, 5):                                       # every edge shows both outcomes of the skip test
        assert frame[kind == k].any() and not frame[kind == k].all(), k
    assert not frame[kind == 5].any() and frame[kind == 0].all()
    assert (want_w == 0).any() and (want_w == 1).any() and ((vis == 0) & frame).any() and ((vis == 1) & ~frame).any()

    j3 = torch.from_numpy(np.concatenate([j, vis[..., None]], -1)).cuda()
    target, weight = render_targets(j3, return_weight=True)
    assert tuple(weight.shape) == (64, 21, 1) and tuple(target.shape) == (64, 21, 64, 64)
    got_w, got_t = weight.cpu().numpy()[..., 0], target.cpu().numpy()
    assert np.array_equal(_bits(got_w), _bits(want_w))
    want_t = np.stack([oh.generate_target(s) for s in j]) * (want_w == 1)[..., None, None].astype(F32)
    assert np.array_equal(_bits(got_t), _bits(want_t))
    assert not got_t[want_w == 0].any()

    plain = render_targets(torch.from_numpy(j).cuda())
    t2, w2 = render_targets(torch.from_numpy(j).cuda(), return_weight=True)
    assert torch.equal(t2.view(torch.int32), plain.view(torch.int32))
    assert np.array_equal(w2.cpu().numpy()[..., 0], frame.astype(F32))
    # a fractional visibility above 0.5 is kept as the weight (upstream multiplies by it), and the plane is rendered
    jf = j3[:1].clone()
    jf[0, :, :2] = 100.0
    v = np.linspace(0.0, 1.0, 21).astype(F32)
    jf[0, :, 2] = torch.from_numpy(v).cuda()
    tf, wf = render_targets(jf, return_weight=True)
    assert np.array_equal(wf.cpu().numpy()[0, :, 0], np.where(v > 0.5, v, 0).astype(F32))
    assert np.array_equal(tf.cpu().numpy()[0].reshape(21, -1).any(1), v > 0.5)
    # the per-sample form with the reference's signature
    tg, wg = generate_target(np.concatenate([j[5], vis[5][:, None]], -1), return_weight=True)
    assert np.array_equal(_bits(tg.numpy()), _bits(want_t[5])) and np.array_equal(wg.numpy()[:, 0], want_w[5])


def _jmse(p, g, w, topk, scale=None, with_grad=True):
    """lh_joints_mse on device tensors -> (loss, joint_loss [b][j], grad) as NumPy."""
    from lighthand_amd import _lib
    lib = _lib.load()
    b, j = p.shape[:2]
    hw = p[0, 0].numel()
    loss = torch.full((), float("nan"), device="cuda")
    jl = torch.full((b, j), float("nan"), device="cuda")
    grad = torch.full_like(p, float("nan")) if with_grad else None
    ws = torch.empty(lib.lh_joints_mse_workspace_bytes(b, j), dtype=torch.uint8, device="cuda")
    gs = None if scale is None else torch.tensor([scale], dtype=torch.float32, device="cuda")
    _lib.check(lib.lh_joints_mse(p.data_ptr(), g.data_ptr(), None if w is None else w.data_ptr(), b, j, hw, topk, loss.data_ptr(),
                                 jl.data_ptr(), None if grad is None else grad.data_ptr(), None if gs is None else gs.data_ptr(),
                                 ws.data_ptr(), _stream()), "lh_joints_mse")
    torch.cuda.synchronize()
    return F32(loss.item()), jl.cpu().numpy(), None if grad is None else grad.cpu().numpy()


def _restate(p, g, w, topk, scale=None):
    """The issue's formulas on the CPU from the same fp32 inputs: d = p - g in fp32, S = w^2 * sum (float)(d * d) in fp64,
    joint_loss = 0.5 * S / hw; the gradient coefficient (w * w) * (scale / (float)n) formed in fp32.
    Returns (loss f64, joint_loss f64 [b][j], grad f32, selected bool [b][j])."""
    p, g = np.asarray(p, F32), np.asarray(g, F32)
    b, j = p.shape[:2]
    d = (p - g).astype(F32).reshape(b, j, -1)
    hw = d.shape[2]
    w = np.ones((b, j), F32) if w is None else np.asarray(w, F32).reshape(b, j)
    S = w.astype(np.float64) ** 2 * (d * d).astype(F32).astype(np.float64).sum(2)
    jl = 0.5 * S / hw
    s = F32(1.0 if scale is None else scale)
    if topk == 0:
        coef = (w * w) * (s / F32(b * j * hw))
        return 0.5 * S.sum() / (b * j * hw), jl, (d * coef[..., None]).astype(F32).reshape(p.shape), np.ones((b, j), bool)
    # the topk largest per sample, the lower joint index among equals: a stable sort of the negated losses
    order = np.argsort(-jl, axis=1, kind="stable")[:, :topk]
    sel = np.zeros((b, j), bool)
    np.put_along_axis(sel, order, True, axis=1)
    coef = (w * w) * (s / F32(b * topk * hw))
    grad = np.where(sel[..., None], (d * coef[..., None]).astype(F32), F32(0)).reshape(p.shape)
    return (jl * sel).sum(1).mean() / topk, jl, grad, sel


def _selection_is_stable(jl, topk):
    """The condition on the input that keeps rounding out of the selection: per sample the topk-th and (topk+1)-th largest loss of
    the CPU statement differ by more than 1e-5 relative, or both are exactly zero (weight 0: exact in the kernel too, and the
    lower-joint-index rule decides).  Returns (ok [b], exact-zero tie [b])."""
    srt = -np.sort(-jl, axis=1)
    gap = (srt[:, topk - 1] - srt[:, topk]) > 1e-5 * srt[:, topk - 1]
    tie0 = (srt[:, topk - 1] == 0) & (srt[:, topk] == 0)
    return gap | tie0, tie0


def _close(got, want, rel=1e-6):
    return np.all(np.abs(np.asarray(got, np.float64) - want) <= rel * np.abs(want))


def _maps(b, j, h, seed):
    rng = np.random.RandomState(seed)
    p = torch.from_numpy(rng.randn(b, j, h, h).astype(F32) * 0.3).cuda()
    g = torch.from_numpy((rng.uniform(0, 1, size=(b, j, h, h)) ** 8).astype(F32)).cuda()
    return p, g


@pytest.mark.parametrize("scale", [None, 1024.0])
@pytest.mark.parametrize("shape", [(16, 21, 64), (5, 7, 6)])
def test_weighted_mse_matches_the_restatement(shape, scale):
    """2. topk = 0: grad bit-equal to (p - g) * float32(w * w * gs) with grad_scale absent and 1024; joint_loss and loss within 1e-6
    relative of the float64 statement.  64 x 64 planes and a 6 x 6 one (fewer vectors than threads), weights 0, 1 and fractions."""
    b, j, h = shape
    p, g = _maps(b, j, h, 11)
    w = torch.from_numpy(np.random.RandomState(12).choice([0.0, 1.0, 1.0, 0.7, 0.9], size=(b, j, 1)).astype(F32)).cuda()
    loss, jl, grad = _jmse(p, g, w, 0, scale)
    want_loss, want_jl, want_grad, _ = _restate(p.cpu().numpy(), g.cpu().numpy(), w.cpu().numpy(), 0, scale)
    assert np.array_equal(_bits(grad), _bits(want_grad))
    assert _close(jl, want_jl) and _close(loss, want_loss)
    assert (jl[w.cpu().numpy()[..., 0] == 0] == 0).all() and want_loss > 0
    # the loss alone (no gradient buffer) is the same value
    loss2, jl2, _ = _jmse(p, g, w, 0, scale, with_grad=False)
    assert loss2 == loss and np.array_equal(jl2, jl)


def test_unit_weights_reproduce_the_plain_loss():
    """2. weight = None: grad is lh_mse_heatmap's bit for bit, the loss agrees within one fp32 ulp (another fp64 summation order)."""
    from lighthand_amd import _lib
    lib = _lib.load()
    p, g = _maps(16, 21, 64, 13)
    for scale in (None, 1024.0):
        loss, _, grad = _jmse(p, g, None, 0, scale)
        ref_loss = torch.zeros((), device="cuda")
        ref_grad = torch.full_like(p, float("nan"))
        ws = torch.empty(lib.lh_mse_workspace_bytes(p.numel()), dtype=torch.uint8, device="cuda")
        gs = None if scale is None else torch.tensor([scale], dtype=torch.float32, device="cuda")
        _lib.check(lib.lh_mse_heatmap(p.data_ptr(), g.data_ptr(), p.numel(), ref_loss.data_ptr(), ref_grad.data_ptr(),
                                      None if gs is None else gs.data_ptr(), ws.data_ptr(), _stream()), "lh_mse_heatmap")
        torch.cuda.synchronize()
        assert np.array_equal(_bits(grad), _bits(ref_grad.cpu().numpy()))
        ref = F32(ref_loss.item())
        assert abs(np.float64(loss) - np.float64(ref)) <= np.spacing(ref)
        ones = torch.ones(16, 21, device="cuda")
        loss1, _, grad1 = _jmse(p, g, ones, 0, scale)
        assert loss1 == loss and np.array_equal(_bits(grad1), _bits(grad))


@pytest.mark.parametrize("scale", [None, 1024.0])
@pytest.mark.parametrize("numel", [3, 7, 1029])
def test_plain_loss_tail_and_tiny_sizes_exact(numel, scale):
    """lh_mse_heatmap where numel is no multiple of 4: 3 = the scalar tail alone, 7 = one 16-byte vector and the tail, 1029 = two
    workgroups of vectors and a tail of one that workgroup 0 adds.  pred and target are multiples of 2^-6 in [-4, 4], so d is a
    multiple of 2^-6 below 2^3, (float)(d * d) a multiple of 2^-12 below 2^6 (18 significant bits) and every fp64 partial sum exact in
    any order: the loss is float32(0.5 * sum / numel) formed in float64 as the kernel forms it, the gradient d * (float32(gs) /
    float32(numel)) in float32, both compared bit for bit, with a gradient buffer and without; the gradient buffer's four elements past
    numel stay as they were."""
    from lighthand_amd import _lib
    lib = _lib.load()
    rng = np.random.RandomState(500 + numel)
    p = (rng.randint(-256, 257, size=numel) / 64.0).astype(F32)
    g = (rng.randint(-256, 257, size=numel) / 64.0).astype(F32)
    d = (p - g).astype(F32)
    assert np.array_equal(d.astype(np.float64), p.astype(np.float64) - g.astype(np.float64)) and d.any()
    total = (d * d).astype(F32).astype(np.float64).sum()
    assert total == (d.astype(np.float64) ** 2).sum() and total * 4096 == np.floor(total * 4096)
    want_loss = F32(0.5 * total / np.float64(numel))
    want_grad = (d * (F32(1.0 if scale is None else scale) / F32(numel))).astype(F32)
    pt, gt = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
    ws = torch.empty(lib.lh_mse_workspace_bytes(numel), dtype=torch.uint8, device="cuda")
    gs = None if scale is None else torch.tensor([scale], dtype=torch.float32, device="cuda")
    for with_grad in (True, False):
        loss = torch.full((), float("nan"), device="cuda")
        grad = torch.full((numel + 4,), float("nan"), device="cuda") if with_grad else None
        _lib.check(lib.lh_mse_heatmap(pt.data_ptr(), gt.data_ptr(), numel, loss.data_ptr(), None if grad is None else grad.data_ptr(),
                                      None if gs is None else gs.data_ptr(), ws.data_ptr(), _stream()), "lh_mse_heatmap")
        torch.cuda.synchronize()
        assert np.array_equal(_bits(loss.cpu().numpy()), _bits(want_loss)), (numel, scale, with_grad)
        if with_grad:
            got = grad.cpu().numpy()
            assert np.array_equal(_bits(got[:numel]), _bits(want_grad))
            assert np.isnan(got[numel:]).all()


def _ohkm_case():
    """b = 32, j = 21, 32 x 32 planes; samples 0..3 have 0, 3, 5 and 7 weighted joints (fewer than topk = 8)."""
    b, j, h = 32, 21, 32
    p, g = _maps(b, j, h, 21)
    rng = np.random.RandomState(22)
    w = (rng.uniform(size=(b, j)) < 0.8).astype(F32)
    for s, n in enumerate((0, 3, 5, 7)):
        w[s] = 0
        w[s, rng.permutation(j)[:n]] = 1
    return p, g, torch.from_numpy(w).cuda()


@pytest.mark.parametrize("scale", [None, 1024.0])
def test_ohkm_selects_the_hardest_joints(scale):
    """3. topk = 8 of 21.  Condition on the input, asserted first: in the CPU statement the 8th and 9th largest per-joint losses
    of a sample differ by more than 1e-5 relative, so rounding cannot flip a selection; in the samples with fewer than 8 weighted
    joints both are EXACTLY zero in the statement and in the kernel alike (w = 0 gives S = 0 without rounding) and the
    lower-joint-index rule decides, which the stable sort of the restatement applies and the signed zeros of the gradient show
    (d * 0 = +-0 on a selected plane of weight 0, +0 on every plane that was not selected).  Where no tie exists the selected set
    is also torch.topk's."""
    topk = 8
    p, g, w = _ohkm_case()
    pn, gn, wn = p.cpu().numpy(), g.cpu().numpy(), w.cpu().numpy()
    want_loss, want_jl, want_grad, sel = _restate(pn, gn, wn, topk, scale)
    ok, tie0 = _selection_is_stable(want_jl, topk)
    gap = ok & ~tie0
    assert ok.all() and tie0.sum() >= 4 and gap.sum() >= 24
    assert ((wn > 0).sum(1) < topk).sum() >= 4
    tk = torch.topk(torch.from_numpy(want_jl), topk, dim=1).indices.numpy()
    for s in np.flatnonzero(gap):
        assert set(tk[s]) == set(np.flatnonzero(sel[s]))
    assert (sel.sum(1) == topk).all()

    loss, jl, grad = _jmse(p, g, w, topk, scale)
    assert _close(jl, want_jl)
    got_sel = grad.reshape(32, 21, -1).any(2)                    # a selected plane of positive weight has a non-zero gradient
    assert np.array_equal(got_sel, sel & (wn > 0))
    assert np.array_equal(_bits(grad), _bits(want_grad))
    assert not _bits(grad).reshape(32, 21, -1)[~sel].any()       # exactly +0.f where not selected
    assert _close(loss, want_loss) and want_loss > 0
    loss2, _, _ = _jmse(p, g, w, topk, scale, with_grad=False)
    assert loss2 == loss
    # topk = j selects everything: the weighted sum of all per-joint losses, normalised by b * j * hw like topk = 0
    loss_all, _, grad_all = _jmse(p, g, w, 21, scale)
    loss_0, _, grad_0 = _jmse(p, g, w, 0, scale)
    assert _close(loss_all, np.float64(loss_0)) and np.array_equal(_bits(grad_all), _bits(grad_0))


def test_loss_module_delivers_the_gradient_through_autograd():
    """3. WeightedJointsMSELoss(topk).backward() hands the kernel's gradient to the prediction; .joint_loss holds the per-joint
    losses; weights of shape [B, J, 1] (what render_targets returns), [B, J] and None are taken."""
    from lighthand_amd.heatmap import WeightedJointsMSELoss
    p, g, w = _ohkm_case()
    for topk in (0, 8):
        for weight in (w[..., None], w, None):
            crit = WeightedJointsMSELoss(topk=topk)
            x = p.clone().requires_grad_(True)
            loss = crit(x, g, weight)
            loss.backward()
            ref_loss, ref_jl, ref_grad = _jmse(p, g, weight if weight is None else weight.reshape(32, 21).contiguous(), topk)
            assert F32(loss.item()) == ref_loss
            assert np.array_equal(_bits(x.grad.cpu().numpy()), _bits(ref_grad))
            assert tuple(crit.joint_loss.shape) == (32, 21) and np.array_equal(crit.joint_loss.cpu().numpy(), ref_jl)
            assert not crit.joint_loss.requires_grad
    with pytest.raises(ValueError):
        WeightedJointsMSELoss()(p, g, w[:, :5])


@pytest.mark.parametrize("topk", [0, 8])
def test_two_calls_give_the_same_bits(topk):
    """4. No atomics, fixed reduction order: loss, joint_loss and grad of two calls on the same inputs are bit-identical."""
    p, g, w = _ohkm_case()
    a = _jmse(p, g, w, topk, 1024.0)
    junk = torch.randn(1 << 22, device="cuda")                   # other work in between
    junk.mul_(2.0)
    b = _jmse(p, g, w, topk, 1024.0)
    assert a[0] == b[0] and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(_bits(a[2]), _bits(b[2]))


# ------------------------------------------------------------------------------------------------ step level
def _model(precision="fp32", seed=9001):
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    torch.manual_seed(seed)
    return get_pose_net(resnet_cfg(18), True).cuda().set_precision(precision)


def _batch(b, size, seed):
    rng = np.random.RandomState(seed)
    return (torch.from_numpy(rng.randn(b, 3, size, size).astype(F32)).cuda(),
            torch.from_numpy(rng.uniform(8, size - 8, size=(b, 21, 2)).astype(F32)).cuda())


def _train(steps, data, **kw):
    from lighthand_amd.runtime import TrainStep
    m = _model()
    st = TrainStep(m, 4, 64, 64, lr=1e-3, **kw)
    losses = []
    for x, j in data[:steps]:
        losses.append(float(st(x, j)))
    torch.cuda.synchronize()
    return st, losses, m.arena().flat.clone()


def test_step_with_every_joint_visible_equals_the_plain_step(monkeypatch):
    """5. R18 fp32 64^2 batch 4, 3 steps: with every joint visible and inside the frame TrainStep(use_target_weight=True) leaves the
    parameters bit-identical to the plain step (the gradient is bit-equal; the loss VALUE agrees within one fp32 ulp); an explicit
    visibility column of ones changes nothing; the captured and the eager form agree like the plain step's do
    (tests/test_gpu_runtime.py::test_graph_step_equals_eager_step_and_dropin_loop)."""
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    data = [_batch(4, 64, 30 + k) for k in range(3)]
    _, l_plain, w_plain = _train(3, data)
    st, l_w, w_w = _train(3, data, use_target_weight=True)
    assert torch.equal(w_plain, w_w)
    assert all(abs(a - b) <= np.spacing(F32(a)) for a, b in zip(l_plain, l_w)) and all(np.isfinite(l_w))
    assert float(st.target_weight.min()) == 1.0 and tuple(st.target_weight.shape) == (4, 21, 1) and tuple(st.joint_loss.shape) == (4, 21)
    assert abs(float(st.joint_loss.double().mean()) - l_w[-1]) <= 1e-6 * l_w[-1]
    data3 = [(x, torch.cat([j, torch.ones_like(j[..., :1])], -1)) for x, j in data]
    _, l_w3, w_w3 = _train(3, data3, use_target_weight=True)
    assert l_w3 == l_w and torch.equal(w_w3, w_w)
    _, l_e, w_e = _train(3, data, use_target_weight=True, use_graph=False)
    assert np.allclose(l_w, l_e, rtol=1e-6) and torch.allclose(w_w, w_e, rtol=1e-5, atol=1e-7)
    # the plain step owns none of the new buffers
    plain = _train(1, data)[0]
    assert plain.vis is None and plain.target_weight is None and plain.joint_loss is None


def test_invisible_joints_do_not_reach_the_parameters(monkeypatch):
    """6. Two weighted runs from the same state whose invisible joints carry different garbage coordinates, all else equal:
    parameters and losses are bit-identical after 3 steps.  The same batches through the plain step differ."""
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    rng = np.random.RandomState(40)
    vis = torch.from_numpy((rng.uniform(size=(3, 4, 21, 1)) < 0.7).astype(F32)).cuda()
    base = [_batch(4, 64, 41 + k) for k in range(3)]
    runs = []
    for seed in (50, 51):
        garbage = torch.from_numpy(np.random.RandomState(seed).uniform(-40, 104, size=(3, 4, 21, 2)).astype(F32)).cuda()
        runs.append([(x, torch.cat([torch.where(vis[k] > 0.5, j, garbage[k]), vis[k]], -1)) for k, (x, j) in enumerate(base)])
    assert not torch.equal(runs[0][0][1], runs[1][0][1]) and float(vis.min()) == 0.0
    (sa, la, wa), (sb, lb, wb) = (_train(3, d, use_target_weight=True) for d in runs)
    assert la == lb and torch.equal(wa, wb) and all(np.isfinite(la))
    assert torch.equal(sa.target_weight, vis[2]) and torch.equal(sa.vis, vis[2][..., 0])
    assert not sa.target[(vis[2][..., 0] == 0)].any()
    (_, pa, va), (_, pb, vb) = (_train(3, [(x, j[..., :2]) for x, j in d]) for d in runs)
    assert pa != pb and not torch.equal(va, vb)
    assert not torch.equal(va, wa)


def test_weight_follows_the_warped_joints(monkeypatch):
    """7. geometric_aug with a fixed generator: after every replay step.target_weight is 0 exactly for the joints whose WARPED patch
    (step.joints_aug) left the map and 1 otherwise, and those planes of the target are zero."""
    from lighthand_amd.runtime import TrainStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    m = _model("bf16")
    geo = {"rotation": 45.0, "scale": 0.4, "shift": 0.4, "generator": torch.Generator().manual_seed(21)}
    st = TrainStep(m, 4, 64, 64, lr=1e-3, input_u8=(48, 56), geometric_aug=geo, use_target_weight=True)
    zeros = ones = 0
    for k in range(3):
        rng = np.random.RandomState(100 + k)
        x = torch.from_numpy(rng.randint(0, 256, size=(4, 48, 56, 3)).astype(np.uint8)).cuda()
        j = torch.from_numpy(rng.uniform(-20, 84, size=(4, 21, 2)).astype(F32)).cuda()
        assert _in_frame(j.cpu().numpy(), 16).all()               # every joint's patch is inside before the warp
        st(x, j)
        torch.cuda.synchronize()
        want = _in_frame(st.joints_aug.cpu().numpy(), 16).astype(F32)
        got = st.target_weight.cpu().numpy()[..., 0]
        assert np.array_equal(got, want)
        assert not st.target.cpu().numpy()[want == 0].any()
        zeros, ones = zeros + int((want == 0).sum()), ones + int((want == 1).sum())
        assert np.isfinite(float(st.loss))
    assert zeros > 0 and ones > 0


@pytest.mark.parametrize("weighted", [False, True])
def test_captured_ohkm_step_matches_the_restatement(weighted, monkeypatch):
    """8. ohkm_topk = 8 (alone, and with use_target_weight and a visibility column): the captured step's loss and plan.dout_nchw
    against the restatement evaluated on the step's own plan.out_nchw, target and target_weight -- gradient bit-equal, loss 1e-6."""
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    data = [_batch(4, 64, 60 + k) for k in range(3)]
    if weighted:
        vis = torch.from_numpy((np.random.RandomState(61).uniform(size=(4, 21, 1)) < 0.6).astype(F32)).cuda()
        vis[0, 3:] = 0                                            # a sample with 3 weighted joints, fewer than topk
        data = [(x, torch.cat([j, vis], -1)) for x, j in data]
    st, losses, _ = _train(3, data, ohkm_topk=8, use_target_weight=weighted)
    out, tgt = st.plan.out_nchw.cpu().numpy(), st.target.cpu().numpy()
    w = st.target_weight.cpu().numpy()[..., 0] if weighted else None
    want_loss, want_jl, want_grad, sel = _restate(out, tgt, w, 8)
    assert _selection_is_stable(want_jl, 8)[0].all()
    assert np.array_equal(_bits(st.plan.dout_nchw.cpu().numpy()), _bits(want_grad))
    assert _close(float(st.loss), want_loss) and _close(st.joint_loss.cpu().numpy(), want_jl)
    assert (sel.sum(1) == 8).all() and not st.plan.dout_nchw.cpu().numpy()[~sel].any()
    if weighted:
        assert np.array_equal(w, vis.cpu().numpy()[..., 0])
    else:
        assert float(st.target_weight.min()) == 1.0
    # mining changes the objective: the plain step on the same batches ends elsewhere
    assert losses != _train(3, [(x, j[..., :2]) for x, j in data])[1]


def test_option_combinations_refused_at_construction(monkeypatch):
    from lighthand_amd._lib import LightHandError
    from lighthand_amd.runtime import TrainStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    m = _model()
    with pytest.raises(LightHandError, match="targets_from_joints"):
        TrainStep(m, 4, 64, 64, targets_from_joints=False, use_target_weight=True)
    with pytest.raises(LightHandError, match="ohkm_topk"):
        TrainStep(m, 4, 64, 64, ohkm_topk=22)
    TrainStep(m, 4, 64, 64, ohkm_topk=21)                        # allowed, and without use_target_weight (weights of 1)
    # mining on targets the caller hands in: weights of 1
    st = TrainStep(m, 4, 64, 64, targets_from_joints=False, ohkm_topk=8)
    x, _ = _batch(4, 64, 1)
    t = _maps(4, 21, 16, 2)[1]
    st(x, target=t)
    torch.cuda.synchronize()
    want_loss, _, want_grad, _ = _restate(st.plan.out_nchw.cpu().numpy(), t.cpu().numpy(), None, 8)
    assert _close(float(st.loss), want_loss) and np.array_equal(_bits(st.plan.dout_nchw.cpu().numpy()), _bits(want_grad))


def test_fp16_dynamic_loss_scale_with_the_weighted_ohkm_loss(monkeypatch):
    """9. R18 fp16, loss_scale="dynamic" from 2**40, use_target_weight + ohkm_topk = 8: the steps whose gradients overflow report
    found_inf, leave the parameters bit-unchanged and halve the scale, as tests/test_gpu_amp.py::test_fp16_overflow_recovery expects
    of the plain loss; every replay's loss gradient (plan.dout_nchw) carries the scale that replay read from the device -- the
    halved one right after a skipped step."""
    from lighthand_amd.amp import DynamicLossScale
    from lighthand_amd.runtime import TrainStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    rng = np.random.RandomState(70)
    x = torch.from_numpy(rng.randn(4, 3, 128, 128).astype(F32)).cuda()
    j = torch.from_numpy(np.concatenate([rng.uniform(8, 120, size=(4, 21, 2)), rng.uniform(size=(4, 21, 1)) < 0.8], -1).astype(F32)).cuda()
    m = _model("fp16")
    st = TrainStep(m, 4, 128, 128, lr=1e-3, loss_scale=DynamicLossScale(init_scale=2.0 ** 40), use_target_weight=True, ohkm_topk=8)
    prev = m.arena().flat.clone()
    found, scales = [], []
    for _ in range(60):
        scale_read = st.scaler.scale                              # what this replay's loss kernel reads
        st(x, j)
        torch.cuda.synchronize()
        f = int(st.scaler.found_inf)
        found.append(f)
        scales.append(st.scaler.scale)
        want_loss, _, want_grad, _ = _restate(st.plan.out_nchw.cpu().numpy(), st.target.cpu().numpy(),
                                              st.target_weight.cpu().numpy()[..., 0], 8, scale_read)
        assert np.array_equal(_bits(st.plan.dout_nchw.cpu().numpy()), _bits(want_grad))
        assert _close(float(st.loss), want_loss)                 # the loss VALUE never carries the scale
        w = m.arena().flat
        if f:
            assert torch.equal(w, prev) and scales[-1] == scale_read * 0.5
        else:
            assert scales[-1] == scale_read
        prev = w.clone()
        if found.count(0) == 5:
            break
    first_ok = found.index(0)
    assert found[0] == 1 and first_ok >= 1 and all(found[:first_ok])
    assert scales[first_ok - 1] == 2.0 ** (40 - first_ok)
    assert found.count(0) == 5 and int(st.optimizer._dev[0]["step"]) == 5 and st.scaler.skipped_steps == len(found) - 5
    assert torch.isfinite(m.arena().flat).all()


def test_train_cli_with_both_flags(tmp_path, capsys, monkeypatch):
    """python -m lighthand_amd.tools.train --synthetic ... --use_target_weight --ohkm_topk 8 end to end: synthetic samples carry
    the visibility column, both the full-size and the short-batch step train with the weighted mining loss, validation scores the
    same criterion, the checkpoint is written."""
    import os
    from lighthand_amd import runtime
    from lighthand_amd.tools import train as T
    made = []
    real_init = runtime.TrainStep.__init__

    def spy(self, *a, **k):
        real_init(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(runtime.TrainStep, "__init__", spy)
    args = T.parse_args(["--root_path", str(tmp_path), "--synthetic", "20", "--val_synthetic", "8", "--batch_size", "8", "--epoch", "2",
                         "--depth", "18", "--size", "64", "--precision", "bf16", "--reset", "--use_target_weight", "--ohkm_topk", "8"])
    best = T.main(args)
    out = capsys.readouterr().out
    assert np.isfinite(best) and "valid loss" in out
    assert {s.joints.shape[0] for s in made} == {8, 4}
    assert all(s.use_target_weight and s.ohkm_topk == 8 for s in made)
    assert any(float(s.vis.min()) == 0.0 for s in made)           # invisible synthetic joints reached the step
    assert os.path.isfile(os.path.join(args.output_dir, "checkpoint-good", "state_dict.bin"))
    # validation with the training criterion differs from the plain one on the same model and data
    model = T.build_model(args).cuda().set_precision("bf16")
    loader = torch.utils.data.DataLoader(T.SyntheticHands(8, 64, 3, invisible=0.3), batch_size=8)
    plain_args = T.parse_args(["--size", "64"])
    lw, pck_w, epe_w = T.validate(model, loader, args)
    lp, pck_p, epe_p = T.validate(model, loader, plain_args)
    assert np.isfinite(lw) and lw != lp and (pck_w, epe_w) == (pck_p, epe_p)      # PCK / EPE stay as they are
