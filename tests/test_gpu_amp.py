"""GPU: dynamic loss scaling inside the captured step (lighthand_amd.amp, Adam.step(amp=...), TrainStep(loss_scale="dynamic")):
the kernels against torch's own AMP primitives, skipped steps that leave the optimizer bit-unchanged, fp16 overflow recovery,
data parallel, the train CLI."""
import os

import numpy as np
import pytest
import torch

from conftest import resnet_cfg

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)


def _model(depth=18, precision="fp32", seed=9001):
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    torch.manual_seed(seed)
    return get_pose_net(resnet_cfg(depth), True).cuda().set_precision(precision)


def _batch(b, size, seed):
    rng = np.random.RandomState(seed)
    return (torch.from_numpy(rng.randn(b, 3, size, size).astype(np.float32)).cuda(),
            torch.from_numpy(rng.uniform(8, size - 8, size=(b, 21, 2)).astype(np.float32)).cuda())


def _targets(b, hs, seed):
    rng = np.random.RandomState(seed)
    return torch.from_numpy(rng.uniform(0, 1, size=(b, 21, hs, hs)).astype(np.float32) ** 8).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lh_found_inf(g):
    from lighthand_amd import _lib
    lib = _lib.load()
    partial = torch.full((lib.lh_amp_check_blocks(),), 7, dtype=torch.int32, device="cuda")
    _lib.check(lib.lh_amp_check(g.data_ptr(), g.numel(), partial.data_ptr(), _stream()), "lh_amp_check")
    p = partial.cpu()
    assert set(p.tolist()) <= {0, 1}                 # every workgroup wrote its slot
    return int(p.any())


def _torch_found_inf(g, inv_scale):
    found = torch.zeros(1, dtype=torch.float32, device="cuda")
    torch._amp_foreach_non_finite_check_and_unscale_([g.clone()], found, torch.tensor([inv_scale], device="cuda"))
    return int(found.item())


@pytest.mark.parametrize("numel", [34_000_003, 11_200_002, 4097, 7, 3])
def test_check_kernel_matches_torch(numel):
    """lh_amp_check against torch._amp_foreach_non_finite_check_and_unscale_ on arena-sized buffers and short ones, numel % 4 != 0
    (the scalar tail): one +inf / -inf / NaN at the first element, in a middle vector, in the last whole vector, in the tail."""
    torch.manual_seed(numel)
    g = torch.randn(numel, device="cuda")
    assert _lh_found_inf(g) == _torch_found_inf(g, 1.0) == 0
    nvec = numel // 4
    where = {0, numel - 1}
    if nvec:
        where |= {(nvec // 2) * 4 + 1, nvec * 4 - 1}
    for i in sorted(where):
        for bad in (float("inf"), float("-inf"), float("nan")):
            keep = g[i].item()
            g[i] = bad
            assert _lh_found_inf(g) == _torch_found_inf(g, 1.0) == 1, (i, bad)
            g[i] = keep
    # every finite value, extremes included, is clean
    g[0] = FLT_MAX
    g[-1] = -FLT_MAX
    g[numel // 2] = 1e-45                           # subnormal
    g[numel // 3] = -1e-40
    assert _lh_found_inf(g) == _torch_found_inf(g, 1.0) == 0
    # the test is on the RAW gradient: scale 2**-4 (inv 16) and a finite 1e38 that unscales to inf is not flagged, by torch either
    g[numel // 2] = 1e38
    assert _lh_found_inf(g) == _torch_found_inf(g, 16.0) == 0


def _update(lib, scaler, found, extra, adam):
    from lighthand_amd import _lib
    scaler._partial.zero_()
    if found:
        scaler._partial[scaler._partial.numel() // 3] = 1
    hyper, step, derived = adam
    _lib.check(lib.lh_amp_update(scaler._partial.data_ptr(), scaler._hyper.data_ptr(), scaler._scale.data_ptr(),
                                 scaler._growth_tracker.data_ptr(), scaler._found_inf.data_ptr(), scaler._skipped.data_ptr(),
                                 scaler._inv.data_ptr(), extra, hyper.data_ptr(), step.data_ptr(), derived.data_ptr(), _stream()),
               "lh_amp_update")


def _adam_state():
    return (torch.tensor([1e-3, 0.9, 0.999, 1e-8], dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
            torch.zeros(8, dtype=torch.float32, device="cuda"))


@pytest.mark.parametrize("init_scale", [2.0 ** 16, 3e38, 1000.0])
def test_scale_state_machine_matches_torch(init_scale):
    """lh_amp_update's scale / growth tracker against torch._amp_update_scale_ over a seeded 300-step found_inf sequence,
    growth_interval 3, bit for bit after every step; from 3e38 the growth to 6e38 would overflow and is not applied (torch keeps
    3e38 with tracker 0).  Adam's step counter moves on finite steps only, `skipped` counts the others, inv = 1 / scale."""
    from lighthand_amd import _lib
    from lighthand_amd.amp import DynamicLossScale
    lib = _lib.load()
    s = DynamicLossScale(init_scale=init_scale, growth_interval=3)
    t_scale = torch.full((1,), init_scale, dtype=torch.float32, device="cuda")
    t_tracker = torch.zeros(1, dtype=torch.int32, device="cuda")
    adam = _adam_state()
    rng = np.random.RandomState(int(init_scale) % 1000)
    seq = [0, 0, 0, 0, 0, 0] + (rng.uniform(size=294) < 0.3).astype(int).tolist()
    saw_capped = False
    for k, f in enumerate(seq):
        before = float(s._scale.item())
        _update(lib, s, f, 1.0, adam)
        torch._amp_update_scale_(t_scale, t_tracker, torch.full((1,), float(f), device="cuda"), 2.0, 0.5, 3)
        assert torch.equal(s._scale, t_scale) and torch.equal(s._growth_tracker, t_tracker), (k, s._scale, t_scale)
        assert int(s.found_inf) == f and float(s._inv.item()) == np.float32(1.0 / np.float64(before))
        saw_capped |= before == np.float32(3e38) and f == 0 and int(t_tracker) == 0 and float(t_scale.item()) == before
    assert int(adam[1]) == len(seq) - sum(seq) and s.skipped_steps == sum(seq)
    if init_scale == 3e38:
        assert saw_capped


def test_guarded_apply_skips_or_equals_adam_step():
    """lh_adam_apply_guarded: with found_inf set, params, moments, step and derived stay bit-unchanged; without it the result is
    bit-equal to lh_adam_step with grad_scale = inv (here extra 0.5 / scale 1024)."""
    from lighthand_amd import _lib
    from lighthand_amd.amp import DynamicLossScale
    lib = _lib.load()
    n = 1_000_003
    torch.manual_seed(3)
    p, g = torch.randn(n, device="cuda"), torch.randn(n, device="cuda") * 100
    m, v = torch.randn(n, device="cuda") * 1e-2, torch.rand(n, device="cuda") * 1e-3
    for found in (1, 0):
        s = DynamicLossScale(init_scale=1024.0)
        adam = _adam_state()
        adam[1].fill_(4)
        adam[2].copy_(torch.arange(8, dtype=torch.float32))
        pp, mm, vv = p.clone(), m.clone(), v.clone()
        _update(lib, s, found, 0.5, adam)
        _lib.check(lib.lh_adam_apply_guarded(pp.data_ptr(), g.data_ptr(), mm.data_ptr(), vv.data_ptr(), n, adam[2].data_ptr(),
                                             s.found_inf.data_ptr(), s._inv.data_ptr(), _stream()), "lh_adam_apply_guarded")
        torch.cuda.synchronize()
        if found:
            assert torch.equal(pp, p) and torch.equal(mm, m) and torch.equal(vv, v)
            assert int(adam[1]) == 4 and torch.equal(adam[2], torch.arange(8, dtype=torch.float32, device="cuda"))
            assert s.scale == 512.0 and s.skipped_steps == 1
            continue
        ref = _adam_state()
        ref[1].fill_(4)
        rp, rm, rv = p.clone(), m.clone(), v.clone()
        _lib.check(lib.lh_adam_step(rp.data_ptr(), g.data_ptr(), rm.data_ptr(), rv.data_ptr(), n, ref[0].data_ptr(), ref[1].data_ptr(),
                                    ref[2].data_ptr(), 0.5 / 1024.0, _stream()), "lh_adam_step")
        torch.cuda.synchronize()
        assert float(s._inv.item()) == 0.5 / 1024.0 and int(adam[1]) == 5
        assert torch.equal(pp, rp) and torch.equal(mm, rm) and torch.equal(vv, rv) and torch.equal(adam[2][:5], ref[2][:5])
        assert not torch.equal(pp, p)


def _run(model, steps, data=None, **kw):
    from lighthand_amd.runtime import TrainStep
    x, j = data or _batch(4, 128, 5)
    st = TrainStep(model, 4, 128, 128, lr=1e-3, **kw)
    losses = []
    for _ in range(steps):
        st(x, j)
        losses.append(float(st.loss))
    torch.cuda.synchronize()
    o = st.optimizer.state["flat"]
    return st, losses, model.arena().flat.clone(), o["exp_avg"].clone(), o["exp_avg_sq"].clone()


@pytest.mark.parametrize("use_graph", [True, False])
def test_dynamic_without_overflow_equals_static(use_graph, monkeypatch):
    """R18 fp16 128^2 batch 4, 20 steps: DynamicLossScale(init_scale=1024, no growth) against the static loss_scale=1024 -- the
    same weights, moments and losses bit for bit, captured and eager."""
    from lighthand_amd.amp import DynamicLossScale
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    _, la, wa, ma, va = _run(_model(18, "fp16"), 20, loss_scale=1024.0, use_graph=use_graph)
    st, lb, wb, mb, vb = _run(_model(18, "fp16"), 20, loss_scale=DynamicLossScale(init_scale=1024.0, growth_interval=10 ** 6),
                              use_graph=use_graph)
    assert st.loss_scale == "dynamic" and st.scaler.scale == 1024.0 and st.scaler.skipped_steps == 0
    assert la == lb and all(np.isfinite(la))
    assert torch.equal(wa, wb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert int(st.optimizer._dev[0]["step"]) == 20


def test_poisoned_step_is_skipped_exactly(monkeypatch):
    """bf16 R18, targets handed in (power-of-two scales are exact here, test_static_loss_scale_is_exact_...).  Run A: 5 clean
    steps.  Run B: 2 clean steps, one whose target holds a NaN, the same 3 clean steps.  B's weights and moments equal A's bit for
    bit, Adam took 5 steps in both, B's found_inf reads 0,0,1,0,0,0, its scale was halved once.  (BatchNorm running statistics
    are not compared: the skipped step's forward updated them, as in torch.)"""
    from lighthand_amd.amp import DynamicLossScale
    from lighthand_amd.runtime import TrainStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    data = [(_batch(4, 128, 40 + k)[0], _targets(4, 32, 50 + k)) for k in range(5)]
    poison = _targets(4, 32, 99)
    poison[1, 3, 7, 9] = float("nan")
    res = {}
    for run in ("A", "B"):
        m = _model(18, "bf16")
        st = TrainStep(m, 4, 128, 128, lr=1e-3, targets_from_joints=False, loss_scale="dynamic")
        seq = data[:2] + ([(data[2][0], poison)] if run == "B" else []) + data[2:]
        found = []
        for x, t in seq:
            st(x, target=t)
            found.append(int(st.scaler.found_inf))
        torch.cuda.synchronize()
        o = st.optimizer.state["flat"]
        res[run] = (found, m.arena().flat.clone(), o["exp_avg"].clone(), o["exp_avg_sq"].clone(), int(st.optimizer._dev[0]["step"]),
                    st.scaler.scale, st.scaler.skipped_steps, st.optimizer.state_dict()["state"][0]["step"])
    a, b = res["A"], res["B"]
    assert a[0] == [0] * 5 and b[0] == [0, 0, 1, 0, 0, 0]
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert a[4] == b[4] == 5 and float(a[7]) == float(b[7]) == 5.0
    assert a[5] == 2.0 ** 16 and b[5] == 2.0 ** 15 and (a[6], b[6]) == (0, 1)


def test_fp16_overflow_recovery(monkeypatch):
    """R18 fp16 with init_scale=2**40: the first steps overflow, report found_inf and leave the weights bit-unchanged; the scale
    falls by powers of two until steps succeed; 40 steps later every weight and moment is finite and the loss is within 2 % of a
    static loss_scale=1024 run that took the same number of successful steps on the same batch (measured on the MI355X: 12
    skipped steps, loss ratio 1.0001; the two runs differ only in where fp16 rounds and underflows).  The same run with a STATIC 2**40 ends with non-finite weights: the
    failure dynamic scaling removes."""
    from lighthand_amd.amp import DynamicLossScale
    from lighthand_amd.runtime import TrainStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    x, j = _batch(4, 128, 7)
    m = _model(18, "fp16")
    st = TrainStep(m, 4, 128, 128, lr=1e-3, loss_scale=DynamicLossScale(init_scale=2.0 ** 40))
    prev = m.arena().flat.clone()
    found, scales = [], []
    for _ in range(80):
        st(x, j)
        f = int(st.scaler.found_inf)
        found.append(f)
        scales.append(st.scaler.scale)
        w = m.arena().flat
        if f:
            assert torch.equal(w, prev)
        elif found.count(0) == 1:
            assert not torch.equal(w, prev)
        prev = w.clone()
        if found.count(0) == 40:
            break
    first_ok = found.index(0)
    assert found[0] == 1 and first_ok >= 1 and all(found[:first_ok])
    assert scales[first_ok - 1] == 2.0 ** (40 - first_ok)           # halved once per skipped step
    good = found.count(0)
    assert good == 40 and int(st.optimizer._dev[0]["step"]) == good
    o = st.optimizer.state["flat"]
    assert torch.isfinite(m.arena().flat).all() and torch.isfinite(o["exp_avg"]).all() and torch.isfinite(o["exp_avg_sq"]).all()
    loss_dyn = float(st.loss)
    _, ls, _, _, _ = _run(_model(18, "fp16"), good, data=(x, j), loss_scale=1024.0)
    _, lb, wb, _, _ = _run(_model(18, "fp16"), 5, data=(x, j), loss_scale=2.0 ** 40)
    ratio = loss_dyn / ls[-1]
    print(f"fp16 overflow recovery: {first_ok} skipped steps, scale {scales[-1]:g}, loss {loss_dyn:.6g} vs static-1024 {ls[-1]:.6g} "
          f"(ratio {ratio:.4f}); static 2**40: finite weights {bool(torch.isfinite(wb).all())}")
    assert abs(ratio - 1.0) < 0.02
    assert not torch.isfinite(wb).all()


def _dp_amp_rank(rank, world, port, compress, q):
    """One data-parallel rank (spawned fresh), both ranks on GPU 0 through gloo: dynamic loss scaling, rank 1's target of step 1
    holds a NaN."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      LH_DIST_BACKEND="gloo")
    import torch.distributed as dist
    from lighthand_amd import parallel
    from lighthand_amd.runtime import TrainStep
    parallel.init_distributed()
    m = _model(18)
    sync = parallel.GradSync(world, bucket_bytes=2 << 20, compress=compress)
    step = TrainStep(m, 4, 64, 64, lr=1e-3, use_graph=True, grad_sync=sync, targets_from_joints=False, loss_scale="dynamic")
    found = []
    for k in range(4):
        x = _batch(4, 64, 11 + rank + 10 * k)[0]
        t = _targets(4, 16, 21 + rank + 10 * k)
        if k == 1 and rank == 1:
            t[2, 5, 3, 3] = float("nan")
        step(x, target=t)
        found.append(int(step.scaler.found_inf))
    torch.cuda.synchronize()
    q.put((rank, m.arena().flat.cpu().numpy(), found, step.scaler.scale, step.scaler.skipped_steps, int(step.optimizer._dev[0]["step"]),
           len(sync.segments(step.plan))))
    dist.barrier()
    step.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("compress", [None, "bf16"])
def test_two_process_data_parallel_skips_on_every_rank(compress, monkeypatch):
    """Two processes, a real collective (gloo), per-segment graphs: a NaN in ONE rank's target makes BOTH ranks skip that step
    (the check reads the all-reduced gradients), both keep the same scale, and the weights stay bit-identical across ranks."""
    import socket
    import torch.multiprocessing as mp
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_amp_rank, args=(r, 2, port, compress, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in procs:
        r = q.get(timeout=300)
        res[r[0]] = r
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    a, b = res[0], res[1]
    assert a[2] == b[2] == [0, 1, 0, 0]
    assert a[3] == b[3] == 2.0 ** 15 and a[4] == b[4] == 1 and a[5] == b[5] == 3 and a[6] >= 2
    assert np.array_equal(a[1], b[1]) and np.isfinite(a[1]).all()


def test_train_cli_dynamic_loss_scale_checkpoint_and_resume(tmp_path, capsys, monkeypatch):
    """--precision fp16 --loss_scale dynamic end to end: the checkpoint holds scaler_state_dict (GradScaler's keys), the epoch line
    reports the scale and the skipped steps, and a resumed run starts from the saved scale and growth tracker."""
    from lighthand_amd.tools import train as T
    argv = ["--root_path", str(tmp_path), "--synthetic", "16", "--val_synthetic", "8", "--batch_size", "8", "--depth", "18",
            "--size", "64", "--precision", "fp16", "--loss_scale", "dynamic"]
    best = T.main(T.parse_args(argv + ["--epoch", "2", "--reset"]))
    out = capsys.readouterr().out
    assert np.isfinite(best) and "loss scale" in out and "skipped" in out
    args = T.parse_args(argv + ["--epoch", "3"])
    path = os.path.join(args.output_dir, "checkpoint-good", "state_dict.bin")
    sd = torch.load(path, map_location="cpu")
    assert sorted(sd["scaler_state_dict"]) == ["_growth_tracker", "backoff_factor", "growth_factor", "growth_interval", "scale"]
    sd["scaler_state_dict"].update(scale=512.0, _growth_tracker=5)
    torch.save(sd, path)
    seen = []
    load = T.load_scaler_state

    def spy(scaler, a):
        ok = load(scaler, a)
        seen.append((ok, scaler.state_dict(), scaler))
        return ok
    monkeypatch.setattr(T, "load_scaler_state", spy)
    T.main(args)
    out = capsys.readouterr().out
    (ok, loaded, scaler), = seen
    assert ok and loaded["scale"] == 512.0 and loaded["_growth_tracker"] == 5
    steps = 2 * (3 - (sd["epoch"] + 1))                 # 16 samples at batch 8, the epochs after the saved one
    skipped = scaler.skipped_steps
    assert scaler.scale == 512.0 * 0.5 ** skipped
    if skipped == 0:
        assert scaler.state_dict()["_growth_tracker"] == 5 + steps
    assert f"loss scale {scaler.scale:g} skipped {skipped}" in out
