"""GPU: the flip test (TEST.FLIP_TEST / SHIFT_HEATMAP / POST_PROCESS of the reference's configs) -- lh_nhwc4_mirror,
lh_heatmap_flip_merge, and InferStep / InferPipeline / the evaluation CLI on top of them.

The merge restated in numpy (fp32; the library is built with -ffp-contract=off):
    shift:    f[y][x] = m[y][W-x] for x >= 1, f[y][0] = m[y][W-1];   no shift: f[y][x] = m[y][W-1-x]
    merged = (a + f) * 0.5f, decoded by lh_heatmap_argmax's rule."""
import os

import numpy as np
import pytest
import torch

from conftest import resnet_cfg

pytestmark = pytest.mark.gpu

DT = {"fp32": (0, torch.float32, torch.int32), "bf16": (1, torch.bfloat16, torch.int16), "fp16": (2, torch.float16, torch.int16)}
F = np.float32


@pytest.fixture
def static_kernel_choice(monkeypatch):
    """Two plans of the same shape are compared bit for bit: the library's static kernel choices (LH_AUTOTUNE=0) keep timing
    near-ties from picking different kernels, and so different summation orders, for the two."""
    monkeypatch.setenv("LH_AUTOTUNE", "0")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def merge_reference(a, m, shift):
    f = m[..., ::-1]
    if shift:
        f = np.concatenate([f[..., :1], f[..., :-1]], -1)
    return ((a + f) * F(0.5)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ lh_nhwc4_mirror
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_nhwc4_mirror_reverses_the_interior_bit_exactly(dtype):
    from lighthand_amd import _lib
    lib = _lib.load()
    code, tdt, idt = DT[dtype]
    shapes = [(2, 5, 9, 0), (2, 5, 9, 3), (3, 4, 8, 0), (3, 4, 8, 3), (2, 3, 1, 3)]
    if dtype == "bf16":
        shapes.append((64, 256, 256, 3))                       # the R50 flip-test input: more pairs than one grid pass
    g = torch.Generator(device="cuda").manual_seed(11)
    lim = 1 << (31 if idt == torch.int32 else 15)
    for n, h, w, pad in shapes:
        wp = w + 2 * pad + 2
        img = torch.full((n, h + 2 * pad, wp, 4), 0x3A5C if idt == torch.int16 else 0x3F2A5C11, dtype=idt, device="cuda")
        img[:, pad:pad + h, pad:pad + w] = torch.randint(-lim, lim, (n, h, w, 4), generator=g, device="cuda", dtype=idt)
        img = img.view(tdt)
        before = img.clone()
        want = before.clone()
        want[:, pad:pad + h, pad:pad + w] = before[:, pad:pad + h, pad:pad + w].flip(2)
        _lib.check(lib.lh_nhwc4_mirror(img.data_ptr(), n, h, w, pad, wp, code, _stream()), "lh_nhwc4_mirror")
        torch.cuda.synchronize()
        assert _same(img, want), (dtype, n, h, w, pad)
        _lib.check(lib.lh_nhwc4_mirror(img.data_ptr(), n, h, w, pad, wp, code, _stream()), "lh_nhwc4_mirror")
        torch.cuda.synchronize()
        assert _same(img, before), (dtype, n, h, w, pad)


# ------------------------------------------------------------------------------------------------ lh_heatmap_flip_merge
def _maps(bj, h, w, seed):
    rng = np.random.RandomState(seed)
    a, m = rng.randn(bj, h, w).astype(np.float32), rng.randn(bj, h, w).astype(np.float32)
    a[0], m[0] = 1.0, 1.0                                      # every element ties: the first wins
    a[1], m[1] = 0.0, 0.0
    a[1, 2, 3] = a[1, 4, 1] = 0.5                              # two equal peaks
    a[2], m[2] = -np.abs(a[2]) - 0.125, -np.abs(m[2]) - 0.125  # all negative: coordinates zeroed
    a[3, 1, 2] = np.nan                                        # NaN counts as the maximum
    m[4, 3, 0] = np.nan                                        # ... also when it comes through the flip
    return a, m


@pytest.mark.parametrize("h,w", [(64, 64), (17, 23), (5, 7), (8, 9)])
@pytest.mark.parametrize("shift", [True, False])
def test_flip_merge_equals_numpy_merge_and_argmax(h, w, shift):
    """5 x 7 = 35 elements: three of the workgroup's four waves hold no candidate and the first is partly filled; 8 x 9 = 72: one
    full wave, eight lanes of the second, two empty waves; from 17 x 23 on every wave has one."""
    from lighthand_amd.heatmap import flip_merge_device, max_preds_device
    from oracle.heatmap import get_max_preds
    b, j = (2, 21) if w == 64 else (1, 6)
    a, m = _maps(b * j, h, w, 3 + w)
    a, m = a.reshape(b, j, h, w), m.reshape(b, j, h, w)
    want = merge_reference(a, m, shift)
    at, mt = torch.from_numpy(a).cuda(), torch.from_numpy(m).cuda()
    preds, maxvals, idx, merged = flip_merge_device(at, mt, shift=shift, scale=4.0)
    torch.cuda.synchronize()
    got = merged.cpu().numpy()
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all() and nan.any()
    assert np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32))
    wp, wm, wi = max_preds_device(torch.from_numpy(want).cuda(), scale=4.0)
    assert torch.equal(preds, wp) and torch.equal(idx, wi)
    assert torch.equal(maxvals.isnan(), wm.isnan()) and torch.equal(maxvals.nan_to_num(), wm.nan_to_num())
    assert np.array_equal(preds.cpu().numpy(), get_max_preds(want)[0] * 4)
    flat = want.reshape(b * j, -1)
    assert int(idx.view(-1)[0]) == 0 and int(idx.view(-1)[1]) == 2 * w + 3
    assert (preds.view(-1, 2)[2] == 0).all() and float(maxvals.view(-1)[2]) < 0
    assert int(idx.view(-1)[3]) == int(np.flatnonzero(np.isnan(flat[3]))[0])
    # merged may alias a: the step writes the merge over its copy of the plain pass's maps
    alias = at.clone()
    p2, m2, i2, out = flip_merge_device(alias, mt, shift=shift, scale=4.0, out=alias)
    torch.cuda.synchronize()
    assert out.data_ptr() == alias.data_ptr()
    assert _same(alias, merged) and torch.equal(p2, preds) and torch.equal(i2, idx) and _same(m2, maxvals)


# ------------------------------------------------------------------------------------------------ InferStep
def _r18(precision, seed=5):
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    torch.manual_seed(seed)
    return get_pose_net(resnet_cfg(18), True).cuda().set_precision(precision)


def _run(step, x):
    step(x)
    torch.cuda.synchronize()
    return step.preds.clone(), step.maxvals.clone(), step.heatmaps.clone()


def _check_flip_step(model, b, h, w, bn_train, seed):
    """InferStep(flip_test=True) against flip_merge_device over two plain InferSteps (x and its mirror), the oracle's decode,
    the eager step and a second call."""
    from lighthand_amd.heatmap import flip_merge_device
    from lighthand_amd.runtime import InferStep
    from oracle.heatmap import get_max_preds
    x = torch.from_numpy(np.random.RandomState(seed).randn(b, 3, h, w).astype(np.float32)).cuda()
    flip = InferStep(model, b, h, w, bn_train=bn_train, flip_test=True)
    p, mv, hm = _run(flip, x)
    _, _, ha = _run(InferStep(model, b, h, w, bn_train=bn_train), x)
    _, _, hf = _run(InferStep(model, b, h, w, bn_train=bn_train), torch.flip(x, [3]))
    scale = float(h // hm.shape[2])
    wp, wmv, _, whm = flip_merge_device(ha, hf, shift=True, scale=scale)
    torch.cuda.synchronize()
    assert _same(hm, whm)
    assert torch.equal(p, wp) and _same(mv, wmv)
    assert not _same(hm, ha)                                   # the mirrored pass contributed
    assert np.array_equal(p.cpu().numpy(), get_max_preds(hm.cpu().numpy())[0] * scale)
    e = _run(InferStep(model, b, h, w, bn_train=bn_train, flip_test=True, use_graph=False), x)
    assert torch.equal(e[0], p) and _same(e[1], mv) and _same(e[2], hm)
    again = _run(flip, x)
    assert torch.equal(again[0], p) and _same(again[1], mv) and _same(again[2], hm)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_infer_step_flip_test_equals_merge_of_two_plain_steps(precision, static_kernel_choice):
    _check_flip_step(_r18(precision).eval(), 4, 96, 96, False, 1)


def test_infer_step_flip_test_train_mode_batchnorm(static_kernel_choice):
    """bn_train: each pass normalises with its own batch statistics, and the running statistics move twice -- exactly as two
    plain bn_train calls on x and on its mirror image do."""
    from lighthand_amd.runtime import InferStep
    model = _r18("bf16", seed=6)
    _check_flip_step(model, 4, 96, 96, True, 2)
    b, h, w = 4, 96, 96
    x = torch.from_numpy(np.random.RandomState(3).randn(b, 3, h, w).astype(np.float32)).cuda()
    running = {k: v for k, v in model.state_dict(keep_vars=True).items() if k.endswith(("running_mean", "running_var"))}
    assert running
    start = {k: v.detach().clone() for k, v in running.items()}
    _run(InferStep(model, b, h, w, bn_train=True, flip_test=True, use_graph=False), x)
    after_flip = {k: v.detach().clone() for k, v in running.items()}
    with torch.no_grad():
        for k, v in running.items():
            v.copy_(start[k])
    plain = InferStep(model, b, h, w, bn_train=True, use_graph=False)
    _run(plain, x)
    _run(plain, torch.flip(x, [3]))
    assert any(not _same(after_flip[k], start[k]) for k in running)
    for k, v in running.items():
        assert _same(after_flip[k], v.detach()), k


def test_infer_step_flip_test_uint8_input(static_kernel_choice):
    """uint8 frames: the mirrored pass reads the mirror of the image the plain uint8 pipeline fed to the stem."""
    from lighthand_amd.heatmap import flip_merge_device
    from lighthand_amd.runtime import InferStep
    model = _r18("bf16", seed=7).eval()
    b, h, w, hs, ws = 4, 96, 96, 100, 80
    frames = torch.randint(0, 256, (b, hs, ws, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    p, mv, hm = _run(InferStep(model, b, h, w, input_u8=(hs, ws), flip_test=True), frames)
    plain8 = InferStep(model, b, h, w, input_u8=(hs, ws))
    _, _, ha = _run(plain8, frames)
    pad = plain8.plan.img_pad
    fed = plain8.plan.img_nhwc4[:, pad:pad + h, pad:pad + w, :3].permute(0, 3, 1, 2).float()       # exact: bf16 -> fp32 -> bf16
    _, _, hf = _run(InferStep(model, b, h, w), torch.flip(fed, [3]).contiguous())
    wp, wmv, _, whm = flip_merge_device(ha, hf, shift=True, scale=4.0)
    torch.cuda.synchronize()
    assert _same(hm, whm) and torch.equal(p, wp) and _same(mv, wmv)


def test_infer_step_post_process(static_kernel_choice):
    """post_process refines the decode of step.heatmaps (the plain maps, or the merged ones with flip_test) in the graph."""
    from lighthand_amd.heatmap import max_preds_device
    from lighthand_amd.runtime import InferStep
    model = _r18("fp32", seed=8).eval()
    b, h, w = 4, 96, 96
    x = torch.from_numpy(np.random.RandomState(5).randn(b, 3, h, w).astype(np.float32)).cuda()
    for flip in (False, True):
        p, _, hm = _run(InferStep(model, b, h, w, flip_test=flip, post_process=True), x)
        want, _, _ = max_preds_device(hm, scale=4.0, post_process=True)
        hard, _, _ = max_preds_device(hm, scale=4.0)
        torch.cuda.synchronize()
        assert torch.equal(p, want), flip
        assert not torch.equal(p, hard), flip
        unrefined, _, hm2 = _run(InferStep(model, b, h, w, flip_test=flip), x)
        assert _same(hm2, hm) and torch.equal(unrefined, hard)


def test_infer_pipeline_flip_test_equals_infer_step(static_kernel_choice):
    from lighthand_amd.runtime import InferPipeline, InferStep
    model = _r18("bf16", seed=9).eval()
    b, h, w = 4, 128, 96
    g = torch.Generator(device="cuda").manual_seed(6)
    batches = [torch.randn(b, 3, h, w, device="cuda", generator=g) for _ in range(5)]
    ref = InferStep(model, b, h, w, flip_test=True, slot=7)
    want = [_run(ref, x)[:2] for x in batches]
    pipe = InferPipeline(model, b, h, w, depth=2, flip_test=True)
    got = list(pipe.map(batches))
    assert len(got) == len(want)
    for (p, m), (pw, mw) in zip(got, want):
        assert torch.equal(p, pw) and _same(m, mw)


def test_infer_step_flip_test_hrnet_lanes(static_kernel_choice):
    """HRNet-W32 (narrower than the reference's W48) at 64 x 64: the branch launches run on stream lanes (Plan._run_lanes), in both passes."""
    from lighthand_amd.modeling.hrnet.pose_hrnet import get_hrnet, hrnet_cfg
    torch.manual_seed(10)
    model = get_hrnet(hrnet_cfg(32), True).cuda().set_precision("fp32").eval()
    _check_flip_step(model, 4, 64, 64, False, 4)


def test_eval_cli_flip_test_post_process(tmp_path, static_kernel_choice):
    """wearable_eval_2d --flip_test --post_process writes the usual files, and its predictions are those of an
    InferStep(flip_test=True, post_process=True) over the same set (bn_train, the CLI's default)."""
    import json
    from lighthand_amd.runtime import InferStep
    from lighthand_amd.tools import wearable_eval_2d as E
    from lighthand_amd.tools.train import build_model
    args = E.build_parser().parse_args(["--depth", "18"])
    args.model = "simplebaseline"
    torch.manual_seed(12)
    sd = build_model(args).state_dict()
    run = tmp_path / "simplebaseline" / "frei" / "run1" / "checkpoint-good"
    run.mkdir(parents=True)
    torch.save({"model_state_dict": sd}, str(run / "state_dict.bin"))
    files = E.main(["--root_path", str(tmp_path), "--model_path", "simplebaseline/frei", "--batch_size", "4", "--depth", "18",
                    "--size", "64", "--synthetic", "10", "--flip_test", "--post_process"])
    assert len(files) == 3 and all(os.path.isfile(f) for f in files)
    ev = json.load(open(os.path.join(str(tmp_path), "simplebaseline/frei/run1", "evaluation.json")))
    assert isinstance(ev, list) and set(ev[0]) == set(E.CATEGORIES)
    model = build_model(args).cuda().set_precision("fp32")
    model.load_state_dict(sd, strict=False)
    model.train()
    loader = torch.utils.data.DataLoader(E.SyntheticEvalSet(10, 64), batch_size=4, shuffle=False)
    got = {c: iter(v["pred"]) for c, v in ev[0].items()}
    steps, n = {}, 0
    for images, _, cats in loader:
        k = images.shape[0]
        if k not in steps:
            steps[k] = InferStep(model, k, 64, 64, bn_train=True, flip_test=True, post_process=True)
        want = _run(steps[k], images.cuda())[0].cpu().numpy()
        for i, c in enumerate(cats):
            assert np.array_equal(np.asarray(next(got[c]), np.float32), want[i])
            n += 1
    assert n == 10
