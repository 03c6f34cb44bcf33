"""GPU: DARK's sub-pixel heat-map coding -- lh_gaussian_target_sub (unbiased target render), lh_heatmap_dark (Taylor decode on the
log of the blurred map) and the options of render_targets / max_preds_device / TrainStep / InferStep on top of them.

The two formulas restated in fp64 NumPy (target_reference, dark_reference below):
    target  window of (2r+1)^2 cells centred on mx = (int)(jx * 0.25f + 0.5f) (fp32, like lh_gaussian_target), value
            exp(-((x - jx/4)^2 + (y - jy/4)^2) / (2 sigma^2)) inside it; weight = (vis > 0.5 ? vis : 0) * in_frame.
    decode  B = plane under the separable zero-padded Gaussian g[t] = exp(-(t-c)^2 / (2 s^2)) / sum, s = 0.3((k-1)/2 - 1) + 0.8;
            C = log(max(B * maxval / max B, 1e-10)); dx, dy, dxx, dyy, dxy by central differences at the peak;
            peak - H^-1 (dx, dy) when 1 < px < w-2, 1 < py < h-2, maxval > 0, det != 0 and the offset is finite."""
import numpy as np
import pytest
import torch

from conftest import resnet_cfg

pytestmark = pytest.mark.gpu

F = np.float32
RADIUS, SIGMA = 6, 2.0


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ fp64 restatements
def target_reference(joints, vis, size, weighted):
    """joints fp32 [n, 2], vis fp32 [n] or None -> (fp64 maps [n, size, size], fp32 weights [n])."""
    n = joints.shape[0]
    out, weight = np.zeros((n, size, size), np.float64), np.ones(n, F)
    ys, xs = np.mgrid[0:size, 0:size]
    for i in range(n):
        jx, jy = F(joints[i, 0]), F(joints[i, 1])
        mx, my = int(jx * F(0.25) + F(0.5)), int(jy * F(0.25) + F(0.5))          # fp32 sum, truncated toward zero
        x0, y0, x1, y1 = mx - RADIUS, my - RADIUS, mx + RADIUS + 1, my + RADIUS + 1
        skip = x0 >= size or y0 >= size or x1 < 0 or y1 < 0
        if weighted:
            v = F(1.0) if vis is None else F(vis[i])
            weight[i] = (v if v > 0.5 else F(0.0)) * F(0.0 if skip else 1.0)
            draw = weight[i] > 0
        else:
            draw = not skip
        if not draw:
            continue
        inside = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
        g = np.exp(-((xs - float(jx) * 0.25) ** 2 + (ys - float(jy) * 0.25) ** 2) / (2 * SIGMA ** 2))
        out[i] = np.where(inside, g, 0.0)
    return out, weight


def blur_taps(k):
    c, s = (k - 1) / 2.0, 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    g = np.exp(-(np.arange(k) - c) ** 2 / (2 * s * s))
    return g / g.sum()


def dark_reference(maps, idx, maxvals, preds, k):
    """maps fp32 [n, h, w], idx / maxvals / preds (cells) of the arg-max -> fp64 preds in cells, [n, 2]; refined[n] marks the
    planes the Taylor step moved."""
    n, h, w = maps.shape
    g, c = blur_taps(k), (k - 1) // 2
    out, refined = preds.astype(np.float64).copy(), np.zeros(n, bool)
    for i in range(n):
        px, py = int(idx[i]) % w, int(idx[i]) // w
        if not (maxvals[i] > 0 and 1 < px < w - 2 and 1 < py < h - 2):
            continue
        p = np.pad(maps[i].astype(np.float64), ((0, 0), (c, c)))
        rows = sum(g[t] * p[:, t:t + w] for t in range(k))
        p = np.pad(rows, ((c, c), (0, 0)))
        b = sum(g[t] * p[t:t + h, :] for t in range(k))
        with np.errstate(all="ignore"):
            cl = np.log(np.maximum(b * (float(maxvals[i]) / b.max()), 1e-10))
        dx, dy = 0.5 * (cl[py, px + 1] - cl[py, px - 1]), 0.5 * (cl[py + 1, px] - cl[py - 1, px])
        dxx = 0.25 * (cl[py, px + 2] - 2 * cl[py, px] + cl[py, px - 2])
        dyy = 0.25 * (cl[py + 2, px] - 2 * cl[py, px] + cl[py - 2, px])
        dxy = 0.25 * (cl[py + 1, px + 1] - cl[py - 1, px + 1] - cl[py + 1, px - 1] + cl[py - 1, px - 1])
        det = dxx * dyy - dxy * dxy
        if det == 0:
            continue
        ox, oy = -(dyy * dx - dxy * dy) / det, -(dxx * dy - dxy * dx) / det
        if np.isfinite(ox) and np.isfinite(oy):
            out[i], refined[i] = (px + ox, py + oy), True
    return out, refined


# ------------------------------------------------------------------------------------------------ lh_gaussian_target_sub
def _target_joints(size, rng):
    """[3, 21, 3] = x, y, visibility in the 4 * size frame: inside, straddling each border, wholly outside (also with the empty
    window the skip test lets through, x1 == 0), on cell centres and at x.5."""
    full = 4.0 * size
    special = [(-10.0, 0.4 * full), (full + 6.0, 0.6 * full), (0.3 * full, -13.0), (0.7 * full, full + 9.0),     # one border each
               (-9.0, -11.0), (full + 5.0, full + 2.5), (1.5, full - 2.25),                                        # corners
               (-40.0, 0.5 * full), (full + 40.0, 20.0), (20.0, -52.0), (24.0, full + 33.0), (-30.0, 0.5 * full),  # outside
               (4.0 * 7, 4.0 * 9), (4.0 * (size - 3), 4.0 * 2), (0.0, 0.0),                                        # cell centres
               (4.0 * 5 + 2.0, 4.0 * 8 + 2.0), (4.0 * 6 + 2.0, 33.3), (1.999, 2.001)]                              # x.5 in cells
    xy = rng.uniform(8.0, full - 8.0, size=(63, 2))
    xy[:len(special)] = special
    vis = rng.choice([0.0, 1.0, 1.0, 1.0, 0.3, 0.7, 0.5], size=63)
    vis[:len(special)] = 1.0
    vis[len(special):len(special) + 4] = [0.0, 0.3, 0.5, 0.7]
    return np.concatenate([xy, vis[:, None]], 1).astype(F).reshape(3, 21, 3)


@pytest.mark.parametrize("size", [64, 17])
def test_unbiased_target_matches_the_fp64_restatement(size):
    """Values within 1e-5 of the fp64 formula rounded to fp32 (the exponent's argument is at most ~10.6 in magnitude, its fp32
    rounding of a few 2^-24 becomes the same relative error of a result <= 1: about 2e-6, x4), cells outside the window exactly 0,
    the weight bit-equal to lh_gaussian_target_w's."""
    from lighthand_amd.heatmap import render_targets
    j3 = _target_joints(size, np.random.RandomState(size))
    dev = torch.from_numpy(j3).cuda()
    flat = j3.reshape(-1, 3)
    # weight == NULL: no visibility test
    got = render_targets(dev[..., :2].contiguous(), size=size, unbiased=True).cpu().numpy().reshape(-1, size, size)
    want, _ = target_reference(flat[:, :2], None, size, weighted=False)
    print(f"size {size}: max |device - fp64| = {np.abs(got - want.astype(F)).max():.3e}")
    assert np.abs(got - want.astype(F)).max() <= 1e-5
    assert not got[want == 0].any() and (want == 0).any() and got.max() <= 1.0
    assert (want.reshape(63, -1).max(1) == 0).sum() >= 5                       # the wholly-outside joints drew nothing
    # with the visibility column: zero maps where the weight is 0, the weight of the quantised renderer
    got_w, weight = render_targets(dev, size=size, return_weight=True, unbiased=True)
    _, weight_q = render_targets(dev, size=size, return_weight=True)
    torch.cuda.synchronize()
    want_w, want_weight = target_reference(flat[:, :2], flat[:, 2], size, weighted=True)
    assert _same(weight, weight_q) and tuple(weight.shape) == (3, 21, 1)
    assert np.array_equal(weight.cpu().numpy().reshape(-1), want_weight)
    assert (want_weight == 0).sum() >= 5 and (want_weight == F(0.7)).any()
    got_w = got_w.cpu().numpy().reshape(-1, size, size)
    assert np.abs(got_w - want_w.astype(F)).max() <= 1e-5
    assert not got_w[want_w == 0].any() and not got_w[want_weight == 0].any()
    # two columns with return_weight: vis == NULL means every joint visible
    got_1, weight_1 = render_targets(dev[..., :2].contiguous(), size=size, return_weight=True, unbiased=True)
    assert np.array_equal(weight_1.cpu().numpy().reshape(-1), target_reference(flat[:, :2], None, size, weighted=True)[1])
    assert np.array_equal(got_1.cpu().numpy().reshape(-1, size, size)[weight_1.cpu().numpy().reshape(-1) > 0],
                          got[weight_1.cpu().numpy().reshape(-1) > 0])


def test_unbiased_target_on_cell_centres_equals_the_quantised_target():
    """x = 4k with k >= 0, inside the map and up to wholly outside past its far edge.  Negative cell centres are not part of the
    statement: int() truncates toward zero, so the window of x = -4 is centred on (int)(-1 + 0.5) = 0, one cell off the joint,
    and the quantised patch and the Gaussian around the joint differ by the formula itself (the fp64 restatement above covers
    negative coordinates)."""
    from lighthand_amd.heatmap import generate_target, render_targets
    rng = np.random.RandomState(5)
    j = (4.0 * rng.randint(0, 72, size=(3, 21, 2))).astype(F)
    assert (j > 4.0 * 70).any() and (j < 4.0 * 6).any()                    # windows past the far edge and over the near one
    dev = torch.from_numpy(j).cuda()
    sub, quant = render_targets(dev, unbiased=True), render_targets(dev)
    torch.cuda.synchronize()
    assert float((sub - quant).abs().max()) <= 1e-5 and float(quant.max()) == 1.0
    assert torch.equal(sub == 0, quant == 0)
    assert torch.equal(generate_target(j[1], unbiased=True), sub[1].cpu())      # the per-sample form renders the same map


# ------------------------------------------------------------------------------------------------ lh_heatmap_dark
def _blobs(n, h, w, seed):
    """Gaussian blobs, sigma 1.5-3, amplitude 0.3-1, centre at least 4 cells inside, plus noise of 1e-3."""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    cx, cy = rng.uniform(4, w - 5, n), rng.uniform(4, h - 5, n)
    s, a = rng.uniform(1.5, 3.0, n), rng.uniform(0.3, 1.0, n)
    maps = a[:, None, None] * np.exp(-((xs - cx[:, None, None]) ** 2 + (ys - cy[:, None, None]) ** 2) / (2 * s[:, None, None] ** 2))
    return (maps + 1e-3 * rng.randn(n, h, w)).astype(F), np.stack([cx, cy], 1)


def _dark(maps, k, scale=4.0):
    """lh_heatmap_argmax then lh_heatmap_dark through max_preds_device; also the arg-max outputs alone."""
    from lighthand_amd.heatmap import max_preds_device
    hm = torch.from_numpy(maps).cuda()[None]
    before = hm.clone()
    hard, maxvals, idx = max_preds_device(hm, scale=scale)
    got, mv2, idx2 = max_preds_device(hm, scale=scale, post_process="dark", blur_kernel=k)
    again, _, _ = max_preds_device(hm, scale=scale, post_process="dark", blur_kernel=k)
    torch.cuda.synchronize()
    assert _same(hm, before), "the heat-maps were modified"
    assert _same(got, again), "two calls differ"
    assert torch.equal(idx, idx2) and torch.equal(maxvals.isnan(), mv2.isnan()) and _same(maxvals.nan_to_num(), mv2.nan_to_num())
    return got[0], hard[0], maxvals[0, :, 0].cpu().numpy(), idx[0].cpu().numpy()


@pytest.mark.parametrize("k", [11, 3])
@pytest.mark.parametrize("n,h,w", [(42, 64, 64), (12, 17, 23), (1, 96, 96)])
def test_dark_decode_matches_the_fp64_restatement(n, h, w, k):
    """Within 1e-4 cells of the fp64 restatement (fp32 against fp64 on the CPU: at most 4.3e-6 cells on such inputs; x25 for a
    different summation order and the device logf, still three orders of magnitude below the quarter-cell effect).
    Device maximum: not measured yet (the test prints it); an fp32 NumPy restatement in the kernel's order gave 2.4e-6."""
    maps, centres = _blobs(n, h, w, 7 * h + k)
    got, hard, maxvals, idx = _dark(maps, k)
    want, refined = dark_reference(maps, idx, maxvals, hard.cpu().numpy().astype(np.float64) / 4.0, k)
    err = np.abs(got.cpu().numpy().astype(np.float64) / 4.0 - want).max()
    print(f"{n} x {h} x {w}, blur {k}: max |device - fp64| = {err:.3e} cells")
    assert refined.all()
    assert err <= 1e-4
    # and it decodes: closer to the blob centres than the hard arg-max (noise and, for blur 3, little smoothing limit how close)
    if n > 1:                                                                  # one blob may sit on a cell centre by chance
        e_dark = np.abs(got.cpu().numpy() / 4.0 - centres).mean()
        e_hard = np.abs(hard.cpu().numpy() / 4.0 - centres).mean()
        assert e_dark < 0.5 * e_hard, (e_dark, e_hard)


@pytest.mark.parametrize("h,w", [(64, 64), (17, 23)])
def test_dark_leaves_the_arg_max_where_it_does_not_apply(h, w):
    """Peaks within 2 cells of a border, an all-zero / all-negative / constant plane and a plane with a NaN: preds bit-identical
    to lh_heatmap_argmax's.  An interior blob in the same batch moves."""
    rng = np.random.RandomState(h)
    peaks = [(0, 5), (1, 6), (w - 2, 7), (w - 1, 8), (5, 0), (6, 1), (7, h - 2), (8, h - 1), (1, 1), (w - 2, h - 2)]
    maps = (1e-3 * rng.rand(len(peaks) + 5, h, w)).astype(F)
    for i, (x, y) in enumerate(peaks):
        maps[i, y, x] = 1.0
    n = len(peaks)
    maps[n] = 0.0
    maps[n + 1] = -np.abs(maps[n + 1]) - 0.125
    maps[n + 2] = 0.75
    maps[n + 3, 9, 9], maps[n + 3, 3, 4] = 1.0, np.nan
    maps[n + 4] = _blobs(1, h, w, 3)[0][0]
    for k in (11, 3):
        got, hard, maxvals, idx = _dark(maps, k)
        assert _same(got[:n + 4], hard[:n + 4]), k
        assert not torch.equal(got[n + 4], hard[n + 4]), k
        assert [(int(i) % w, int(i) // w) for i in idx[:n]] == peaks
        assert maxvals[n] == 0 and maxvals[n + 1] < 0 and idx[n + 2] == 0 and np.isnan(maxvals[n + 3])


def test_round_trip_of_unbiased_targets_through_the_dark_decode():
    """400 seeded joints whose patch lies fully inside the 64 x 64 map: render_targets(unbiased=True) -> max_preds_device("dark")
    returns them within 0.01 input px (fp64 on the CPU: 0.0017; x6 for fp32 on the device); the hard arg-max of the same maps is
    off by more than 0.5 px on average."""
    from lighthand_amd.heatmap import max_preds_device, render_targets
    joints = np.random.RandomState(2020).uniform(4 * 6.5, 4 * 56.5, size=(20, 20, 2)).astype(F)
    maps = render_targets(torch.from_numpy(joints).cuda(), unbiased=True)
    dark, _, _ = max_preds_device(maps, scale=4.0, post_process="dark")
    hard, _, _ = max_preds_device(maps, scale=4.0)
    torch.cuda.synchronize()
    e_dark, e_hard = np.abs(dark.cpu().numpy() - joints), np.abs(hard.cpu().numpy() - joints)
    print(f"round trip: DARK max {e_dark.max():.5f} mean {e_dark.mean():.5f} px; arg-max max {e_hard.max():.3f} mean {e_hard.mean():.3f} px")
    assert e_dark.max() <= 0.01
    assert e_hard.mean() > 0.5


# ------------------------------------------------------------------------------------------------ steps
def _r18(precision="fp32", seed=5):
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    torch.manual_seed(seed)
    return get_pose_net(resnet_cfg(18), True).cuda().set_precision(precision)


def _run(step, x):
    step(x)
    torch.cuda.synchronize()
    return step.preds.clone(), step.maxvals.clone(), step.heatmaps.clone()


def test_infer_step_dark_decode(monkeypatch):
    """R18, batch 2, 128^2, captured: post_process="dark" gives the bits of the eager max_preds_device on step.heatmaps; with the
    flip test those of flip_merge_device followed by the DARK launch; post_process=True is still the quarter-pixel rule."""
    from lighthand_amd import _lib
    from lighthand_amd.heatmap import dark_refine_device, flip_merge_device, max_preds_device
    from lighthand_amd.runtime import InferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _r18().eval()
    b, h, w = 2, 128, 128
    x = torch.from_numpy(np.random.RandomState(5).randn(b, 3, h, w).astype(F)).cuda()
    p, mv, hm = _run(InferStep(model, b, h, w, post_process="dark"), x)
    want, wmv, _ = max_preds_device(hm, scale=4.0, post_process="dark")
    hard, _, idx = max_preds_device(hm, scale=4.0)
    torch.cuda.synchronize()
    assert _same(p, want) and _same(mv, wmv) and not torch.equal(p, hard)
    # flip test: the DARK launch reads the merged maps
    pf, mvf, hmf = _run(InferStep(model, b, h, w, flip_test=True, post_process="dark"), x)
    _, _, ha = _run(InferStep(model, b, h, w), x)
    _, _, hf = _run(InferStep(model, b, h, w), torch.flip(x, [3]))
    wp, wmv, widx, merged = flip_merge_device(ha, hf, shift=True, scale=4.0)
    unrefined = wp.clone()
    dark_refine_device(merged, widx, wmv, wp, scale=4.0)
    torch.cuda.synchronize()
    assert _same(hmf, merged) and _same(pf, wp) and _same(mvf, wmv) and not torch.equal(wp, unrefined)
    # True keeps its meaning: lh_heatmap_refine on the arg-max of the same maps
    pq, _, hq = _run(InferStep(model, b, h, w, post_process=True), x)
    quarter = hard.clone()
    _lib.check(_lib.load().lh_heatmap_refine(hq.data_ptr(), idx.data_ptr(), mv.data_ptr(), b * 21, 32, 32, 4.0, quarter.data_ptr(),
                                             _stream()), "lh_heatmap_refine")
    named, _, _ = max_preds_device(hq, scale=4.0, post_process="quarter")
    torch.cuda.synchronize()
    assert _same(hq, hm) and _same(pq, quarter) and _same(pq, named) and not torch.equal(pq, p)


def _batch(b, size, seed):
    rng = np.random.RandomState(seed)
    return (torch.from_numpy(rng.randn(b, 3, size, size).astype(F)).cuda(),
            torch.from_numpy(rng.uniform(8, size - 8, size=(b, 21, 2)).astype(F)).cuda())


def test_train_step_unbiased_encoding(monkeypatch):
    """R18, batch 4, 128^2, static kernel choice: after one step step.target is render_targets(joints, unbiased=True) bit for bit,
    and the captured and the eager step report the same loss bits."""
    from lighthand_amd.heatmap import render_targets
    from lighthand_amd.runtime import TrainStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    x, j = _batch(4, 128, 31)
    want = render_targets(j, size=32, unbiased=True)
    losses = []
    for graph in (True, False):
        st = TrainStep(_r18(), 4, 128, 128, lr=1e-3, target_encoding="unbiased", use_graph=graph)
        loss = st(x, j).clone()
        torch.cuda.synchronize()
        assert _same(st.target, want), graph
        assert np.isfinite(float(loss))
        losses.append(loss)
    assert _same(losses[0], losses[1]), [float(v) for v in losses]
    assert not _same(want, render_targets(j, size=32))


def test_train_step_default_encoding_is_the_quantised_target(monkeypatch):
    from lighthand_amd.heatmap import render_targets
    from lighthand_amd.runtime import TrainStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    x, j = _batch(4, 128, 32)
    st = TrainStep(_r18(), 4, 128, 128, lr=1e-3)
    st(x, j)
    torch.cuda.synchronize()
    assert st.target_encoding == "quantised" and _same(st.target, render_targets(j, size=32))


def test_train_step_unbiased_encoding_with_warp_and_target_weight(monkeypatch):
    """geometric_aug + use_target_weight + the unbiased encoding in one captured step: target and weight are rendered from
    step.joints_aug (the warped joints) and the caller's visibility."""
    from lighthand_amd.heatmap import render_targets
    from lighthand_amd.runtime import TrainStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    geo = {"rotation": 30.0, "scale": 0.3, "shift": 0.3, "generator": torch.Generator().manual_seed(21)}
    st = TrainStep(_r18("bf16"), 4, 128, 128, lr=1e-3, input_u8=(100, 112), geometric_aug=geo, use_target_weight=True,
                   target_encoding="unbiased")
    rng = np.random.RandomState(33)
    x = torch.from_numpy(rng.randint(0, 256, size=(4, 100, 112, 3)).astype(np.uint8)).cuda()
    j = torch.from_numpy(np.concatenate([rng.uniform(0, 128, size=(4, 21, 2)), rng.rand(4, 21, 1) > 0.2], -1).astype(F)).cuda()
    loss = st(x, j)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
    assert not torch.equal(st.joints_aug, st.joints) and torch.equal(st.joints, j[..., :2])
    want, want_w = render_targets(torch.cat([st.joints_aug, j[..., 2:]], -1), size=32, return_weight=True, unbiased=True)
    assert _same(st.target, want) and _same(st.target_weight, want_w)
    assert float(want_w.min()) == 0.0 and float(want_w.max()) == 1.0
