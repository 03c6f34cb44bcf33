"""The three fused, persistent MFMA kernels -- lh_stem_pool, lh_stem_conv (csrc/stem_pool.hip) and lh_bottleneck_infer
(csrc/bottleneck_infer_kernel.h) -- straight through the C ABI, bf16 and fp16, in two legs.

Exact leg.  Integer operands and power-of-two scales (tests/exact_data.py; tests/test_exact_host.py proves on the CPU that every sum any
kernel order can form is exact in fp32): the stored 16-bit values must equal ONE round-to-nearest-even of the fp64 reference at each of
the kernel's storage points, compared as int16 bit patterns, tolerance zero -- a zero must be +0.  The references are plain restatements:
F.conv2d / matrix products in fp64, F.relu, F.max_pool2d over the rounded values.  lh_stem_conv's statistics slab is held row by row to
the fp64 sums over the pixels the kernel's tile loop gives each workgroup ("stats" flavour: both rows exact; "exact" flavour: the sums row
is exact, the sums of squares of values that need roundings cannot stay below 2^24 and take the rtol rule of
tests/test_gpu_epilogue_modes.py).

Shapes: less than one tile; ragged in both directions (odd and even convolution sizes, one-pixel last tiles); and a multi-tile case with
more than twice as many tiles as the launch has workgroups and a tile count that is no multiple of the grid -- asserted against the
library's grid queries (lh_stem_pool_grid, lh_stem_conv_rows, lh_bottleneck_infer_grid) -- so that the persistent loops, the register
prefetch of the next tile, the zero-filled prefetch behind the last tile and the bottleneck's LDS-DMA ring across tile boundaries all
run: cin = 64, 96, 160, 256 give 7, 8, 10, 13 ring stages per tile, every residue of the four-slot ring.

Second leg.  Normal random operands, general scales and shifts, the multi-tile shapes: the fused launch must equal the launches it
replaces BIT FOR BIT on the same packs (lh_igemm + lh_maxpool3x3s2_fwd; lh_igemm; three lh_igemm launches with the residual as the third
one's addend) -- the promise of include/lighthand_hip.h.

Every output buffer is pre-filled with NaN and stands between two 2 KiB sentinel margins that must come back untouched."""
import ctypes as C

import pytest
import torch

import exact_data as E

pytestmark = pytest.mark.gpu

_TD = {"bf16": torch.bfloat16, "fp16": torch.float16}
_DT = {"bf16": 1, "fp16": 2}                       # LH_BF16, LH_F16
SENTINEL = 7.0
MARGIN_BYTES = 2048
_T3 = [(r - 1, s - 1) for r in range(3) for s in range(3)]


def _lib():
    from lighthand_amd import _lib
    return _lib, _lib.load()


def _guarded(numel, dtype):
    """(whole buffer, the NaN-filled output inside it, margin in elements): the output between two sentinel margins of 2 KiB."""
    m = MARGIN_BYTES // torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((numel + 2 * m,), SENTINEL, dtype=dtype, device="cuda")
    buf[m:m + numel] = float("nan")
    return buf, buf[m:m + numel], m


def _margins_untouched(buf, m):
    return bool((buf[:m].float() == SENTINEL).all()) and bool((buf[-m:].float() == SENTINEL).all())


def _assert_same_bits(got, want, what):
    """Two 16-bit tensors of one shape, as int16 bit patterns."""
    g, w = got.cpu().contiguous().view(torch.int16), want.cpu().contiguous().view(torch.int16)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    if bool(bad.any()):
        first = tuple(int(v) for v in bad.nonzero()[0])
        zero = bad & ((g & 0x7fff) == 0) & ((w & 0x7fff) == 0)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} stored values differ, first at {first}: {float(got.cpu()[first])} against "
                             f"{float(want.cpu()[first])}; {int(zero.sum())} of them in the sign of a zero only")


def _pack(w, n_out, n_in, strides, taps_rs, precision):
    """lh_pack_weight of an fp32 device tensor -> the uint8 pack image."""
    L, lib = _lib()
    arr = (C.c_int * (2 * len(taps_rs)))(*[v for t in taps_rs for v in t])
    need = C.c_size_t(0)
    L.check(lib.lh_pack_weight(None, None, C.byref(need), n_out, n_in, *strides, len(taps_rs), arr, _DT[precision], None), "lh_pack_weight size")
    out = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    L.check(lib.lh_pack_weight(w.data_ptr(), out.data_ptr(), None, n_out, n_in, *strides, len(taps_rs), arr, _DT[precision], None), "lh_pack_weight")
    torch.cuda.synchronize()
    return out


def _desc(n, hi, wi, stride, k_run, ho, wo, s, cout, taps, relu):
    from lighthand_amd.graph import _desc as make
    d = make(n, hi, wi, stride, k_run, ho, wo, s, s, cout, ho, wo, 1, 1, 0, 0, cout, taps)
    d.relu = relu
    return d


def _igemm(d, src, pack, dst, addend, bias, scale, shift, stats, precision, what):
    L, lib = _lib()
    p = lambda t: None if t is None else t.data_ptr()
    L.check(lib.lh_igemm(C.byref(d), src.data_ptr(), pack.data_ptr(), dst.data_ptr(), p(addend), None, p(bias), p(scale), p(shift), p(stats),
                         _DT[precision], None), what)


# ------------------------------------------------------------------------------------------------ the stem
_STEM = {}


def _stem_operands(x, w, precision):
    """Device operands of the stem kernels from an NCHW image and the [64][3][7][7] weights (values the run precision holds): the padded
    NHWC4 image and the pack lh_pack_weight makes of the staging tensor with one tap per kernel row, as engine.Plan._c_stem does -- held
    against the layout stem_pool.hip documents ([64 pad 128][7 kernel rows][64 elements], 32 of them the K run)."""
    td = _TD[precision]
    img, stage = E.fused_stem_layout(x, w)
    assert torch.equal(img.to(td).float(), img.float())
    pack = _pack(stage.float().contiguous().cuda(), 64, 32, (7 * 32, 1, 32, 0), [(r, 0) for r in range(7)], precision)
    want = torch.zeros(128, 7, 64, dtype=td)
    want[:64, :, :32] = stage.reshape(64, 7, 32).to(td)
    _assert_same_bits(pack.view(td).view(128, 7, 64), want, "stem weight pack")
    return img.to(td).contiguous().cuda(), pack


def _stem_case(image, precision, flavour):
    """Operands on the device and what the kernels must store (host, 16-bit), made once per case."""
    key = (image, precision, flavour)
    if key not in _STEM:
        for k in [k for k in _STEM if k[0] == "multi" and k != key]:      # one multi-tile case at a time
            del _STEM[k]
        d = E.fused_stem_data(image, precision, flavour)
        r = E.fused_stem_reference(d, precision)
        E.fused_stem_check(d, r)
        img, pack = _stem_operands(d["x"], d["w"], precision)
        dev = dict(img=img, pack=pack, bias=d["bias"].cuda(), scale=d["scale"].cuda(), shift=d["shift"].cuda())
        _STEM[key] = (dev, {k: r[k] for k in ("conv16", "pooled", "s1", "s2")})
    return _STEM[key]


def _run_stem_pool(dev, image, precision):
    L, lib = _lib()
    n, h, w, hp, wp, ch, cw, ph, pw = E.fused_stem_sizes(image)
    buf, out, m = _guarded(n * ph * pw * 64, _TD[precision])
    L.check(lib.lh_stem_pool(dev["img"].data_ptr(), n, hp, wp, dev["pack"].data_ptr(), dev["bias"].data_ptr(), dev["scale"].data_ptr(),
                             dev["shift"].data_ptr(), out.data_ptr(), ch, cw, 1, _DT[precision], None), "lh_stem_pool")
    torch.cuda.synchronize()
    assert _margins_untouched(buf, m), "lh_stem_pool wrote a margin of its output"
    return out.view(n, ph, pw, 64)


def _run_stem_conv(dev, image, precision):
    L, lib = _lib()
    n, h, w, hp, wp, ch, cw, ph, pw = E.fused_stem_sizes(image)
    rows = lib.lh_stem_conv_rows(n, ch, cw)
    buf, out, m = _guarded(n * ch * cw * 64, _TD[precision])
    sbuf, stats, sm = _guarded(rows * 2 * 64, torch.float32)
    L.check(lib.lh_stem_conv(dev["img"].data_ptr(), n, hp, wp, dev["pack"].data_ptr(), out.data_ptr(), stats.data_ptr(), ch, cw, _DT[precision], None),
            "lh_stem_conv")
    torch.cuda.synchronize()
    assert _margins_untouched(buf, m) and _margins_untouched(sbuf, sm), "lh_stem_conv wrote a margin of its output or of its statistics"
    assert not bool(torch.isnan(stats).any()), "a statistics row was not written"
    return out.view(n, ch, cw, 64), stats.view(rows, 2, 64).cpu()


def _walks(tiles, grid, what):
    """The multi-tile condition: more than two tiles per workgroup on average, and no multiple of the grid."""
    most = -(-tiles // grid)
    print(f"{what}: {tiles} tiles on {grid} workgroups: {tiles % grid} of them take {most} tiles, the others {tiles // grid}")
    assert tiles > 2 * grid and tiles % grid != 0 and most >= 3, (what, tiles, grid)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("image", list(E.FUSED_STEM_IMAGES))
def test_stem_pool_stores_the_rounded_reference(image, precision):
    """lh_stem_pool against conv (fp64) -> relu(acc * scale + (bias * scale + shift)) -> one rounding -> F.max_pool2d(3, 2, 1), bit for bit;
    a dead channel stores +0 everywhere (stem_pool.hip clears the sign on purpose)."""
    _, lib = _lib()
    dev, want = _stem_case(image, precision, "exact")
    n, h, w, hp, wp, ch, cw, ph, pw = E.fused_stem_sizes(image)
    if image == "multi":
        _walks(n * -(-ph // 8) * -(-pw // 8), lib.lh_stem_pool_grid(n, ch, cw), "lh_stem_pool")
    out = _run_stem_pool(dev, image, precision)
    _assert_same_bits(out, want["pooled"], f"lh_stem_pool {image} {precision}")
    assert bool((out[..., E.FUSED_STEM_DEAD].view(torch.int16) == 0).all())


@pytest.mark.parametrize("flavour", ["exact", "stats"])
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("image", list(E.FUSED_STEM_IMAGES))
def test_stem_conv_stores_the_rounded_convolution_and_its_sums(image, precision, flavour):
    """lh_stem_conv: the raw convolution rounded once, bit for bit; one statistics row per workgroup (lh_stem_conv_rows), each the sums
    over exactly the pixels of the tiles the kernel's loop gives that workgroup (module docstring for what is exact in which flavour)."""
    _, lib = _lib()
    dev, want = _stem_case(image, precision, flavour)
    n, h, w, hp, wp, ch, cw, ph, pw = E.fused_stem_sizes(image)
    rows = lib.lh_stem_conv_rows(n, ch, cw)
    if image == "multi":
        _walks(n * -(-ch // 16) * -(-cw // 16), rows, "lh_stem_conv")
    out, stats = _run_stem_conv(dev, image, precision)
    assert stats.shape[0] == rows
    _assert_same_bits(out, want["conv16"], f"lh_stem_conv {image} {precision} {flavour}")
    v = want["conv16"].double().reshape(-1, 64)
    rid = E.stem_conv_row_of_pixel(n, ch, cw, rows).reshape(-1)
    for which, term in ((0, v), (1, v * v)):
        per_row = torch.zeros(rows, 64, dtype=torch.float64).index_add_(0, rid, term)
        worst = float(torch.zeros(rows, 64, dtype=torch.float64).index_add_(0, rid, term.abs()).max())      # the largest row's sum of magnitudes
        holds = worst < E.LIMIT
        assert holds or (which == 1 and flavour == "exact"), (which, worst)
        got = stats[:, which].double()
        if holds:
            assert torch.equal(got, per_row), (which, "a statistics row differs from the sums over its workgroup's pixels")
            assert torch.equal(got.sum(0), want["s2" if which else "s1"])
        else:
            assert torch.allclose(got.sum(0), term.sum(0), rtol=2e-3, atol=2e-3 * float(term.abs().sum(0).max())), which


def _random_stem(precision):
    """Normal random operands of the multi-tile image, general affine (no powers of two), rounded to the run precision."""
    key = ("random", precision)
    if key not in _STEM:
        for k in [k for k in _STEM if k[0] in ("multi", "random") and k != key]:
            del _STEM[k]
        td = _TD[precision]
        n, h, w = E.FUSED_STEM_IMAGES["multi"]
        g = torch.Generator().manual_seed(4321)
        x = torch.randn(n, 3, h, w, generator=g).to(td).float()
        wt = (torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5).to(td).float()
        img, pack = _stem_operands(x, wt, precision)
        sign = 2.0 * torch.randint(0, 2, (64,), generator=g) - 1.0
        _STEM[key] = dict(img=img, pack=pack, bias=(torch.randn(64, generator=g) * 0.3).cuda(), scale=((torch.rand(64, generator=g) + 0.5) * sign).cuda(),
                          shift=(torch.randn(64, generator=g) * 0.3).cuda())
    return _STEM[key]


def _stem_desc(image, relu):
    n, h, w, hp, wp, ch, cw, ph, pw = E.fused_stem_sizes(image)
    return _desc(n, hp, wp, 4, 32, ch, cw, 2, 64, [(r, 0) for r in range(7)], relu)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_stem_pool_equals_convolution_then_pool_bit_for_bit(precision):
    """Random data, several tiles per workgroup: lh_stem_pool = lh_igemm (bias, affine, ReLU) followed by lh_maxpool3x3s2_fwd on the same pack."""
    L, lib = _lib()
    dev = _random_stem(precision)
    n, h, w, hp, wp, ch, cw, ph, pw = E.fused_stem_sizes("multi")
    _walks(n * -(-ph // 8) * -(-pw // 8), lib.lh_stem_pool_grid(n, ch, cw), "lh_stem_pool")
    fused = _run_stem_pool(dev, "multi", precision)
    abuf, act, am = _guarded(n * ch * cw * 64, _TD[precision])
    _igemm(_stem_desc("multi", 1), dev["img"], dev["pack"], act, None, dev["bias"], dev["scale"], dev["shift"], None, precision, "lh_igemm stem")
    pbuf, pooled, pm = _guarded(n * ph * pw * 64, _TD[precision])
    L.check(lib.lh_maxpool3x3s2_fwd(act.data_ptr(), pooled.data_ptr(), None, n, ch, cw, 64, _DT[precision], None), "lh_maxpool3x3s2_fwd")
    torch.cuda.synchronize()
    assert _margins_untouched(abuf, am) and _margins_untouched(pbuf, pm)
    assert float((pooled.float() > 0).float().mean()) > 0.5
    _assert_same_bits(fused, pooled.view(n, ph, pw, 64), f"lh_stem_pool against lh_igemm + lh_maxpool3x3s2_fwd, {precision}")


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_stem_conv_equals_the_tiled_convolution_bit_for_bit(precision):
    """Random data, several tiles per workgroup: lh_stem_conv's output = lh_igemm's on the same pack; its statistics rows add up to the sums
    of the stored values (rtol rule of tests/test_gpu_epilogue_modes.py: random data is not exact)."""
    _, lib = _lib()
    dev = _random_stem(precision)
    n, h, w, hp, wp, ch, cw, ph, pw = E.fused_stem_sizes("multi")
    _walks(n * -(-ch // 16) * -(-cw // 16), lib.lh_stem_conv_rows(n, ch, cw), "lh_stem_conv")
    out, stats = _run_stem_conv(dev, "multi", precision)
    tbuf, tiled, tm = _guarded(n * ch * cw * 64, _TD[precision])
    _igemm(_stem_desc("multi", 0), dev["img"], dev["pack"], tiled, None, None, None, None, None, precision, "lh_igemm stem")
    torch.cuda.synchronize()
    assert _margins_untouched(tbuf, tm)
    _assert_same_bits(out, tiled.view(n, ch, cw, 64), f"lh_stem_conv against lh_igemm, {precision}")
    v = out.double().reshape(-1, 64)
    for which, term in ((0, v), (1, v * v)):
        assert torch.allclose(stats[:, which].double().sum(0), term.sum(0).cpu(), rtol=2e-3, atol=2e-3 * float(term.abs().sum(0).max())), which


# ------------------------------------------------------------------------------------------------ the bottleneck
def _bneck_operands(d, precision):
    """Device operands of lh_bottleneck_infer and of the three lh_igemm launches from fp64 / fp32 host tensors (exact_data.bneck_data's
    layout): activations in the run precision, packs from lh_pack_weight with the engine's strides and (r, s) tap order, fp32 affines."""
    td = _TD[precision]
    cin = d["x"].shape[-1]
    dev = dict(x=d["x"].to(td).contiguous().cuda(), res=d["res"].to(td).contiguous().cuda())
    dev["w1"] = _pack(d["w1"].float().contiguous().cuda(), 64, cin, (cin, 1, 1, 1), [(0, 0)], precision)
    dev["w2"] = _pack(d["w2"].float().contiguous().cuda(), 64, 64, (64 * 9, 9, 3, 1), [(r, s) for r in range(3) for s in range(3)], precision)
    dev["w3"] = _pack(d["w3"].float().contiguous().cuda(), 256, 64, (64, 1, 1, 1), [(0, 0)], precision)
    assert dev["w1"].numel() == 128 * ((cin + 63) // 64 * 64) * 2 and dev["w2"].numel() == 128 * 9 * 64 * 2 and dev["w3"].numel() == 256 * 64 * 2
    for l in (1, 2, 3):
        dev[f"s{l}"], dev[f"b{l}"] = d[f"s{l}"].float().cuda(), d[f"b{l}"].float().cuda()
    return dev


def _run_bottleneck(dev, cin, shape, precision, residual):
    L, lib = _lib()
    n, h, w = E.BNECK_SHAPES[shape]
    bd = L.BottleneckDesc(n, h, w, cin, 64, 256)
    buf, out, m = _guarded(n * h * w * 256, _TD[precision])
    L.check(lib.lh_bottleneck_infer(C.byref(bd), dev["x"].data_ptr(), dev["w1"].data_ptr(), dev["w2"].data_ptr(), dev["w3"].data_ptr(),
                                    dev["s1"].data_ptr(), dev["b1"].data_ptr(), dev["s2"].data_ptr(), dev["b2"].data_ptr(), dev["s3"].data_ptr(),
                                    dev["b3"].data_ptr(), residual.data_ptr(), out.data_ptr(), _DT[precision], None), "lh_bottleneck_infer")
    torch.cuda.synchronize()
    assert _margins_untouched(buf, m), "lh_bottleneck_infer wrote a margin of its output"
    return out.view(n, h, w, 256)


def _bneck_walks(cin, shape):
    L, lib = _lib()
    n, h, w = E.BNECK_SHAPES[shape]
    grid = lib.lh_bottleneck_infer_grid(C.byref(L.BottleneckDesc(n, h, w, cin, 64, 256)))
    _walks(n * -(-h // 16) * -(-w // 16), grid, f"lh_bottleneck_infer, {cin // 32 + 5} ring stages per tile")


_BNECK_RUNS = [(cin, shape, res) for cin in E.BNECK_CIN for shape in E.BNECK_SHAPES for res in (("separate", "x") if cin == 256 else ("separate",))]


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("cin,shape,res", _BNECK_RUNS)
def test_bottleneck_stores_the_rounded_reference(cin, shape, res, precision):
    """lh_bottleneck_infer against exact_data.bneck_reference -- a rounding behind each of the three convolutions and behind the residual
    sum, conv2 reading zeros outside the image -- bit for bit; cin = 256 also as an identity block (residual = x, the same pointer)."""
    d = E.bneck_data(cin, shape, precision)
    r = E.bneck_reference(d, precision, d["x"] if res == "x" else None)
    E.bneck_check(d, r)
    dev = _bneck_operands(d, precision)
    if shape == "multi":
        _bneck_walks(cin, shape)
    out = _run_bottleneck(dev, cin, shape, precision, dev["x"] if res == "x" else dev["res"])
    _assert_same_bits(out, r["out"].float().to(_TD[precision]), f"lh_bottleneck_infer cin {cin} {shape} residual {res} {precision}")


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("cin,res", [(c, "separate") for c in E.BNECK_CIN] + [(256, "x")])
def test_bottleneck_equals_its_three_launches_bit_for_bit(cin, res, precision):
    """Random data, several tiles per workgroup, every ring residue: lh_bottleneck_infer = lh_igemm (1x1, affine, ReLU) -> lh_igemm (3x3,
    affine, ReLU) -> lh_igemm (1x1, affine, residual as the addend, ReLU) on the same packs."""
    td = _TD[precision]
    n, h, w = E.BNECK_SHAPES["multi"]
    g = torch.Generator().manual_seed(5000 + cin)
    d = dict(x=torch.randn(n, h, w, cin, generator=g).to(td).float(), res=torch.randn(n, h, w, 256, generator=g).to(td).float(),
             w1=(torch.randn(64, cin, generator=g) / cin ** 0.5).to(td).float(), w2=(torch.randn(64, 64, 3, 3, generator=g) / 24.0).to(td).float(),
             w3=(torch.randn(256, 64, generator=g) / 8.0).to(td).float())
    for l, c in ((1, 64), (2, 64), (3, 256)):
        d[f"s{l}"] = (torch.rand(c, generator=g) + 0.5) * (2.0 * torch.randint(0, 2, (c,), generator=g) - 1.0)
        d[f"b{l}"] = torch.randn(c, generator=g) * 0.3
    dev = _bneck_operands(d, precision)
    residual = dev["x"] if res == "x" else dev["res"]
    _bneck_walks(cin, "multi")
    fused = _run_bottleneck(dev, cin, "multi", precision, residual)
    b1, a1, m1 = _guarded(n * h * w * 64, td)
    b2, a2, m2 = _guarded(n * h * w * 64, td)
    b3, out, m3 = _guarded(n * h * w * 256, td)
    _igemm(_desc(n, h, w, cin, cin, h, w, 1, 64, [(0, 0)], 1), dev["x"], dev["w1"], a1, None, None, dev["s1"], dev["b1"], None, precision, "lh_igemm conv1")
    _igemm(_desc(n, h, w, 64, 64, h, w, 1, 64, _T3, 1), a1, dev["w2"], a2, None, None, dev["s2"], dev["b2"], None, precision, "lh_igemm conv2")
    _igemm(_desc(n, h, w, 64, 64, h, w, 1, 256, [(0, 0)], 1), a2, dev["w3"], out, residual, None, dev["s3"], dev["b3"], None, precision, "lh_igemm conv3")
    torch.cuda.synchronize()
    assert _margins_untouched(b1, m1) and _margins_untouched(b2, m2) and _margins_untouched(b3, m3)
    assert 0.2 < float((out.float() > 0).float().mean()) < 0.8
    _assert_same_bits(fused, out.view(n, h, w, 256), f"lh_bottleneck_infer against three lh_igemm launches, cin {cin} residual {res} {precision}")
