"""Every mode of the tiled convolution kernel's epilogue (igemm_epilogue.h) on every tile form, straight through the C ABI.

The BatchNorm-backward gate is compiled into kernels of its own (igemm_ring_gated_kernel); the plain kernel carries none of it.  Both are
driven here with the configuration forced through lh_igemm_desc.cfg: plain, statistics rows, addend, addend + mask, ReLU, gate from x,
gate from mask bits, gate + addend -- on the 256 x 256, 128 x 256, 128 x 128 dense-wave and 64 x 64 forms, bf16 and fp16.  All forms share
one K order and one epilogue, so the stored outputs agree BIT FOR BIT between them; each is also held against a host fp32 evaluation of the
same descriptor.

Shapes: batch 2, 3x3 stride 1, 40 -> 72 channels at 13 x 11 (286 pixels: a ragged second 256-pixel tile; 72 channels fill neither a 128 nor
a 256 tile).  The library refuses the 256-channel tile for 72 channels (weight packs are padded to 128 rows: one block, a 256-row tile would
read past it -- cfg_safe, igemm_ring.hip), so that shape runs on the other three forms, the refusal is asserted, and the same convolution
with 136 channels (two blocks; still fills neither tile) runs on all four.  The third case is one sub-pixel phase of a stride-2 transposed
convolution: 2 x 2 taps, output pixel (2a + 1, 2b) of an 18 x 14 image -- the epilogue's strided (non-dense) placement; the pixels of the
other phases keep what the buffer held.

Statistics rows: a launch writes one row per pixel tile, so forms with different tile pixels write different row COUNTS and cannot be
compared row by row; forms that share the pixel tile (256 x 256 and 128 x 256) are compared bit for bit, and every form's column totals are
held to the stored values as tests/test_gpu_ops.py's gate test does (rtol = 2e-3, atol = 2e-3 x the largest column's sum of magnitudes).

Data flavours.  "random": normal operands, the assertions above.  "exact" and "exact_small" (tests/exact_data.py): integer x, w, addend and
BN input, integer mean and shift, invstd and scale from {0.5, 1, 2} -- every accumulator and every epilogue sum is exact in fp32, so the
stored outputs must equal _host(...) BIT FOR BIT (compared as int16) in every mode on every form: the accumulator rounded to 16 bits, the
addend added in fp32, the sum rounded again, then ReLU, then the gate (igemm_epilogue.h).  A statistics row is exact as well wherever the
sums of magnitudes of its terms stay below 2^24: then the fp64 sum of the slab rows EQUALS the fp64 sums over the stored values.  That
holds for every row of "exact_small" (asserted) and for the rows of "exact" whose bound holds on the host values (sums: always; sums of
squares of values that need rounding cannot stay below 2^24, see exact_data.EPILOGUE_RANGES -- those rows keep the rtol check)."""
import ctypes as C

import pytest
import torch

import exact_data as E

pytestmark = pytest.mark.gpu

TOL = {"bf16": 3e-2, "fp16": 4e-3}                 # tests/test_gpu_ops.py
_TD = {"bf16": torch.bfloat16, "fp16": torch.float16}
_DT = {"bf16": 1, "fp16": 2}                       # LH_BF16, LH_F16
FORMS = {"256x256": (256, 256, 2, 128), "128x256": (128, 256, 3, 64), "128x128 dense": (128, 128, 22, 128), "64x64": (64, 64, 2, 64)}
MODES = ["plain", "stats", "addend", "addend_mask", "relu", "gate_x", "gate_mask", "gate_addend"]
SENTINEL = 7.0

# name -> (n, hi, wi, cin, ho, wo, cout, OH, OW, osh, osw, ooh, oow, taps (dh, dw), forms)
_T3 = [(r - 1, s - 1) for r in range(3) for s in range(3)]
CASES = {
    "c72": (2, 13, 11, 40, 13, 11, 72, 13, 11, 1, 1, 0, 0, _T3, ["128x256", "128x128 dense", "64x64"]),
    "c136": (2, 13, 11, 40, 13, 11, 136, 13, 11, 1, 1, 0, 0, _T3, list(FORMS)),
    "phase": (2, 9, 7, 40, 9, 7, 136, 18, 14, 2, 2, 1, 0, [(1, 0), (1, -1), (0, 0), (0, -1)], list(FORMS)),
}


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _desc(case, form):
    from lighthand_amd import _lib
    n, hi, wi, cin, ho, wo, cout, OH, OW, osh, osw, ooh, oow, taps, _ = CASES[case]
    d = _lib.IgemmDesc()
    d.n, d.hi, d.wi, d.in_pix_stride, d.k_run = n, hi, wi, cin, cin
    d.ho, d.wo, d.sh, d.sw, d.cout = ho, wo, 1, 1, cout
    d.OH, d.OW, d.osh, d.osw, d.ooh, d.oow, d.out_pix_stride = OH, OW, osh, osw, ooh, oow, cout
    d.ntaps, d.relu = len(taps), 0
    for t, (dh, dw) in enumerate(taps):
        d.dh[t], d.dw[t] = dh, dw
    for i, v in enumerate(FORMS[form]):
        d.cfg[i] = v
    return d


_DATA = {}


def _data(case, precision, flavour="random"):
    """Operands (on the device, rounded to the run precision) and the host fp32 accumulator of one case: made once, never changed."""
    key = (case, precision, flavour)
    if key in _DATA:
        return _DATA[key]
    n, hi, wi, cin, ho, wo, cout, OH, OW, osh, osw, ooh, oow, taps, _ = CASES[case]
    td = _TD[precision]
    P = OH * OW * n
    if flavour == "random":
        g = torch.Generator().manual_seed(1234 + len(case))
        x = torch.randn(n, hi, wi, cin, generator=g).to(td)
        w = (torch.randn(cout, len(taps), cin, generator=g) / (len(taps) * cin) ** 0.5).to(td)
        addend = torch.randn(P, cout, generator=g).to(td)
        gx = torch.randn(P, cout, generator=g).to(td)
        amask = torch.randint(0, 256, (P * cout // 8,), generator=g, dtype=torch.uint8)
        gmask = torch.randint(0, 256, (P * cout // 8,), generator=g, dtype=torch.uint8)
        mean, shift = torch.randn(cout, generator=g) * 0.3, torch.randn(cout, generator=g) * 0.3
        invstd, scale = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    else:
        assert CASES[case][:14] == E.EPILOGUE_CASES[case]
        d = E.epilogue_data(case, precision, flavour)
        E.check_exact_epilogue(case, d)                  # every sum of magnitudes below 2^24: the accumulator is exact in any order
        x, w, addend, gx = (d[k].to(td) for k in ("x", "w", "addend", "gx"))
        assert all(torch.equal(t.float(), d[k]) for t, k in ((x, "x"), (w, "w"), (addend, "addend"), (gx, "gx")))
        amask, gmask, mean, shift, invstd, scale = (d[k] for k in ("amask", "gmask", "mean", "shift", "invstd", "scale"))
    # host fp32: acc[n][a][b][co] = sum_t sum_k x[n][a + dh_t][b + dw_t][k] * w[co][t][k], zero outside the image
    acc = E.tap_conv(x.float(), w.float(), taps, ho, wo)
    # the weight pack: [rows padded to 128][taps][K padded to 128 bytes], zero padding
    kpad = (cin * 2 + 127) // 128 * 64
    pack = torch.zeros((cout + 127) // 128 * 128, len(taps), kpad, dtype=td)
    pack[:cout, :, :cin] = w
    # where the launch's pixels sit in the [n][OH][OW] output
    pos = ((torch.arange(n).view(n, 1, 1) * OH + torch.arange(ho).view(1, ho, 1) * osh + ooh) * OW
           + torch.arange(wo).view(1, 1, wo) * osw + oow).reshape(-1)
    bits = torch.arange(8, dtype=torch.uint8).view(1, 8)
    host = dict(acc=acc.reshape(-1, cout), pos=pos, addend=addend.float(), gx=gx.float(), mean=mean, invstd=invstd, scale=scale, shift=shift,
                amask=((amask.view(-1, 1) >> bits) & 1).bool().view(P, cout), gmask=((gmask.view(-1, 1) >> bits) & 1).bool().view(P, cout))
    dev = {k: v.cuda() for k, v in dict(x=x, pack=pack, addend=addend, gx=gx, amask=amask, gmask=gmask, mean=mean, invstd=invstd,
                                        scale=scale, shift=shift).items()}
    _DATA[key] = (host, dev)
    return _DATA[key]


def _host(case, precision, mode, flavour="random"):
    """(expected stored values of the launch's pixels, gate-on mask or None) in fp32 with the epilogue's roundings."""
    h, _ = _data(case, precision, flavour)
    td, pos = _TD[precision], h["pos"]
    v = h["acc"].to(td).float()
    if mode in ("addend", "addend_mask", "gate_addend"):
        a = h["addend"][pos]
        if mode == "addend_mask":
            a = torch.where(h["amask"][pos], a, torch.zeros_like(a))
        v = (v + a).to(td).float()
    if mode == "relu":
        v = v.clamp_min(0.0)
    on = None
    if mode in ("gate_x", "gate_addend"):
        on = (h["gx"][pos] * h["scale"] + h["shift"]) > 0
    elif mode == "gate_mask":
        on = h["gmask"][pos]
    if on is not None:
        v = torch.where(on, v, torch.zeros_like(v))
    return v, on


def _launch(case, precision, mode, form, flavour="random"):
    """One launch -> (whole output buffer, slab rows or None), on the host."""
    from lighthand_amd import _lib
    lib = _lib.load()
    _, dv = _data(case, precision, flavour)
    d = _desc(case, form)
    d.relu = 1 if mode == "relu" else 0
    n, cout, OH, OW = CASES[case][0], CASES[case][6], CASES[case][7], CASES[case][8]
    out = torch.full((n * OH * OW, cout), SENTINEL, dtype=_TD[precision], device="cuda")
    addend = dv["addend"].data_ptr() if mode in ("addend", "addend_mask", "gate_addend") else None
    amask = dv["amask"].data_ptr() if mode == "addend_mask" else None
    slab = None
    if mode.startswith("gate"):
        rows = lib.lh_igemm_gated_rows(C.byref(d), _DT[precision], 1)
        slab = torch.full((rows, 2, cout), float("nan"), device="cuda")
        masked = mode == "gate_mask"
        gate = _lib.BnBwdGate(dv["gx"].data_ptr(), dv["mean"].data_ptr(), dv["invstd"].data_ptr(), None if masked else dv["scale"].data_ptr(),
                              None if masked else dv["shift"].data_ptr(), slab.data_ptr(), dv["gmask"].data_ptr() if masked else None)
        _lib.check(lib.lh_igemm_gated(C.byref(d), dv["x"].data_ptr(), dv["pack"].data_ptr(), out.data_ptr(), addend, amask, C.byref(gate),
                                      _DT[precision], None), f"lh_igemm_gated {case} {mode} {form}")
    else:
        if mode == "stats":
            rows = lib.lh_igemm_stats_rows(C.byref(d), _DT[precision])
            slab = torch.full((rows, 2, cout), float("nan"), device="cuda")
        _lib.check(lib.lh_igemm(C.byref(d), dv["x"].data_ptr(), dv["pack"].data_ptr(), out.data_ptr(), addend, amask, None, None, None,
                                slab.data_ptr() if slab is not None else None, _DT[precision], None), f"lh_igemm {case} {mode} {form}")
    torch.cuda.synchronize()
    return out.cpu(), (slab.cpu() if slab is not None else None)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("case", list(CASES))
def test_epilogue_mode_on_every_tile_form(case, precision, mode):
    _check(case, precision, mode, "random")


@pytest.mark.parametrize("flavour", ["exact", "exact_small"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("case", list(CASES))
def test_epilogue_mode_exact_on_every_tile_form(case, precision, mode, flavour):
    """Integer data: the stored bits equal the host's in every mode on every form, and the statistics rows equal the sums of the stored
    values wherever the 2^24 bound holds (module docstring)."""
    _check(case, precision, mode, flavour)


def _check(case, precision, mode, flavour):
    exact = flavour != "random"
    h, _ = _data(case, precision, flavour)
    want, on = _host(case, precision, mode, flavour)
    pos, cout = h["pos"], CASES[case][6]
    M = pos.numel()
    untouched = torch.ones(CASES[case][0] * CASES[case][7] * CASES[case][8], dtype=torch.bool)
    untouched[pos] = False
    first, slabs = None, {}
    for form in CASES[case][14]:
        out, slab = _launch(case, precision, mode, form, flavour)
        stored = out[pos].float()
        assert bool((out[untouched].float() == SENTINEL).all()), (form, "a pixel outside the launch was written")
        if exact:
            same = out[pos].view(torch.int16) == want.to(_TD[precision]).view(torch.int16)
            assert bool(same.all()), (form, f"{int((~same).sum())} of {same.numel()} stored values differ from the host's bits, first at "
                                            f"{tuple(int(v) for v in (~same).nonzero()[0])}")
        err = rel_err(stored, want)
        print(f"{case} {precision} {mode} {form}: rel err vs host fp32 {err:.3e}")
        assert err < TOL[precision], (form, err)
        if first is None:
            first = (form, out)
        else:
            assert torch.equal(out.view(torch.int16), first[1].view(torch.int16)), f"{form} and {first[0]} store different bits"
        if on is not None:
            assert float(stored[~on].abs().max()) == 0.0, (form, "a gated-off element is not exactly zero")
        if slab is None:
            continue
        bp = FORMS[form][1]
        assert slab.shape[0] == (M + bp - 1) // bp and not bool(torch.isnan(slab).any()), (form, slab.shape)
        sd = stored.double()
        if on is None:
            second = sd * sd
        else:
            second = sd * (h["gx"][pos].double() - h["mean"].double()) * h["invstd"].double()
        got = slab.double().sum(0)
        for which, term in ((0, sd), (1, second)):
            # exact flavours: every term is a multiple of the quantum (integers; the gate's second row carries invstd's halves), so a row
            # whose sums of magnitudes stay below 2^24 quanta is exact in fp32 in any order
            holds, worst = E.check_exact_rows(term, 0.5 if (on is not None and which == 1) else 1.0) if exact else (False, 0.0)
            if exact and (which == 0 or flavour == "exact_small"):      # the sums row is exact in every exact flavour, both rows in "exact_small"
                assert holds, (form, which, worst)
            if holds:
                assert torch.equal(got[which], term.sum(0)), (form, which, "a statistics row differs from the sums of the stored values")
            else:
                assert torch.allclose(got[which], term.sum(0), rtol=2e-3, atol=2e-3 * float(term.abs().sum(0).max())), (form, which)
        # the rows of forms that share the pixel tile: same rows of the same stored values, summed in the same order
        if bp in slabs:
            assert torch.equal(slab, slabs[bp][1]), f"{form} and {slabs[bp][0]} write different statistics rows"
        else:
            slabs[bp] = (form, slab)


def test_wide_tile_is_refused_where_the_weight_pack_has_one_block():
    """72 output channels: the pack holds 128 rows, so the 256-channel tile is not a legal choice (see the module docstring)."""
    from lighthand_amd import _lib
    lib = _lib.load()
    _, dv = _data("c72", "bf16")
    d = _desc("c72", "256x256")
    out = torch.zeros(2 * 13 * 11, 72, dtype=torch.bfloat16, device="cuda")
    rc = lib.lh_igemm(C.byref(d), dv["x"].data_ptr(), dv["pack"].data_ptr(), out.data_ptr(), None, None, None, None, None, None, 1, None)
    assert rc != 0 and b"does not fit" in lib.lh_last_error()
