"""Every mode of the tiled convolution kernel's epilogue (igemm_epilogue.h) on every tile form, straight through the C ABI.

The BatchNorm-backward gate is compiled into kernels of its own (igemm_ring_gated_kernel); the plain kernel carries none of it.  Both are
driven here with the configuration forced through lh_igemm_desc.cfg: plain, statistics rows, addend, addend + mask, ReLU, gate from x,
gate from mask bits, gate + addend -- on the 256 x 256, 128 x 256, 128 x 128 dense-wave and 64 x 64 forms, bf16 and fp16.  All forms share
one K order and one epilogue, so the stored outputs agree BIT FOR BIT between them; each is also held against a host fp32 evaluation of the
same descriptor.

Shapes: batch 2, 3x3 stride 1, 40 -> 72 channels at 13 x 11 (286 pixels: a ragged second 256-pixel tile; 72 channels fill neither a 128 nor
a 256 tile).  The library refuses the 256-channel tile for 72 channels (weight packs are padded to 128 rows: one block, a 256-row tile would
read past it -- cfg_safe, igemm_plan.hip), so that shape runs on the other three forms, the refusal is asserted, and the same convolution
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
squares of values that need rounding cannot stay below 2^24, see exact_data.EPILOGUE_RANGES -- those rows keep the rtol check).

Bias and folded affine (igemm_epilogue_consts): "bias" stores round16(acc + bias), "affine_relu" stores relu(round16(acc * scale + (bias *
scale + shift))) -- integer bias and shift, scale from +-{0.5, 1, 2}: every intermediate is exact in fp32.

The output buffer stands between two sentinel margins of 2 KiB, which every launch must leave as they were.

The helpers below also serve tests/test_gpu_persistent_epilogue.py, which runs the same modes on the persistent kernels (pointwise and direct
3x3: FORMS with ring depth 1 / 100, the cases of CASES beyond TILED_CASES): their epilogue is igemm_wave_epilogue.h, their statistics rows
are one per workgroup (the library reports how many), and the pointwise kernel has a mode of its own, "gate2": mask bits and TWO BatchNorm
terms, the second one's sums in a slab of its own.  SLACK gives a case operand rows / output rows that are longer than the K run / the
channels: the slack of the operand is NaN (a kernel that reads past the K run stores NaN), that of the output keeps the sentinel.  The host
side of a long case (E.EPILOGUE_LONG: tens of MB) is evaluated by torch on the device -- the accumulator still comes from the CPU (exact in
any order), what follows it is element-wise and exact, and the column sums are fp64 sums of integers."""
import ctypes as C

import pytest
import torch

import exact_data as E

pytestmark = pytest.mark.gpu

TOL = {"bf16": 3e-2, "fp16": 4e-3}                 # tests/test_gpu_ops.py
_TD = {"bf16": torch.bfloat16, "fp16": torch.float16}
_DT = {"bf16": 1, "fp16": 2}                       # LH_BF16, LH_F16
FORMS = {"256x256": (256, 256, 2, 128), "128x256": (128, 256, 3, 64), "128x128 dense": (128, 128, 22, 128), "64x64": (64, 64, 2, 64)}
TILED_FORMS = list(FORMS)
# the persistent kernels: (panel channels, pixels per wave step, 1, panel K) of every compiled pointwise configuration; the direct 3x3 kernel
FORMS.update({f"pw {bm}x{kc}x{pt}": (bm, 16 * pt, 1, kc) for bm, kc, pt in E.PW_CFGS})
FORMS.update({f"direct {c}": (64, 256, 100, c) for c in (32, 64)})
MODES = ["plain", "stats", "addend", "addend_mask", "relu", "bias", "affine_relu", "gate_x", "gate_mask", "gate_addend"]
MASKED = ("addend_mask", "gate_mask", "gate2")      # mask bits index 16-byte chunks of a DENSE output: these modes take no output slack
SENTINEL = 7.0
MARGIN = 1024                                      # elements (2 KiB) of sentinel in front of and behind the output buffer

# name -> (n, hi, wi, cin, ho, wo, cout, OH, OW, osh, osw, ooh, oow, taps (dh, dw), forms)
_T3 = [(r - 1, s - 1) for r in range(3) for s in range(3)]
CASES = {
    "c72": (2, 13, 11, 40, 13, 11, 72, 13, 11, 1, 1, 0, 0, _T3, ["128x256", "128x128 dense", "64x64"]),
    "c136": (2, 13, 11, 40, 13, 11, 136, 13, 11, 1, 1, 0, 0, _T3, TILED_FORMS),
    "phase": (2, 9, 7, 40, 9, 7, 136, 18, 14, 2, 2, 1, 0, [(1, 0), (1, -1), (0, 0), (0, -1)], TILED_FORMS),
}
TILED_CASES = list(CASES)
# the persistent kernels' cases (exact_data.py): every pointwise configuration of the case's K class -- the K = 40 case on the tiled 64 x 64
# form as well, which must store the same bits --, the direct kernel, and one long case per configuration
for _kc, _k in E.PW_K.items():
    _forms = [f for f, c in FORMS.items() if c[2] == 1 and c[3] == _kc]
    CASES[f"pw{_k}"] = E.EPILOGUE_CASES[f"pw{_k}"] + (_forms + (["64x64"] if _k == 40 else []),)
    CASES[f"long_pw{_k}"] = E.EPILOGUE_CASES[f"long_pw{_k}"] + ([],)
    for _f in _forms:
        _name = f"long_pw{_k}_{FORMS[_f][0]}x{FORMS[_f][1] // 16}"
        CASES[_name] = E.EPILOGUE_CASES[_name] + ([_f],)
for _c in (32, 64):
    CASES[f"d{_c}"] = E.EPILOGUE_CASES[f"d{_c}"] + ([f"direct {_c}"],)
    CASES[f"long_d{_c}"] = E.EPILOGUE_CASES[f"long_d{_c}"] + ([f"direct {_c}"],)
CASES["m35"] = E.EPILOGUE_CASES["m35"] + ([],)       # a member of tests/test_gpu_multi_exact.py's calls: no form of this file runs it
# case -> (operand slack, output slack) in channels
SLACK = {"pw72": (8, 0), "pw136": (0, 8)}


def _is_long(case):
    return case.startswith("long")


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _desc(case, form, mode="plain"):
    from lighthand_amd import _lib
    n, hi, wi, cin, ho, wo, cout, OH, OW, osh, osw, ooh, oow, taps, _ = CASES[case]
    islack, oslack = SLACK.get(case, (0, 0))
    d = _lib.IgemmDesc()
    d.n, d.hi, d.wi, d.in_pix_stride, d.k_run = n, hi, wi, cin + islack, cin
    d.ho, d.wo, d.sh, d.sw, d.cout = ho, wo, 1, 1, cout
    d.OH, d.OW, d.osh, d.osw, d.ooh, d.oow, d.out_pix_stride = OH, OW, osh, osw, ooh, oow, cout + (0 if mode in MASKED else oslack)
    d.ntaps, d.relu = len(taps), 0
    for t, (dh, dw) in enumerate(taps):
        d.dh[t], d.dw[t] = dh, dw
    for i, v in enumerate(FORMS[form]):
        d.cfg[i] = v
    return d


_DATA = {}
_PIXEL_KEYS = ("addend", "gx", "gx2", "amask", "gmask")      # [output pixels][channels] on the host side


def _data(case, precision, flavour="random"):
    """Operands (on the device, rounded to the run precision) and the host fp32 accumulator of one case: made once, never changed."""
    key = (case, precision, flavour)
    if key in _DATA:
        return _DATA[key]
    n, hi, wi, cin, ho, wo, cout, OH, OW, osh, osw, ooh, oow, taps, _ = CASES[case]
    td = _TD[precision]
    P = OH * OW * n
    if case in E.EPILOGUE_BASE:                           # the first rows of the base's one image: views of its tensors, host and device
        assert flavour != "random" and CASES[case][:14] == E.EPILOGUE_CASES[case]
        hb, db = _data(E.EPILOGUE_BASE[case], precision, flavour)
        host = {**hb, **{k: hb[k][:P] for k in _PIXEL_KEYS + ("acc", "pos")}}
        dev = {**db, **{k: db[k][:P] for k in ("addend", "gx", "gx2")}, "x": db["x"][:, :hi], "amask": db["amask"][:P * cout // 8],
               "gmask": db["gmask"][:P * cout // 8]}
        return host, dev
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
        bias, gx2 = torch.randn(cout, generator=g) * 0.3, torch.randn(P, cout, generator=g).to(td)
        mean2, invstd2 = torch.randn(cout, generator=g) * 0.3, torch.rand(cout, generator=g) + 0.5
    else:
        assert CASES[case][:14] == E.EPILOGUE_CASES[case]
        d = E.epilogue_data(case, precision, flavour)
        E.check_exact_epilogue(case, d)                  # every sum of magnitudes below 2^24: the accumulator is exact in any order
        x, w, addend, gx, gx2 = (d[k].to(td) for k in ("x", "w", "addend", "gx", "gx2"))
        assert all(torch.equal(t.float(), d[k]) for t, k in ((x, "x"), (w, "w"), (addend, "addend"), (gx, "gx"), (gx2, "gx2")))
        amask, gmask, mean, shift, invstd, scale, bias, mean2, invstd2 = (
            d[k] for k in ("amask", "gmask", "mean", "shift", "invstd", "scale", "bias", "mean2", "invstd2"))
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
    host = dict(acc=acc.reshape(-1, cout), pos=pos, addend=addend.float(), gx=gx.float(), gx2=gx2.float(), mean=mean, invstd=invstd, scale=scale,
                shift=shift, bias=bias, mean2=mean2, invstd2=invstd2,
                amask=((amask.view(-1, 1) >> bits) & 1).bool().view(P, cout), gmask=((gmask.view(-1, 1) >> bits) & 1).bool().view(P, cout))
    dev = dict(x=x, pack=pack, addend=addend, gx=gx, gx2=gx2, amask=amask, gmask=gmask, mean=mean, invstd=invstd, scale=scale, shift=shift,
               bias=bias, mean2=mean2, invstd2=invstd2)
    islack, oslack = SLACK.get(case, (0, 0))
    if islack:                                            # operand rows longer than the K run, the slack NaN
        dev["x"] = torch.cat([x, torch.full((n, hi, wi, islack), float("nan"), dtype=td)], 3)
    if oslack:                                            # addend and BN input in the layout of a slack output, their slack NaN
        for k in ("addend", "gx"):
            dev[k + "_s"] = torch.cat([dev[k], torch.full((P, oslack), float("nan"), dtype=td)], 1)
    dev = {k: v.contiguous().cuda() for k, v in dev.items()}
    if _is_long(case):                                    # one long case at a time; its host side lives on the device (module docstring)
        for k in [k for k in _DATA if _is_long(k[0])]:
            del _DATA[k]
        host = {k: v.cuda() for k, v in host.items()}
    _DATA[key] = (host, dev)
    return _DATA[key]


def _host(case, precision, mode, flavour="random"):
    """(expected stored values of the launch's pixels, gate-on mask or None) in fp32 with the epilogue's roundings."""
    h, _ = _data(case, precision, flavour)
    td, pos = _TD[precision], h["pos"]
    if mode == "bias":
        v = (h["acc"] + h["bias"]).to(td).float()
    elif mode == "affine_relu":                           # the constants as igemm_epilogue_consts folds them
        v = (h["acc"] * h["scale"] + (h["bias"] * h["scale"] + h["shift"])).to(td).float().clamp_min(0.0)
    else:
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
    elif mode in ("gate_mask", "gate2"):
        on = h["gmask"][pos]
    if on is not None:
        v = torch.where(on, v, torch.zeros_like(v))
    return v, on


def _launch(case, precision, mode, form, flavour="random", status_only=False):
    """One launch -> (output buffer with its two margins, slabs [one per BatchNorm term, or none], output row pitch), on the device of the
    case's host side.  status_only: the library's return code instead, nothing is read back."""
    from lighthand_amd import _lib
    lib = _lib.load()
    h, dv = _data(case, precision, flavour)
    d = _desc(case, form, mode)
    d.relu = 1 if mode in ("relu", "affine_relu") else 0
    n, cout, OH, OW = CASES[case][0], CASES[case][6], CASES[case][7], CASES[case][8]
    pitch = d.out_pix_stride
    sfx = "_s" if pitch != cout else ""
    buf = torch.full((2 * MARGIN + n * OH * OW * pitch,), SENTINEL, dtype=_TD[precision], device="cuda")
    out = buf.data_ptr() + MARGIN * buf.element_size()
    addend = dv["addend" + sfx].data_ptr() if mode in ("addend", "addend_mask", "gate_addend") else None
    amask = dv["amask"].data_ptr() if mode == "addend_mask" else None
    slabs = []
    if mode.startswith("gate"):
        two = mode == "gate2"
        rows = lib.lh_igemm_gated_rows(C.byref(d), _DT[precision], 2 if two else 1)
        slabs = [torch.full((rows, 2, cout), float("nan"), device="cuda") for _ in range(2 if two else 1)]
        masked = mode in ("gate_mask", "gate2")
        gate = _lib.BnBwdGate(dv["gx" + sfx].data_ptr(), dv["mean"].data_ptr(), dv["invstd"].data_ptr(), None if masked else dv["scale"].data_ptr(),
                              None if masked else dv["shift"].data_ptr(), slabs[0].data_ptr(), dv["gmask"].data_ptr() if masked else None)
        if two:
            gate.x2, gate.mean2, gate.invstd2, gate.partial2 = dv["gx2"].data_ptr(), dv["mean2"].data_ptr(), dv["invstd2"].data_ptr(), slabs[1].data_ptr()
        rc = lib.lh_igemm_gated(C.byref(d), dv["x"].data_ptr(), dv["pack"].data_ptr(), out, addend, amask, C.byref(gate), _DT[precision], None)
    else:
        if mode == "stats":
            rows = lib.lh_igemm_stats_rows(C.byref(d), _DT[precision])
            slabs = [torch.full((rows, 2, cout), float("nan"), device="cuda")]
        bias = dv["bias"].data_ptr() if mode in ("bias", "affine_relu") else None
        scale, shift = (dv["scale"].data_ptr(), dv["shift"].data_ptr()) if mode == "affine_relu" else (None, None)
        rc = lib.lh_igemm(C.byref(d), dv["x"].data_ptr(), dv["pack"].data_ptr(), out, addend, amask, bias, scale, shift,
                          slabs[0].data_ptr() if slabs else None, _DT[precision], None)
    if status_only:
        torch.cuda.synchronize()
        return rc
    _lib.check(rc, f"lh_igemm {case} {mode} {form}")
    torch.cuda.synchronize()
    where = h["acc"].device
    return buf.to(where), [s.to(where) for s in slabs], pitch


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("case", TILED_CASES)
def test_epilogue_mode_on_every_tile_form(case, precision, mode):
    _check(case, precision, mode, "random")


@pytest.mark.parametrize("flavour", ["exact", "exact_small"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("case", TILED_CASES)
def test_epilogue_mode_exact_on_every_tile_form(case, precision, mode, flavour):
    """Integer data: the stored bits equal the host's in every mode on every form, and the statistics rows equal the sums of the stored
    values wherever the 2^24 bound holds (module docstring)."""
    _check(case, precision, mode, flavour)


def _check(case, precision, mode, flavour):
    exact = flavour != "random"
    h, _ = _data(case, precision, flavour)
    want, on = _host(case, precision, mode, flavour)
    pos, cout = h["pos"], CASES[case][6]
    M, P = pos.numel(), CASES[case][0] * CASES[case][7] * CASES[case][8]
    untouched = torch.ones(P, dtype=torch.bool, device=pos.device)
    untouched[pos] = False
    # the rows that must be exact: the sums in every exact flavour, both rows in "exact_small" -- but for the long cases, whose pixels
    # are too many for the second row's bound (they take the rtol rule where check_exact_rows does not hold)
    must_hold = () if not exact else (0,) if flavour == "exact" or _is_long(case) else (0, 1)
    first, tiled_slabs = None, {}
    for form in CASES[case][14]:
        tiled = FORMS[form][2] not in (1, 100)
        if mode == "gate2" and FORMS[form][2] != 1:
            continue                                     # two BatchNorm terms: the pointwise kernel only (the refusal has a test of its own)
        buf, slabs, pitch = _launch(case, precision, mode, form, flavour)
        assert bool((buf[:MARGIN].float() == SENTINEL).all()) and bool((buf[-MARGIN:].float() == SENTINEL).all()), (form, "a margin of the output was written")
        full = buf[MARGIN:-MARGIN].view(P, pitch)
        assert bool((full[:, cout:].float() == SENTINEL).all()), (form, "a slack column of the output was written")
        out = full[:, :cout]
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
        assert len(slabs) == (2 if mode == "gate2" else 1 if mode == "stats" or on is not None else 0)
        bp = FORMS[form][1]
        sd = stored.double()
        for term2, slab in enumerate(slabs):
            # the slab has the rows the library reported (_launch), and every one of them was written; a tiled launch writes one per pixel tile
            assert not bool(torch.isnan(slab).any()), (form, slab.shape)
            assert not tiled or slab.shape[0] == (M + bp - 1) // bp, (form, slab.shape)
            if on is None:
                second = sd * sd
            elif term2:
                second = sd * (h["gx2"][pos].double() - h["mean2"].double()) * h["invstd2"].double()
            else:
                second = sd * (h["gx"][pos].double() - h["mean"].double()) * h["invstd"].double()
            got = slab.double().sum(0)
            for which, term in ((0, sd), (1, second)):
                # exact flavours: every term is a multiple of the quantum (integers; the gate's second row carries invstd's halves), so a row
                # whose sums of magnitudes stay below 2^24 quanta is exact in fp32 in any order
                holds, worst = E.check_exact_rows(term, 0.5 if (on is not None and which == 1) else 1.0) if exact else (False, 0.0)
                if which in must_hold:
                    assert holds, (form, which, worst)
                if holds:
                    assert torch.equal(got[which], term.sum(0)), (form, term2, which, "a statistics row differs from the sums of the stored values")
                else:
                    assert torch.allclose(got[which], term.sum(0), rtol=2e-3, atol=2e-3 * float(term.abs().sum(0).max())), (form, term2, which)
            # the rows of tiled forms that share the pixel tile: same rows of the same stored values, summed in the same order
            if tiled and bp in tiled_slabs:
                assert torch.equal(slab, tiled_slabs[bp][1]), f"{form} and {tiled_slabs[bp][0]} write different statistics rows"
            elif tiled:
                tiled_slabs[bp] = (form, slab)


def test_wide_tile_is_refused_where_the_weight_pack_has_one_block():
    """72 output channels: the pack holds 128 rows, so the 256-channel tile is not a legal choice (see the module docstring)."""
    from lighthand_amd import _lib
    lib = _lib.load()
    _, dv = _data("c72", "bf16")
    d = _desc("c72", "256x256")
    out = torch.zeros(2 * 13 * 11, 72, dtype=torch.bfloat16, device="cuda")
    rc = lib.lh_igemm(C.byref(d), dv["x"].data_ptr(), dv["pack"].data_ptr(), out.data_ptr(), None, None, None, None, None, None, 1, None)
    assert rc != 0 and b"does not fit" in lib.lh_last_error()


def test_two_batchnorm_terms_are_refused_on_a_tiled_form():
    """lh_bn_bwd_gate.x2 is the pointwise kernel's: a tiled form answers LH_ERR_UNSUPPORTED and writes nothing."""
    from lighthand_amd import _lib
    assert _launch("c136", "bf16", "gate2", "64x64", status_only=True) == -3          # LH_ERR_UNSUPPORTED
    assert b"two BatchNorm terms are gated by the pointwise kernel only" in _lib.load().lh_last_error()
