"""Preconditions of the exact-arithmetic GPU tests (tests/exact_data.py), proved on the CPU for every case and precision those tests run:
(a) every sum of magnitudes, in units of the product quantum, is below 2^24 -- so an fp32 accumulator is exact in any order;
(b) no expected fp16 value overflows;
(c) out and dx together hold at least 10 exact ties and at least 100 values that need rounding -- so a wrong rounding mode cannot pass.
Plus: the hand-written tap loop that serves as the epilogue test's host side agrees with F.conv2d / F.conv_transpose2d in fp64.
The last section does the same for the fused stem and bottleneck kernels of tests/test_gpu_exact_fused.py."""
import pytest
import torch
import torch.nn.functional as F

import exact_data as E

_PLAN_CASES = [(c, False, None) for c in E.CONV_CASES] + [(c, True, b) for c in E.DECONV_CASES for b in (False, True)]


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("case,transposed,bias", _PLAN_CASES)
def test_plan_level_cases_meet_the_preconditions(case, transposed, bias, precision):
    x, w, b, dy = E.conv_data(case, precision, bias=bias, transposed=transposed)
    ax, aw = E.ranges(case, precision)
    assert ax >= E.RANGES[precision][0] and aw >= E.RANGES[precision][1]                # widened, never narrowed
    dt = E.DTYPES[precision]
    for t in (x, w, dy) + ((b,) if b is not None else ()):
        assert torch.equal(t.to(dt).float(), t) and torch.equal(t, t.round())         # integers the type holds exactly
    worst = E.check_exact(x, w, b, dy, case, transposed)                                # (a)
    r = E.reference(x, w, b, dy, case, transposed)
    if precision == "fp32":
        for k in ("out", "dx", "dw"):
            assert torch.equal(r[k].float().double(), r[k])
        return
    peak = max(float(r["out"].abs().max()), float(r["dx"].abs().max()))
    if precision == "fp16":
        assert peak <= E.FP16_MAX                                                       # (b)
        assert bool(torch.isfinite(E.expected_16(r["out"], dt)).all()) and bool(torch.isfinite(E.expected_16(r["dx"], dt)).all())
    (ro, to), (rd, td) = E.rounding_counts(r["out"], dt), E.rounding_counts(r["dx"], dt)
    print(case, precision, f"largest sum of magnitudes {worst:.0f}, peak {peak:.0f}, need rounding {ro + rd}, ties {to + td}")
    assert to + td >= 10 and ro + rd >= 100, (ro + rd, to + td)                         # (c)


def test_strided_1x1_data_gradient_leaves_the_other_phases_zero():
    """(64, 136, 1, 2, 0, 2, 9, 7): the data gradient writes pixels (2a, 2b) only; the host's dx is exactly zero elsewhere, and the
    GPU comparison is exact -- this states the property on the host reference so that it cannot go unnoticed."""
    case = E.CONV_CASES[3]
    x, w, b, dy = E.conv_data(case, "bf16")
    dx = E.reference(x, w, b, dy, case)["dx"]
    off = torch.ones_like(dx, dtype=torch.bool)
    off[:, :, 0::2, 0::2] = False
    assert float(dx[off].abs().max()) == 0.0 and float((dx[~off] != 0).double().mean()) > 0.9


def test_rounding_counts_agree_with_the_conversion():
    """rounding_counts against the type conversion itself, on every integer of a range with known ties."""
    v = torch.arange(-5000, 5001, dtype=torch.float64)
    for dt, first in ((torch.bfloat16, 257), (torch.float16, 2049)):
        need, ties = E.rounding_counts(v, dt)
        assert need == int((v.float().to(dt).double() != v).sum())
        assert E.rounding_counts(torch.tensor([float(first)]), dt) == (1, 1) and E.rounding_counts(torch.tensor([float(first - 1)]), dt) == (0, 0)
        assert E.rounding_counts(torch.tensor([float(2 * first + 1)]), dt) == (1, 0)
        # a tie goes to the even neighbour: 257 -> 256 and 259 -> 260 in bf16, 2049 -> 2048 and 2051 -> 2052 in fp16
        assert float(E.expected_16(torch.tensor([float(first)]), dt)) == first - 1 and float(E.expected_16(torch.tensor([first + 2.0]), dt)) == first + 3
        assert ties > 100


@pytest.mark.parametrize("flavour", list(E.EPILOGUE_RANGES))
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("case", E.EPILOGUE_SHORT)
def test_epilogue_cases_meet_the_preconditions(case, precision, flavour):
    d = E.epilogue_data(case, precision, flavour)
    dt = E.DTYPES[precision]
    for k in ("x", "w", "addend", "gx", "gx2", "bias", "shift", "mean", "mean2"):
        assert torch.equal(d[k].to(dt).float(), d[k]) and torch.equal(d[k], d[k].round()), k
    assert set(d["invstd"].tolist()) <= {0.5, 1.0, 2.0} and set(d["scale"].abs().tolist()) <= {0.5, 1.0, 2.0} and bool((d["scale"] < 0).any())
    assert set(d["invstd2"].tolist()) <= {0.5, 1.0, 2.0}
    ax, aw, _ = E.epilogue_ranges(case, precision, flavour)
    assert ax >= E.EPILOGUE_RANGES[flavour][precision][0] and aw >= E.EPILOGUE_RANGES[flavour][precision][1]       # widened, never narrowed
    worst = E.check_exact_epilogue(case, d)
    ho, wo, taps = E.EPILOGUE_CASES[case][4], E.EPILOGUE_CASES[case][5], E.EPILOGUE_CASES[case][13]
    acc = E.tap_conv(d["x"], d["w"], taps, ho, wo, torch.float64)
    peak = float(acc.abs().max())
    assert peak + float(d["addend"].abs().max()) <= E.FP16_MAX
    # "bias" and "affine_relu": |acc * scale + (bias * scale + shift)| with |scale| <= 2 stays inside fp16 as well
    assert 2.0 * (peak + float(d["bias"].abs().max())) + float(d["shift"].abs().max()) <= E.FP16_MAX
    need, ties = E.rounding_counts(acc, dt)
    biased = E.rounding_counts(acc + d["bias"].double(), dt)
    affine = E.rounding_counts(acc * d["scale"].double() + (d["bias"] * d["scale"] + d["shift"]).double(), dt)
    print(case, precision, flavour, f"largest sum of magnitudes {worst:.0f}, peak {peak:.0f}, accumulators that need rounding {need}, ties {ties}; "
          f"with the bias {biased}, with the affine {affine}")
    if flavour == "exact":
        assert need >= 100 and ties >= 10
        assert biased[0] >= 100 and biased[1] >= 10 and affine[0] >= 100 and affine[1] >= 10
    else:
        # the flavour whose statistics rows are exact: sums of squares of the (rounded) accumulators, the largest term of any mode's rows
        sq = E.expected_16(acc, dt).double().reshape(-1, acc.shape[-1]) ** 2
        assert E.check_exact_rows(sq)[0]


def test_long_cases_walk_the_tile_loop_for_every_grid_the_library_may_pick():
    """The arithmetic of the long cases on the shapes alone: a pointwise grid has at most G = 1024 / cb / 8 * 8 workgroups per channel
    block (lh_pw_grid with occupancy 4), four waves each, a direct grid at most 512 / cb / 8 * 8 workgroups (lh_d3_rows with occupancy
    2); every such unit takes at least two tiles and some take three, and the pixel count is no multiple of 16."""
    seen = set()
    for case, base in E.EPILOGUE_BASE.items():
        k, (bm, pt) = int(base[len("long_pw"):]), map(int, case.rsplit("_", 1)[1].split("x"))
        n, hi, wi, cin = E.EPILOGUE_CASES[case][:4]
        kc = next(kc for kc, kk in E.PW_K.items() if kk == k)
        assert (bm, kc, pt) in E.PW_CFGS and cin == k and n == 1 and hi <= E.EPILOGUE_CASES[base][1]
        seen.add((bm, kc, pt))
        M, units = hi * wi, 4 * E.pw_long_grid_cap(bm)
        ntile = (M + 16 * pt - 1) // (16 * pt)
        assert M % 16 != 0 and ntile >= 2 * units + 1 and M * E.PERSISTENT_COUT * 2 <= 70e6 and M * cin * 2 <= 70e6, (case, M, ntile, units)
    assert seen == set(E.PW_CFGS)
    for c in (32, 64):
        n, hi, wi = E.EPILOGUE_CASES[f"long_d{c}"][:3]
        assert n * ((hi + 15) // 16) * ((wi + 15) // 16) >= 2 * (512 // 3 // 8 * 8) + 1 and (n * hi * wi) % 16 != 0


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("case", E.EPILOGUE_LONG)
def test_long_epilogue_cases_meet_the_preconditions(case, precision):
    """"exact_small" data at up to 172 000 pixels: the accumulator is exact, and the sums row of every statistics slab -- plain, with the
    masked addend, gated -- is exact in any grouping: the columns' sums of magnitudes of |stored value| <= |round16(acc)| + |addend| stay
    below 2^24.  The prefixes of a base case (exact_data.EPILOGUE_BASE) sum fewer of the same terms."""
    d = E.epilogue_data(case, precision, "exact_small")
    dt = E.DTYPES[precision]
    for k in ("x", "w", "addend", "gx", "gx2"):
        assert torch.equal(d[k].to(dt).float(), d[k]) and torch.equal(d[k], d[k].round()), k
    worst = E.check_exact_epilogue(case, d)
    ho, wo, cout, taps = E.EPILOGUE_CASES[case][4], E.EPILOGUE_CASES[case][5], E.EPILOGUE_CASES[case][6], E.EPILOGUE_CASES[case][13]
    acc = E.tap_conv(d["x"], d["w"], taps, ho, wo, torch.float64).reshape(-1, cout)
    assert float(acc.abs().max()) + float(d["addend"].abs().max()) <= E.FP16_MAX
    plain, plain_worst = E.check_exact_rows(E.expected_16(acc, dt).double())
    both, both_worst = E.check_exact_rows(E.expected_16(acc, dt).double().abs() + d["addend"].double().abs())
    print(case, precision, f"{acc.shape[0]} pixels, largest sum of magnitudes of an accumulator {worst:.0f}; largest column sum of magnitudes of "
          f"the stored values {plain_worst:.4g}, with the addend {both_worst:.4g}")
    assert plain and both


def test_tap_loop_equals_conv2d_and_conv_transpose2d():
    """The tap loop of the epilogue test's host side (exact_data.tap_conv) in fp64 against torch: the 3 x 3 tap list is F.conv2d with
    padding 1, and the four taps of the 'phase' case are output pixels (2a + 1, 2b) of F.conv_transpose2d(kernel 4, stride 2, padding 1),
    with tap (dh, dw) reading kernel element (ky, kx) = (2 - 2 dh, 1 - 2 dw)."""
    g = torch.Generator().manual_seed(100)
    n, hi, wi, cin, cout = 2, 5, 4, 8, 16
    x = E.ints((n, hi, wi, cin), 8, g)
    taps3 = E.EPILOGUE_CASES["c72"][13]
    w3 = E.ints((cout, 9, cin), 4, g)
    got = E.tap_conv(x, w3, taps3, hi, wi, torch.float64)
    want = F.conv2d(x.double().permute(0, 3, 1, 2), w3.double().view(cout, 3, 3, cin).permute(0, 3, 1, 2), None, 1, 1)
    assert torch.equal(got, want.permute(0, 2, 3, 1))
    taps = E.EPILOGUE_CASES["phase"][13]
    wd = E.ints((cin, cout, 4, 4), 4, g)                            # ConvTranspose2d layout
    wt = torch.stack([wd[:, :, 2 - 2 * dh, 1 - 2 * dw].t() for dh, dw in taps], 1)      # [cout][taps][cin]
    got = E.tap_conv(x, wt, taps, hi, wi, torch.float64)
    full = F.conv_transpose2d(x.double().permute(0, 3, 1, 2), wd.double(), None, 2, 1, 0)
    assert full.shape[2:] == (2 * hi, 2 * wi)
    assert torch.equal(got, full[:, :, 1::2, 0::2].permute(0, 2, 3, 1))


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_chain_meets_the_preconditions(precision):
    """The chain of the table-launch test: check_exact per layer with that layer's quanta (inside chain_reference), weights in
    {-1, 0, 1} * 2^-s, and magnitudes that stay level and inside the type."""
    x, params, dy = E.chain_data()
    for name, *_rest, nz, sh in E.CHAIN_LAYERS:
        w = params[name + ".weight"]
        assert set((w * 2.0 ** sh).unique().tolist()) <= {-1.0, 0.0, 1.0}
    out, dx, grads, worst = E.chain_reference(x, params, dy, precision)
    print(precision, "largest sums of magnitudes per layer, in quanta:", [(n, f"{m:.0f}") for n, m in worst])
    assert max(m for _, m in worst) < E.LIMIT
    assert float(out.abs().max()) <= E.FP16_MAX and float(dx.abs().max()) <= E.FP16_MAX
    for k, g in grads.items():
        assert torch.equal(g.float().double(), g), k                  # fp32 holds every expected gradient exactly
        assert float((g != 0).double().mean()) > 0.5, k               # and the gradients are dense: every pixel counts


# ---------------------------------------------------------------------------------------------------------------------------------
# The BatchNorm grid of tests/test_gpu_exact_bn.py: its proof obligation, its rounding shares, the interval condition of the ragged
# cases, and the route table pinned through lh_fuse_bwd_plan / lh_fuse_fwd_plan (host arithmetic: no GPU).
@pytest.mark.parametrize("name,precision", E.BN_BWD_RUNS)
def test_bn_backward_cases_are_exact_and_need_rounding(name, precision):
    """check_bn_exact on every case and precision the GPU test runs; and, in the spirit of (c): at least 10 % of the BatchNorm terms' dx
    elements differ from their 16-bit rounding and at least one is an exact tie.  (A node of identity terms only has dx = g or g + g,
    which the type of dout always holds: there the condition cannot be met by any data and the exact comparison is about order.)"""
    spec = E.BN_BWD_CASES[name]
    d = E.bn_node(name, spec, precision)
    assert d["a"] >= E.BN_A                                                              # widened, never narrowed
    worst = E.check_bn_exact(d, spec, precision)
    assert float(d["gate"].mean()) > 0.2 and (spec.get("pre") or spec["relu"] == "off" or float(d["gate"].mean()) < 0.8)
    dt = E.DTYPES[precision]
    tot = torch.cat([t["total"].reshape(-1) for t, p in zip(d["terms"], d["prm"]) if p is not None] or [torch.zeros(0, dtype=torch.float64)])
    if precision == "fp32":
        assert torch.equal(tot.float().double(), tot)
        return
    if tot.numel() == 0:
        return
    need, ties = E.rounding_counts(tot, dt)
    print(name, precision, f"largest column sum {worst:.0f} quanta, dx elements that need rounding {need} of {tot.numel()} "
          f"({100.0 * need / tot.numel():.1f} %), ties {ties}")
    assert need >= 0.1 * tot.numel() and ties >= 1, (need, ties, tot.numel())


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(E.BN_RAGGED_CASES))
def test_bn_ragged_cases_pin_all_but_two_percent_of_the_elements(name, precision):
    """Pixel counts 180, 35, 663: the sums stay exact (check_bn_exact), the division by the count does not, and a stored dx must lie in
    [RNE(ref - E), RNE(ref + E)] (E: exact_data.bn_dx_bound).  Condition: the two ends differ for at most 2 % of the elements, so at
    least 98 % of them are held to one value."""
    spec = E.BN_RAGGED_CASES[name]
    d = E.bn_node(name, spec, precision)
    E.check_bn_exact(d, spec, precision)
    ref, bound = d["terms"][0]["dx"], E.bn_dx_bound(d, 0)
    lo, hi, strict = E.interval_16(ref, bound, E.DTYPES[precision])
    want = E.store(ref, E.DTYPES[precision])
    assert bool((lo.double() <= want.double()).all()) and bool((want.double() <= hi.double()).all())
    loose = 1.0 - float(strict.double().mean())
    need, ties = E.rounding_counts(ref, E.DTYPES[precision])
    print(name, precision, f"ends differ for {100 * loose:.2f} % of {ref.numel()} elements; {need} need rounding")
    assert loose <= 0.02 and need >= 0.1 * ref.numel()
    assert float((bound / ref.abs().clamp_min(1e-30)).median()) < 2.0 ** -18            # the bound is a few fp32 ulps, not a tolerance


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("case", E.BN_FWD_CASES, ids=[c[0] for c in E.BN_FWD_CASES])
def test_bn_forward_cases_are_exact_and_need_rounding(case, precision):
    """Every term, and every partial sum in term order, is held by fp32 exactly (bn_fwd_data asserts it as it goes); in the 16-bit types
    at least 2 % of the results need a rounding (behind the ReLU: at least one), one is a tie, and none overflows."""
    dt = E.DTYPES[precision]
    for relu in (0, 1):
        d = E.bn_fwd_data(case, precision, relu)
        for x in d["x"]:
            assert torch.equal(x.to(dt).float(), x)
        if precision == "fp32":
            continue
        assert float(d["exact"].abs().max()) <= E.FP16_MAX
        need, ties = E.rounding_counts(d["exact"], dt)
        print(case[0], precision, "relu" if relu else "no relu", f"need rounding {need} of {d['exact'].numel()}, ties {ties}")
        assert need >= (1 if relu else 0.02 * d["exact"].numel()) and ties >= 1


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("case", E.STEM_CASES, ids=["x".join(map(str, c)) for c in E.STEM_CASES])
def test_stem_chain_is_exact(case, precision):
    """The pool's input gradient is a sum of up to four integers (exact; with the wide range some need a rounding), the slab rows of the
    gated pass sum exactly in any grouping with either range, and with the narrow range the BatchNorm backward behind the rounded, gated
    gradient passes check_bn_exact; the 63-pixel shape meets the 2 % condition."""
    dt = E.DTYPES[precision]
    s = E.stem_data(case, precision)
    for which in ("dout", "dout_pool"):
        r = E.stem_reference(s, precision, which)
        need, _ = E.rounding_counts(r["gpool"], dt)
        t = r["node"]["terms"][0]
        assert float(r["gpool"].abs().max()) <= E.FP16_MAX and (need >= 10 or which == "dout")
        worst = max(E._sum_fits(t["g"], 1.0, "sum g"), E._sum_fits(t["g"] * t["xhat"], 0.25, "sum g * xhat"))
        print(case, precision, which, f"pool gradients that need rounding: {need}; largest column sum {worst:.0f} quanta")
    r = E.stem_reference(s, precision)
    E.check_bn_exact(r["node"], None, precision)
    need, ties = E.rounding_counts(r["node"]["terms"][0]["dx"], dt)
    assert need >= 0.1 * r["node"]["terms"][0]["dx"].numel()
    cnt = case[0] * case[1] * case[2]
    if cnt & (cnt - 1):
        _, _, strict = E.interval_16(r["node"]["terms"][0]["dx"], E.bn_dx_bound(r["node"], 0), dt)
        assert 1.0 - float(strict.double().mean()) <= 0.02


_FAKE = 1 << 20           # a non-null address the planners never dereference


def _fake_bwd_desc(spec):
    from lighthand_amd import _lib
    d = _lib.FuseBwdDesc()
    relu, terms, pre = spec["relu"], spec["terms"], spec.get("pre", 0)
    d.dout, d.relu, d.nterms, d.strips_cap = _FAKE, int(relu != "off"), len(terms), spec.get("cap", 0)
    d.out = _FAKE if relu in ("out", "shift") else None
    d.relu_mask = _FAKE if relu == "mask" else None
    for i, (bn, l, acc, same) in enumerate(terms):
        if bn:
            d.x[i] = d.scale[i] = d.save_mean[i] = d.save_invstd[i] = d.dgamma[i] = d.dbeta[i] = _FAKE
            d.shift[i] = _FAKE if relu == "shift" else None
        d.dx[i] = _FAKE + 4096 * (i if same is None else same)
        d.log2up[i], d.accumulate[i] = l, acc
    if pre:
        d.pre_partial, d.pre_rows = _FAKE, pre
        if sum(bn for bn, *_ in terms) == 2:
            d.pre_partial2 = _FAKE
    return d


def test_bn_route_table_is_what_the_planners_return(monkeypatch):
    """lh_fuse_bwd_plan / lh_fuse_fwd_plan on every case of exact_data.BN_BWD_CASES, BN_RAGGED_CASES and BN_FWD_CASES: exactly the kinds,
    grids (= strips for the reduce records) and fold rows the tables name -- so every GPU case reaches the route it was written for --
    and between them all eight backward and all three forward kinds."""
    import ctypes as C
    from lighthand_amd import _lib
    lib = _lib.load()
    kb = dict(RG=_lib.LH_FB_REDUCE_GEN, RF=_lib.LH_FB_REDUCE_FLAT, RFX=_lib.LH_FB_REDUCE_FLAT_X, CO=_lib.LH_FB_COEF, AG=_lib.LH_FB_APPLY_GEN,
              AF=_lib.LH_FB_APPLY_FLAT, AFX=_lib.LH_FB_APPLY_FLAT_X, A2=_lib.LH_FB_APPLY2)
    kf = dict(GEN=_lib.LH_FF_GEN, FLAT1=_lib.LH_FF_FLAT1, FLAT2=_lib.LH_FF_FLAT2)
    assert sorted(kb.values()) == list(range(8)) and sorted(kf.values()) == list(range(3))
    code = dict(bf16=_lib.LH_BF16, fp16=_lib.LH_F16, fp32=_lib.LH_F32)
    seen = set()
    for name, precision in E.BN_BWD_RUNS:
        spec = E.BN_BWD_CASES[name]
        monkeypatch.delenv("LH_FOLD_IN_APPLY", raising=False)
        if spec.get("env"):
            monkeypatch.setenv("LH_FOLD_IN_APPLY", "0")
        got = E.bn_planned_route(lib, _fake_bwd_desc(spec), *spec["shape"], E.bn_case_c(spec, precision), _FAKE, code[precision])
        assert got == [(kb[k], g, f) for k, g, f in E.bn_case_route(spec, precision)], (name, precision, got)
        seen |= {k for k, _, _ in got}
    monkeypatch.delenv("LH_FOLD_IN_APPLY", raising=False)
    assert seen == set(range(8))
    for name, spec in E.BN_RAGGED_CASES.items():
        got = E.bn_planned_route(lib, _fake_bwd_desc(spec), *spec["shape"], spec["c"], _FAKE, _lib.LH_BF16)
        assert [k for k, _, _ in got] == [kb[k] for k in spec["kinds"]], (name, got)
    # a record buffer shorter than the plan: the count is still returned, nothing is written past `cap`
    spec = E.BN_BWD_CASES["mixed3"]
    kinds = (C.c_int * 3)(-1, -1, -1)
    assert lib.lh_fuse_bwd_plan(C.byref(_fake_bwd_desc(spec)), *spec["shape"], spec["c"], _FAKE, _lib.LH_BF16, kinds, None, None, 2) == 6
    assert list(kinds) == [kb["RF"], kb["AF"], -1]
    assert lib.lh_fuse_bwd_plan(C.byref(_fake_bwd_desc(spec)), *spec["shape"], 12, _FAKE, _lib.LH_BF16, kinds, None, None, 2) == -1
    seen_f = set()
    for name, (n, h, w), c, terms, want in E.BN_FWD_CASES:
        for precision in ("bf16", "fp16", "fp32"):
            d = _lib.FuseDesc()
            d.nterms, d.relu = len(terms), 1
            for i, (bn, l) in enumerate(terms):
                d.x[i], d.log2up[i] = _FAKE, l
                d.scale[i] = d.shift[i] = _FAKE if bn else None
            kind, grid = C.c_int(-1), C.c_int(-1)
            assert lib.lh_fuse_fwd_plan(C.byref(d), _FAKE, n, h, w, c, code[precision], C.byref(kind), C.byref(grid)) == 0, lib.lh_last_error()
            chunks = n * h * w * c // (4 if precision == "fp32" else 8)
            assert kind.value == kf[want] and grid.value == (-(-chunks // 256) if want == "GEN" else max(1, -(-chunks // 1024))), (name, precision)
            seen_f.add(kind.value)
    assert seen_f == set(range(3))


# ---------------------------------------------------------------------------------------------------------------------------------
# The fused stem and bottleneck kernels of tests/test_gpu_exact_fused.py: (a) - (c) for every case and precision it runs, the statistics
# rows of lh_stem_conv on the kernel's own tile-to-workgroup partition, the multi-tile conditions against the library's grid queries
# (host arithmetic: no GPU), and the hand-written references against F.conv2d.
def _held_exactly(t, dt):
    return torch.equal(t.float().to(dt).double(), t.double())


def _no_fp16_trouble(tensors, what):
    """(b): finite, and no nonzero value below the smallest normal fp16 (2^-14): the comparison never rests on subnormal handling."""
    for k, t in tensors.items():
        a = t.double().abs()
        assert float(a.max()) <= E.FP16_MAX and bool(torch.isfinite(t.float().to(torch.float16)).all()), (what, k, float(a.max()))
        assert not bool(((a > 0) & (a < 2.0 ** -14)).any()), (what, k, "a subnormal fp16 value")


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("image", list(E.FUSED_STEM_IMAGES))
def test_fused_stem_cases_meet_the_preconditions(image, precision):
    """lh_stem_pool and lh_stem_conv, "exact" flavour: integer operands the type holds, (a) through fused_stem_check, (b) on the raw
    convolution and the activation, (c) on the raw convolution (what lh_stem_conv stores) and on the pooled map (asked of the exact value
    behind each pooled maximum); one channel is dead, one has a negative scale, no two images are equal, and the sums row of every
    lh_stem_conv workgroup stays below 2^24 (its squares row does not: that is the "stats" flavour's)."""
    dt = E.DTYPES[precision]
    d = E.fused_stem_data(image, precision)
    got, base = E.fused_stem_ranges(image, precision, "exact"), E.FUSED_STEM_RANGES["exact"][precision]
    assert all(g >= b for g, b in zip(got, base))                                       # widened, never narrowed
    assert _held_exactly(d["x"], dt) and _held_exactly(d["w"], dt)
    n, h, w, hp, wp, ch, cw, ph, pw = E.fused_stem_sizes(image)
    assert len(torch.unique(d["x"].reshape(n, -1), dim=0)) == n
    r = E.fused_stem_reference(d, precision)
    assert r["acc"].shape == (n, ch, cw, 64) and r["pooled"].shape == (n, ph, pw, 64)
    worst = E.fused_stem_check(d, r)                                                    # (a)
    peak = max(float(r["acc"].abs().max()), float(r["act"].max()))
    if precision == "fp16":
        _no_fp16_trouble(dict(acc=r["acc"], act=r["act"]), image)                       # (b)
    assert float(r["pooled"][..., E.FUSED_STEM_DEAD].abs().max()) == 0.0 and float(r["act"][..., E.FUSED_STEM_DEAD].max()) == 0.0
    assert float(d["scale"][E.FUSED_STEM_NEG]) < 0 and float(r["pooled"][..., E.FUSED_STEM_NEG].max()) > 0
    (rc, tc), (rp, tp) = E.rounding_counts(r["acc"], dt), E.rounding_counts(E.pooled_source(r), dt)
    assert torch.equal(E.expected_16(E.pooled_source(r), dt), r["pooled"])              # rounding is monotonic: pooled_source is what it says
    rows = _library().lh_stem_conv_rows(n, ch, cw)
    rid = E.stem_conv_row_of_pixel(n, ch, cw, rows).reshape(-1)
    sums = torch.zeros(rows, 64, dtype=torch.float64).index_add_(0, rid, r["conv16"].double().abs().reshape(-1, 64))
    print(image, precision, f"largest sum of magnitudes {worst:.0f}, peak {peak:.0f}; convolution: need rounding {rc}, ties {tc}; pooled map: need "
          f"rounding {rp}, ties {tp}; largest statistics row, sum of magnitudes {float(sums.max()):.0f}")
    assert rc >= 100 and tc >= 10 and rp >= 100 and tp >= 10                            # (c)
    assert float(sums.max()) < E.LIMIT


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("image", list(E.FUSED_STEM_IMAGES))
def test_stem_conv_statistics_rows_are_exact(image, precision):
    """"stats" flavour: workgroup b of stem_conv_kernel sums the stored values and their squares over the valid pixels of tiles b, b + grid,
    ... (exact_data.stem_conv_row_of_pixel restates the tile loop); every row's sum of squares -- all terms non-negative integers -- stays
    below 2^24, so each row is exact in fp32 in any order and the fp64 total of the rows equals the fp64 sums of the stored values."""
    dt = E.DTYPES[precision]
    d = E.fused_stem_data(image, precision, "stats")
    r = E.fused_stem_reference(d, precision)
    E.fused_stem_check(d, r)
    n, h, w, hp, wp, ch, cw, ph, pw = E.fused_stem_sizes(image)
    rows = _library().lh_stem_conv_rows(n, ch, cw)
    rid = E.stem_conv_row_of_pixel(n, ch, cw, rows).reshape(-1)
    assert rid.numel() == n * ch * cw and int(rid.max()) == rows - 1 and len(torch.unique(rid)) == rows
    v = r["conv16"].double().reshape(-1, 64)
    assert torch.equal(v, r["acc"].reshape(-1, 64))                                     # no value of this flavour needs a rounding
    s1 = torch.zeros(rows, 64, dtype=torch.float64).index_add_(0, rid, v)
    s1m = torch.zeros(rows, 64, dtype=torch.float64).index_add_(0, rid, v.abs())
    s2 = torch.zeros(rows, 64, dtype=torch.float64).index_add_(0, rid, v * v)
    print(image, precision, f"{rows} rows; largest row: sum of magnitudes {float(s1m.max()):.0f}, sum of squares {float(s2.max()):.0f}")
    assert float(s1m.max()) < E.LIMIT and float(s2.max()) < E.LIMIT
    assert torch.equal(s1.float().double(), s1) and torch.equal(s2.float().double(), s2)
    assert torch.equal(s1.sum(0), r["s1"]) and torch.equal(s2.sum(0), r["s2"])


def test_stem_tap_loop_equals_conv2d():
    """The stem convolution restated on the kernels' operands -- padded NHWC4 image, weight rows of 8 pixels x 4 channels
    (exact_data.fused_stem_layout, fused_stem_tap_conv) -- against F.conv2d(stride 2, padding 3) in fp64, on the odd-sized cases."""
    for image in ("tiny", "ragged"):
        d = E.fused_stem_data(image, "fp16")
        n, h, w, hp, wp, ch, cw, ph, pw = E.fused_stem_sizes(image)
        img, stage = E.fused_stem_layout(d["x"], d["w"])
        assert img.shape == (n, hp, wp, 4) and hp >= 2 * (ch - 1) + 7 and wp >= 2 * (cw - 1) + 8
        want = F.conv2d(d["x"].double(), d["w"].double(), None, 2, 3).permute(0, 2, 3, 1)
        assert torch.equal(E.fused_stem_tap_conv(img, stage, ch, cw), want)
        assert torch.equal(E.fused_stem_reference(d, "fp16")["acc"], want)


_BNECK_RUNS = [(cin, shape, res) for cin in E.BNECK_CIN for shape in E.BNECK_SHAPES for res in (("separate", "x") if cin == 256 else ("separate",))]


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("cin,shape,res", _BNECK_RUNS)
def test_bottleneck_cases_meet_the_preconditions(cin, shape, res, precision):
    """lh_bottleneck_infer: (a) for each of the three layers and for the last sum (bneck_check), (b) on every value any of the four
    roundings meets, ReLU or not, (c) on the block output, and at least 100 real roundings in front of each intermediate; several
    channels of b1 and b2 are strictly positive and alive."""
    dt = E.DTYPES[precision]
    d = E.bneck_data(cin, shape, precision)
    rng, base = E.bneck_ranges(cin, shape, precision), E.BNECK_RANGES[precision]
    assert all(rng[k] >= base[k] for k in ("x", "w1", "w2", "w3", "res")) and all(a >= b for a, b in zip(rng["k"], base["k"]))   # never narrowed
    for k in ("x", "w1", "w2", "w3", "res"):
        assert _held_exactly(d[k], dt) and torch.equal(d[k], d[k].round()), k
    for l in (1, 2, 3):
        assert torch.equal(d[f"s{l}"].float().double(), d[f"s{l}"]) and torch.equal(d[f"b{l}"].float().double(), d[f"b{l}"])
    assert float(d["b1"][:E.BNECK_POSITIVE].min()) > 0 and float(d["b2"][:E.BNECK_POSITIVE].min()) > 0
    r = E.bneck_reference(d, precision, d["x"] if res == "x" else None)
    worst = E.bneck_check(d, r)                                                         # (a)
    # a positive shift that matters: relu(b1) would be stored in the halo by a kernel that forgot conv2's zero padding
    assert float(E.expected_16(torch.relu(d["b1"][:E.BNECK_POSITIVE]), dt).min()) > 0 and float(r["a2"][..., :E.BNECK_POSITIVE].max()) > 0
    peak = max(float(r[k].abs().max()) for k in ("raw1", "raw2", "pre3", "pre_out"))
    if precision == "fp16":
        _no_fp16_trouble({k: r[k] for k in ("raw1", "raw2", "pre3", "pre_out", "a1", "a2", "y3", "out")}, (cin, shape))     # (b)
    counts = {k: E.rounding_counts(r[k], dt) for k in ("pre1", "pre2", "pre3", "pre_out")}
    print(cin, shape, res, precision, "largest sums of magnitudes (conv1, conv2, conv3, y3 + residual): " + ", ".join(f"{m:.0f}" for m in worst)
          + f"; peak {peak:.0f}; (need rounding, ties) of a1, a2, y3, out: {list(counts.values())}")
    assert counts["pre_out"][0] >= 100 and counts["pre_out"][1] >= 10                   # (c)
    assert all(counts[k][0] >= 100 for k in ("pre1", "pre2", "pre3"))


def test_bottleneck_reference_equals_three_conv2d_calls():
    """exact_data.bneck_reference (matrix products on NHWC for the 1x1 layers) against three F.conv2d calls on NCHW with the same roundings."""
    for cin, precision in ((96, "bf16"), (256, "fp16")):
        dt = E.DTYPES[precision]
        d = E.bneck_data(cin, "ragged", precision)
        r = E.bneck_reference(d, precision)
        r16 = lambda t: t.float().to(dt).double()
        aff = lambda t, l: t * d[f"s{l}"].view(1, -1, 1, 1) + d[f"b{l}"].view(1, -1, 1, 1)
        x = d["x"].permute(0, 3, 1, 2)
        a1 = r16(torch.relu(aff(F.conv2d(x, d["w1"].view(64, cin, 1, 1)), 1)))
        a2 = r16(torch.relu(aff(F.conv2d(a1, d["w2"], None, 1, 1), 2)))
        y3 = r16(aff(F.conv2d(a2, d["w3"].view(256, 64, 1, 1)), 3))
        out = r16(torch.relu(y3 + d["res"].permute(0, 3, 1, 2)))
        assert torch.equal(out.permute(0, 2, 3, 1), r["out"]) and torch.equal(a2.permute(0, 2, 3, 1), r["a2"])


def _library():
    from lighthand_amd import _lib
    return _lib.load()


def test_multi_tile_cases_walk_the_persistent_loops():
    """The grid queries (host arithmetic) on the shapes alone: lh_stem_pool_grid, lh_stem_conv_rows and lh_bottleneck_infer_grid answer
    min(tiles, cap) -- one workgroup per tile on the small cases --, and on the multi-tile cases every workgroup takes at least two tiles,
    some take one more, and the tile count is no multiple of the grid (the prefetch behind a workgroup's last tile is the zero fill)."""
    import ctypes as C
    from lighthand_amd import _lib
    lib = _lib.load()
    up = lambda a, b: -(-a // b)
    for image in E.FUSED_STEM_IMAGES:
        n, h, w, hp, wp, ch, cw, ph, pw = E.fused_stem_sizes(image)
        for grid, tiles in ((lib.lh_stem_pool_grid(n, ch, cw), n * up(ph, 8) * up(pw, 8)), (lib.lh_stem_conv_rows(n, ch, cw), n * up(ch, 16) * up(cw, 16))):
            assert 0 < grid <= tiles
            if image == "multi":
                assert tiles > 2 * grid and tiles % grid != 0 and up(tiles, grid) >= 3, (tiles, grid)
            else:
                assert grid == tiles
    assert E.fused_stem_sizes("tiny")[5:] == (5, 4, 3, 2) and E.fused_stem_sizes("ragged")[5:] == (35, 45, 18, 23) and E.fused_stem_sizes("multi")[5:] == (33, 33, 17, 17)
    for shape, (n, h, w) in E.BNECK_SHAPES.items():
        for cin in E.BNECK_CIN:
            bd = _lib.BottleneckDesc(n, h, w, cin, 64, 256)
            grid, tiles = lib.lh_bottleneck_infer_grid(C.byref(bd)), n * up(h, 16) * up(w, 16)
            assert 0 < grid <= tiles
            if shape == "multi":
                assert tiles > 2 * grid and tiles % grid != 0 and up(tiles, grid) >= 3, (tiles, grid)
            else:
                assert grid == tiles
    assert lib.lh_bottleneck_infer_grid(C.byref(_lib.BottleneckDesc(0, 17, 17, 64, 64, 256))) == 0 and lib.lh_bottleneck_infer_grid(None) == 0
    assert sorted((cin // 32 + 5) % 4 for cin in E.BNECK_CIN) == [0, 1, 2, 3]           # every phase of the four-slot ring at a tile boundary


# ---------------------------------------------------------------------------------------------------------------------------------
# The multi-problem launches of tests/test_gpu_multi_exact.py: the configuration lists against the library's candidate queries, the
# arithmetic of the members (stages, splits, launch order), their preconditions, and that no two members of a call expect the same
# values -- a launch that pairs a member with another member's buffer cannot pass (host arithmetic: no GPU).
_CODE = dict(bf16=1, fp16=2, fp32=0)                  # LH_BF16, LH_F16, LH_F32


def _epilogue_desc(case, cfg=None):
    from lighthand_amd import _lib
    n, hi, wi, cin, ho, wo, cout, OH, OW, osh, osw, ooh, oow, taps = E.EPILOGUE_CASES[case]
    d = _lib.IgemmDesc()
    d.n, d.hi, d.wi, d.in_pix_stride, d.k_run = n, hi, wi, cin, cin
    d.ho, d.wo, d.sh, d.sw, d.cout = ho, wo, 1, 1, cout
    d.OH, d.OW, d.osh, d.osw, d.ooh, d.oow, d.out_pix_stride = OH, OW, osh, osw, ooh, oow, cout
    d.ntaps = len(taps)
    for t, (dh, dw) in enumerate(taps):
        d.dh[t], d.dw[t] = dh, dw
    for i, v in enumerate(cfg or ()):
        d.cfg[i] = v
    return d


def _igemm_candidates(lib, d, code):
    import ctypes as C
    buf = (C.c_int * (5 * 320))()
    nc = lib.lh_igemm_candidates(C.byref(d), code, buf, 320)
    assert 0 < nc < 320
    return [tuple(buf[5 * i:5 * i + 4]) for i in range(nc)]


def _engine_merges(c):
    """The rule of BatchGroups._merge_groups for a tiled member configuration (bm, bp, depth, kb)."""
    from lighthand_amd.batch_groups import BatchGroups
    return 2 <= c[2] < 10 and (c[0], c[1]) in BatchGroups._MULTI_TILES


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_multi_ring_cfgs_are_the_four_wave_candidates_and_the_engine_s_partition(precision):
    """exact_data.MULTI_RING_CFGS against the library and the engine: lh_igemm_candidates offers the largest member every entry; every
    candidate of any member that the engine's rule would merge is an entry (the GPU test runs every entry), every other candidate is one
    the rule rejects; and no entry is refused for any member (cfg_safe: K = 40 is 80 bytes, above the 64 of the 128-byte stage)."""
    import ctypes as C
    lib = _library()
    copy = set(E.MULTI_RING_CFGS)
    assert len(E.MULTI_RING_CFGS) == len(copy) == 21 and all(_engine_merges(c) for c in copy)
    cands = _igemm_candidates(lib, _epilogue_desc("c136"), _CODE[precision])
    assert copy <= set(cands), copy - set(cands)
    assert {c for c in cands if 2 <= c[2] < 10 and c[0] <= 128 and c[1] <= 128} == copy
    rejected = set()
    for case in E.MULTI_MEMBERS:
        for c in _igemm_candidates(lib, _epilogue_desc(case), _CODE[precision]):
            assert _engine_merges(c) == (c in copy), (case, c)
            if not _engine_merges(c):
                rejected.add(c)
        for c in E.MULTI_RING_CFGS:
            got = (C.c_int * 5)()
            assert lib.lh_igemm_config(C.byref(_epilogue_desc(case, c)), _CODE[precision], got) == 0, (case, c, lib.lh_last_error())
            assert tuple(got[:4]) == c
    # what the rule rejects and the GPU test must see refused: dense-wave forms, 256-wide tiles, the pointwise kernel
    assert {_kind(c) for c in rejected} == {"dense", "wide", "pointwise"}, rejected


def _kind(c):
    from lighthand_amd import _lib
    k = _lib.conv_kind(c[2])
    return "wide" if k == "tiled" and max(c[0], c[1]) == 256 else k


def test_multi_igemm_members_sit_where_the_test_says():
    """m35 is one workgroup under a 128-channel tile and the smallest member; the library's sort (longest K loop first, stable) is a real
    permutation of the first four members and of the n = 3 call for both stage sizes; every mode is used, "phase" never with mask bits,
    and the members of a call never share a mode (but in the all-"stats" call)."""
    assert E.EPILOGUE_CASES["m35"][:9] == (1, 5, 7, 40, 5, 7, 72, 5, 7) and len(E.EPILOGUE_CASES["m35"][13]) == 1
    for bm, bp, _, kb in E.MULTI_RING_CFGS:
        tiles = {m: -(-(E.EPILOGUE_CASES[m][0] * E.EPILOGUE_CASES[m][4] * E.EPILOGUE_CASES[m][5]) // bp) * -(-E.EPILOGUE_CASES[m][6] // bm) for m in E.MULTI_MEMBERS}
        assert tiles["m35"] == (1 if bm == 128 else 2) and all(tiles[m] > tiles["m35"] for m in E.MULTI_MEMBERS if m != "m35"), tiles
        for members in (E.MULTI_MEMBERS[:4], E.MULTI_TRIPLE):
            order = E.multi_launch_order(members, kb)
            assert sorted(order) == list(range(len(members))) and order != list(range(len(members))), (members, kb, order)
        assert E.multi_launch_order(E.MULTI_MEMBERS[:4], kb) == [3, 1, 0, 2]
    used = set()
    for name, flavour, call in E.multi_igemm_calls():
        modes = [mode for _, mode in call]
        used |= set(modes)
        assert ("phase", "addend_mask") not in call and (len(set(modes)) == len(modes) or name == "five stats")
    assert used == set(E.MULTI_MODES) and len(E.MULTI_MODES) == 7
    for m in E.MULTI_MEMBERS:              # an addend and an epilogue vector at least once each, and a call without either
        mine = {E.multi_mode(m, r) for r in range(3)}
        assert mine & {"addend", "addend_mask"} and mine & {"bias", "affine_relu"} and len(mine) == 3, (m, mine)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_multi_igemm_members_expect_different_values(precision):
    """For every call of the GPU test, any two members' expected outputs differ in EVERY one of the first min(rows) rows they share (on the
    channels they share), and in the all-"stats" call any two members' column sums differ in both rows: no swap of two members' output,
    addend, vector or slab pointers can pass.  The rows that must be exact are: the sums of any "stats" member, and in "exact_small" the sums
    of squares as well."""
    dt = E.DTYPES[precision]
    for name, flavour, call in E.multi_igemm_calls():
        want = [E.epilogue_expected(m, precision, mode, flavour) for m, mode in call]
        for i in range(len(call)):
            for j in range(i + 1, len(call)):
                r, c = min(want[i].shape[0], want[j].shape[0]), min(want[i].shape[1], want[j].shape[1])
                assert bool((want[i][:r, :c] != want[j][:r, :c]).any(1).all()), (name, call[i], call[j])
        sums = {}
        for (m, mode), v in zip(call, want):
            assert torch.equal(v.to(dt).float(), v)
            if mode == "stats":
                sd = v.double()
                assert E.check_exact_rows(sd)[0] and (flavour == "exact" or E.check_exact_rows(sd * sd)[0]), (name, m)
                sums[m] = torch.stack([sd.sum(0), (sd * sd).sum(0)])
        for a in sums:
            for b in sums:
                if a < b:
                    c = min(sums[a].shape[1], sums[b].shape[1])
                    differ = (sums[a][:, :c] != sums[b][:, :c]).double().mean(1)
                    assert float(differ.min()) > 0.9, (name, a, b, differ)


def test_wgrad_multi_cfgs_are_the_four_wave_candidates():
    """exact_data.WGRAD_MULTI_CFGS against lh_wgrad_candidates on a member both of whose channel counts fill more than half of any tile: the
    four-wave plans offered are exactly the copy; the 256 x 256 tile is offered to (and resolves for) the members with 136 channels on both
    sides only."""
    import ctypes as C
    from lighthand_amd import _lib
    lib = _library()
    assert len(set(E.WGRAD_MULTI_CFGS)) == 16
    for precision in ("bf16", "fp16"):
        seen = {}
        for member, (cin, cout, *_rest) in E.WGRAD_MULTI_CASES.items():
            buf = (C.c_int * (5 * 320))()
            nc = lib.lh_wgrad_candidates(C.byref(E.wgrad_desc(_lib.IgemmDesc(), member)), cout, cin, _CODE[precision], buf, 320)
            assert 0 < nc < 320
            seen[member] = {(buf[5 * i], buf[5 * i + 1], (buf[5 * i + 2] >> 16) & 0xff, (buf[5 * i + 2] >> 24) & 0xff) for i in range(nc)}
            assert {c for c in seen[member] if c[0] <= 128 and c[1] <= 128} == set(E.WGRAD_MULTI_CFGS), member
            big = C.byref(E.wgrad_desc(_lib.IgemmDesc(), member, E.WGRAD_BIG_CFG, 1))
            out = [C.c_int() for _ in range(4)]
            rc = lib.lh_wgrad_tile(big, cout, cin, _CODE[precision], *[C.byref(v) for v in out])
            assert (rc == 0) == (E.WGRAD_BIG_CFG in seen[member]) == (cin == 136 and cout == 136), (member, rc)
        assert E.WGRAD_BIG_CFG in seen["W5"]
    # fp32 has no LDS-DMA weight gradient: no candidates, and an explicit ring plan is refused (LH_ERR_UNSUPPORTED)
    d = E.wgrad_desc(_lib.IgemmDesc(), "W5", E.WGRAD_MULTI_CFGS[0])
    out = [C.c_int() for _ in range(4)]
    assert lib.lh_wgrad_candidates(C.byref(d), 136, 136, 0, (C.c_int * 50)(), 10) == 0
    assert lib.lh_wgrad_tile(C.byref(d), 136, 136, 0, *[C.byref(v) for v in out]) == -3 and b"is not available for this launch" in lib.lh_last_error()


def test_wgrad_multi_stage_and_split_arithmetic():
    """The members' pixel counts, stage counts and ragged last stages from the shapes; the plans lh_wgrad_tile resolves for every compiled
    four-wave configuration and fitting member -- the requested tile, stage, depth and split count, unchanged --; at least two members
    fit every configuration; and the library's order of every first launch (most stages per split first, stable) is a real permutation of
    the caller's.  Static plans (cfg[5..7] = 0) put all five members into one tile class."""
    import ctypes as C
    from lighthand_amd import _lib
    lib = _library()
    assert {m: E.wgrad_sizes(m) for m in E.WGRAD_MULTI_CASES} == {"W1": (286, 13, 11), "W2": (35, 5, 7), "W3": (20, 5, 4), "W4": (189, 7, 9), "W5": (60, 6, 10)}
    assert E.wgrad_plan("W1", 32) == (9, 3, 3) and E.wgrad_plan("W1", 64) == (5, 2, 3) and 286 % 32 == 286 % 64 == 30      # ragged last stage
    assert E.wgrad_plan("W4", 32) == (6, 3, 2) and E.wgrad_plan("W4", 64) == (3, 2, 2) and 189 % 32 == 29 and 189 % 64 == 61
    assert E.wgrad_plan("W2", 64) == (1, 1, 1) and E.wgrad_plan("W2", 32) == (2, 2, 1) and E.wgrad_plan("W3", 32) == (1, 1, 1) and E.wgrad_plan("W5", 32) == (2, 2, 1)
    for cfg in E.WGRAD_MULTI_CFGS:
        bo, bi, kps, depth = cfg
        members = E.WGRAD_MULTI_ORDER[(bo, bi)]
        assert members == [m for m in members if E.wgrad_fits(m, bo, bi)] and set(members) == {m for m in E.WGRAD_MULTI_CASES if E.wgrad_fits(m, bo, bi)}
        assert len(members) >= 2
        order = E.wgrad_launch_order(members[:4], kps)
        assert sorted(order) == list(range(len(order))) and order != list(range(len(order))), (cfg, order)
        for precision in ("bf16", "fp16"):
            for m in members:
                cin, cout, k = E.WGRAD_MULTI_CASES[m][:3]
                d = E.wgrad_desc(_lib.IgemmDesc(), m, cfg)
                out = [C.c_int() for _ in range(4)]
                assert lib.lh_wgrad_tile(C.byref(d), cout, cin, _CODE[precision], *[C.byref(v) for v in out]) == 0, (cfg, m, lib.lh_last_error())
                assert [v.value for v in out] == [bo, bi, E.wgrad_plan(m, kps)[2], kps * 10 + depth], (cfg, m)
                assert out[2].value == E.WGRAD_MULTI_SPLITS.get(m, 1)                     # the request, unchanged
                assert lib.lh_wgrad_workspace_bytes(C.byref(d), cout, cin, _CODE[precision]) == out[2].value * k * k * cout * cin * 4
    # members the slack / layout / accumulate variations sit on run under every tile class they fit
    assert E.WGRAD_MULTI_ACCUMULATE in E.WGRAD_MULTI_ORDER[(64, 64)] and all(E.WGRAD_MULTI_TRANSPOSED in v for v in E.WGRAD_MULTI_ORDER.values())
    for precision in ("bf16", "fp16"):
        plans = set()
        for m, (cin, cout, *_r) in E.WGRAD_MULTI_CASES.items():
            out = [C.c_int() for _ in range(4)]
            assert lib.lh_wgrad_tile(C.byref(E.wgrad_desc(_lib.IgemmDesc(), m)), cout, cin, _CODE[precision], *[C.byref(v) for v in out]) == 0
            plans.add((out[0].value, out[1].value, out[3].value))
        assert plans == {(128, 128, 324)}


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("member", list(E.WGRAD_MULTI_CASES))
def test_wgrad_multi_members_meet_the_preconditions(member, precision):
    """check_exact on every member in every precision; fp32 holds the expected gradient (with the accumulating member's prefill) exactly;
    the gradient is dense, so every pixel counts; and the slack fill is held by both 16-bit types."""
    m = E.wgrad_member(member, precision)
    dt = E.DTYPES[precision]
    for k in ("x", "dy"):
        assert torch.equal(m[k].to(dt).float(), m[k]) and torch.equal(m[k], m[k].round())
    worst = E.check_exact(m["x"], m["w"], None, m["dy"], E.WGRAD_MULTI_CASES[member])
    want = E.wgrad_expected(member, precision)
    cin, cout, k = E.WGRAD_MULTI_CASES[member][:3]
    assert want.shape == ((cin, cout, k, k) if member == E.WGRAD_MULTI_TRANSPOSED else (cout, cin, k, k)) and want.dtype == torch.float32
    assert float((m["dw"] != 0).double().mean()) > 0.9
    assert (m["pre"] is not None) == (member == E.WGRAD_MULTI_ACCUMULATE)
    assert float(torch.tensor(E.WGRAD_SLACK_FILL).to(torch.bfloat16)) == float(torch.tensor(E.WGRAD_SLACK_FILL).to(torch.float16)) == E.WGRAD_SLACK_FILL
    print(member, precision, f"largest sum of magnitudes {worst:.0f}, largest gradient element {float(m['dw'].abs().max()):.0f}")


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_wgrad_multi_members_expect_different_gradients(precision):
    """Any two members' expected gradient tensors differ in most of the elements they share (compared flat, in the layout each is stored
    in, over the shorter one's length): a gradient folded from another member's slab, or written to another member's tensor, cannot pass."""
    want = {m: E.wgrad_expected(m, precision).flatten() for m in E.WGRAD_MULTI_CASES}
    for a in want:
        for b in want:
            if a < b:
                n = min(want[a].numel(), want[b].numel())
                assert float((want[a][:n] != want[b][:n]).double().mean()) > 0.9, (a, b)
