"""Exact-arithmetic data for the convolution tests: operands that are integer multiples of a power-of-two quantum, small enough that
EVERY partial sum of every output, input-gradient and weight-gradient element, in any order, is an integer (times the product quantum)
below 2^24 -- which fp32 holds exactly.  An fp32 accumulator is then exact whatever the tile, ring depth, split count or MFMA order, and a
stored 16-bit value must equal ONE round-to-nearest-even of the exact result: the tests compare with torch.equal, tolerance zero.

The bound is derived, not measured: |any partial sum| <= sum of the magnitudes of its terms <= the same convolution of |x|, |w|, |dy|
(check_exact computes exactly that, in fp64, on the reference alone).  The reference is torch.nn.functional in float64 on the CPU: sums of
integers below 2^53 are exact there in any order too."""
import torch
import torch.nn.functional as F

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
# precision -> (a for x and dy, a for w): values are drawn uniformly from the integers [-a, a]
RANGES = {"bf16": (8, 4), "fp16": (32, 8), "fp32": (32, 8)}
LIMIT = float(1 << 24)
FP16_MAX = 65504.0
_SIG = {torch.bfloat16: (8, -126), torch.float16: (11, -14), torch.float32: (24, -126)}     # significand bits, smallest normal exponent

# Plan-level cases of tests/test_gpu_exact_conv.py: (cin, cout, k, stride, pad, n, h, w)
CONV_CASES = [
    (40, 72, 3, 1, 1, 2, 13, 11),       # partial K stage (80 of 128 bytes), 286 pixels (ragged second pixel tile), 72 channels fill no tile
    (48, 96, 3, 2, 1, 1, 9, 7),         # stride 2 on odd sizes: the data gradient's sub-pixel phases have unequal grids
    (96, 48, 1, 1, 0, 1, 5, 7),         # pointwise, 35 pixels (less than one wave step), K no multiple of 64
    (64, 136, 1, 2, 0, 2, 9, 7),        # strided 1x1: the data gradient writes a strided placement, other phases exactly zero
    (256, 21, 1, 1, 0, 1, 8, 8),        # padded output channels, bias (its gradient: lh_channel_sum_nhwc)
    (32, 64, 3, 1, 1, 1, 7, 5),         # direct 3x3, map smaller than an 8 x 16 tile
    (64, 32, 3, 1, 1, 2, 9, 17),        # direct 3x3 across tile borders in both directions; the data gradient has K = 32
    (8, 32, 3, 1, 1, 1, 6, 10),         # K run shorter than a ring stage
    (128, 256, 3, 1, 1, 2, 9, 9),       # K = 1152, 162 pixels: the 256 x 256 tile
    (512, 128, 1, 1, 0, 1, 8, 8),       # pointwise at its K limit
    (16, 16, 3, 1, 1, 1, 3, 3),         # every pixel is a border pixel
    # added from reading wgrad_plan.h (wgrad_splits keeps >= 256 pixels per workgroup, so the cases above run split-free or in two
    # halves): 663 pixels give THREE pixel splits -- of unequal length with 64-row stages (4 + 4 + 3) --, a ragged last stage (663 = 20 x 32
    # + 23) and images (221 pixels) that straddle every split boundary; forward and data gradient get a ragged third 256-pixel tile
    (16, 24, 3, 1, 1, 3, 13, 17),
]
# Transposed cases: (cin, cout, k, n, h, w), stride 2, padding / output padding as in tests/test_gpu_ops.py
DECONV_CASES = [(32, 16, 2, 1, 4, 4), (32, 32, 3, 1, 5, 3), (64, 32, 4, 2, 5, 3)]
DECONV_PAD = {4: (1, 0), 3: (1, 1), 2: (0, 0)}

# Ranges widened where the default ones leave condition (c) of tests/test_exact_host.py unmet (too few sums large enough to need a
# rounding in a small case): (case, precision) -> (a for x and dy, a for w).  Filled from that test's failures; never narrower.
WIDER = {
    ((96, 48, 1, 1, 0, 1, 5, 7), "bf16"): (16, 4), ((96, 48, 1, 1, 0, 1, 5, 7), "fp16"): (64, 8), ((96, 48, 1, 1, 0, 1, 5, 7), "fp32"): (64, 8),
    ((64, 136, 1, 2, 0, 2, 9, 7), "fp16"): (64, 8), ((64, 136, 1, 2, 0, 2, 9, 7), "fp32"): (64, 8),
    ((8, 32, 3, 1, 1, 1, 6, 10), "bf16"): (16, 4), ((8, 32, 3, 1, 1, 1, 6, 10), "fp16"): (64, 8), ((8, 32, 3, 1, 1, 1, 6, 10), "fp32"): (64, 8),
    ((16, 16, 3, 1, 1, 1, 3, 3), "bf16"): (32, 8), ((16, 16, 3, 1, 1, 1, 3, 3), "fp16"): (128, 16), ((16, 16, 3, 1, 1, 1, 3, 3), "fp32"): (128, 16),
    ((32, 16, 2, 1, 4, 4), "bf16"): (16, 8), ((32, 16, 2, 1, 4, 4), "fp16"): (64, 16), ((32, 16, 2, 1, 4, 4), "fp32"): (64, 16),
    ((32, 32, 3, 1, 5, 3), "bf16"): (16, 4), ((32, 32, 3, 1, 5, 3), "fp16"): (64, 8), ((32, 32, 3, 1, 5, 3), "fp32"): (64, 8),
}


def case_bias(case):
    return case[1] == 21


def ranges(case, precision):
    return WIDER.get((tuple(case), precision), RANGES[precision])


def ints(shape, a, gen):
    """Integers drawn uniformly from [-a, a], as float32."""
    return torch.randint(-a, a + 1, tuple(shape), generator=gen).float()


def conv_data(case, precision, seed=100, bias=None, transposed=False):
    """x, w, bias (or None), dy of a case as float32 tensors of small integers (NCHW / the torch weight layouts)."""
    g = torch.Generator().manual_seed(seed)
    ax, aw = ranges(case, precision)
    if transposed:
        cin, cout, k, n, h, w = case
        pad, opad = DECONV_PAD[k]
        ho, wo = (h - 1) * 2 - 2 * pad + k + opad, (w - 1) * 2 - 2 * pad + k + opad
        wshape = (cin, cout, k, k)
    else:
        cin, cout, k, s, p, n, h, w = case
        ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        wshape = (cout, cin, k, k)
        if bias is None:
            bias = case_bias(case)
    x = ints((n, cin, h, w), ax, g)
    wt = ints(wshape, aw, g)
    b = ints((cout,), ax, g) if bias else None
    dy = ints((n, cout, ho, wo), ax, g)
    return x, wt, b, dy


def _conv(x, w, b, case, transposed):
    if transposed:
        pad, opad = DECONV_PAD[case[2]]
        return F.conv_transpose2d(x, w, b, 2, pad, opad)
    return F.conv2d(x, w, b, case[3], case[4])


def reference(x, w, b, dy, case, transposed=False):
    """fp64 host reference: dict(out, dx, dw, db) -- exact for integer operands (every sum stays far below 2^53)."""
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if b is not None else None
    out = _conv(xr, wr, br, case, transposed)
    out.backward(dy.double())
    return dict(out=out.detach(), dx=xr.grad, dw=wr.grad, db=br.grad if br is not None else None)


def check_exact(x, w, b, dy, case, transposed=False, qx=1.0, qw=1.0, qdy=1.0):
    """The precondition, on the reference alone: the same convolution of |x|, |w|, |dy| (+ |bias|), divided by the product quantum, stays
    below 2^24 for every output, input-gradient, weight-gradient and bias-gradient element.  qx, qw, qdy: the power-of-two quanta of
    which x, w and dy are integer multiples (the bias is a multiple of qx * qw).  Returns the largest such sum, in quanta."""
    for t, q in ((x, qx), (w, qw), (dy, qdy)) + (((b, qx * qw),) if b is not None else ()):
        assert bool((t.double() / q == torch.round(t.double() / q)).all()), f"{case}: an operand is no integer multiple of its quantum {q}"
    mag = reference(x.abs(), w.abs(), b.abs() if b is not None else None, dy.abs(), case, transposed)
    quanta = dict(out=qx * qw, dx=qdy * qw, dw=qx * qdy, db=qdy)
    worst = 0.0
    for k, v in mag.items():
        if v is None:
            continue
        m = float(v.max()) / quanta[k]
        assert m < LIMIT, f"{case}: sum of magnitudes of {k} is {m:.0f} >= 2^24"
        worst = max(worst, m)
    return worst


def expected_16(v, dtype):
    """What a kernel must store for the exact value v: one round-to-nearest-even (fp32 holds v exactly under check_exact)."""
    return v.float().to(dtype)


def rounding_counts(v, dtype):
    """(elements of the exact tensor v that are not representable in dtype, those of them that sit exactly half-way between two
    neighbours): the ties are where round-to-nearest-even differs from round-half-away and both differ from truncation."""
    sig, emin = _SIG[dtype]
    a = v.double().abs()
    _, ex = torch.frexp(a)                                   # a = m * 2^ex with m in [0.5, 1)
    ulp = torch.ldexp(torch.ones_like(a), ex.clamp_min(emin + 1) - sig)
    frac = torch.remainder(a, ulp)
    return int((frac != 0).sum()), int((frac == ulp / 2).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# Tap-list convolution on NHWC operands: the host side of tests/test_gpu_epilogue_modes.py (tests/test_exact_host.py holds it against
# F.conv2d / F.conv_transpose2d).
def tap_conv(x, w, taps, ho, wo, dtype=torch.float32):
    """acc[n][a][b][co] = sum_t sum_k x[n][a + dh_t][b + dw_t][k] * w[co][t][k], zero outside the image; x [n][hi][wi][cin], w [cout][taps][cin]."""
    n, hi, wi, cin = x.shape
    pad = 2
    xp = torch.zeros(n, hi + 2 * pad, wi + 2 * pad, cin, dtype=dtype)
    xp[:, pad:pad + hi, pad:pad + wi] = x.to(dtype)
    acc = torch.zeros(n, ho, wo, w.shape[0], dtype=dtype)
    for t, (dh, dw) in enumerate(taps):
        acc += xp[:, pad + dh:pad + dh + ho, pad + dw:pad + dw + wo] @ w[:, t].to(dtype).t()
    return acc


# Epilogue-mode cases (tests/test_gpu_epilogue_modes.py): name -> (n, hi, wi, cin, ho, wo, cout, OH, OW, osh, osw, ooh, oow, taps (dh, dw))
_T3 = [(r - 1, s - 1) for r in range(3) for s in range(3)]
EPILOGUE_CASES = {
    "c72": (2, 13, 11, 40, 13, 11, 72, 13, 11, 1, 1, 0, 0, _T3),
    "c136": (2, 13, 11, 40, 13, 11, 136, 13, 11, 1, 1, 0, 0, _T3),
    "phase": (2, 9, 7, 40, 9, 7, 136, 18, 14, 2, 2, 1, 0, [(1, 0), (1, -1), (0, 0), (0, -1)]),
}
# Exact flavours of the epilogue data: flavour -> precision -> (a for x and gx, a for w, a for the addend).
#   "exact": the ranges of the plan-level tests; the addend spans the integers the type holds exactly, so both roundings of an
#            addend mode (accumulator, then accumulator + addend) move bits.
#   "exact_small": small enough that the sums of SQUARES of the stored values stay below 2^24 as well.  No data can do both in fp16: a
#            value that needs rounding has more than 11 significant bits, so its square is above 2^22 quanta and four of them pass
#            2^24 -- the statistics' second row is exact only on values that need no rounding.
EPILOGUE_RANGES = {"exact": {"bf16": (8, 4, 255), "fp16": (32, 8, 2047)}, "exact_small": {"bf16": (4, 2, 64), "fp16": (4, 2, 64)}}

# ---- the persistent kernels (tests/test_gpu_persistent_epilogue.py): pointwise (igemm_pw_kernel.h) and direct 3x3 (conv3x3_direct_kernel.h).
# The compiled pointwise configurations (BM, KC, PT) = channels of the resident weight panel, padded K of the panel, 16-pixel sub-tiles a
# wave takes per step: a copy of LH_PW_CFGS (igemm_pw_cfgs.h), held against lh_igemm_candidates by the GPU test.
PW_CFGS = [(256, 64, 1), (128, 64, 2), (64, 64, 2), (64, 64, 4), (256, 128, 1), (128, 128, 2), (64, 128, 2),
           (256, 256, 1), (128, 256, 1), (128, 256, 2), (64, 256, 1), (64, 256, 2), (128, 512, 1), (64, 512, 1)]
PW_K = {64: 40, 128: 72, 256: 136, 512: 264}        # panel K -> the K run of its cases: ragged against the panel (136: kpad 192 of 256, 264: 320 of 512)
PERSISTENT_COUT = 136      # a 256-channel panel part-filled, a second 128-channel block of 8 channels, a third 64-channel block of 8


def _same(n, h, w, cin, taps, cout=PERSISTENT_COUT):
    """A stride-1, same-size, dense case in the layout of EPILOGUE_CASES."""
    return (n, h, w, cin, h, w, cout, h, w, 1, 1, 0, 0, taps)


# Short cases: 286 pixels (ragged against 16, 32 and 64 pixels per wave step) for the pointwise kernel, 21 x 19 (ragged against 16 x 16 tiles,
# every border) for the direct one.
EPILOGUE_CASES.update({f"pw{k}": _same(2, 13, 11, k, [(0, 0)]) for k in PW_K.values()})
EPILOGUE_CASES.update({f"d{c}": _same(2, 21, 19, c, _T3) for c in (32, 64)})
EPILOGUE_SHORT = ["c72", "c136", "phase"] + [f"pw{k}" for k in PW_K.values()] + ["d32", "d64"]
# "exact" ranges widened where the default ones leave too few accumulators that need rounding (one tap, short K): (case, precision) ->
# (a for x and gx, a for w).  From the failures of tests/test_exact_host.py; never narrower.
EPILOGUE_WIDER = {("pw40", "bf16"): (16, 8), ("pw40", "fp16"): (64, 16), ("pw72", "fp16"): (64, 16)}


# Long cases: enough pixels that EVERY wave of a pointwise launch (workgroup of a direct one) walks its tile loop at least twice and some
# three times, at any occupancy the library may pick.  Pointwise: the grid has at most G = 1024 / cb / 8 * 8 workgroups per channel block
# (occupancy <= 4: pw_occupancy; cb channel blocks), four waves each, so 8 G + 5 wave tiles of 16 PT pixels do it; + 3 pixels keep the
# last tile ragged.  One image of width 61; the cases of one K class are row prefixes of the class's largest (EPILOGUE_BASE).
# Direct: at most g = 512 / cb / 8 * 8 = 168 workgroups per channel block; 2 x 197 x 211 is 2 x 13 x 14 = 364 >= 2 g + 5 tiles of 16 x 16.
def pw_long_grid_cap(bm, cout=PERSISTENT_COUT):
    return 1024 // ((cout + bm - 1) // bm) // 8 * 8


def _pw_long_rows(bm, pt, wo=61):
    need = 16 * pt * (8 * pw_long_grid_cap(bm) + 5) + 3
    ho = (need + wo - 1) // wo
    while (ho * wo) % 16 == 0:
        ho += 1
    return ho


EPILOGUE_BASE = {}
for _kc, _k in PW_K.items():
    _rows = {(bm, pt): _pw_long_rows(bm, pt) for bm, kc, pt in PW_CFGS if kc == _kc}
    EPILOGUE_CASES[f"long_pw{_k}"] = _same(1, max(_rows.values()), 61, _k, [(0, 0)])
    for (_bm, _pt), _ho in _rows.items():
        EPILOGUE_CASES[f"long_pw{_k}_{_bm}x{_pt}"] = _same(1, _ho, 61, _k, [(0, 0)])
        EPILOGUE_BASE[f"long_pw{_k}_{_bm}x{_pt}"] = f"long_pw{_k}"
EPILOGUE_CASES.update({f"long_d{c}": _same(2, 197, 211, c, _T3) for c in (32, 64)})
EPILOGUE_LONG = [f"long_pw{k}" for k in PW_K.values()] + ["long_d32", "long_d64"]      # the cases that own data; EPILOGUE_BASE's are prefixes


def epilogue_ranges(case, precision, flavour):
    ax, aw, aa = EPILOGUE_RANGES[flavour][precision]
    if flavour == "exact":
        ax, aw = EPILOGUE_WIDER.get((case, precision), (ax, aw))
    return ax, aw, aa


def _epilogue_seed(case):
    return 100 + len(case) if case in ("c72", "c136", "phase") else 1000 + sum(ord(c) * (i + 1) for i, c in enumerate(case))


def epilogue_data(case, precision, flavour):
    """Integer operands of an epilogue-mode case (host tensors, float32 holding values the 16-bit type holds exactly; masks uint8).
    bias: integers; gx2, mean2, invstd2: the second BatchNorm term of lh_bn_bwd_gate (x2).  A case of EPILOGUE_BASE takes the first rows
    of its base's image (views: nothing is drawn twice)."""
    n, hi, wi, cin, ho, wo, cout, OH, OW = EPILOGUE_CASES[case][:9]
    if case in EPILOGUE_LONG:                   # tens of MB each: the latest one is kept for its prefixes
        key = (case, precision, flavour)
        if key not in _LONG:
            _LONG.clear()
            _LONG[key] = _epilogue_draw(case, precision, flavour)
        return _LONG[key]
    if case in EPILOGUE_BASE:
        b = epilogue_data(EPILOGUE_BASE[case], precision, flavour)
        P = OH * OW * n
        assert n == 1 and EPILOGUE_CASES[EPILOGUE_BASE[case]][1] >= hi
        cut = dict(x=b["x"][:, :hi], amask=b["amask"][:P * cout // 8], gmask=b["gmask"][:P * cout // 8])
        cut.update({k: b[k][:P] for k in ("addend", "gx", "gx2")})
        return {**b, **cut}
    return _epilogue_draw(case, precision, flavour)


_LONG = {}


def _epilogue_draw(case, precision, flavour):
    n, hi, wi, cin, ho, wo, cout, OH, OW = EPILOGUE_CASES[case][:9]
    taps = EPILOGUE_CASES[case][13]
    ax, aw, aa = epilogue_ranges(case, precision, flavour)
    g = torch.Generator().manual_seed(_epilogue_seed(case))
    P = OH * OW * n
    half = torch.tensor([0.5, 1.0, 2.0])
    d = dict(x=ints((n, hi, wi, cin), ax, g), w=ints((cout, len(taps), cin), aw, g), addend=ints((P, cout), aa, g), gx=ints((P, cout), ax, g),
             amask=torch.randint(0, 256, (P * cout // 8,), generator=g, dtype=torch.uint8),
             gmask=torch.randint(0, 256, (P * cout // 8,), generator=g, dtype=torch.uint8),
             mean=ints((cout,), 4, g), shift=ints((cout,), 4, g), invstd=half[torch.randint(0, 3, (cout,), generator=g)],
             scale=half[torch.randint(0, 3, (cout,), generator=g)] * (2.0 * torch.randint(0, 2, (cout,), generator=g) - 1.0))
    d.update(bias=ints((cout,), 16, g), gx2=ints((P, cout), ax, g), mean2=ints((cout,), 4, g), invstd2=half[torch.randint(0, 3, (cout,), generator=g)])
    return d


def check_exact_epilogue(case, d):
    """The accumulator's precondition for an epilogue-mode case: the tap-list convolution of |x| and |w| below 2^24 everywhere; the
    second-rounding sum |acc| + |addend| too, and the affine acc * scale + (bias * scale + shift) in its quantum 0.5 (|scale| <= 2).
    Returns the largest sum of magnitudes."""
    ho, wo, taps = EPILOGUE_CASES[case][4], EPILOGUE_CASES[case][5], EPILOGUE_CASES[case][13]
    mag = float(tap_conv(d["x"].abs(), d["w"].abs(), taps, ho, wo, torch.float64).max())
    affine = 2.0 * (2.0 * (mag + float(d["bias"].abs().max())) + float(d["shift"].abs().max()))
    worst = max(mag + float(d["addend"].abs().max()), affine)
    assert worst < LIMIT, f"{case}: sum of magnitudes {worst:.0f} >= 2^24"
    return worst


def check_exact_rows(terms, quantum=1.0):
    """A statistics row is a sum over pixels of `terms` ([pixels][channels], fp64) in some order: exact in fp32 when every column's sum of
    magnitudes, in units of the quantum, is below 2^24.  Returns (holds, largest column)."""
    m = float(terms.abs().sum(0).max()) / quantum
    return m < LIMIT, m


# ---------------------------------------------------------------------------------------------------------------------------------
# The chain of tests/test_gpu_wgrad_table.py (ChainNet): name, cin, cout, k, stride, pad, transposed, weights that are nonzero per output
# channel (drawn from {-1, 1}, the rest 0), shift s (the weights are {-1, 0, 1} * 2^-s).
#
# Why sparse weights: exactness is scale-free -- what counts is (sum of magnitudes) / (finest quantum), and a layer whose outputs sum z
# nonzero terms multiplies that ratio by about sqrt(z) for the values and z for the bound.  A weight gradient sums activation x gradient
# over the pixels, so its ratio collects the growth of EVERY layer of the chain (those before it through the activation, those after it
# through the gradient).  About a dozen nonzero weights per output keeps the product of all seven layers and 720 pixels below 2^24 with
# room to spare (check_exact_chain asserts it layer by layer); activations and gradients stay dense, so every weight-gradient element
# still sums over every pixel.  The shift s ~ log2(sqrt(z)) keeps the magnitudes level from layer to layer.
CHAIN_LAYERS = [
    ("c0", 64, 128, 3, 1, 1, False, 12, 2), ("c1", 128, 256, 1, 1, 0, False, 12, 2), ("c2", 256, 256, 3, 1, 1, False, 12, 2),
    ("c3", 256, 256, 1, 2, 0, False, 12, 2), ("d4", 256, 128, 4, 2, 1, True, 12, 1), ("c5", 128, 256, 3, 1, 1, False, 12, 2),
    ("c6", 256, 21, 1, 1, 0, False, 12, 2),
]
CHAIN_INPUT = (3, 64, 12, 20)     # 720 pixels (180 behind the strided c3): 22.5 32-row stages -- the weight gradients split, the last stage is ragged
CHAIN_RANGE = 4          # input and upstream gradient: integers in [-4, 4]


def chain_data(seed=100):
    """(x, {param name: tensor}, dy): integer input and upstream gradient, sparse weights in {-1, 0, 1} * 2^-s, integer bias on c6."""
    g = torch.Generator().manual_seed(seed)
    x = ints(CHAIN_INPUT, CHAIN_RANGE, g)
    params = {}
    for name, cin, cout, k, s, p, tr, nz, sh in CHAIN_LAYERS:
        kk = cin * k * k
        w = torch.zeros(cout, kk)
        for co in range(cout):
            idx = torch.randperm(kk, generator=g)[:nz]
            w[co, idx] = (2.0 * torch.randint(0, 2, (nz,), generator=g) - 1.0) * 2.0 ** -sh
        w = w.view(cout, cin, k, k)
        params[name + ".weight"] = w.transpose(0, 1).contiguous() if tr else w
    params["c6.bias"] = ints((21,), CHAIN_RANGE, g)
    dy = ints((CHAIN_INPUT[0], 21, CHAIN_INPUT[2], CHAIN_INPUT[3]), CHAIN_RANGE, g)
    return x, params, dy


def chain_reference(x, params, dy, precision):
    """What the engine stores, in fp64 with its roundings: every activation rounded to the run precision once after its layer, every
    activation gradient once after its data-gradient launch; weight and bias gradients are fp32 sums of exact products -- exact.
    check_exact runs per layer with that layer's quanta.  Returns (out, dx, {param name: exact gradient}, [per-layer worst sums])."""
    dt = DTYPES[precision]

    def r16(t):
        return t.float().to(dt).double()
    acts, qa = [x.double()], [1.0]
    for name, cin, cout, k, s, p, tr, nz, sh in CHAIN_LAYERS:
        case = (cin, cout, k) if tr else (cin, cout, k, s, p)
        b = params.get(name + ".bias")
        out = _conv(acts[-1], params[name + ".weight"].double(), b.double() if b is not None else None, case, tr)
        acts.append(r16(out))
        qa.append(qa[-1] * 2.0 ** -sh)
    grads, worst = {}, []
    gcur, qg = dy.double(), 1.0
    for i in range(len(CHAIN_LAYERS) - 1, -1, -1):
        name, cin, cout, k, s, p, tr, nz, sh = CHAIN_LAYERS[i]
        case = (cin, cout, k) if tr else (cin, cout, k, s, p)
        w, b = params[name + ".weight"], params.get(name + ".bias")
        worst.append((name, check_exact(acts[i], w, b, gcur, case, tr, qx=qa[i], qw=2.0 ** -sh, qdy=qg)))
        r = reference(acts[i], w, b, gcur, case, tr)
        grads[name + ".weight"] = r["dw"]
        if b is not None:
            grads[name + ".bias"] = r["db"]
        gcur, qg = r16(r["dx"]), qg * 2.0 ** -sh
    return acts[-1], gcur, grads, worst[::-1]
