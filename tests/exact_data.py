"""Exact-arithmetic data for the convolution tests: operands that are integer multiples of a power-of-two quantum, small enough that
EVERY partial sum of every output, input-gradient and weight-gradient element, in any order, is an integer (times the product quantum)
below 2^24 -- which fp32 holds exactly.  An fp32 accumulator is then exact whatever the tile, ring depth, split count or MFMA order, and a
stored 16-bit value must equal ONE round-to-nearest-even of the exact result: the tests compare with torch.equal, tolerance zero.

The bound is derived, not measured: |any partial sum| <= sum of the magnitudes of its terms <= the same convolution of |x|, |w|, |dy|
(check_exact computes exactly that, in fp64, on the reference alone).  The reference is torch.nn.functional in float64 on the CPU: sums of
integers below 2^53 are exact there in any order too.

The second half of the file ("The BatchNorm grid") does the same for the BatchNorm / fused elementwise / pooling kernels, the last
section for the fused stem and bottleneck kernels."""
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
# "m35" (tests/test_gpu_multi_exact.py): one tap, 40 -> 72 channels, 35 pixels -- ONE workgroup under any tile with 128 channels, a
# single-workgroup member that sits between larger ones in a multi-problem launch
EPILOGUE_CASES["m35"] = (1, 5, 7, 40, 5, 7, 72, 5, 7, 1, 1, 0, 0, [(0, 0)])
EPILOGUE_SHORT = ["c72", "c136", "phase"] + [f"pw{k}" for k in PW_K.values()] + ["d32", "d64", "m35"]
# "exact" ranges widened where the default ones leave too few accumulators that need rounding (one tap, short K): (case, precision) ->
# (a for x and gx, a for w).  From the failures of tests/test_exact_host.py; never narrower.
EPILOGUE_WIDER = {("pw40", "bf16"): (16, 8), ("pw40", "fp16"): (64, 16), ("pw72", "fp16"): (64, 16),
                  ("m35", "bf16"): (16, 8), ("m35", "fp16"): (64, 16)}


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


# ---------------------------------------------------------------------------------------------------------------------------------
# The BatchNorm grid (tests/test_gpu_exact_bn.py): data on which the BatchNorm statistics, the fused affine / upsample / ReLU op (forward and
# backward) and the stem's pooling are exact in fp32, so that a stored 16-bit value must be ONE round-to-nearest-even of the fp64 result.
#   x, dout, addends: multiples of 1/2, |v| <= 4;  saved mean, beta: multiples of 1/2, |v| <= 2;  invstd in {1/2, 1, 2};  gamma in
#   {1/2, 1, 3/2, 2};  scale = gamma * invstd and shift = beta - mean * scale (both exact);  pixel counts that are powers of two, so the
#   division of a column sum by the count only moves the exponent.
# Nothing here is exact by decree: check_bn_exact walks every intermediate either apply form can produce, on the fp64 reference alone.
BN_A = 8                      # x and dout are k / 2 with k drawn uniformly from the integers [-BN_A, BN_A]
BN_DX_FILL = 0.5              # what a gradient buffer holds before the call: the addend of an accumulating term (on the grid)
_INVSTD = torch.tensor([0.5, 1.0, 2.0])
_GAMMA = torch.tensor([0.5, 1.0, 1.5, 2.0])
_B, _I = (True, 0, 0, None), (False, 0, 0, None)        # a term: (BatchNorm?, log2 of its upsampling, accumulate, writes the dx of term #)

# Backward cases with power-of-two pixel counts.  shape (n, h, w); c for the 16-bit types (c32: the fp32 form of the case, where there is
# one); relu: the source of the ReLU gate -- "out" (stored activation), "mask" (mask bits), "shift" (recomputed from x * scale + shift);
# cap: lh_fuse_bwd_desc.strips_cap; env: planned and run under LH_FOLD_IN_APPLY=0; pre: rows of the caller's partial-sum slab(s);
# route: the launch records lh_fuse_bwd_plan must return, (kind, grid, fold_rows) -- RG / RF / RFX reduce (generic, flat, flat with the
# gate from x), CO coefficient fold, AG / AF / AFX apply, A2 the two-term apply.  How each route follows from the shape is worked out in
# the comments; the planner is csrc/fuse_bwd_plan.h.
BN_BWD_CASES = {
    # 512 pixels, 4 chunks: strips of 16 rows -> 32; 32 * 64 floats is far below the 16 Ki the apply pass folds itself
    "flat_out": dict(shape=(2, 16, 16), c=32, terms=[_B], relu="out", route=[("RF", 32, 32), ("AF", 2, 32)]),
    "flat_mask": dict(shape=(2, 16, 16), c=32, terms=[_B], relu="mask", route=[("RF", 32, 32), ("AF", 2, 32)]),
    "flat_shift": dict(shape=(2, 16, 16), c=32, terms=[_B], relu="shift", route=[("RFX", 32, 32), ("AFX", 2, 32)]),
    # ceil(512 / 17) = 31 rows per strip: 16 strips of 31 and one of 16
    "cap17": dict(shape=(2, 16, 16), c=32, terms=[_B], relu="out", cap=17, route=[("RF", 17, 17), ("AF", 2, 17)]),
    # the fold launch: 32 rows = two per row lane of slab_lane16, neither unrolled loop
    "coef32": dict(shape=(2, 16, 16), c=32, terms=[_B], relu="out", env=True, route=[("RF", 32, 0), ("CO", 2, 0), ("AF", 2, 0)]),
    # 128 rows: one trip of the 8-deep loop of slab_lane16 in every row lane
    "coef128": dict(shape=(2, 32, 32), c=32, terms=[_B], relu="out", env=True, route=[("RF", 128, 0), ("CO", 2, 0), ("AF", 8, 0)]),
    # 512 rows: the wide fold (c / 4 workgroups), one trip of its 8-deep loop
    "coef512": dict(shape=(8, 32, 32), c=32, terms=[_B], relu="out", env=True, route=[("RF", 512, 0), ("CO", 8, 0), ("AF", 32, 0)]),
    # 256 rows: the wide fold, its 4-deep loop only
    "coef256": dict(shape=(4, 32, 32), c=32, terms=[_B], relu="mask", env=True, route=[("RF", 256, 0), ("CO", 8, 0), ("AF", 16, 0)]),
    # 256 rows * 64 = 16 Ki floats: the largest slab an apply pass folds itself
    "fold256": dict(shape=(4, 32, 32), c=32, terms=[_B], relu="out", route=[("RF", 256, 256), ("AF", 16, 256)]),
    # 2c = 512 columns: two columns per thread, every row; the strips are capped at 16 Ki / 512 = 32
    "fold_2c512": dict(shape=(2, 16, 16), c=256, terms=[_B], relu="out", route=[("RF", 32, 32), ("AF", 16, 32)]),
    # c > 256: flat kernels, but the fold is a launch
    "c512": dict(shape=(2, 16, 16), c=512, terms=[_B], relu="mask", route=[("RF", 32, 0), ("CO", 32, 0), ("AF", 32, 0)]),
    # 6 chunks: no power of two -> generic kernels
    "gen48": dict(shape=(2, 16, 16), c=48, terms=[_B], relu="out", route=[("RG", 32, 0), ("CO", 3, 0), ("AG", 12, 0)]),
    # 257 chunks: a second trip of the generic reduce's chunk loop with ONE chunk; 32 pixels = 2 strips
    "gen257": dict(shape=(1, 4, 8), c=2056, c32=1028, terms=[_B], relu="out", route=[("RG", 2, 0), ("CO", 129, 0), ("AG", 33, 0)],
                   route32=[("RG", 2, 0), ("CO", 65, 0), ("AG", 33, 0)]),
    "pair_out": dict(shape=(2, 16, 16), c=32, terms=[_B, _I], relu="out", route=[("RF", 32, 32), ("A2", 2, 0)]),
    "pair_mask": dict(shape=(2, 16, 16), c=32, terms=[_B, _I], relu="mask", route=[("RF", 32, 32), ("A2", 2, 0)]),
    # two coefficient blocks in one apply pass; the second term adds into its buffer
    "pair_bnbn": dict(shape=(2, 16, 16), c=32, terms=[_B, (True, 0, 1, None)], relu="out", route=[("RF", 32, 32), ("RF", 32, 32), ("A2", 2, 0)]),
    # flat and generic records of one call: the l = 1 term has 128 cells = 8 strips (and accumulates), the l = 2 identity term 32 cells
    "mixed3": dict(shape=(2, 16, 16), c=32, terms=[_B, (True, 1, 1, None), (False, 2, 0, None)], relu="mask",
                   route=[("RF", 32, 32), ("AF", 2, 32), ("RG", 8, 0), ("CO", 2, 0), ("AG", 2, 0), ("AG", 1, 0)]),
    # two identity terms that write ONE buffer, the second adding: the passes keep their recorded order
    "acc_same": dict(shape=(2, 16, 16), c=32, terms=[_I, (False, 0, 1, 0)], relu="mask", route=[("A2", 2, 0)]),
    # dout is the gated gradient already and its partial sums come with it: no reduce record.  3 rows fold in the apply pass, 300 rows
    # (300 * 64 floats > 16 Ki) take the wide fold launch
    "pre3": dict(shape=(2, 16, 16), c=32, terms=[_B], relu="out", pre=3, route=[("AF", 2, 3)]),
    "pre300": dict(shape=(2, 16, 16), c=32, terms=[_B], relu="out", pre=300, route=[("CO", 8, 0), ("AF", 2, 0)]),
    "pre3_pair": dict(shape=(2, 16, 16), c=32, terms=[_B, _I], relu="out", pre=3, route=[("A2", 2, 0)]),
    "pre300_pair": dict(shape=(2, 16, 16), c=32, terms=[_B, _I], relu="out", pre=300, route=[("CO", 8, 0), ("A2", 2, 0)]),
    "pre3_bnbn": dict(shape=(2, 16, 16), c=32, terms=[_B, _B], relu="out", pre=3, route=[("A2", 2, 0)]),
    "pre300_bnbn": dict(shape=(2, 16, 16), c=32, terms=[_B, _B], relu="out", pre=300, route=[("CO", 8, 0), ("CO", 8, 0), ("A2", 2, 0)]),
}
# Ragged pixel counts (180, 35, 663: the division by the count is inexact, see bn_dx_bound): c = 32 flat, c = 40 generic (5 chunks).
BN_RAGGED_CASES = {f"{n}x{h}x{w}x{c}": dict(shape=(n, h, w), c=c, terms=[_B], relu=relu, kinds=("RF", "AF") if c == 32 else ("RG", "CO", "AG"))
                   for (n, h, w) in ((3, 6, 10), (1, 5, 7), (3, 13, 17)) for c, relu in ((32, "out"), (40, "mask"))}
# (case, precision) the GPU test runs: every case in both 16-bit types, fp32 where the case names its fp32 form
BN_BWD_RUNS = [(k, p) for k, v in BN_BWD_CASES.items() for p in ("bf16", "fp16", "fp32") if p != "fp32" or "c32" in v]
# Ranges widened where the default one leaves the rounding condition of tests/test_exact_host.py unmet: (case, precision) -> BN_A.
BN_WIDER = {("gen257", "fp16"): 16}          # 32 pixels: the coefficients have few fraction bits
# The stem chain: (n, h, w, c); x on the grid, integer gradients of the pooled map drawn from [-a, a] (large enough that a sum of up to four
# window gradients needs a rounding, small enough that the BatchNorm backward behind it stays exact: check_bn_exact decides)
STEM_CASES = [(2, 16, 16, 64), (1, 9, 7, 64)]
STEM_DOUT = {"bf16": 96, "fp16": 96}
POOL_DOUT = {"bf16": 255, "fp16": 2047}          # the pool passes alone, gated or not: every integer the type holds exactly

# Forward cases: (name, (n, h, w), c, terms (BatchNorm?, log2 of the upsampling), kind lh_fuse_fwd_plan must return).  c = 48 is 6 (fp32:
# 12) chunks -- no power of two -- and c = 8 one (two) chunks; 35 and 180 pixels leave a ragged last workgroup.
BN_FWD_CASES = [
    ("flat1", (2, 16, 16), 32, [(True, 0)], "FLAT1"), ("flat1_35px", (1, 5, 7), 8, [(True, 0)], "FLAT1"),
    ("flat2_bn_id", (2, 16, 16), 32, [(True, 0), (False, 0)], "FLAT2"), ("flat2_bn_bn", (2, 16, 16), 32, [(True, 0), (True, 0)], "FLAT2"),
    ("flat2_bn_id_35px", (1, 5, 7), 8, [(True, 0), (False, 0)], "FLAT2"),
    ("gen_6chunks", (3, 6, 10), 48, [(True, 0)], "GEN"), ("gen_6chunks_two", (3, 6, 10), 48, [(True, 0), (False, 0)], "GEN"),
    ("gen_three", (2, 16, 16), 32, [(True, 0), (True, 0), (False, 0)], "GEN"), ("gen_four", (1, 5, 7), 8, [(True, 0), (False, 0), (True, 0), (True, 0)], "GEN"),
    ("gen_up1", (2, 16, 16), 32, [(True, 0), (True, 1)], "GEN"), ("gen_up2", (2, 16, 16), 32, [(True, 2), (False, 0)], "GEN"),
    ("gen_up1_up2", (2, 16, 16), 32, [(True, 0), (True, 1), (False, 2)], "GEN"), ("gen_up1_6chunks", (3, 6, 10), 48, [(False, 0), (True, 1)], "GEN"),
]
# forward x = k / 2 with |k| <= this, the widest range whose values the type holds exactly: on the backward grid (|k| <= 8) a sum of terms has
# too few significant bits to need a rounding
BN_FWD_A = {"bf16": 128, "fp16": 2048, "fp32": 2048}


def halves(shape, a, gen):
    """k / 2 with k drawn uniformly from the integers [-a, a], as float32."""
    return ints(shape, a, gen) / 2


def bn_params(c, gen):
    """gamma, beta, saved mean, invstd of one BatchNorm on the grid, and scale = gamma * invstd, shift = beta - mean * scale (exact)."""
    mean, beta = halves((c,), 4, gen), halves((c,), 4, gen)
    invstd = _INVSTD[torch.randint(0, 3, (c,), generator=gen)]
    gamma = _GAMMA[torch.randint(0, 4, (c,), generator=gen)]
    scale = gamma * invstd
    return dict(gamma=gamma, beta=beta, mean=mean, invstd=invstd, scale=scale, shift=beta - mean * scale)


def upsample(t, l):
    return t.repeat_interleave(1 << l, 1).repeat_interleave(1 << l, 2) if l else t


def cell_sum(t, l):
    """[n][h][w][c] summed over the 2^l x 2^l cells of a nearest-neighbour upsampling."""
    if not l:
        return t
    n, h, w, c = t.shape
    f = 1 << l
    return t.reshape(n, h // f, f, w // f, f, c).sum((2, 4))


def mask_bits(stored, epc):
    """lh_fuse_fwd's relu_mask of a stored activation: one byte per 16-byte chunk, bit e = (element e > 0)."""
    pos = (stored.double() > 0).reshape(-1, epc).to(torch.int32)
    return (pos << torch.arange(epc, dtype=torch.int32)).sum(1).to(torch.uint8)


def store(v, dtype):
    """What a kernel must store for the exact fp64 value v (which fp32 holds exactly): v itself in fp32, one RNE of it in a 16-bit type."""
    return v.float().to(dtype)


def uneven_groups(count, rows, gen):
    """Group index of each of `count` pixels: `rows` consecutive groups of uneven, non-zero length."""
    assert 1 <= rows <= count
    cuts = (torch.randperm(count - 1, generator=gen)[:rows - 1] + 1).sort().values
    return torch.searchsorted(cuts, torch.arange(count), right=True)


def group_slab(cols, gid, rows):
    """[rows][len(cols)][c] float32: the totals of every column tensor ([pixels][c], fp64) over each pixel group."""
    slab = torch.zeros(rows, len(cols), cols[0].shape[1], dtype=torch.float64)
    for k, v in enumerate(cols):
        slab[:, k].index_add_(0, gid, v)
    assert torch.equal(slab.float().double(), slab)
    return slab.float()


def bn_case_c(spec, precision):
    return spec.get("c32", spec["c"]) if precision == "fp32" else spec["c"]


def bn_case_route(spec, precision):
    return spec.get("route32", spec["route"]) if precision == "fp32" else spec["route"]


def bn_node(name, spec, precision, seed=None):
    """Data and fp64 reference of one lh_fuse_bwd node: dict(shape, c, dout, x[], prm[] (bn_params or None), stored (the forward result as
    stored), gate, terms[] = dict(g (gated gradient summed over the term's cell), dx (exact, before the old value is added), old (what an
    accumulating term adds: fp64 tensor or None), total (dx + old), xhat, s0, s1, count), slabs[] (float32 [pre][2][c] per BatchNorm term)).
    With `pre` dout is the gated gradient itself (no gate is applied)."""
    dt = DTYPES[precision]
    n, h, w = spec["shape"]
    c = bn_case_c(spec, precision)
    a = BN_WIDER.get((name, precision), spec.get("a", BN_A))
    gen = torch.Generator().manual_seed(seed if seed is not None else 500 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    d = dict(name=name, shape=(n, h, w), c=c, a=a, dout=halves((n, h, w, c), a, gen), x=[], prm=[], terms=[], slabs=[])
    pre_act = torch.zeros(n, h, w, c, dtype=torch.float64)
    for bn, l, acc, same in spec["terms"]:
        x = halves((n, h >> l, w >> l, c), a, gen)
        p = bn_params(c, gen) if bn else None
        d["x"].append(x)
        d["prm"].append(p)
        pre_act += upsample(x.double() * p["scale"].double() + p["shift"].double() if bn else x.double(), l)
    relu, pre = spec["relu"], spec.get("pre", 0)
    d["stored"] = store(torch.relu(pre_act) if relu != "off" else pre_act, dt)
    d["gate"] = torch.ones_like(pre_act) if (pre or relu == "off") else (d["stored"].double() > 0).double()
    gg = d["dout"].double() * d["gate"]
    for i, (bn, l, acc, same) in enumerate(spec["terms"]):
        g = cell_sum(gg, l)
        t = dict(g=g, count=g.shape[0] * g.shape[1] * g.shape[2], old=None)
        if bn:
            p = {k: v.double() for k, v in d["prm"][i].items()}
            t["xhat"] = (d["x"][i].double() - p["mean"]) * p["invstd"]
            t["s0"], t["s1"] = g.sum((0, 1, 2)), (g * t["xhat"]).sum((0, 1, 2))
            t["dx"] = p["scale"] * (g - t["s0"] / t["count"] - t["xhat"] * (t["s1"] / t["count"]))
            if pre:
                gid = uneven_groups(t["count"], pre, gen)
                d["slabs"].append(group_slab([g.reshape(-1, c), (g * t["xhat"]).reshape(-1, c)], gid, pre))
        else:
            t["dx"] = g
        if acc:         # what the buffer holds: its fill, or -- two terms that write one buffer -- the earlier term's stored result
            t["old"] = store(d["terms"][same]["total"], dt).double() if same is not None else torch.full_like(g, BN_DX_FILL)
        t["total"] = t["dx"] + t["old"] if acc else t["dx"]
        d["terms"].append(t)
    return d


def _fits(v, what):
    """fp32 holds the fp64 value v exactly: v = k * q with q the largest power of two that divides it and |k| < 2^24 -- which is
    float32(v) == v -- and the fp64 evaluation that produced it was exact itself (multiples of 2^-32 below 2^20: 52 bits)."""
    v = v.double()
    scaled = v * 2.0 ** 32
    assert bool((scaled == torch.round(scaled)).all()) and float(v.abs().max()) < 2.0 ** 20, f"{what}: outside the range the fp64 evaluation is exact on"
    bad = v.float().double() != v
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} values need more than 24 significant bits"
    return v


def _sum_fits(terms, q, what):
    """Column sums over ANY subset of the rows of terms ([..][c]) in any order: every term a multiple of q, the column's sum of magnitudes
    below 2^24 q.  Returns the largest column, in quanta."""
    terms = terms.double().reshape(-1, terms.shape[-1])
    assert bool((terms / q == torch.round(terms / q)).all()), f"{what}: a term is no multiple of {q}"
    ok, m = check_exact_rows(terms, q)
    assert ok, f"{what}: sum of magnitudes {m:.0f} quanta >= 2^24"
    return m


def check_bn_exact(d, spec, precision):
    """The proof obligation of the BatchNorm grid, on the fp64 reference alone (bn_node): every intermediate any kernel form can produce is
    an integer multiple of a power-of-two quantum below 2^24 quanta (_fits, _sum_fits), and no fp16 value overflows.  Walks, per term:
    the gated gradient summed over its cell; x - mean, xhat, g * (x - mean), g * xhat; the column sums over any subset of rows; with a
    power-of-two count c0, c1 and both apply forms -- scale * ((g - c0) - xhat * c1) and A g + B x + C with B = -(A invstd) c1,
    C = -(A c0) - B mean -- product by product and sum by sum; the sum with the old dx.  Returns the largest column sum, in quanta."""
    dt = DTYPES[precision]
    worst = 0.0
    _fits(d["dout"], "dout")
    assert torch.equal(d["dout"].to(dt).float(), d["dout"])
    for i, t in enumerate(d["terms"]):
        tag = f"{d['name']} term {i}"
        g = _fits(t["g"], tag + " g")
        assert torch.equal(d["x"][i].to(dt).float(), d["x"][i])
        if d["prm"][i] is not None:
            p = {k: v.double() for k, v in d["prm"][i].items()}
            x = d["x"][i].double()
            assert torch.equal(p["scale"], p["gamma"] * p["invstd"]) and torch.equal(p["shift"], p["beta"] - p["mean"] * p["scale"])
            xm = _fits(x - p["mean"], tag + " x - mean")
            xhat = _fits(xm * p["invstd"], tag + " xhat")
            assert torch.equal(xhat, t["xhat"])
            gxm = _fits(g * xm, tag + " g * (x - mean)")
            gxh = _fits(gxm * p["invstd"], tag + " g * xhat")
            assert torch.equal(gxh, g * xhat)
            worst = max(worst, _sum_fits(g, 0.5, tag + " sum g"), _sum_fits(gxh, 0.125, tag + " sum g * xhat"))
            _fits(t["s0"], tag + " dbeta")
            _fits(t["s1"], tag + " dgamma")
            cnt = t["count"]
            if cnt & (cnt - 1) == 0:
                c0, c1 = _fits(t["s0"] / cnt, tag + " c0"), _fits(t["s1"] / cnt, tag + " c1")
                A = p["scale"]
                # scale * (g - c0 - xhat * c1): fuse_bwd_apply
                f1 = _fits(A * _fits(_fits(g - c0, tag + " g - c0") - _fits(xhat * c1, tag + " xhat * c1"), tag + " g - c0 - xhat * c1"), tag + " dx")
                # A g + B x + C: term_coefs and the flat applies
                B = _fits(-_fits(A * p["invstd"], tag + " A * invstd") * c1, tag + " B")
                C = _fits(-_fits(A * c0, tag + " A * c0") - _fits(B * p["mean"], tag + " B * mean"), tag + " C")
                f2 = _fits(_fits(_fits(A * g, tag + " A * g") + _fits(B * x, tag + " B * x"), tag + " A g + B x") + C, tag + " dx (flat)")
                assert torch.equal(f1, f2) and torch.equal(f1, t["dx"]), tag + ": the two apply forms disagree"
        if t["count"] & (t["count"] - 1) == 0 or d["prm"][i] is None:
            _fits(t["total"], tag + " dx + old")
        if precision == "fp16":
            assert float(t["total"].abs().max()) <= FP16_MAX and bool(torch.isfinite(store(t["total"], dt)).all())
    if precision == "fp16":
        assert float(d["stored"].double().abs().max()) <= FP16_MAX
    return worst


def bn_dx_bound(d, i):
    """Per-element bound E on |stored fp32 dx - exact dx| of BatchNorm term i when the pixel count is no power of two, from the fp64
    operands: E = 8 * 2^-24 * M with M = |scale| (|g| + |c0| + |invstd c1| (|x| + |mean|)), the sum of the magnitudes of the terms of the
    formula.  Derivation, with u = 2^-24 (one fp32 rounding, first order; the column sums are exact, so c0 = fl(s0 / N) and c1 = fl(s1 / N)
    carry u each, everything else on the grid is exact):
      scale * ((g - c0) - xhat * c1):  fl(xhat c1) 2u |xhat c1|;  fl(g - c0) u (|g| + 2 |c0|);  their difference u (2 |g| + 3 |c0| +
        3 |xhat c1|);  times scale: u |scale| (3 |g| + 4 |c0| + 4 |xhat c1|), and |xhat| <= invstd (|x| + |mean|).
      A g + B x + C:  B = fl((A invstd) c1) 2u |B|;  C = fl(fl(A c0) - fl(B mean)) u (3 |A c0| + 4 |B mean|);  fl(B x) 3u |B x|;
        fl(A g + B x) u (|A g| + 4 |B x|);  the last sum u (2 |A g| + 5 |B x| + 4 |A c0| + 5 |B mean|).
    Both stay below 5u M; the factor 8 leaves room for the second-order terms and the fp64 roundings of the fold."""
    t, p = d["terms"][i], {k: v.double() for k, v in d["prm"][i].items()}
    c0, c1 = t["s0"] / t["count"], t["s1"] / t["count"]
    M = p["scale"].abs() * (t["g"].abs() + c0.abs() + (p["invstd"] * c1).abs() * (d["x"][i].double().abs() + p["mean"].abs()))
    return 8.0 * 2.0 ** -24 * M


def interval_16(ref, E, dtype):
    """(low, high, strict): the closed interval [RNE(ref - E), RNE(ref + E)] a stored value must lie in, and where its ends coincide."""
    lo, hi = store(ref - E, dtype), store(ref + E, dtype)
    return lo, hi, lo == hi


def bn_fwd_data(case, precision, relu):
    """x[], prm[], exact fp64 result and the partial sums of one forward case (term order: the kernels add in it)."""
    name, (n, h, w), c, terms, _ = case
    gen = torch.Generator().manual_seed(700 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    d = dict(x=[], prm=[], parts=[])
    acc = torch.zeros(n, h, w, c, dtype=torch.float64)
    for bn, l in terms:
        x = halves((n, h >> l, w >> l, c), BN_FWD_A[precision], gen)
        p = bn_params(c, gen) if bn else None
        v = _fits(x.double() * p["scale"].double(), name + " x * scale") + p["shift"].double() if bn else x.double()
        acc = acc + upsample(_fits(v, name + " term"), l)
        d["x"].append(x)
        d["prm"].append(p)
        d["parts"].append(_fits(acc, name + " partial sum"))
    d["exact"] = torch.relu(acc) if relu else acc
    return d


def stem_data(case, precision, seed=900):
    """The stem chain's inputs: x on the grid, one BatchNorm, integer gradients of the pooled map (for the chain / for the plain pool)."""
    n, h, w, c = case
    gen = torch.Generator().manual_seed(seed + h)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return dict(x=halves((n, h, w, c), BN_A, gen), prm=bn_params(c, gen), dout=ints((n, ho, wo, c), STEM_DOUT[precision], gen),
                dout_pool=ints((n, ho, wo, c), POOL_DOUT[precision], gen))


def stem_reference(s, precision, which="dout"):
    """fp64 reference of bn + relu + maxpool and its backward: a (the activation as it would be stored), pooled, the pool's input gradient
    (exact sum of up to four window gradients) and a bn_node-style dict of the BatchNorm backward behind it, whose `dout` is the ROUNDED,
    gated pool gradient and whose gate is all ones (lh_fuse_bwd's pre_partial form)."""
    dt = DTYPES[precision]
    p = {k: v.double() for k, v in s["prm"].items()}
    x = s["x"].double()
    pre_act = x * p["scale"] + p["shift"]
    a = store(torch.relu(pre_act), dt).double().permute(0, 3, 1, 2).requires_grad_(True)
    pooled = F.max_pool2d(a, 3, 2, 1)
    pooled.backward(s[which].double().permute(0, 3, 1, 2))
    gpool = a.grad.permute(0, 2, 3, 1).contiguous()
    g = store(gpool, dt).double() * (pre_act > 0)             # rounded as the ungated pass stores it, then gated by the ReLU
    xhat = (x - p["mean"]) * p["invstd"]
    cnt = x.shape[0] * x.shape[1] * x.shape[2]
    t = dict(g=g, count=cnt, old=None, xhat=xhat, s0=g.sum((0, 1, 2)), s1=(g * xhat).sum((0, 1, 2)))
    t["dx"] = t["total"] = p["scale"] * (g - t["s0"] / cnt - xhat * (t["s1"] / cnt))
    node = dict(name=f"stem{x.shape[1]}", shape=tuple(x.shape[:3]), c=x.shape[3], dout=g.float(), x=[s["x"]], prm=[s["prm"]], terms=[t], slabs=[],
                stored=store(torch.relu(pre_act), dt))
    return dict(a=a.detach().permute(0, 2, 3, 1), pooled=pooled.detach().permute(0, 2, 3, 1).contiguous(), gpool=gpool, node=node)


def bn_planned_route(lib, desc, n, h, w, c, workspace, dtype_code):
    """[(kind, grid, fold_rows)] of lh_fuse_bwd_plan for a descriptor (ctypes); raises on an error status."""
    import ctypes as C
    cap = 16
    kinds, grids, folds = (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)()
    nrec = lib.lh_fuse_bwd_plan(C.byref(desc), n, h, w, c, workspace, dtype_code, kinds, grids, folds, cap)
    assert 0 < nrec <= cap, (nrec, lib.lh_last_error())
    return [(kinds[i], grids[i], folds[i]) for i in range(nrec)]


# ---------------------------------------------------------------------------------------------------------------------------------
# The fused stem and bottleneck kernels (tests/test_gpu_exact_fused.py): lh_stem_pool, lh_stem_conv (csrc/stem_pool.hip) and
# lh_bottleneck_infer (csrc/bottleneck_infer_kernel.h), all three persistent.  Same rules as above: integer operands, power-of-two scales,
# every sum of magnitudes below 2^24 product quanta (fused_stem_check / bneck_check, on the fp64 reference alone).
#
# Stem images (n, h, w) -> convolution 7x7 / s2 / p3, pool 3x3 / s2 / p1:
#   tiny    9 x 7:   conv 5 x 4, pooled 3 x 2 -- less than one tile of either kernel
#   ragged  70 x 90: conv 35 x 45 (odd both; the last convolution row reads past the image, the last column does not), pooled 18 x 23
#                    = 3 x 3 pool tiles of 8 x 8, 3 x 3 conv tiles of 16 x 16
#   multi   66 x 66: conv 33, pooled 17: 3 x 3 tiles per image with a one-pixel last tile, for both kernels; 171 images = 1539 tiles =
#                    3 x 512 + 3: with the grid of 512 three workgroups take four tiles, the others three, and the prefetch behind the last
#                    tile is the zero fill (the GPU test asserts this against lh_stem_pool_grid / lh_stem_conv_rows, not against 512)
FUSED_STEM_IMAGES = {"tiny": (1, 9, 7), "ragged": (2, 70, 90), "multi": (171, 66, 66)}
# flavour -> precision -> (a for the image, a for the weights, a for the shift).  "exact": sums large enough to need roundings; the shift
# spans the values with one more bit than the type holds, so that the pooled maxima need roundings too.  "stats": small enough that the
# sums of SQUARES of the stored convolution outputs of one lh_stem_conv workgroup (up to four tiles of 256 pixels) stay below 2^24 --
# which no data that needs roundings can do (EPILOGUE_RANGES): the rounded values are then the sums themselves.
FUSED_STEM_RANGES = {"exact": {"bf16": (8, 4, 512), "fp16": (32, 8, 4096)}, "stats": {"bf16": (4, 2, 64), "fp16": (4, 2, 64)}}
# "exact" ranges widened where a small case leaves condition (c) of tests/test_exact_host.py unmet: (image, precision) -> (a image, a weights,
# a shift).  From that test's failures; never narrower.
FUSED_STEM_WIDER = {("tiny", "bf16"): (32, 8, 512), ("tiny", "fp16"): (128, 16, 4096)}
FUSED_STEM_DEAD, FUSED_STEM_NEG = 5, 9       # a channel whose shift leaves nothing above zero; a channel with negative scale (others: drawn)


def fused_stem_ranges(image, precision, flavour):
    r = FUSED_STEM_RANGES[flavour][precision]
    return FUSED_STEM_WIDER.get((image, precision), r) if flavour == "exact" else r


def fused_stem_sizes(image):
    """(n, h, w, hp, wp, ch, cw, ph, pw): image, its padded NHWC4 form (engine.Plan._c_stem: hp = h + 6, wp = w + 8), convolution, pool."""
    n, h, w = FUSED_STEM_IMAGES[image]
    ch, cw = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
    return n, h, w, h + 6, w + 8, ch, cw, (ch - 1) // 2 + 1, (cw - 1) // 2 + 1


def fused_stem_data(image, precision, flavour="exact"):
    """x [n][3][h][w], w [64][3][7][7], bias, shift: integers; scale from +-{0.5, 1, 2}.  Channel FUSED_STEM_DEAD has a shift below minus
    the largest value the affine can reach (every output of it is zero), channel FUSED_STEM_NEG a negative scale."""
    n, h, w = FUSED_STEM_IMAGES[image]
    ax, aw, ash = fused_stem_ranges(image, precision, flavour)
    g = torch.Generator().manual_seed(2000 + 7 * h + w)
    half = torch.tensor([0.5, 1.0, 2.0])
    d = dict(x=ints((n, 3, h, w), ax, g), w=ints((64, 3, 7, 7), aw, g), bias=ints((64,), 16, g), shift=ints((64,), ash, g),
             scale=half[torch.randint(0, 3, (64,), generator=g)] * (2.0 * torch.randint(0, 2, (64,), generator=g) - 1.0))
    d["scale"][FUSED_STEM_NEG] = -d["scale"][FUSED_STEM_NEG].abs()
    d["shift"][FUSED_STEM_DEAD] = -(2.0 * (147 * ax * aw + 16) + 1.0)
    return d


def fused_stem_layout(x, w):
    """The operands as the kernels read them (engine.Plan._c_stem): the zero-padded NHWC4 image [n][h + 6][w + 8][4] with pixel (y, x) at
    (y + 3, x + 3), and the weight staging [64][7 kernel rows][8 pixels][4 channels] whose rows are the K runs of the pack (pixel 7 and
    channel 3 are zero)."""
    n, _, h, wd = x.shape
    img = torch.zeros(n, h + 6, wd + 8, 4, dtype=x.dtype)
    img[:, 3:3 + h, 3:3 + wd, :3] = x.permute(0, 2, 3, 1)
    stage = torch.zeros(w.shape[0], 7, 8, 4, dtype=w.dtype)
    stage[:, :, :7, :3] = w.permute(0, 2, 3, 1)
    return img, stage


def fused_stem_tap_conv(img, stage, ch, cw):
    """The stem convolution as the direct kernels form it, in fp64: acc[n][a][b][co] = sum over kernel rows r and the 32 elements j of
    the row's K run of img[n][2 a + r][2 b + j / 4][j % 4] * stage[co][r][j]."""
    img, stage = img.double(), stage.double()
    acc = torch.zeros(img.shape[0], ch, cw, stage.shape[0], dtype=torch.float64)
    for r in range(7):
        for px in range(8):
            acc += img[:, r:r + 2 * ch - 1:2, px:px + 2 * cw - 1:2] @ stage[:, r, px].t()
    return acc


def fused_stem_reference(d, precision):
    """fp64 reference, NHWC.  acc: the exact convolution; mag: the same of |x|, |w|; act: relu(acc * scale + (bias * scale + shift)) before
    its rounding; conv16 / act16: the ONE round-to-nearest-even of acc / act (what lh_stem_conv stores / what lh_stem_pool keeps in LDS);
    pooled: F.max_pool2d(3, 2, 1) over act16; s1, s2: per-channel sums / sums of squares of conv16.  Zeros are +0."""
    dt = DTYPES[precision]
    acc = F.conv2d(d["x"].double(), d["w"].double(), None, 2, 3).permute(0, 2, 3, 1).contiguous()
    mag = F.conv2d(d["x"].double().abs(), d["w"].double().abs(), None, 2, 3).permute(0, 2, 3, 1)
    sc = d["scale"].double()
    act = torch.relu(acc * sc + (d["bias"].double() * sc + d["shift"].double())) + 0.0
    conv16, act16 = expected_16(acc + 0.0, dt), expected_16(act, dt)
    pooled = F.max_pool2d(act16.double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    c = conv16.double().reshape(-1, 64)
    return dict(acc=acc, mag=mag, act=act, conv16=conv16, act16=act16, pooled=expected_16(pooled, dt), s1=c.sum(0), s2=(c * c).sum(0))


def fused_stem_check(d, r):
    """(a) for the stem: the convolution's sum of magnitudes below 2^24, and the affine acc * scale + (bias * scale + shift) in its quantum
    0.5 (|scale| <= 2).  Returns the larger, in quanta."""
    for k in ("x", "w", "bias", "shift"):
        assert torch.equal(d[k], d[k].round()), k
    assert set(d["scale"].abs().tolist()) <= {0.5, 1.0, 2.0}
    mag = float(r["mag"].max())
    worst = max(mag, 2.0 * (2.0 * (mag + float(d["bias"].abs().max())) + float(d["shift"].abs().max())))
    assert worst < LIMIT, f"stem: sum of magnitudes {worst:.0f} >= 2^24"
    return worst


def pooled_source(r):
    """The exact (unrounded) activation behind every pooled value: the window's largest exact value -- rounding is monotonic, so it rounds
    to the window's largest stored value.  What rounding_counts is asked about the pooled map."""
    return F.max_pool2d(r["act"].permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)


def stem_conv_row_of_pixel(n, ch, cw, rows):
    """Statistics row of every convolution output [n][ch][cw], as stem_conv_kernel's tile loop assigns it (csrc/stem_pool.hip: tiles of
    16 x 16 outputs numbered image-major, then tile row, then tile column; workgroup b takes tiles b, b + grid, ...; one row per workgroup)."""
    ty, tx = (ch + 15) // 16, (cw + 15) // 16
    tile = (torch.arange(n).view(n, 1, 1) * ty + torch.arange(ch).view(1, ch, 1) // 16) * tx + torch.arange(cw).view(1, 1, cw) // 16
    return tile % rows


# The bottleneck: cin -> stages per tile cin / 32 + 5 = 7, 8, 10, 13: ring residues 3, 0, 2, 1; 96 and 160 are no multiple of 64 (kpad1 != cin)
BNECK_CIN = (64, 96, 160, 256)
#   tiny    5 x 7:   every pixel is a border pixel, the whole halo lies outside the image
#   ragged  17 x 33: 2 x 3 tiles whose last row and column of tiles are one pixel deep
#   multi   17 x 17: 4 tiles per image, 130 images = 520 tiles = 2 x 256 + 8: with the grid of 256 eight workgroups take three tiles
BNECK_SHAPES = {"tiny": (1, 5, 7), "ragged": (2, 17, 33), "multi": (130, 17, 17)}
# precision -> a for x, w1, w2, w3; largest |k| of the shifts b = k * quantum of layers 1, 2, 3; a for a separate residual; log2 of the
# scales: layer l draws |s| from 2^-(e_l + {0, 1}).  The shifts of layers 1 and 2 reach past the values the type holds exactly, so that
# the intermediates need roundings whatever cin; e_l keeps the magnitudes level (and every fp16 value normal and finite).
# The bit budget that sets the ranges: a stored activation that needs a rounding has more than 8 / 11 significant bits in ITS channel's
# quantum, the next accumulator counts in the FINEST channel's quantum (one more bit: two exponents per layer), and sums 576 or 64 such
# terms times |w| -- in fp16 2^12 * 576 * mean|w2| is about 2^22, and conv3 behind it only fits with w3 from {-1, 0, 1} and the last
# sum with a residual of at most 128.  Three exponents per layer, w3 = 2 or a residual of 2047 pass 2^24 (bneck_check says where).
BNECK_RANGES = {"bf16": dict(x=8, w1=4, w2=2, w3=2, k=(512, 8192, 65536), res=128, e=(1, 4, 4)),
                "fp16": dict(x=32, w1=8, w2=2, w3=1, k=(4096, 131072, 524288), res=128, e=(3, 6, 2))}
BNECK_WIDER = {}        # (cin, shape, precision) -> dict of the entries of BNECK_RANGES that are widened; never narrower
BNECK_POSITIVE = 8      # channels 0 .. 7 of b1 and b2 are strictly positive: relu(shift) in the halo instead of conv2's zero padding must show


def bneck_ranges(cin, shape, precision):
    return {**BNECK_RANGES[precision], **BNECK_WIDER.get((cin, shape, precision), {})}


def _pow2_scale(c, e, gen):
    return 2.0 ** -(e + torch.randint(0, 2, (c,), generator=gen).double()) * (2.0 * torch.randint(0, 2, (c,), generator=gen).double() - 1.0)


def bneck_data(cin, shape, precision):
    """Operands of one bottleneck case, fp64 holding values fp32 and (x, w, res) the 16-bit type hold exactly: x [n][h][w][cin], w1 [64][cin],
    w2 [64][64][3][3], w3 [256][64], res [n][h][w][256] integers; s_l = +- a power of two per channel; b_l = k * q_l |s_l| with integer k and
    q_l the quantum of layer l's accumulator (q: the three of them)."""
    n, h, w = BNECK_SHAPES[shape]
    r = bneck_ranges(cin, shape, precision)
    g = torch.Generator().manual_seed(3000 + cin + 7 * h + w)
    d = dict(x=ints((n, h, w, cin), r["x"], g).double(), w1=ints((64, cin), r["w1"], g).double(), w2=ints((64, 64, 3, 3), r["w2"], g).double(),
             w3=ints((256, 64), r["w3"], g).double(), res=ints((n, h, w, 256), r["res"], g).double())
    q, qs = 1.0, []
    for l, c in ((1, 64), (2, 64), (3, 256)):
        s = _pow2_scale(c, r["e"][l - 1], g)
        k = ints((c,), r["k"][l - 1], g).double()
        if l < 3:
            k[:BNECK_POSITIVE] = k[:BNECK_POSITIVE].abs() + 1.0
        d[f"s{l}"], d[f"k{l}"], d[f"b{l}"] = s, k, k * q * s.abs()
        qs.append(q)
        q = q * float(s.abs().min())            # the quantum of the stored activation = that of the next accumulator (integer weights)
    d["q"] = qs
    return d


def bneck_reference(d, precision, residual=None):
    """fp64 reference with every storage point of bottleneck_infer_kernel.h (residual: default d["res"]; pass d["x"] for an identity block):
      a1 = round16(relu(acc1 * s1 + b1))                     conv1 epilogue, lines 323-326 (rounded, then ReLU: the same value)
      a2 = round16(relu(acc2 * s2 + b2)), acc2 from a1 with ZERO padding outside the image (line 327: `if (!inside) pk.u = 0`), lines 405-408
      y3 = round16(acc3 * s3 + b3)                           bneck_epilogue_half, lines 63-66 (igemm_wave_epilogue.h:45-48)
      out = round16(relu(y3 + residual))                     lines 83-84 (igemm_wave_epilogue.h:122-128)
    pre1 / pre2 / pre3 / pre_out: the exact values in front of those four roundings (raw1 / raw2: without the ReLU, which the kernel applies
    behind the rounding); mag1 / mag2 / mag3: the layers' sums of magnitudes
    |input| * |w| + |k|, in the accumulator's quanta.  Zeros are +0."""
    dt = DTYPES[precision]

    def r16(t):
        return (t + 0.0).float().to(dt).double()
    res = d["res"] if residual is None else residual
    q1, q2, q3 = d["q"]
    acc1 = d["x"] @ d["w1"].t()
    pre1 = torch.relu(acc1 * d["s1"] + d["b1"])
    a1 = r16(pre1)
    conv2 = lambda a, w: F.conv2d(a.permute(0, 3, 1, 2), w, None, 1, 1).permute(0, 2, 3, 1)
    acc2 = conv2(a1, d["w2"])
    pre2 = torch.relu(acc2 * d["s2"] + d["b2"])
    a2 = r16(pre2)
    acc3 = a2 @ d["w3"].t()
    pre3 = acc3 * d["s3"] + d["b3"]
    y3 = r16(pre3)
    pre_out = torch.relu(y3 + res)
    out = r16(pre_out)
    mag1 = (d["x"].abs() @ d["w1"].abs().t() + d["k1"].abs()) / q1
    mag2 = conv2(a1.abs(), d["w2"].abs()) / q2 + d["k2"].abs()
    mag3 = (a2.abs() @ d["w3"].abs().t()) / q3 + d["k3"].abs()
    return dict(acc1=acc1, acc2=acc2, acc3=acc3, raw1=acc1 * d["s1"] + d["b1"], raw2=acc2 * d["s2"] + d["b2"], pre1=pre1, a1=a1, pre2=pre2, a2=a2, pre3=pre3, y3=y3, pre_out=pre_out, out=out,
                mag1=mag1, mag2=mag2, mag3=mag3, res=res)


def bneck_check(d, r):
    """(a) per layer: every operand a multiple of its quantum and the layer's sum of magnitudes below 2^24 quanta, so acc * s + b is exact
    in fp32 (s a power of two, b = k quanta * |s|); the last sum y3 + residual in the quantum of y3 as well.  Returns the three layer
    maxima and that of the last sum, in quanta."""
    q1, q2, q3 = d["q"]
    for t, q, what in ((d["x"], 1.0, "x"), (d["w1"], 1.0, "w1"), (d["w2"], 1.0, "w2"), (d["w3"], 1.0, "w3"), (r["res"], 1.0, "residual"),
                       (r["a1"], q2, "a1"), (r["a2"], q3, "a2")):
        assert bool((t / q == torch.round(t / q)).all()), f"{what} is no multiple of its quantum {q}"
    for l in (1, 2, 3):
        s = d[f"s{l}"].abs()
        assert bool((torch.log2(s) == torch.round(torch.log2(s))).all()) and torch.equal(d[f"b{l}"], d[f"k{l}"] * d["q"][l - 1] * s)
    q4 = q3 * d["s3"].abs()                                      # per channel: y3 and the integer residual are multiples of it
    assert float(q4.max()) <= 1.0 and bool((r["y3"] / q4 == torch.round(r["y3"] / q4)).all())
    last = float(((r["y3"].abs() + r["res"].abs()) / q4).max())
    worst = [float(r["mag1"].max()), float(r["mag2"].max()), float(r["mag3"].max()), last]
    assert max(worst) < LIMIT, f"bottleneck: sums of magnitudes {worst} (>= 2^24 somewhere)"
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# The multi-problem launches (tests/test_gpu_multi_exact.py): lh_igemm_multi and lh_wgrad_fused_multi.
#
# A. lh_igemm_multi.  The four-wave tiled configurations the multi-problem kernel is instantiated for, (tile channels, tile pixels, ring
# depth, K bytes per stage): a literal copy of LH_RING_CFGS_MID + LH_RING_CFGS_SMALL (csrc/igemm_ring_cfgs.h), held against
# lh_igemm_candidates by tests/test_exact_host.py.
MULTI_RING_CFGS = [
    (128, 128, 2, 64), (128, 128, 3, 64), (128, 128, 4, 64), (128, 128, 2, 128), (128, 128, 3, 128), (128, 128, 4, 128),
    (128, 64, 2, 64), (128, 64, 4, 64), (128, 64, 2, 128), (128, 64, 3, 128), (128, 64, 4, 128),
    (64, 128, 2, 64), (64, 128, 4, 64), (64, 128, 2, 128), (64, 128, 3, 128), (64, 128, 4, 128),
    (64, 64, 2, 64), (64, 64, 4, 64), (64, 64, 2, 128), (64, 64, 3, 128), (64, 64, 4, 128),
]
# The members of a call, in caller order: the K loop (taps x K steps per tap: 1, 4, 1, 9, 9) is no descending sequence, so the library's
# stable sort by loop length really permutes the first four -- (c72, phase, pw40, m35) -- and the fifth runs alone on the plain kernel.
MULTI_MEMBERS = ["pw40", "phase", "m35", "c72", "c136"]
MULTI_PAIR = ["c136", "pw40"]                      # n = 2
MULTI_TRIPLE = ["phase", "m35", "c72"]             # n = 3: sorted to (c72, phase, m35)
# The mixed-mode assignments: member i of MULTI_MEMBERS takes MULTI_MODES[i + r] in rotation r.  Rotations 0 and 1 are the two calls of all
# five members, rotation 2 is spread over the n = 2 and n = 3 calls.  The order is chosen so that every window of three holds an addend mode
# and an epilogue-vector mode: every member has an addend, an epilogue vector and (rotation 0 of pw40, and the all-"stats" call) a slab at
# least once and lacks each of them at least once, the members of one call never agree, and "phase" -- whose placement is strided, while
# mask bits index a dense output -- never meets "addend_mask" (its window is bias, addend, relu).
MULTI_MODES = ["stats", "bias", "addend", "relu", "affine_relu", "addend_mask", "plain"]


def multi_mode(member, rotation):
    return MULTI_MODES[MULTI_MEMBERS.index(member) + rotation]


def multi_igemm_calls():
    """Every call the GPU test makes per configuration and precision: (name, flavour, [(member, mode)])."""
    return [("five r0", "exact", [(m, multi_mode(m, 0)) for m in MULTI_MEMBERS]),
            ("five r1", "exact", [(m, multi_mode(m, 1)) for m in MULTI_MEMBERS]),
            ("five stats", "exact_small", [(m, "stats") for m in MULTI_MEMBERS]),
            ("pair r2", "exact", [(m, multi_mode(m, 2)) for m in MULTI_PAIR]),
            ("triple r2", "exact", [(m, multi_mode(m, 2)) for m in MULTI_TRIPLE])]


def multi_launch_order(members, kb):
    """The order lh_igemm_multi gives the members of one launch (<= 4): longest K loop first, ties in caller order."""
    def steps(m):
        return len(EPILOGUE_CASES[m][13]) * -(-EPILOGUE_CASES[m][3] * 2 // kb)
    return sorted(range(len(members)), key=lambda i: -steps(members[i]))


_EXPECTED = {}


def epilogue_expected(case, precision, mode, flavour):
    """Host-only twin of tests/test_gpu_epilogue_modes._host for the modes lh_igemm_multi takes (no gate): the values a launch must store
    at its own pixels, [pixels of the launch][cout] float32 -- the accumulator rounded to 16 bits, the (masked) addend added in fp32, the sum
    rounded again, then ReLU; "bias" and "affine_relu" as igemm_epilogue_consts folds them.  The GPU test holds it against _host."""
    key = (case, precision, mode, flavour)
    if key in _EXPECTED:
        return _EXPECTED[key]
    n, hi, wi, cin, ho, wo, cout, OH, OW, osh, osw, ooh, oow, taps = EPILOGUE_CASES[case]
    dt = DTYPES[precision]
    if (case, precision, flavour) not in _EXPECTED:
        d = epilogue_data(case, precision, flavour)
        check_exact_epilogue(case, d)
        _EXPECTED[(case, precision, flavour)] = (d, tap_conv(d["x"], d["w"], taps, ho, wo).reshape(-1, cout))
    d, acc = _EXPECTED[(case, precision, flavour)]
    pos = ((torch.arange(n).view(n, 1, 1) * OH + torch.arange(ho).view(1, ho, 1) * osh + ooh) * OW
           + torch.arange(wo).view(1, 1, wo) * osw + oow).reshape(-1)
    if mode == "bias":
        v = (acc + d["bias"]).to(dt).float()
    elif mode == "affine_relu":
        v = (acc * d["scale"] + (d["bias"] * d["scale"] + d["shift"])).to(dt).float().clamp_min(0.0)
    else:
        v = acc.to(dt).float()
    if mode in ("addend", "addend_mask"):
        a = d["addend"][pos]
        if mode == "addend_mask":
            bits = ((d["amask"].view(-1, 1) >> torch.arange(8, dtype=torch.uint8).view(1, 8)) & 1).bool().view(n * OH * OW, cout)
            a = torch.where(bits[pos], a, torch.zeros_like(a))
        v = (v + a).to(dt).float()
    if mode == "relu":
        v = v.clamp_min(0.0)
    assert mode in MULTI_MODES
    _EXPECTED[key] = v
    return v


# B. lh_wgrad_fused_multi.  Members (cin, cout, k, stride, pad, n, h, w): channel counts from {72, 136}, so that every four-wave tile
# fits (wcfg_fits: more than half a 128-wide tile) and is ragged.
#   W1  286 pixels: 9 stages of 32 rows or 5 of 64, the last one ragged (30 rows)       W2  35 pixels: less than one 64-row stage
#   W3  stride 2, 5 x 4 = 20 output pixels                                              W4  strided 1x1, 3 x 7 x 9 = 189 pixels
#   W5  60 pixels
WGRAD_MULTI_CASES = {
    "W1": (72, 136, 3, 1, 1, 2, 13, 11), "W2": (136, 72, 1, 1, 0, 1, 5, 7), "W3": (72, 72, 3, 2, 1, 1, 9, 7),
    "W4": (136, 136, 1, 2, 0, 3, 13, 17), "W5": (136, 136, 3, 1, 1, 1, 6, 10),
}
# (tile output channels, tile input channels, pixel rows per ring stage, ring depth): a literal copy of the four-wave entries of
# LH_WGRAD_CFGS (csrc/wgrad_cfgs.h), held against lh_wgrad_candidates by tests/test_exact_host.py
WGRAD_MULTI_CFGS = [(bo, bi, kps, d) for bo, bi in ((128, 128), (128, 64), (64, 128), (64, 64)) for kps, d in ((32, 2), (32, 4), (64, 2), (64, 3))]
WGRAD_BIG_CFG = (256, 256, 32, 3)                  # the eight-wave tile: not batchable, fits 136 x 136 only
# Requested pixel splits (cfg[7], low 16 bits); the rest take one.  W1: 3 + 3 + 3 stages of 32 rows or 2 + 2 + 1 of 64; W4: 3 + 3 or 2 + 1.
WGRAD_MULTI_SPLITS = {"W1": 3, "W4": 2}
# What varies inside one call: W3 adds onto a gradient that holds small integers, W5 writes the ConvTranspose layout [cin][cout][k][k]
# (so = k * k, si = cout * k * k), W2 has operand rows 8 channels longer than the run, the slack filled with a large finite integer.
WGRAD_MULTI_ACCUMULATE, WGRAD_MULTI_TRANSPOSED, WGRAD_MULTI_SLACK = "W3", "W5", "W2"
WGRAD_SLACK_FILL = 16384.0
WGRAD_PREFILL = 16                                 # the accumulating member's gradient holds integers from [-16, 16]
# Caller order per tile class: tiles with bo = 128 take the members with cout = 136, tiles with bi = 128 those with cin = 136.  Each order is
# chosen so that the library's stable sort of a launch by stages per split (longest first) is no identity (tests/test_exact_host.py).
WGRAD_MULTI_ORDER = {(64, 64): ["W1", "W2", "W3", "W4", "W5"], (128, 64): ["W5", "W1", "W4"], (64, 128): ["W2", "W4", "W5"], (128, 128): ["W5", "W4"]}


def wgrad_fits(member, bo, bi):
    cin, cout = WGRAD_MULTI_CASES[member][:2]
    return (bo < 128 or cout == 136) and (bi < 128 or cin == 136)


def wgrad_sizes(member):
    """(output pixels, ho, wo) of a member."""
    cin, cout, k, s, p, n, h, w = WGRAD_MULTI_CASES[member]
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    return n * ho * wo, ho, wo


def wgrad_slack(member):
    return 8 if member == WGRAD_MULTI_SLACK else 0


def wgrad_desc(desc, member, cfg=None, splits=None):
    """Fill an lh_igemm_desc (lighthand_amd._lib.IgemmDesc) with the forward convolution of a member, as Plan._c_conv does: taps (r - p,
    s - p), sh = sw = stride, k_run = cin; cfg = (bo, bi, kps, depth) goes to cfg[5..7] with the member's split request.  Returns desc."""
    cin, cout, k, s, p, n, h, w = WGRAD_MULTI_CASES[member]
    _, ho, wo = wgrad_sizes(member)
    desc.n, desc.hi, desc.wi, desc.in_pix_stride, desc.k_run = n, h, w, cin + wgrad_slack(member), cin
    desc.ho, desc.wo, desc.sh, desc.sw, desc.cout = ho, wo, s, s, cout
    desc.OH, desc.OW, desc.osh, desc.osw, desc.ooh, desc.oow, desc.out_pix_stride = ho, wo, 1, 1, 0, 0, cout
    desc.ntaps, desc.relu = k * k, 0
    for t in range(k * k):
        desc.dh[t], desc.dw[t] = t // k - p, t % k - p
    if cfg is not None:
        bo, bi, kps, depth = cfg
        want = WGRAD_MULTI_SPLITS.get(member, 1) if splits is None else splits
        desc.cfg[5], desc.cfg[6], desc.cfg[7] = bo, bi, want | (kps << 16) | (depth << 24)
    return desc


def wgrad_plan(member, kps, splits=None):
    """(stages, stages per split, splits) as wgrad_plan (csrc/wgrad_plan.h) resolves an explicit request."""
    want = WGRAD_MULTI_SPLITS.get(member, 1) if splits is None else splits
    stages = -(-wgrad_sizes(member)[0] // kps)
    sps = -(-stages // want)
    return stages, sps, -(-stages // sps)


def wgrad_launch_order(members, kps):
    """The order lh_wgrad_fused_multi gives the weight-gradient launch of <= 4 members: most stages per split first, ties in caller order."""
    return sorted(range(len(members)), key=lambda i: -wgrad_plan(members[i], kps)[1])


_WGRAD = {}


def wgrad_member(member, precision):
    """Integer x, w, dy (NCHW, float32) of a member, the fp64 weight gradient [cout][cin][k][k] and the integer prefill of the accumulating
    member (or None): made once, never changed."""
    key = (member, precision)
    if key not in _WGRAD:
        case = WGRAD_MULTI_CASES[member]
        x, w, _, dy = conv_data(case, precision, seed=300 + int(member[1]), bias=False)
        dw = reference(x, w, None, dy, case)["dw"]
        pre = None
        if member == WGRAD_MULTI_ACCUMULATE:
            pre = ints(dw.shape, WGRAD_PREFILL, torch.Generator().manual_seed(399))
        _WGRAD[key] = dict(x=x, w=w, dy=dy, dw=dw, pre=pre)
    return _WGRAD[key]


def wgrad_expected(member, precision):
    """The fp32 tensor a member's gradient buffer must hold, in the layout the member writes."""
    m = wgrad_member(member, precision)
    g = m["dw"] + (m["pre"].double() if m["pre"] is not None else 0.0)
    assert torch.equal(g.float().double(), g)
    g = g.float()
    return g.permute(1, 0, 2, 3).contiguous() if member == WGRAD_MULTI_TRANSPOSED else g
