"""Exact-arithmetic tests of the BatchNorm statistics and finalize (csrc/bn_stats.hip, bn_fold.h), the fused affine / upsample / ReLU op,
forward and backward (csrc/fuse_fwd.hip, fuse_bwd.hip, fuse_bwd_kernel.h, fuse_bwd_plan.h) and the stem's pooling with its
BatchNorm-backward gate (csrc/pool.hip), through the C ABI alone.

The data sit on a power-of-two grid (tests/exact_data.py, "The BatchNorm grid"): every intermediate of every kernel form is held by fp32
exactly, in any summation order, so a stored 16-bit value must be ONE round-to-nearest-even of the fp64 host result and an fp32 value must
be that result.  Every comparison is torch.equal unless its test says otherwise; output buffers are pre-filled, so an element that is not
written shows.  The preconditions (exactness of every intermediate, enough values that need a rounding, ties among them, the 2 % condition
of the interval criterion) are proved on the CPU by tests/test_exact_host.py, which also pins the route table through lh_fuse_bwd_plan /
lh_fuse_fwd_plan; here every case asserts the route again on the descriptor it runs.

What this catches that the tolerances of the model-level tests do not: truncation in place of round-to-nearest-even, a second rounding, a
row dropped or counted twice at a strip boundary or in an unrolled fold loop's tail, a subnormal fp16 result flushed to zero, a
num_batches_tracked that moves twice."""
import contextlib
import ctypes as C
import functools
import os

import pytest
import torch

import exact_data as E
from lighthand_amd import _lib
from lighthand_amd._lib import BnBwdGate, BnFinalizeCall
from test_gpu_fuse_routes import DT, DX_FILL, PARAM_FILL, BwdNode, FwdCall, Term, bwd_multi, bwd_single, fwd_single

pytestmark = pytest.mark.gpu

assert DX_FILL == E.BN_DX_FILL
KB = dict(RG=_lib.LH_FB_REDUCE_GEN, RF=_lib.LH_FB_REDUCE_FLAT, RFX=_lib.LH_FB_REDUCE_FLAT_X, CO=_lib.LH_FB_COEF, AG=_lib.LH_FB_APPLY_GEN,
          AF=_lib.LH_FB_APPLY_FLAT, AFX=_lib.LH_FB_APPLY_FLAT_X, A2=_lib.LH_FB_APPLY2)
KF = dict(GEN=_lib.LH_FF_GEN, FLAT1=_lib.LH_FF_FLAT1, FLAT2=_lib.LH_FF_FLAT2)
MULTI_MAX = 4                 # LH_MULTI_MAX of csrc/multi.h: problems per multi-problem launch


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same(tag, name, got, want, exact=None):
    """torch.equal; a failure names the first differing index, the value got, the exact value and the expected rounding."""
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, name, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = got != want
    i = tuple(int(v) for v in bad.nonzero()[0])
    raise AssertionError(f"{tag} {name}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result, first at {i}: got {float(got[i])}, "
                         f"exact {float(exact[i]) if exact is not None else float(want[i])}, expected {float(want[i])}")


def _inside(tag, name, got, ref, bound, td):
    """The interval criterion for a pixel count that is no power of two (exact_data.bn_dx_bound): every stored value lies in the closed
    interval [RNE(ref - E), RNE(ref + E)], and wherever the two ends coincide it equals RNE(ref)."""
    got = got.detach().cpu()
    lo, hi, strict = E.interval_16(ref, bound, td)
    g = got.double()
    bad = (g < lo.double()) | (g > hi.double())
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{tag} {name}: {int(bad.sum())} of {bad.numel()} elements outside [RNE(ref - E), RNE(ref + E)], first at {i}: got {float(got[i])}, "
                             f"exact {float(ref[i])}, E {float(bound[i]):.3e}, interval [{float(lo[i])}, {float(hi[i])}]")
    want = E.store(ref, td)
    _same(tag, name + " (where the interval is one value)", torch.where(strict, got, want), want, ref)
    return 1.0 - float(strict.double().mean())


@contextlib.contextmanager
def _fold_env(off):
    """LH_FOLD_IN_APPLY=0 (the planner reads it at every call) for the cases that must take the fold launch; restored afterwards."""
    saved = os.environ.pop("LH_FOLD_IN_APPLY", None)
    if off:
        os.environ["LH_FOLD_IN_APPLY"] = "0"
    try:
        yield
    finally:
        os.environ.pop("LH_FOLD_IN_APPLY", None)
        if saved is not None:
            os.environ["LH_FOLD_IN_APPLY"] = saved


class ExactNode(BwdNode):
    """A BwdNode whose inputs come from exact_data.bn_node instead of randn; keeps the fp64 reference (self.ref)."""

    def __init__(self, name, spec, dtype, ref=None):
        td, _ = DT[dtype]
        d = ref if ref is not None else E.bn_node(name, spec, dtype)
        n, h, w = spec["shape"]
        self.name, self.spec, self.ref = name, spec, d
        self.dtype, self.td, self.shape, self.relu, self.strips_cap = dtype, td, (n, h, w, d["c"]), spec["relu"], spec.get("cap", 0)
        self.terms = [Term(bn=bn, l=l, acc=acc, same_dx_as=same) for bn, l, acc, same in spec["terms"]]
        self.epc = 16 // torch.empty(0, dtype=td).element_size()
        self.dout = d["dout"].to(td).cuda()
        self.x = [x.to(td).cuda() for x in d["x"]]
        for k in ("scale", "shift", "mean", "invstd"):
            setattr(self, k, [p[k].float().cuda() if p is not None else None for p in d["prm"]])
        self.out = d["stored"].cuda()
        self.mask = E.mask_bits(d["stored"], self.epc).cuda() if spec["relu"] == "mask" else None
        self.pre = [s.cuda() for s in d["slabs"]] or None
        self.touch = None

    def route(self, lib, o):
        return E.bn_planned_route(lib, o["desc"], *self.shape, o["ws"].data_ptr(), DT[self.dtype][1])

    def check(self, o, tag, ragged=False):
        """dx of every term (the last writer of a shared buffer), dgamma and dbeta against the reference.  Returns the share of dx
        elements the interval criterion leaves two values for (ragged) or 0."""
        loose = 0.0
        for i, (t, term) in enumerate(zip(self.ref["terms"], self.terms)):
            if any(later.same_dx_as == i for later in self.terms[i + 1:]):
                continue
            if ragged and term.bn:
                loose = max(loose, _inside(tag, f"dx[{i}]", o["dx"][i], t["total"], E.bn_dx_bound(self.ref, i), self.td))
            else:
                _same(tag, f"dx[{i}]", o["dx"][i], E.store(t["total"], self.td), t["total"])
            if term.bn:
                _same(tag, f"dgamma[{i}]", o["dgamma"][i], t["s1"].float(), t["s1"])
                _same(tag, f"dbeta[{i}]", o["dbeta"][i], t["s0"].float(), t["s0"])
        return loose


@functools.lru_cache(maxsize=None)
def _node(name, dtype):
    return ExactNode(name, E.BN_BWD_CASES[name], dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# a. lh_bn_stats
@pytest.mark.parametrize("dtype,c", [("bf16", 8), ("bf16", 40), ("bf16", 2056), ("fp16", 8), ("fp16", 40), ("fp16", 2056), ("fp32", 4), ("fp32", 1028)])
@pytest.mark.parametrize("m", [1, 127, 128, 129, 300])
def test_bn_stats_rows_are_exact(m, c, dtype):
    """Integers |y| <= 8: slab row r holds exactly the sums and sums of squares of rows [128 r, 128 r + 128) (at most 128 * 64 = 2^13 per
    column), rows_out == lh_bn_stats_rows, and nothing behind the slab is written.  c = 2056 / 1028 is 257 chunks: a second trip of the
    kernel's chunk loop with one chunk."""
    lib = _lib.load()
    td, code = DT[dtype]
    y = E.ints((m, c), 8, torch.Generator().manual_seed(1000 + m + c))
    rows = lib.lh_bn_stats_rows(m, c)
    assert rows == (m + 127) // 128
    buf = torch.full(((lib.lh_bn_stats_slab_bytes(rows, c) + 3) // 4,), PARAM_FILL, device="cuda")
    rows_out = C.c_int(-1)
    yd = y.to(td).cuda()
    _lib.check(lib.lh_bn_stats(yd.data_ptr(), m, c, buf.data_ptr(), C.byref(rows_out), code, _stream()), "lh_bn_stats")
    torch.cuda.synchronize()
    assert rows_out.value == rows
    want = torch.zeros(rows, 2, c, dtype=torch.float64)
    for r in range(rows):
        blk = y[128 * r:128 * r + 128].double()
        want[r, 0], want[r, 1] = blk.sum(0), (blk * blk).sum(0)
    _same((m, c, dtype), "slab", buf[:rows * 2 * c].view(rows, 2, c), want.float(), want)
    assert bool((buf[rows * 2 * c:] == PARAM_FILL).all()), "lh_bn_stats wrote behind its slab"


# ---------------------------------------------------------------------------------------------------------------------------------
# b. lh_bn_finalize / lh_bn_finalize_multi
U = 2.0 ** -24                # relative error of ONE fp32 rounding (round to nearest)
SLOP = 1.0 + 2.0 ** -20       # the second-order terms of a product of (1 + U) factors and the fp64 roundings of the fold (2^-53 each)
MOMENTUM, EPS = 0.1, 1e-5
NBT0 = 41


@functools.lru_cache(maxsize=None)
def _finalize_case(rows, c):
    """A statistics slab as an epilogue would have written it: integer data |y| <= 8 (channel 0 constant) in `rows` uneven pixel groups,
    the sums and sums of squares of each group (exact in fp32: at most 3907 * 64 < 2^18 per column)."""
    gen = torch.Generator().manual_seed(2000 + 7 * rows + c)
    m = 3 * rows + 7
    y = E.ints((m, c), 8, gen).double()
    y[:, 0] = 3.0
    slab = E.group_slab([y, y * y], E.uneven_groups(m, rows, gen), rows)
    return dict(rows=rows, c=c, count=m, y=y, slab=slab, gamma=(1.0 + 0.5 * torch.randn(c, generator=gen)), beta=0.3 * torch.randn(c, generator=gen),
                rmean=torch.randn(c, generator=gen), rvar=0.5 + torch.rand(c, generator=gen))


def _finalize_buffers(lib, fc):
    rows, c = fc["rows"], fc["c"]
    stats = torch.zeros((lib.lh_bn_stats_slab_bytes(rows, c) + 3) // 4, device="cuda")           # the slab and the fold's fp64 scratch
    stats[:rows * 2 * c] = fc["slab"].reshape(-1).cuda()
    b = dict(stats=stats, gamma=fc["gamma"].cuda(), beta=fc["beta"].cuda(), running_mean=fc["rmean"].clone().cuda(), running_var=fc["rvar"].clone().cuda(),
             nbt=torch.full((1,), NBT0, dtype=torch.int64, device="cuda"))
    for k in ("scale", "shift", "save_mean", "save_invstd"):
        b[k] = torch.full((c,), PARAM_FILL, device="cuda")
    return b


_FIN_OUT = ("scale", "shift", "save_mean", "save_invstd", "running_mean", "running_var", "nbt")


def _finalize_single(lib, fc):
    b = _finalize_buffers(lib, fc)
    _lib.check(lib.lh_bn_finalize(b["stats"].data_ptr(), fc["rows"], fc["count"], fc["c"], b["gamma"].data_ptr(), b["beta"].data_ptr(),
                                  b["running_mean"].data_ptr(), b["running_var"].data_ptr(), b["nbt"].data_ptr(), MOMENTUM, EPS, b["scale"].data_ptr(),
                                  b["shift"].data_ptr(), b["save_mean"].data_ptr(), b["save_invstd"].data_ptr(), _stream()), "lh_bn_finalize")
    torch.cuda.synchronize()
    return {k: b[k].cpu() for k in _FIN_OUT}


def _within(tag, name, got, ref, bound):
    err = (got.double() - ref).abs()
    bad = err > bound
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{tag} {name}: {int(bad.sum())} of {bad.numel()} channels outside the derived bound, first {i}: got {float(got[i])!r}, "
                             f"fp64 {float(ref[i])!r}, error {float(err[i]):.3e}, bound {float(bound[i]):.3e}")


@pytest.mark.parametrize("rows", [1, 15, 17, 50, 130, 255, 256, 300, 449, 700, 1024, 1025, 1300])
def test_bn_finalize_against_fp64_with_derived_bounds(rows):
    """rows < 256: the 16-lane fold (its 8-deep loop from 128 rows on, its 4-deep loop from 64, tails); 256 .. 1024: the 64-lane fold
    (8-deep from 512 rows on); > 1024: the two-launch route.  c = 20 and 70 leave a ragged last workgroup at 16 and at 4 channels per
    workgroup.  The fold is exact (integer totals, fp64), so the saved mean is float32(mean64) bit for bit; every other output gets a
    bound counted from the fp32 roundings of bn_finalize_channel (bn_fold.h), written next to the line it comes from."""
    lib = _lib.load()
    for c in (4, 20, 70):
        fc = _finalize_case(rows, c)
        got = _finalize_single(lib, fc)
        tag = (rows, c)
        n = fc["count"]
        mom, eps = float(torch.tensor(MOMENTUM, dtype=torch.float32)), float(torch.tensor(EPS, dtype=torch.float32))      # the floats the call passes
        s0, s1 = fc["y"].sum(0), (fc["y"] * fc["y"]).sum(0)
        assert torch.equal(fc["slab"][:, 0].double().sum(0), s0) and torch.equal(fc["slab"][:, 1].double().sum(0), s1)
        mean = s0 / n                                           # const double mean = s0 / count;  (one fp64 division of exact integers)
        var = (s1 / n - mean * mean).clamp_min(0.0)             # double var = s1 / count - mean * mean;  if (var < 0.0) var = 0.0;
        assert float(var[0]) == 0.0 and float(mean[0]) == 3.0   # the constant channel: 3 n / n and 9 n / n are exact quotients
        invstd = 1.0 / torch.sqrt(var + eps)
        g, b = fc["gamma"].double(), fc["beta"].double()
        scale, shift = g * invstd, b - mean * (g * invstd)
        unb = var * (n / (n - 1.0)) if n > 1 else var           # running_var takes the unbiased variance
        rmean, rvar = (1.0 - mom) * fc["rmean"].double() + mom * mean, (1.0 - mom) * fc["rvar"].double() + mom * unb
        # p.smean[ch] = (float)mean: the one rounding of the same fp64 value
        _same(tag, "save_mean", got["save_mean"], mean.float(), mean)
        # const float invstd = (float)(1.0 / sqrt(var + eps)): fp64 arithmetic (errors of 2^-53), then ONE rounding to fp32 -- the stored
        # value is float32(ref) or, where the fp64 errors move the quotient across a rounding boundary, its neighbour: 1 ulp of float32(ref)
        r32 = invstd.float()
        ulp = (torch.nextafter(r32, torch.full_like(r32, float("inf"))) - r32).double()
        _within(tag, "save_invstd", got["save_invstd"], r32.double(), ulp)
        assert abs(float(got["save_invstd"][0]) - float(torch.tensor(1.0 / eps ** 0.5).float())) <= float(ulp[0])       # var = 0: 1 / sqrt(eps)
        # const float sc = g * invstd: invstd carries one rounding, the product a second
        _within(tag, "scale", got["scale"], scale, 2 * U * SLOP * scale.abs())
        # const float sh = b - (float)mean * sc: (float)mean one rounding, sc two, their product one more -- 4 U on |mean * scale| --, and
        # the subtraction one rounding of the result
        _within(tag, "shift", got["shift"], shift, SLOP * (4 * U * (mean * scale).abs() + U * shift.abs()))
        # rmean = (1.f - momentum) * rmean + momentum * (float)mean: (1.f - momentum) one rounding and its product one; (float)mean one
        # and its product one; the sum one rounding of the result
        _within(tag, "running_mean", got["running_mean"], rmean, SLOP * (2 * U * (((1 - mom) * fc["rmean"].double()).abs() + (mom * mean).abs()) + U * rmean.abs()))
        # rvar = (1.f - momentum) * rvar + momentum * (float)unb: the same count of roundings
        _within(tag, "running_var", got["running_var"], rvar, SLOP * (2 * U * (((1 - mom) * fc["rvar"].double()).abs() + (mom * unb).abs()) + U * rvar.abs()))
        assert int(got["nbt"]) == NBT0 + 1, f"{tag}: num_batches_tracked moved by {int(got['nbt']) - NBT0}"


def test_bn_finalize_multi_equals_the_single_calls_bit_for_bit():
    """Six layers in one lh_bn_finalize_multi call: five of them share multi-problem launches (four, then a leftover), the 1300-row one
    takes the two-launch route in between.  Every output of every layer equals the single call's (which the test above holds against
    fp64), and num_batches_tracked rises by exactly 1 per layer."""
    lib = _lib.load()
    layers = [_finalize_case(r, c) for r, c in ((15, 4), (300, 20), (1300, 70), (130, 20), (700, 4), (17, 70))]
    bufs = [_finalize_buffers(lib, fc) for fc in layers]
    calls = (BnFinalizeCall * len(layers))()
    for q, fc, b in zip(calls, layers, bufs):
        q.stats, q.rows, q.count, q.c = b["stats"].data_ptr(), fc["rows"], fc["count"], fc["c"]
        q.gamma, q.beta, q.running_mean, q.running_var = b["gamma"].data_ptr(), b["beta"].data_ptr(), b["running_mean"].data_ptr(), b["running_var"].data_ptr()
        q.num_batches_tracked, q.momentum, q.eps = b["nbt"].data_ptr(), MOMENTUM, EPS
        q.scale, q.shift, q.save_mean, q.save_invstd = (b[k].data_ptr() for k in ("scale", "shift", "save_mean", "save_invstd"))
    _lib.check(lib.lh_bn_finalize_multi(calls, len(layers), _stream()), "lh_bn_finalize_multi")
    torch.cuda.synchronize()
    for fc, b in zip(layers, bufs):
        one = _finalize_single(lib, fc)
        for k in _FIN_OUT:
            _same((fc["rows"], fc["c"]), k, b[k], one[k])
        assert int(b["nbt"]) == NBT0 + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# c. lh_fuse_fwd
class ExactFwd(FwdCall):
    """A FwdCall whose inputs come from exact_data.bn_fwd_data."""

    def __init__(self, case, dtype, relu):
        name, (n, h, w), c, terms, _ = case
        td, _code = DT[dtype]
        d = E.bn_fwd_data(case, dtype, relu)
        self.ref = d
        self.dtype, self.td, self.shape, self.relu = dtype, td, (n, h, w, c), relu
        self.terms = [(bn, l, False) for bn, l in terms]
        self.epc = 16 // torch.empty(0, dtype=td).element_size()
        self.x = [x.to(td).cuda() for x in d["x"]]
        self.scale = [p["scale"].float().cuda() if p is not None else None for p in d["prm"]]
        self.shift = [p["shift"].float().cuda() if p is not None else None for p in d["prm"]]
        self.touch = None
        self.stats, self.gamma, self.beta = [None] * len(terms), [None] * len(terms), [None] * len(terms)


@pytest.mark.parametrize("relu", [0, 1], ids=["linear", "relu"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("case", E.BN_FWD_CASES, ids=[c[0] for c in E.BN_FWD_CASES])
def test_fuse_fwd_is_one_rounding_of_the_exact_sum(case, dtype, relu):
    """out is one RNE of the exact sum of terms (fp32: the sum itself), relu_mask the sign bits of the ROUNDED stored values, and the
    call runs the kernel the case was written for (lh_fuse_fwd_plan)."""
    lib = _lib.load()
    call = ExactFwd(case, dtype, relu)
    o = fwd_single(lib, [call])[0]
    kind, grid = C.c_int(-1), C.c_int(-1)
    _lib.check(lib.lh_fuse_fwd_plan(C.byref(o["desc"]), o["out"].data_ptr(), *call.shape, DT[dtype][1], C.byref(kind), C.byref(grid)), "lh_fuse_fwd_plan")
    assert kind.value == KF[case[4]], (case[0], dtype, kind.value)
    want = E.store(call.ref["exact"], call.td)
    _same((case[0], dtype, relu), "out", o["out"], want, call.ref["exact"])
    _same((case[0], dtype, relu), "relu_mask", o["mask"], E.mask_bits(want, call.epc))


# ---------------------------------------------------------------------------------------------------------------------------------
# d. lh_fuse_bwd, power-of-two pixel counts
@pytest.mark.parametrize("name,dtype", E.BN_BWD_RUNS)
def test_fuse_bwd_alone_is_exact_on_its_route(name, dtype):
    """Every case of exact_data.BN_BWD_CASES run alone: the launch records are the ones the table names (kind, grid = strips for a
    reduce record, fold rows), dx is one RNE of the fp64 result (fp32: the result), dgamma and dbeta are the exact sums."""
    lib = _lib.load()
    spec = E.BN_BWD_CASES[name]
    nd = _node(name, dtype)
    with _fold_env(spec.get("env")):
        o = bwd_single(lib, [nd])[0]
        route = nd.route(lib, o)
    assert route == [(KB[k], g, f) for k, g, f in E.bn_case_route(spec, dtype)], (name, dtype, route)
    nd.check(o, (name, dtype))


def _leftover_kinds(routes, kinds):
    """Of the records of `kinds` over all routes: (a kind fills a whole multi-problem launch, the kinds among the leftovers)."""
    count = {k: sum(r[0] == KB[k] for route in routes for r in route) for k in kinds}
    return any(v >= MULTI_MAX for v in count.values()), {k for k, v in count.items() if v % MULTI_MAX}


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_fuse_bwd_multi_calls_are_exact(dtype):
    """The same nodes through lh_fuse_bwd_multi -- each must give the exact result, which says more than "single equals multi".  Three
    calls, because two things hold for a whole call: the planner reads LH_FOLD_IN_APPLY once per node of the call it plans, and two
    passes that write ONE buffer put every record of their call on the in-order route.
      1. every case without the switch except the shared-buffer one: more than LH_MULTI_MAX records of several kinds per phase, so whole
         groups of one kind run through that kind's kernel and the leftovers through the mixed kernels (asserted on the planned routes);
      2. the cases under LH_FOLD_IN_APPLY=0, with a generic and a three-term node beside them (those two then take fold launches too);
      3. the shared-buffer node beside another one: every record in recorded order."""
    lib = _lib.load()
    plain = [k for k, v in E.BN_BWD_CASES.items() if not v.get("env") and k != "acc_same"]
    forced = [k for k, v in E.BN_BWD_CASES.items() if v.get("env")] + ["gen48", "mixed3"]
    for names, off in ((plain, False), (forced, True), (["acc_same", "flat_shift"], False)):
        nodes = [_node(k, dtype) for k in names]
        with _fold_env(off):
            outs = bwd_multi(lib, nodes)
            routes = [nd.route(lib, o) for nd, o in zip(nodes, outs)]
        if names is not forced:
            for nd, r in zip(nodes, routes):
                assert r == [(KB[k], g, f) for k, g, f in E.bn_case_route(nd.spec, dtype)], (nd.name, r)
        if len(names) > 2:
            for kinds in (("RG", "RF", "RFX"), ("AG", "AF", "AFX")):
                whole, left = _leftover_kinds(routes, kinds)
                assert whole and len(left) >= 2, (kinds, whole, left)
            assert sum(r[0] == KB["CO"] for route in routes for r in route) > MULTI_MAX
        for nd, o in zip(nodes, outs):
            nd.check(o, (nd.name, dtype, "multi"))


# ---------------------------------------------------------------------------------------------------------------------------------
# e. lh_fuse_bwd, ragged pixel counts
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_fuse_bwd_ragged_pixel_counts_stay_inside_the_derived_interval(dtype):
    """180, 35 and 663 pixels (the last strip of 35 has 3 rows), c = 32 flat and c = 40 generic, alone and all six in one multi call.
    dgamma and dbeta are exact sums whatever the count.  The division by the count is inexact, so dx is held to the interval criterion:
    with E = 8 * 2^-24 * (sum of the magnitudes of the terms of the formula) -- derived in exact_data.bn_dx_bound for both apply forms --
    every stored value lies in [RNE(ref - E), RNE(ref + E)] and equals RNE(ref) wherever the two ends coincide; tests/test_exact_host.py
    proves on the reference alone that they differ for at most 2 % of the elements of a case."""
    lib = _lib.load()
    nodes = [ExactNode(k, v, dtype) for k, v in E.BN_RAGGED_CASES.items()]
    for how, outs in (("alone", bwd_single(lib, nodes)), ("multi", bwd_multi(lib, nodes))):
        for nd, o in zip(nodes, outs):
            assert [k for k, _, _ in nd.route(lib, o)] == [KB[k] for k in nd.spec["kinds"]], nd.name
            loose = nd.check(o, (nd.name, dtype, how), ragged=True)
            print(nd.name, dtype, how, f"two values allowed for {100 * loose:.2f} % of the dx elements")
            assert loose <= 0.02


# ---------------------------------------------------------------------------------------------------------------------------------
# f. the stem chain
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", E.STEM_CASES, ids=["x".join(map(str, c)) for c in E.STEM_CASES])
def test_stem_chain_is_exact(case, dtype):
    """lh_bn_relu_maxpool3x3s2_fwd -> lh_maxpool3x3s2_bwd_gated -> lh_fuse_bwd with the pool's slab as pre_partial, each kernel fed with
    what the one before it wrote.  Pooled values and window positions (through the gradients they route), the gated dx -- a sum of up to
    four integer window gradients, rounded once, then gated -- and every slab column total (summed in fp64 here) are exact, with the
    narrow gradient range the BatchNorm backward stays exact behind and with the widest the type holds; dgamma / dbeta are exact, the
    final dx is exact at 512 pixels and inside the derived interval at 63.  The first shape also goes through the plain
    lh_maxpool3x3s2_fwd / _bwd against F.max_pool2d in fp64 (exact_data.stem_reference)."""
    lib = _lib.load()
    td, code = DT[dtype]
    n, h, w, c = case
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    tag = (case, dtype)
    s = E.stem_data(case, dtype)
    x = s["x"].to(td).cuda()
    prm = {k: v.float().cuda() for k, v in s["prm"].items()}
    pooled = torch.full((n, ho, wo, c), DX_FILL, dtype=td, device="cuda")
    idx = torch.full((n, ho, wo, c), 0xEE, dtype=torch.uint8, device="cuda")
    _lib.check(lib.lh_bn_relu_maxpool3x3s2_fwd(x.data_ptr(), prm["scale"].data_ptr(), prm["shift"].data_ptr(), pooled.data_ptr(), idx.data_ptr(),
                                               n, h, w, c, code, _stream()), "lh_bn_relu_maxpool3x3s2_fwd")
    torch.cuda.synchronize()
    ref = E.stem_reference(s, dtype)
    _same(tag, "pooled", pooled, E.store(ref["pooled"], td), ref["pooled"])
    assert int(idx.max()) <= 8
    rows = lib.lh_maxpool3x3s2_bwd_gated_rows(n, h, w, c, code)
    assert rows == min(1024, (n * h * w * c // 8 + 255) // 256)
    for which in ("dout_pool", "dout"):                         # the narrow range last: its outputs feed lh_fuse_bwd
        r = E.stem_reference(s, dtype, which)
        t = r["node"]["terms"][0]
        dout = s[which].to(td).cuda()
        gdx = torch.full((n, h, w, c), DX_FILL, dtype=td, device="cuda")
        slab = torch.full((rows, 2, c), PARAM_FILL, device="cuda")
        gate = BnBwdGate()
        gate.x, gate.mean, gate.invstd, gate.scale, gate.shift, gate.partial = (x.data_ptr(), prm["mean"].data_ptr(), prm["invstd"].data_ptr(),
                                                                                prm["scale"].data_ptr(), prm["shift"].data_ptr(), slab.data_ptr())
        _lib.check(lib.lh_maxpool3x3s2_bwd_gated(dout.data_ptr(), idx.data_ptr(), gdx.data_ptr(), C.byref(gate), n, h, w, c, code, _stream()),
                   "lh_maxpool3x3s2_bwd_gated")
        torch.cuda.synchronize()
        _same(tag, f"gated dx ({which})", gdx, t["g"].float().to(td), r["gpool"])
        tot = slab.cpu().double().sum(0)
        _same(tag, f"slab totals of g ({which})", tot[0], t["s0"])
        _same(tag, f"slab totals of g * xhat ({which})", tot[1], t["s1"])
    spec = dict(shape=(n, h, w), c=c, terms=[E._B], relu="out", pre=rows)
    nd = ExactNode(r["node"]["name"], spec, dtype, ref=r["node"])
    nd.dout, nd.pre = gdx, [slab]
    o = bwd_single(lib, [nd])[0]
    assert nd.route(lib, o) == [(KB["AF"], max(1, (n * h * w * c // 8 + 1023) // 1024), rows)], nd.route(lib, o)       # no reduce record; the apply pass folds the pool's rows
    cnt = n * h * w
    loose = nd.check(o, tag, ragged=bool(cnt & (cnt - 1)))
    assert loose <= 0.02
    if case != E.STEM_CASES[0]:
        return
    # the plain pool on the activation as stored, against F.max_pool2d and its autograd in fp64
    r = E.stem_reference(s, dtype, "dout_pool")
    a = r["a"].float().to(td).cuda()
    pooled2 = torch.full((n, ho, wo, c), DX_FILL, dtype=td, device="cuda")
    idx2 = torch.full((n, ho, wo, c), 0xEE, dtype=torch.uint8, device="cuda")
    _lib.check(lib.lh_maxpool3x3s2_fwd(a.data_ptr(), pooled2.data_ptr(), idx2.data_ptr(), n, h, w, c, code, _stream()), "lh_maxpool3x3s2_fwd")
    dx = torch.full((n, h, w, c), DX_FILL, dtype=td, device="cuda")
    dout = s["dout_pool"].to(td).cuda()
    _lib.check(lib.lh_maxpool3x3s2_bwd(dout.data_ptr(), idx2.data_ptr(), dx.data_ptr(), n, h, w, c, code, _stream()), "lh_maxpool3x3s2_bwd")
    torch.cuda.synchronize()
    _same(tag, "plain pooled", pooled2, E.store(r["pooled"], td), r["pooled"])
    _same(tag, "window positions (fused against plain)", idx, idx2.cpu())
    _same(tag, "plain pool dx", dx, E.store(r["gpool"], td), r["gpool"])
