"""Exact-arithmetic tests of the convolution paths at plan level: forward, data gradient, weight gradient and bias gradient of Conv2d and
ConvTranspose2d through the engine, with EVERY forward / data-gradient kernel configuration (tiled ring depths, dense-wave forms, the
pointwise and the direct 3x3 kernel: Plan.force_cfg) and EVERY weight-gradient plan (Plan.force_wgrad) forced in turn.

Operands are small integers (tests/exact_data.py), chosen so that every partial sum in any order is an integer below 2^24: the fp32
accumulator is exact whatever the tile, ring depth, split count or MFMA order, so a stored 16-bit value must be ONE round-to-nearest-even
of the fp64 host result and an fp32 value must be that result.  Every comparison is torch.equal -- tolerance zero.  The preconditions
(the 2^24 bound, no fp16 overflow, enough ties and roundings in every case) are proved on the CPU by tests/test_exact_host.py.

What this catches that a relative tolerance of a few ulps of the LARGEST element does not: truncation instead of round-to-nearest-even, a
second rounding, one product dropped or duplicated at an image border / K tail / ragged tile, a pixel split that loses a pixel."""
import ctypes as C

import pytest
import torch

import exact_data as E
from test_gpu_ops import _mods, _run_plan, forced_plans  # noqa: F401  (forced_plans is a fixture)

pytestmark = pytest.mark.gpu

# What a case must be offered AND run on (16-bit precisions; fp32 has the tiled kernel only), by case index of E.CONV_CASES: the families
# of the forward launch, those of the data-gradient launch (each direction has its own candidate list and is asserted on its own), and
# the least number of pixel splits among the weight-gradient plans.  The data gradient of 128 -> 256 has 128 output channels: one
# 128-row block of the weight pack, so the 256-row tile is not legal there (cfg_safe, igemm_plan.hip).
_NEEDS = {2: ({"pointwise"}, {"pointwise"}, 1), 5: ({"direct"}, {"direct"}, 1), 6: ({"direct"}, {"direct"}, 1), 8: ({"256x256"}, set(), 1),
          9: ({"pointwise"}, {"pointwise"}, 1), 11: (set(), set(), 3)}


def _family(c):
    from lighthand_amd._lib import conv_kind
    return conv_kind(c[2])


def _kernel_of(c):
    """(start, middle, end) of what Plan._kname prints for a forced configuration (engine.py) -- kernel, tile, ring depth and stage bytes:
    the library resolved the launch to exactly this configuration."""
    kind = _family(c)
    if kind == "pointwise":
        return "igemm_pw_kernel<", f" {c[0]}, {c[3]}, {c[1] // 16},", ">"
    if kind == "direct":
        return "conv3x3_direct_kernel<", f" {c[3]},", ">"
    return "igemm_ring_kernel<", f" {c[0]}, {c[1]},", f", {c[2] - 20 if kind == 'dense' else c[2]}, {c[3]}>"


def _wgrad_plans_of(plan):
    """(tile, tile, cfg[7] encoding = pixel splits | rows per stage << 16 | ring depth << 24) the library resolves for every
    weight-gradient launch of the plan (lh_wgrad_tile on the launch's own descriptor: what lh_wgrad_fused runs)."""
    from lighthand_amd import _lib
    got = []
    for _, call, name, _, _ in plan.profile_meta:
        if not name.startswith("wgrad"):
            continue
        bo, bi, ns, ring = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check(plan.lib.lh_wgrad_tile(C.byref(call.args[0]._obj), call.args[5], call.args[6], plan.dt, C.byref(bo), C.byref(bi), C.byref(ns),
                                          C.byref(ring)), "lh_wgrad_tile")
        if ring.value:                      # the LDS-DMA kernel (16-bit types): the profile's kernel name carries tile, ring depth, stage rows
            assert name.startswith("wgrad_ring_kernel<") and f" {bo.value}, {bi.value}," in name and \
                name.endswith(f", {ring.value % 10}, {ring.value // 10}>"), (name, ring.value)
        got.append((bo.value, bi.value, ns.value | (ring.value // 10) << 16 | (ring.value % 10) << 24))
    return got


def _walk(case, precision, Plan, transposed=False, bias=None):
    """Every configuration index in turn, forward / data-gradient configuration and weight-gradient plan advanced together (a launch
    with fewer candidates wraps around): each run is compared with the host.  Returns (configurations seen per launch, in the order the
    plan chooses them -- forward first, then the data gradient --, weight-gradient plans seen)."""
    ConvNet, _ = _mods()
    x, w, b, dy = E.conv_data(case, precision, bias=bias, transposed=transposed)
    ref = E.reference(x, w, b, dy, case, transposed)
    dt = E.DTYPES[precision]
    want = {k: (E.expected_16(ref[k], dt).float() if k in ("out", "dx") else ref[k].float()) for k in ("out", "dx", "dw")}
    want["db"] = ref["db"].float() if b is not None else None
    cfgs, wplans = [], set()
    idx, total = 0, 1
    while idx < total:
        chosen, wchosen = [], []

        def pick(cands, idx=idx, chosen=chosen):
            c = cands[idx % len(cands)]
            chosen.append((c, len(cands)))
            return c

        def wpick(cands, idx=idx, wchosen=wchosen):
            c = cands[idx % len(cands)]
            wchosen.append((c, len(cands)))
            return c[:3]
        Plan.force_cfg, Plan.force_wgrad = pick, wpick
        if transposed:
            m = ConvNet(case[0], case[1], case[2], 2, 1, bias=b is not None, transposed=True)
        else:
            m = ConvNet(*case[:5], bias=b is not None)
        with torch.no_grad():
            m.conv.weight.copy_(w)
            if b is not None:
                m.conv.bias.copy_(b)
        out, dx, grads = _run_plan(m, x, lambda o: dy, precision)
        tag = (case, precision, [c for c, _ in chosen], [c for c, _ in wchosen])
        assert chosen, "no launch of this plan offered candidates"
        assert out.shape == want["out"].shape, tag
        for name, got, exp in (("out", out.float(), want["out"]), ("dx", dx, want["dx"]), ("dw", grads["conv.weight"], want["dw"])):
            if not torch.equal(got, exp):
                bad = got != exp
                i = tuple(int(v) for v in bad.nonzero()[0])
                raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result, first at {i}: "
                                     f"got {float(got[i])}, exact {float(ref[name][i])}, expected {float(exp[i])}; {tag}")
        if b is not None:
            assert torch.equal(grads["conv.bias"], want["db"]), tag
        # the forced configurations are the ones that ran
        plan = next(iter(m._lh_plans.values()))
        names = [meta[2] for meta in plan.profile_meta]
        for c, _ in chosen:
            head, args, tail = _kernel_of(c)
            assert any(nm.startswith(head) and args in nm and nm.endswith(tail) for nm in names), (c, names)
        ran = _wgrad_plans_of(plan)
        for c, _ in wchosen:
            assert tuple(c[:3]) in ran, (c, ran)
        cfgs += [set() for _ in range(len(chosen) - len(cfgs))]
        for i, (c, _) in enumerate(chosen):
            cfgs[i].add(c)
        wplans |= {c[:3] for c, _ in wchosen}
        total = max([nc for _, nc in chosen] + [nc for _, nc in wchosen])
        idx += 1
    Plan.force_cfg = Plan.force_wgrad = None
    return cfgs, wplans


def _families(launch):
    fam = {}
    for c in launch:
        fam[_family(c)] = fam.get(_family(c), 0) + 1
    if any(c[:2] == (256, 256) for c in launch):
        fam["256x256"] = sum(c[:2] == (256, 256) for c in launch)
    return fam


def _report(case, precision, cfgs, wplans):
    """Prints the counts; returns the families of every launch (forward first, then the data gradient)."""
    fams = [_families(launch) for launch in cfgs]
    print(f"{case} {precision}: configurations per launch {[len(launch) for launch in cfgs]} (forward, data gradient) {fams}, "
          f"{len(wplans)} weight-gradient plans (tile, tile, pixel splits, rows per stage, ring depth) "
          f"{sorted((c[0], c[1], c[2] & 0xffff, (c[2] >> 16) & 0xff, c[2] >> 24) for c in wplans)}")
    return fams


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("index", range(len(E.CONV_CASES)), ids=["-".join(map(str, c)) for c in E.CONV_CASES])
def test_conv_exact_on_every_configuration(index, precision, forced_plans):
    case = E.CONV_CASES[index]
    cfgs, wplans = _walk(case, precision, forced_plans)
    fams = _report(case, precision, cfgs, wplans)
    assert len(fams) >= 2 and all(f.get("tiled", 0) >= 1 for f in fams)
    if precision != "fp32":
        assert len(wplans) >= 1, "no weight-gradient plan was offered"
        fwd, dgrad, splits = _NEEDS.get(index, (set(), set(), 1))
        for need in fwd:
            assert fams[0].get(need, 0) >= 1, f"the forward launch was offered no {need} configuration"
        for need in dgrad:
            assert fams[1].get(need, 0) >= 1, f"the data-gradient launch was offered no {need} configuration"
        assert max(c[2] & 0xffff for c in wplans) >= splits, f"no weight-gradient plan with {splits} pixel splits was offered"


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("case", E.DECONV_CASES, ids=["-".join(map(str, c)) for c in E.DECONV_CASES])
def test_deconv_exact_on_every_configuration(case, bias, precision, forced_plans):
    cfgs, wplans = _walk(case, precision, forced_plans, transposed=True, bias=bias)
    fams = _report(case, precision, cfgs, wplans)
    assert all(f.get("tiled", 0) >= 1 for f in fams)
    if precision != "fp32":
        assert len(wplans) >= 1, "no weight-gradient plan was offered"
