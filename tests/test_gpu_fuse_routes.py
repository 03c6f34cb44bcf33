"""The launch routes of the fused BatchNorm / ReLU elementwise op (csrc/fuse_fwd.hip, fuse_bwd.hip + fuse_bwd_kernel.h / fuse_bwd_plan.h),
driven through the C ABI: a call computes the same bytes alone and as one entry of a multi-problem call (its own kernel, a
multi-problem launch of that kernel, the mixed kernels, the in-order route of two passes that write one buffer), and the generic
reduce pass is right in value past 256 channel chunks."""
import ctypes as C

import pytest
import torch

from lighthand_amd import _lib
from lighthand_amd._lib import BnFinalizeCall, FuseBwdCall, FuseBwdDesc, FuseDesc, FuseFwdCall

pytestmark = pytest.mark.gpu

DT = {"fp32": (torch.float32, _lib.LH_F32), "bf16": (torch.bfloat16, _lib.LH_BF16), "fp16": (torch.float16, _lib.LH_F16)}
DX_FILL, PARAM_FILL = 0.5, -7.0          # what output buffers hold before a call (DX_FILL is the addend of an accumulating term)


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _up(t, l):
    return t.repeat_interleave(1 << l, 1).repeat_interleave(1 << l, 2) if l else t


def _mask_bits(out, epc):
    """lh_fuse_fwd's relu_mask of a stored activation: one byte per 16-byte chunk, bit e = (element e > 0)."""
    pos = (out.float() > 0).reshape(-1, epc).to(torch.int32)
    return (pos << torch.arange(epc, device=out.device, dtype=torch.int32)).sum(1).to(torch.uint8)


class Term:
    def __init__(self, bn=True, l=0, acc=0, want=True, same_dx_as=None):
        self.bn, self.l, self.acc, self.want, self.same_dx_as = bn, l, acc, want, same_dx_as


class BwdNode:
    """One lh_fuse_bwd node: fixed inputs; fresh() makes new, identically filled output buffers and the descriptor over them.
    relu: "off", "out" (stored activation), "mask" (mask bits, no activation), "shift" (activation and the forward shift vectors)."""

    def __init__(self, seed, dtype, n, h, w, c, terms, relu, strips_cap=0, coarse=False, pre=False, l2_touch=False):
        td, _ = DT[dtype]
        g = torch.Generator().manual_seed(seed)
        self.dtype, self.td, self.shape, self.terms, self.relu, self.strips_cap = dtype, td, (n, h, w, c), terms, relu, strips_cap
        self.epc = 16 // torch.empty(0, dtype=td).element_size()

        def rnd(*shape):
            v = torch.randn(*shape, generator=g)
            return ((v * 8).round().clamp(-32, 32) / 8 if coarse else v).to(td).cuda()       # coarse: multiples of 1/8, |v| <= 4
        self.dout = rnd(n, h, w, c)
        self.x, self.scale, self.shift, self.mean, self.invstd = [], [], [], [], []
        acc = torch.zeros(n, h, w, c, device="cuda")
        for t in terms:
            x = rnd(n, h >> t.l, w >> t.l, c)
            self.x.append(x)
            if t.bn:
                self.scale.append((0.5 + torch.rand(c, generator=g)).cuda())
                self.shift.append((0.3 * torch.randn(c, generator=g)).cuda())
                self.mean.append((0.1 * torch.randn(c, generator=g)).cuda())
                self.invstd.append((0.5 + torch.rand(c, generator=g)).cuda())
                acc += _up(x.float() * self.scale[-1] + self.shift[-1], t.l)
            else:
                self.scale.append(None); self.shift.append(None); self.mean.append(None); self.invstd.append(None)
                acc += _up(x.float(), t.l)
        self.out = torch.relu(acc).to(td) if relu != "off" else acc.to(td)
        self.mask = _mask_bits(self.out, self.epc) if relu == "mask" else None
        self.pre = None
        if pre:          # the gated gradient's partial sums come with dout (lh_igemm_gated): any slab will do for a route comparison
            self.pre = [torch.randn(pre, 2, c, generator=g).cuda() for _ in terms]
        self.touch = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda") if l2_touch else None

    def fresh(self, lib):
        n, h, w, c = self.shape
        o = {"dx": [], "dgamma": [], "dbeta": []}
        for i, t in enumerate(self.terms):
            if t.same_dx_as is not None:
                o["dx"].append(o["dx"][t.same_dx_as])
            else:
                o["dx"].append(torch.full((n, h >> t.l, w >> t.l, c), DX_FILL, dtype=self.td, device="cuda") if t.want else None)
            o["dgamma"].append(torch.full((c,), PARAM_FILL, device="cuda") if t.bn else None)
            o["dbeta"].append(torch.full((c,), PARAM_FILL, device="cuda") if t.bn else None)
        o["ws"] = torch.full((lib.lh_fuse_bwd_workspace_bytes(n, h, w, c),), 0x5A, dtype=torch.uint8, device="cuda")
        d = FuseBwdDesc()
        d.dout = _ptr(self.dout)
        d.out = _ptr(self.out) if self.relu in ("out", "shift") else None
        d.relu_mask = _ptr(self.mask)
        d.relu = 0 if self.relu == "off" else 1
        d.nterms = len(self.terms)
        d.strips_cap = self.strips_cap
        for i, t in enumerate(self.terms):
            d.x[i] = _ptr(self.x[i]) if t.bn else None
            d.scale[i], d.save_mean[i], d.save_invstd[i] = _ptr(self.scale[i]), _ptr(self.mean[i]), _ptr(self.invstd[i])
            d.shift[i] = _ptr(self.shift[i]) if self.relu == "shift" else None
            d.dx[i], d.dgamma[i], d.dbeta[i] = _ptr(o["dx"][i]), _ptr(o["dgamma"][i]), _ptr(o["dbeta"][i])
            d.log2up[i], d.accumulate[i] = t.l, t.acc
        if self.pre:
            d.pre_partial, d.pre_rows = _ptr(self.pre[0]), self.pre[0].shape[0]
            if len(self.terms) == 2 and self.terms[0].bn and self.terms[1].bn:
                d.pre_partial2 = _ptr(self.pre[1])
        if self.touch is not None:
            d.l2_touch, d.l2_touch_bytes = _ptr(self.touch), self.touch.numel()
        o["desc"] = d
        return o

    @staticmethod
    def buffers(o):
        seen, res = set(), []
        for k in ("dx", "dgamma", "dbeta"):
            for i, t in enumerate(o[k]):
                if t is not None and t.data_ptr() not in seen:
                    seen.add(t.data_ptr())
                    res.append((f"{k}[{i}]", t))
        return res


def bwd_single(lib, nodes):
    s = torch.cuda.current_stream().cuda_stream
    outs = [nd.fresh(lib) for nd in nodes]
    for nd, o in zip(nodes, outs):
        _lib.check(lib.lh_fuse_bwd(C.byref(o["desc"]), *nd.shape, o["ws"].data_ptr(), DT[nd.dtype][1], s), "lh_fuse_bwd")
    torch.cuda.synchronize()
    return outs


def bwd_multi(lib, nodes):
    s = torch.cuda.current_stream().cuda_stream
    outs = [nd.fresh(lib) for nd in nodes]
    calls = (FuseBwdCall * len(nodes))()
    for i, (nd, o) in enumerate(zip(nodes, outs)):
        calls[i].d = C.pointer(o["desc"])
        calls[i].n, calls[i].h, calls[i].w, calls[i].c = nd.shape
        calls[i].workspace = o["ws"].data_ptr()
    _lib.check(lib.lh_fuse_bwd_multi(calls, len(nodes), DT[nodes[0].dtype][1], s), "lh_fuse_bwd_multi")
    torch.cuda.synchronize()
    return outs


def assert_same_bwd(a, b):
    for i, (oa, ob) in enumerate(zip(a, b)):
        for (name, ta), (_, tb) in zip(BwdNode.buffers(oa), BwdNode.buffers(ob)):
            assert torch.equal(ta, tb), f"node {i} {name} differs"


def hetero_bwd_nodes(dtype):
    """Five nodes at n = 3, h = 6, w = 10 (180 pixels: 12 strips of 16 rows, the last one short)."""
    c4, c6 = (32, 48) if dtype != "fp32" else (16, 24)          # 4 chunks (flat kernels) | 6 chunks, no power of two (generic kernels)
    T = Term
    return [BwdNode(11, dtype, 3, 6, 10, c4, [T()], "shift"),                                     # mask-from-x kernels
            BwdNode(12, dtype, 3, 6, 10, c4, [T(), T(bn=False)], "mask"),                         # two-term apply
            BwdNode(13, dtype, 3, 6, 10, c4, [T(), T(l=1)], "out"),                               # flat beside generic: mixed kernels
            BwdNode(14, dtype, 3, 6, 10, c6, [T()], "out"),                                       # generic kernels at l = 0
            BwdNode(15, dtype, 3, 6, 10, c4, [T(acc=1), T(bn=False, l=1, want=False), T(bn=False)], "mask")]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_fuse_bwd_single_calls_equal_the_multi_call(dtype):
    lib = _lib.load()
    nodes = hetero_bwd_nodes(dtype)             # five: more than one multi-problem launch holds, so a leftover group exists
    assert_same_bwd(bwd_single(lib, nodes), bwd_multi(lib, nodes))


class FwdCall:
    """One lh_fuse_fwd call; terms: (bn, l, pending) -- pending: the term's BatchNorm finalize is part of the call (lh_fuse_desc.fin)."""

    def __init__(self, seed, dtype, n, h, w, c, terms, relu=1, l2_touch=False):
        td, _ = DT[dtype]
        g = torch.Generator().manual_seed(seed)
        self.dtype, self.td, self.shape, self.terms, self.relu = dtype, td, (n, h, w, c), terms, relu
        self.epc = 16 // torch.empty(0, dtype=td).element_size()
        self.x = [torch.randn(n, h >> l, w >> l, c, generator=g).to(td).cuda() for _, l, _ in terms]
        self.scale = [(0.5 + torch.rand(c, generator=g)).cuda() if bn else None for bn, _, _ in terms]
        self.shift = [(0.3 * torch.randn(c, generator=g)).cuda() if bn else None for bn, _, _ in terms]
        self.touch = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda") if l2_touch else None
        self.stats, self.gamma, self.beta = [], [], []
        for (bn, l, pending), x in zip(terms, self.x):
            if not pending:
                self.stats.append(None); self.gamma.append(None); self.beta.append(None)
                continue
            flat = x.float().reshape(-1, c)
            tot = torch.stack([flat.sum(0), (flat * flat).sum(0)])         # sums / sums of squares, spread over three slab rows
            slab = torch.zeros((_lib.load().lh_bn_stats_slab_bytes(3, c) + 3) // 4, device="cuda")      # the slab and its fold scratch
            slab[:3 * 2 * c] = torch.stack([tot * 0.5, tot * 0.25, tot * 0.25]).reshape(-1)
            self.stats.append(slab)
            self.gamma.append((0.5 + torch.rand(c, generator=g)).cuda())
            self.beta.append((0.3 * torch.randn(c, generator=g)).cuda())

    def fresh(self):
        n, h, w, c = self.shape
        o = {"out": torch.full((n, h, w, c), DX_FILL, dtype=self.td, device="cuda"),
             "mask": torch.full((n * h * w * c // self.epc,), 0xEE, dtype=torch.uint8, device="cuda"), "fin": [], "keep": []}
        d = FuseDesc()
        d.nterms, d.relu, d.relu_mask = len(self.terms), self.relu, o["mask"].data_ptr()
        for i, (bn, l, pending) in enumerate(self.terms):
            d.x[i], d.log2up[i] = self.x[i].data_ptr(), l
            scale, shift = self.scale[i], self.shift[i]
            if pending:          # the finalize writes scale / shift / saved statistics and updates the running ones
                vec = {k: torch.full((c,), PARAM_FILL, device="cuda") for k in ("scale", "shift", "save_mean", "save_invstd")}
                vec["running_mean"], vec["running_var"] = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
                vec["nbt"] = torch.zeros(1, dtype=torch.int64, device="cuda")
                f = BnFinalizeCall()
                f.stats, f.rows, f.count, f.c = self.stats[i].data_ptr(), 3, n * (h >> l) * (w >> l), c
                f.gamma, f.beta = self.gamma[i].data_ptr(), self.beta[i].data_ptr()
                f.running_mean, f.running_var, f.num_batches_tracked = vec["running_mean"].data_ptr(), vec["running_var"].data_ptr(), vec["nbt"].data_ptr()
                f.momentum, f.eps = 0.1, 1e-5
                f.scale, f.shift, f.save_mean, f.save_invstd = (vec[k].data_ptr() for k in ("scale", "shift", "save_mean", "save_invstd"))
                d.fin[i] = C.pointer(f)
                o["keep"].append(f)
                o["fin"].append(vec)
                scale, shift = vec["scale"], vec["shift"]
            d.scale[i], d.shift[i] = _ptr(scale), _ptr(shift)
        if self.touch is not None:
            d.l2_touch, d.l2_touch_bytes = self.touch.data_ptr(), self.touch.numel()
        o["desc"] = d
        return o

    @staticmethod
    def buffers(o):
        return [("out", o["out"]), ("mask", o["mask"])] + [(f"fin{i}.{k}", v) for i, vec in enumerate(o["fin"]) for k, v in vec.items()]


def fwd_single(lib, calls):
    s = torch.cuda.current_stream().cuda_stream
    outs = [cl.fresh() for cl in calls]
    for cl, o in zip(calls, outs):
        _lib.check(lib.lh_fuse_fwd(C.byref(o["desc"]), o["out"].data_ptr(), *cl.shape, DT[cl.dtype][1], s), "lh_fuse_fwd")
    torch.cuda.synchronize()
    return outs


def fwd_multi(lib, calls):
    s = torch.cuda.current_stream().cuda_stream
    outs = [cl.fresh() for cl in calls]
    arr = (FuseFwdCall * len(calls))()
    for i, (cl, o) in enumerate(zip(calls, outs)):
        arr[i].d, arr[i].out = C.pointer(o["desc"]), o["out"].data_ptr()
        arr[i].n, arr[i].h, arr[i].w, arr[i].c = cl.shape
    _lib.check(lib.lh_fuse_fwd_multi(arr, len(calls), DT[calls[0].dtype][1], s), "lh_fuse_fwd_multi")
    torch.cuda.synchronize()
    return outs


def assert_same_fwd(a, b):
    for i, (oa, ob) in enumerate(zip(a, b)):
        for (name, ta), (_, tb) in zip(FwdCall.buffers(oa), FwdCall.buffers(ob)):
            assert torch.equal(ta, tb), f"call {i} {name} differs"


def hetero_fwd_calls(dtype, upsampled):
    c = 32 if dtype != "fp32" else 16
    calls = [FwdCall(21, dtype, 3, 6, 10, c, [(True, 0, True)]), FwdCall(22, dtype, 2, 4, 6, c, [(True, 0, False)]),
             FwdCall(23, dtype, 1, 9, 8, 2 * c, [(True, 0, True)]), FwdCall(24, dtype, 3, 6, 10, c, [(True, 0, False)]),
             FwdCall(25, dtype, 2, 6, 4, c, [(True, 0, True)])]
    if upsampled:            # one call of another kind: the calls run one by one
        calls[2] = FwdCall(26, dtype, 3, 6, 10, c, [(True, 0, True), (True, 1, False)])
    return calls


@pytest.mark.parametrize("upsampled", [False, True], ids=["one_kind", "upsampled_among_them"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_fuse_fwd_single_calls_equal_the_multi_call(dtype, upsampled):
    lib = _lib.load()
    calls = hetero_fwd_calls(dtype, upsampled)
    assert_same_fwd(fwd_single(lib, calls), fwd_multi(lib, calls))


@pytest.mark.parametrize("shape", ["pair", "triple"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_two_terms_that_write_one_gradient_keep_their_order(dtype, shape):
    """Two identity terms of one node write the same dx, the second accumulating: the passes run in recorded order, alone and
    beside another node; on values where every sum is exact (multiples of 1/8, |v| <= 4) the result equals the sum of two
    single-term calls into separate buffers.  pair: the two-term apply pass; triple: two one-term passes and a third term."""
    lib = _lib.load()
    c = 32 if dtype != "fp32" else 16
    T = Term
    terms = [T(bn=False), T(bn=False, acc=1, same_dx_as=0)] + ([T(l=1)] if shape == "triple" else [])
    node = BwdNode(31, dtype, 3, 6, 10, c, terms, "mask", coarse=True)
    other = BwdNode(32, dtype, 3, 6, 10, c, [T()], "shift")
    alone, beside = bwd_single(lib, [node, other]), bwd_multi(lib, [node, other])
    assert_same_bwd(alone, beside)
    parts = []
    for k in range(2):
        one = BwdNode(31, dtype, 3, 6, 10, c, [T(bn=False)], "mask", coarse=True)
        one.dout, one.out, one.mask = node.dout, node.out, node.mask
        parts.append(bwd_single(lib, [one])[0]["dx"][0])
    assert torch.equal(alone[0]["dx"][0].float(), parts[0].float() + parts[1].float())
    assert float(parts[0].float().abs().max()) > 0


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_two_term_node_with_an_unwanted_batchnorm_gradient(dtype):
    """Two flat terms, BatchNorm + identity, dx[0] = NULL: the two-term apply pass skips the BatchNorm term (it has no
    coefficients: its reduce pass and fold were not planned) and writes the identity term's dx = dout * (out > 0); the
    unwanted term's dgamma / dbeta stay untouched.  Alone and beside another node."""
    lib = _lib.load()
    c = 32 if dtype != "fp32" else 16
    node = BwdNode(51, dtype, 3, 6, 10, c, [Term(want=False), Term(bn=False)], "mask")
    other = BwdNode(52, dtype, 3, 6, 10, c, [Term()], "out")
    alone, beside = bwd_single(lib, [node, other]), bwd_multi(lib, [node, other])
    assert_same_bwd(alone, beside)
    want = torch.where(node.out.float() > 0, node.dout.float(), torch.zeros((), device="cuda")).to(node.td)
    assert torch.equal(alone[0]["dx"][1], want)
    assert alone[0]["dx"][0] is None
    assert float((alone[0]["dgamma"][0] - PARAM_FILL).abs().max()) == 0 and float((alone[0]["dbeta"][0] - PARAM_FILL).abs().max()) == 0


def test_generic_reduce_past_256_chunks_matches_the_formula():
    """fp32, c = 1028: 257 channel chunks, so the generic reduce pass takes a second round of its chunk loop with ONE chunk (the
    path of fp32 ResNet-50 at full size).  dx / dgamma / dbeta against an fp64 evaluation of the formula in include/lighthand_hip.h.
    Bounds: the op's fp32 bounds of test_gpu_ops.py::test_bn_fuse_fwd_bwd_fp32 (2e-4 dx, 3e-4 parameter gradients).
    Measured on the commit before the split of fuse_bwd.hip: dx 9.08e-08, dgamma 8.00e-08, dbeta 8.26e-08 -- inside them."""
    lib = _lib.load()
    n, h, w, c = 1, 4, 8, 1028
    node = BwdNode(41, "fp32", n, h, w, c, [Term()], "out")
    o = bwd_single(lib, [node])[0]
    g = node.dout.double() * (node.out > 0)
    xhat = (node.x[0].double() - node.mean[0].double()) * node.invstd[0].double()
    s0, s1 = g.sum((0, 1, 2)), (g * xhat).sum((0, 1, 2))
    cnt = n * h * w
    dx = node.scale[0].double() * (g - s0 / cnt - xhat * s1 / cnt)
    e_dx, e_dg, e_db = rel_err(o["dx"][0], dx), rel_err(o["dgamma"][0], s1), rel_err(o["dbeta"][0], s0)
    print(f"c = 1028 fp32: rel err dx {e_dx:.3e}, dgamma {e_dg:.3e}, dbeta {e_db:.3e}")
    assert e_dx < 2e-4 and e_dg < 3e-4 and e_db < 3e-4
