"""The BatchNorm-backward gate of a training plan: the launch that first writes the gradient of a = relu(BN(x)) [+ r] -- a convolution's data
gradient (lh_igemm_gated) or the max-pool's backward -- stores the ReLU-gated gradient and the BatchNorm-backward partial sums of its tiles,
and the node's lh_fuse_bwd skips its reduce pass.  Which nodes may be gated, which launches take the gate, and the gated launch itself.
A mixin of ``engine.Plan`` (split out of engine.py in round 7).  Reference: loss.backward() through relu(bn(conv(x))),
src/modeling/simplebaseline/pose_resnet.py:60-66 and :96-97."""
import ctypes as C

import torch

from . import _lib
from .graph import _Call, _ptr


class BnGate:
    def _note_gate(self, out, terms, bn_state, relu_bits):
        """_c_fuse: record in _gate_info what a gated launch needs of ReLU node ``out``, when it has one of the three gateable forms."""
        if not (self.training and self.with_bwd) or any(l != 0 for _, _, l in terms):
            return
        bn_terms = [i for i, (_, bn, _) in enumerate(terms) if bn is not None]
        if relu_bits is None:
            if len(terms) == 1 and bn_terms:                  # a = relu(BN(raw))
                self._gate_info[id(out)] = dict(raw=terms[0][0], st=bn_state[0])
        elif len(terms) == 2 and all(a.c == out.c for a, _, _ in terms):
            if len(bn_terms) == 1:                            # a residual tail relu(BN(raw) + identity): its sign is in the mask bits
                self._gate_info[id(out)] = dict(raw=terms[bn_terms[0]][0], st=bn_state[bn_terms[0]], mask=relu_bits)
            elif len(bn_terms) == 2:                          # ... with a projection shortcut: relu(BN(raw) + BN2(raw2))
                self._gate_info[id(out)] = dict(raw=terms[0][0], st=bn_state[0], mask=relu_bits, raw2=terms[1][0], st2=bn_state[1])

    def _gate_kind(self, gi, x, masked_addend):
        """May the first writer of x.grad, a data gradient, take the BatchNorm-backward gate of x's node (lh_igemm_gated)?  None | 'x' | 'mask'.
        'x': a single-term node a = relu(BN(raw)) whose only consumer is this convolution.  'mask' (round 6): a residual tail
        relu(BN(raw) + r) -- this convolution is its only consumer, or the other one is the next tail, whose identity gradient has been
        folded into this launch as its masked addend."""
        if gi is None or x.c != x.c_valid:
            return None
        uses = len(self._uses.get(id(x), []))
        if gi.get("mask") is not None:
            ok = self.opt.bn_gate_tail and (uses == 1 or (uses == 2 and masked_addend))
            return None if not ok else "mask2" if gi.get("raw2") is not None else "mask"
        return "x" if uses == 1 else None

    def _cfg_gateable(self, cfg, kind, nbytes):
        """Does kernel configuration cfg take the gate for a tensor of nbytes?  The tiled kernels up to LH_BN_GATE_MAX_MB (measured,
        rounds 4-6: beyond it the epilogue's read of raw costs a tile-per-workgroup launch more than the reduce pass it replaces), the
        persistent kernels (pointwise, direct 3x3: streams of independent waves, the extra read rides with the others) up to
        LH_BN_GATE_PW_MAX_MB; tails up to LH_BN_GATE_TAIL_MAX_MB on either."""
        kernel = _lib.conv_kind(cfg[2])
        pw, tiled = kernel in ("pointwise", "direct"), kernel in ("tiled", "dense")
        opt, mb = self.opt, nbytes / (1 << 20)
        if not (tiled or (pw and opt.bn_gate_pw)):
            return False
        if kind == "mask2":                # two BatchNorm terms (a projection shortcut): the pointwise kernel only
            return kernel == "pointwise" and opt.bn_gate_tail2 and mb <= opt.bn_gate_tail_max_mb
        if kind == "mask":
            return mb <= (opt.bn_gate_tail_max_mb if pw else min(opt.bn_gate_tail_max_mb, opt.bn_gate_tiled_tail_max_mb))
        return mb <= (opt.bn_gate_pw_max_mb if pw else opt.bn_gate_max_mb)

    def _make_gate(self, gi, partial, partial2=None):
        """The lh_bn_bwd_gate of the node recorded as ``gi``: its BatchNorm input(s), saved statistics, mask bits and the partial-sum slab(s)."""
        st = gi["st"]
        gate = _lib.BnBwdGate(gi["raw"].buf.data_ptr(), st["mean"].data_ptr(), st["invstd"].data_ptr(), st["scale"].data_ptr(),
                              st["shift"].data_ptr(), partial.data_ptr(), _ptr(gi.get("mask")))
        if partial2 is not None:
            st2 = gi["st2"]
            gate.x2, gate.mean2, gate.invstd2, gate.partial2 = gi["raw2"].buf.data_ptr(), st2["mean"].data_ptr(), st2["invstd"].data_ptr(), partial2.data_ptr()
        self.keep.append(gate)
        return gate

    def _gated_dgrad(self, dd, dy, pk, x, dx, addend, amask, gi, gkind, what):
        """x = relu(BN(raw)) with this convolution as its only consumer -- or a residual tail relu(BN(raw) + r) whose other
        consumer, the next tail's identity term, rides in as this launch's masked addend: the launch stores the ReLU-gated
        gradient and the BatchNorm-backward partial sums of its tile (the node's backward skips its reduce pass)."""
        two = gkind == "mask2"
        rows = self.lib.lh_igemm_gated_rows(C.byref(dd), self.dt, 2 if two else 1)
        partial = self._alloc(rows * 2 * x.c, dtype=torch.float32)
        partial2 = self._alloc(rows * 2 * x.c, dtype=torch.float32) if two else None
        gate = self._make_gate(gi, partial, partial2)
        self.keep.append(dd)
        c = _Call(self.lib.lh_igemm_gated, (C.byref(dd), _ptr(dy), _ptr(pk), _ptr(dx), _ptr(addend), _ptr(amask), C.byref(gate), self.dt),
                  what + " + BN-backward gate" + (" (mask bits)" if gi.get("mask") is not None else ""))
        c.keep = dd
        c.ig = dict(src=1, dst=3, addend=4, addend_mask=5)
        self.bwd.append(c)
        self._gated[id(x)] = (partial, rows, partial2)

    def _gate_meta(self, dd, x):
        """(kernel name, extra algorithmic bytes) of the data gradient just emitted when it is a gated launch (lh_igemm_gated): every kernel
        has gate instantiations of its own (igemm_ring_gated_kernel<..>, igemm_pw_kernel<.., true, terms>, conv3x3_direct_kernel<.., true, true>),
        and the epilogue reads the BatchNorm input of every gated term (what the reduce pass of lh_fuse_bwd no longer reads) plus the mask bits."""
        c = self.bwd[-1]
        if getattr(c, "fn", None) is not self.lib.lh_igemm_gated:
            return None, 0.0
        g = self._gated[id(x)]
        terms = 2 if len(g) > 2 and g[2] is not None else 1
        name = self._kname(dd, stats=True)
        if name.startswith("igemm_pw_kernel"):
            name = name[:-1] + f", {terms}>"
        elif name.startswith("conv3x3_direct_kernel"):
            name = name[:-1] + ", true>"
        elif name.startswith("igemm_ring_kernel"):
            name = name.replace("igemm_ring_kernel", "igemm_ring_gated_kernel", 1)
        return name, float(terms) * x.pixels * x.c * self.es + (x.pixels * x.c / 8 if "mask" in c.what else 0.0)
