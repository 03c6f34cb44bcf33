"""Static-shape execution engine: turns a model's layer description into two flat lists
of pre-bound HIP launches (forward, backward) over pre-allocated NHWC buffers.

There is no tracing compiler and no per-op autograd: a model describes itself once through
``GraphBuilder`` (conv / deconv / fuse / maxpool nodes that name their parameters by the
reference's state_dict keys), ``Plan`` allocates every activation, gradient, weight pack
and workspace for one (batch, H, W, precision, mode), and running the network is a loop
of ctypes calls on the caller's HIP stream -- which is exactly what a hipGraph captures
(``lighthand_amd.runtime.TrainStep``).
"""
import ctypes as C

import torch

from . import _lib
from ._lib import FuseBwdDesc, FuseDesc, IgemmDesc, check, conv_kind
from .batch_groups import BatchGroups
from .bn_gate import BnGate
from .graph import BN_EPS, BN_MOMENTUM, PRECISIONS, Act, GraphBuilder, _Call, _Marker, _desc, _ptr, _taps_array  # noqa: F401 (re-exported)
from .infer_rewrites import InferRewrites
from .options import PlanOptions
from .runner import Runner
from .tuner import Tuner
from .weight_packs import WeightPacks
from .wgrad_schedule import WgradSchedule


# --------------------------------------------------------------------------------------- plan
class Plan(Tuner, WgradSchedule, BatchGroups, InferRewrites, WeightPacks, BnGate, Runner):
    """Everything needed to run one model at one static shape."""

    def __init__(self, model, n, h, w, precision="fp32", training=True, backward=None, device=None, wgrad_bucket_bytes=None, options=None):
        self.lib = _lib.load()
        self.opt = options if options is not None else PlanOptions.from_env()     # the LH_* planning switches, resolved once (options.py)
        self.precision = precision
        self.tdtype = PRECISIONS[precision]
        self.dt = _lib.dtype_code(self.tdtype)
        self.es = self.tdtype.itemsize if hasattr(self.tdtype, "itemsize") else torch.tensor([], dtype=self.tdtype).element_size()
        self.epc = 16 // self.es
        self.training = training                 # BatchNorm mode: batch statistics + running update
        self.with_bwd = training if backward is None else backward
        self.n, self.h, self.w = n, h, w
        self.params = dict(model.state_dict(keep_vars=True))
        self.device = device or next(iter(self.params.values())).device
        if self.device.type != "cuda":
            raise _lib.LightHandError("lighthand_amd runs on a HIP device only; move the model with .to('cuda')")
        self.grads = {}
        arena = getattr(model, "_lh_arena", None)
        self.arena_offsets = arena.offsets if arena is not None else {}
        self.arena_numel = arena.numel if arena is not None else 0
        if self.with_bwd:
            for k, p in self.params.items():
                if isinstance(p, torch.nn.Parameter):
                    self.grads[k] = arena.grad_view(k) if arena is not None else torch.zeros_like(p)
        gb = GraphBuilder(n, h, w, self.params)
        model.describe(gb)
        self.nodes = gb.nodes
        self.node_lanes = gb.node_lanes
        self.node_branch, inside = [], False                   # node sits inside a fork .. join region (branch 0 runs on lane 0, and
        for kind, _ in gb.nodes:                                # _batch_order moves grouped regions to lane 0: the lanes do not say it)
            inside = (inside or kind == "fork") and kind != "join"
            self.node_branch.append(inside)
        self.n_lanes = max(gb.node_lanes) + 1 if gb.node_lanes else 1
        self.use_lanes = self.n_lanes > 1
        # Multi-problem launches: the nodes at the same position of the parallel chains of a fork .. join region (HRNet's
        # branches) are compiled as a GROUP whose launches merge into lh_*_multi calls (one grid for 2-4 problems) on the
        # main stream, instead of one launch per branch on stream lanes.  16-bit types; LH_BATCH=0 keeps the lanes.
        self.batch = self.opt.batch and self.es == 2 and self.n_lanes > 1
        self.wgrad_batch = self.opt.wgrad_batch and self.es == 2
        # Table launches (round 6): ALL weight gradients of a deferred group that share a tile class run as ONE grid with a split count
        # per layer + at most one fold grid (lh_wgrad_table_run; _table_wgrads).  LH_WGRAD_TABLE=0: one launch (+ fold) per layer.
        self.wgrad_table = self.opt.wgrad_table and self.es == 2
        self.wgrad_tables = []             # (call, info, member names) of every table launch of the plan
        self._forced = None                # kernel choices of the group being compiled (see _tune_group)
        self._n_groups = 0
        self._lane_streams = {L: torch.cuda.Stream(device=self.device) for L in range(1, self.n_lanes)} if self.use_lanes else {}
        self._cur_lane = 0
        self._emit_group = 1           # size of the batch group whose backward blocks are being emitted
        # Deferred weight gradients: the weight-gradient launches (+ folds) of a GROUP of layers are appended behind one
        # event and run on a side stream while the stream that produced their dy walks on (the main stream of a
        # single-lane network; a branch lane of HRNet: its chain inside one module).  Groups alternate over the side
        # streams, each with its own split-K slab.  LH_WGRAD_GROUP = layers per group (0 = weight gradients in place).
        n_convs = sum(1 for k, _ in self.nodes if k in ("conv", "deconv"))
        auto_group = max(4, -(-n_convs * 62 // 100))         # 36 layers for R50 (re-measured in round 3: 24: 9.65 ms, 32-40: 9.59-9.61, 48: 9.77)
        if self.n_lanes > 1:
            auto_group = 16                                   # branch lanes hand over at every module end; 16 on the main lane
        self.wgrad_group = (auto_group if self.opt.wgrad_group is None else self.opt.wgrad_group) if self.with_bwd else 0
        # data-parallel plans: a deferred group ALSO ends as soon as its layers hold one gradient bucket's worth of
        # parameters, so the first bucket's all-reduce starts early in the backward pass (parallel.wgrad_group_cuts)
        self.wgrad_bucket_bytes = wgrad_bucket_bytes
        if self.wgrad_group > 0:
            self.use_lanes = True
            self._w_lanes = (2 if self.n_lanes == 1 else 4) if self.opt.wgrad_lanes is None else self.opt.wgrad_lanes
            for i in range(self._w_lanes):
                self._lane_streams[-1 - i] = torch.cuda.Stream(device=self.device)
        self._pend = {}                    # source lane -> dict(calls, names, layers, ws)
        self._w_flushes = 0
        self._ready = {}
        self.out_act = gb.out
        self.fwd, self.bwd, self.packs = [], [], []
        self._pack_items = []
        self._pack_convs = {}              # id(weight) -> PackConv (LDS-tiled transposing pack)
        self._late_packs = None            # (pack buffers of the late group, pack buffers of the conv whose first use is the fork point)
        self._packjoin_at = self._pack_stream = None                     # weight_packs._place_pack_markers
        self._pack_event = self._pack_event2 = self._pack_late = None    # between refresh_packs(overlap=True) and the markers of one forward
        self._regions = []                 # [fork marker, join marker or None] of every branch region of the forward list
        self._in_branch = self._head_fused = False       # emitting the backward of a node inside a branch region; _fuse_head wrote the output
        self._n_l2_touch = self._n_fused_bottlenecks = 0
        self.bn_bwd_8d_bytes = 0.0         # what SURVEY 8(d)'s traffic model charges to the BatchNorm backward (bench.py)
        self._producers = {}               # id(raw conv output Act) -> the igemm calls that write it (eval-mode BN folding)
        self.keep = []                     # ctypes objects / tensors referenced by raw pointer
        self._ws_wgrad = 0
        self._ws_fuse = 0
        self._ws_users = []
        self._ws_users_fuse = []
        self.profile_meta = []             # (list name, call object, kernel name, flops, bytes)
        self._tune_bufs = {}
        Plan._tune_cache_io()
        n_tuned = len(Plan._tune_measured)
        self._compile()
        self._tune_bufs = {}               # scratch operands of the autotuner are only needed while compiling
        if len(Plan._tune_measured) != n_tuned:
            Plan._tune_cache_io(save=True)

    # ------------------------------------------------------------------ helpers
    def _alloc(self, *shape, dtype=None, zero=False):
        f = torch.zeros if zero else torch.empty
        t = f(*shape, dtype=dtype or self.tdtype, device=self.device)
        self.keep.append(t)
        return t

    def _act_buf(self, a):
        if a.buf is None:
            a.buf = self._alloc(a.n, a.h, a.w, a.c, zero=a.c != a.c_valid)
        return a.buf

    def _act_grad(self, a):
        if a.grad is None:
            a.grad = self._alloc(a.n, a.h, a.w, a.c, zero=True)
        return a.grad

    # positions of lh_igemm's arguments inside a _Call.args tuple
    _IG = dict(desc=0, src=1, pack=2, dst=3, addend=4, addend_mask=5, bias=6, scale=7, shift=8, stats=9)

    def _igemm(self, lst, d, src, pack, dst, addend, bias, stats, what, flops=0, produces=None, addend_mask=None):
        self.keep.append(d)
        c = _Call(self.lib.lh_igemm, (C.byref(d), _ptr(src), _ptr(pack), _ptr(dst), _ptr(addend), _ptr(addend_mask), _ptr(bias), 0, 0,
                                      _ptr(stats), self.dt), what)
        c.keep = d
        lst.append(c)
        if produces is not None:
            self._producers.setdefault(id(produces), []).append(c)
        return c

    def _dgrad(self, descs, dy, packs, x, what):
        """Data-gradient launches into x.grad (the first writer of a gradient buffer overwrites, later ones add)."""
        dx = self._act_grad(x)
        first = self._first_write(x)
        if not first and len(descs) > 1:          # accumulating: a phase without taps would add zeros -- drop it
            keep = [i for i, dd in enumerate(descs) if dd.ntaps > 0]
            descs, packs = [descs[i] for i in keep], [packs[i] for i in keep]
        addend, amask = (None if first else dx), None
        pend = self._masked_addend.pop(id(x), None)
        if pend is not None:
            # the identity-shortcut gradient of a residual tail, dout * mask, was NOT written by that tail's lh_fuse_bwd:
            # this first writer of dx adds it straight from dout (one tensor write and one read less per block)
            assert first
            addend, amask = pend
        kind = "masked" if amask is not None else ("plain" if addend is not None else None)
        if self._phase_rows(descs) > 0:
            self._tune(descs, addend=kind)
            self._igemm_phases(self.bwd, descs, dy, packs, dx, addend, None, None, what, addend_mask=amask)
            yield max(descs, key=lambda d: d.ntaps), sum(d.ntaps for d in descs)
            return
        for dd, pk in zip(descs, packs):
            # (networks with parallel branches: gated OUTSIDE their branch regions only -- HRNet's stem, layer1, transitions: 12.93 -> 12.84 ms.
            #  Inside them the members of a batch group run merged tiled launches whose reduce passes are merged too: carrying the gates into
            #  lh_igemm_multi was measured +0.26 ms SLOWER, round 6; a plan computes the same sums whether its branches run as groups or lanes)
            in_branch = self._emit_group > 1 or self._cur_lane != 0 or self._in_branch
            gi = self._gate_info.get(id(x)) if (self.opt.bn_gate and first and len(descs) == 1 and self.es == 2 and
                                                (self.n_lanes == 1 or (self.opt.bn_gate_branches and not in_branch))) else None
            gkind, gbytes = self._gate_kind(gi, x, amask is not None), x.pixels * x.c * self.es
            self._tune([dd], addend=kind, role="dgrad", gate=(gkind, gbytes) if gkind else None)
            cfg = (C.c_int * 5)()
            if gkind and self.lib.lh_igemm_config(C.byref(dd), self.dt, cfg) == 0 and self._cfg_gateable(cfg, gkind, gbytes):
                self._gated_dgrad(dd, dy, pk, x, dx, addend, amask, gi, gkind, what)
            else:
                self._igemm(self.bwd, dd, dy, pk, dx, addend, None, None, what, addend_mask=amask)
            yield dd, dd.ntaps

    def _patch(self, call, relu=None, **ptrs):
        a = list(call.args)
        ig = call.ig or self._IG
        for k, v in ptrs.items():
            a[ig[k]] = v
        call.args = tuple(a)
        if relu is not None:
            for d in (call.keep if isinstance(call.keep, list) else [call.keep]):
                d.relu = int(relu)

    _IGP = dict(src=2, dst=4, addend=5, addend_mask=6, bias=7, scale=8, shift=9, stats=10)      # lh_igemm_phases argument positions

    def _phase_rows(self, descs):
        """Rows of the stats slab ONE phase of a batched launch writes, or -1 when the phases cannot be batched."""
        if len(descs) < 2 or len(descs) > 4:
            return -1
        arr = (C.POINTER(IgemmDesc) * len(descs))(*[C.pointer(d) for d in descs])
        return self.lib.lh_igemm_phases_rows(arr, len(descs), self.dt)

    def _igemm_phases(self, lst, descs, src, packs, dst, addend, bias, stats, what, produces=None, addend_mask=None):
        """The sub-pixel phases of a stride-2 transposed form as one launch (lh_igemm_phases)."""
        arr = (C.POINTER(IgemmDesc) * len(descs))(*[C.pointer(d) for d in descs])
        parr = (C.c_void_p * len(descs))(*[pk.data_ptr() if pk is not None else None for pk in packs])
        self.keep += [arr, parr] + list(descs)
        c = _Call(self.lib.lh_igemm_phases, (arr, len(descs), _ptr(src), parr, _ptr(dst), _ptr(addend), _ptr(addend_mask), _ptr(bias), 0, 0,
                                             _ptr(stats), self.dt), what + f" ({len(descs)} phases)")
        c.keep, c.ig = list(descs), self._IGP
        lst.append(c)
        if produces is not None:
            self._producers.setdefault(id(produces), []).append(c)
        return c

    def _copy4(self, dst, src, what, lane=0):
        """dst.copy_(src) for two fp32 views of equal shape (<= 4 dims, any strides) as one C-ABI launch."""
        assert dst.dtype == src.dtype == torch.float32 and tuple(dst.shape) == tuple(src.shape) and dst.dim() <= 4
        pad = 4 - dst.dim()
        shape = (C.c_int * 4)(*([1] * pad + list(dst.shape)))
        ds = (C.c_long * 4)(*([0] * pad + list(dst.stride())))
        ss = (C.c_long * 4)(*([0] * pad + list(src.stride())))
        return _Call(self.lib.lh_copy_strided_f32, (dst.data_ptr(), src.data_ptr(), shape, ds, ss), what, keep=(shape, ds, ss, dst, src), lane=lane)

    def _bias_grad(self, dy, y, cout, gb_):
        """d(bias) of a convolution / transposed convolution inside the network = the per-channel sum of its output
        gradient (NHWC, run precision): lh_channel_sum_nhwc, fp64 partial sums in a fixed order."""
        ws = self._alloc(self.lib.lh_channel_sum_workspace_bytes(cout), dtype=torch.uint8)
        return _Call(self.lib.lh_channel_sum_nhwc, (dy.data_ptr(), y.pixels, cout, y.c, gb_.data_ptr(), ws.data_ptr(), self.dt), "bias grad", lane=1)

    def _padded_bias(self, nd, y, cout):
        """The fp32 bias of convolution node nd padded to y's channel count (refilled with the weight packs); None without a bias."""
        if not nd["bias"]:
            return None
        bias = self._alloc(y.c, dtype=torch.float32, zero=True)
        self.packs.append(self._copy4(bias[:cout], self.params[nd["bias"]].detach(), "bias pad"))
        return bias

    def _wgrad_call(self, a, what, slab_bytes, flops, nbytes, wbufs=None, keep_desc=None):
        """One lh_wgrad_fused call (weight gradient + fold of its pixel splits, argument list ``a``; the slab a[7] is bound by _ws_note) into
        the weight-gradient list of the node being emitted, which is returned.  wbufs: the tensors behind a's x / dy pointers -- the call
        may then join a table launch (_table_wgrads); keep_desc: its descriptor -- it may then merge with same-shape launches (_batch_wgrads)."""
        cw = _Call(self.lib.lh_wgrad_fused, None, what, keep=a[13], lane=1)
        cw.keep_desc = keep_desc
        if wbufs is not None:
            cw.wargs, cw.wbufs = a, wbufs

        def set_ws(ptr):
            a[7] = ptr
            cw.args = tuple(a)
        cw.ws_ent = self._ws_note(set_ws, slab_bytes)
        wl = self._wl()
        wl.append(cw)
        self.profile_meta.append(("bwd", cw, self._kname(a[0]._obj, wgrad=(a[5], a[6])), flops, nbytes))
        return wl

    def _kname(self, d, wgrad=None, stats=False):
        """Kernel instantiation name as rocprofv3 prints it (for roofline attribution)."""
        t = {"fp32": "float", "bf16": "__bf16", "fp16": "_Float16"}[self.precision]
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        if wgrad is None:
            cfg = (C.c_int * 5)()
            check(self.lib.lh_igemm_config(C.byref(d), self.dt, cfg), "lh_igemm_config")
            bm, bp, depth, kb = cfg[0], cfg[1], cfg[2], cfg[3]
            kind = conv_kind(depth)
            if kind == "pointwise":
                return f"igemm_pw_kernel<{t}, {bm}, {kb}, {bp // 16}, {'true' if stats else 'false'}>"
            if kind == "direct":
                return f"conv3x3_direct_kernel<{t}, {kb}, {'true' if stats else 'false'}>"
            wc, wp = {(256, 256): (2, 4), (128, 256): (2, 2), (256, 128): (4, 2), (128, 128): (2, 2), (128, 64): (4, 1), (64, 128): (1, 4), (64, 64): (2, 2)}[(bm, bp)]
            if kind == "dense":                 # eight waves on the 4-wave tiles; the code is ring depth + 20 (igemm_ring_cfgs.h)
                wc, wp = {(128, 128): (2, 4), (128, 64): (4, 2), (64, 128): (2, 4), (64, 64): (2, 4), (128, 256): (2, 4), (256, 128): (4, 2)}[(bm, bp)]
                depth -= 20
            if kind == "staged":
                return f"igemm_kernel<{t}, {bm}, {bp}, {wc}, {wp}>"
            return f"igemm_ring_kernel<{t}, {bm}, {bp}, {wc}, {wp}, {depth}, {kb}>"
        r = C.c_int(0)
        check(self.lib.lh_wgrad_tile(C.byref(d), wgrad[0], wgrad[1], self.dt, C.byref(a), C.byref(b), C.byref(c), C.byref(r)), "lh_wgrad_tile")
        wo, wi = {(256, 256): (2, 4), (128, 128): (2, 2), (128, 64): (4, 1), (64, 128): (1, 4), (64, 64): (2, 2)}[(a.value, b.value)]
        if r.value:
            return f"wgrad_ring_kernel<{t}, {a.value}, {b.value}, {wo}, {wi}, {r.value % 10}, {r.value // 10}>"
        return f"wgrad_kernel<{t}, {a.value}, {b.value}, {wo}, {wi}>"

    def _first_write(self, a):
        """True the first time a gradient buffer is produced in the backward list (every writer calls this once)."""
        n = self._nwrites.get(id(a), 0)
        self._nwrites[id(a)] = n + 1
        return n == 0

    def _alloc_stats(self, y, rows):
        """The BatchNorm statistics slab of y: ``rows`` rows of [2][C] fp32 partial sums, written by the launches that produce y."""
        y.stats = self._alloc((self.lib.lh_bn_stats_slab_bytes(rows, y.c) + 3) // 4, dtype=torch.float32)
        y.stats_rows = rows
        return y.stats

    def _stats_for(self, y, descs):
        """One slab for the launches of ``descs``; returns the byte offset of each launch's rows."""
        rows = [self.lib.lh_igemm_stats_rows(C.byref(d), self.dt) for d in descs]
        self._alloc_stats(y, sum(rows))
        offs, o = [], 0
        for r in rows:
            offs.append(o)
            o += r * 2 * y.c * 4
        return offs

    # ------------------------------------------------------------------ compile
    def _compile(self):
        consumers_bn = set()
        for kind, nd in self.nodes:
            if kind == "fuse":
                for a, bn, _ in nd["terms"]:
                    if bn is not None:
                        consumers_bn.add(id(a))
        self._bn_inputs = consumers_bn
        self._nwrites = {}
        self._masked_addend = {}           # id(activation) -> (dout, relu mask bits) a later data-gradient launch adds
        # BatchNorm-backward gate (lh_igemm_gated): id(activation a = relu(BN(x))) -> what the data gradient that writes a.grad
        # needs (recorded by _c_fuse), and id(a) -> (partial sums, rows) once such a launch has been planned (read by the node's
        # backward, which then skips its reduce pass).  LH_BN_GATE=0: off; the LH_BN_GATE_* switches and caps: options.py.
        self._gate_info, self._gated = {}, {}
        self._bnrelu_info = {}             # id(a = relu(BN(x))) -> its lh_fuse_fwd call and BN state (training plans; _c_maxpool)
        # consumers of every activation in forward order: (kind, node) -- backward visits them in reverse
        self._uses = {}
        for kind, nd in self.nodes:
            if kind in ("conv", "deconv", "maxpool"):
                self._uses.setdefault(id(nd["x"]), []).append((kind, nd))
            elif kind == "fuse":
                for a, _, _ in nd["terms"]:
                    self._uses.setdefault(id(a), []).append((kind, nd))
            elif kind == "output":
                self._uses.setdefault(id(nd["y"]), []).append((kind, nd))
        items = self._batch_order()        # lists of node indices; more than one = a batch group
        bwd_blocks, group_forced = {}, {}
        for item in items:
            gid = None
            if len(item) > 1:
                self._n_groups += 1
                gid = self._n_groups
                self._forced = self._tune_group([self.nodes[i][1] for i in item]) if self.nodes[item[0]][0] == "conv" else None
                group_forced[item[0]] = self._forced
            for j, i in enumerate(item):
                (kind, nd), lane = self.nodes[i], self.node_lanes[i]
                if self._forced is not None:
                    self._forced["member"] = j
                blk = []
                n0 = len(self.fwd)
                getattr(self, "_c_" + kind)(nd, blk)
                for k, c in enumerate(self.fwd[n0:]):
                    c.slane = lane
                    if gid is not None and isinstance(c, _Call):
                        c.mtag = (gid, "f", j, k)
                out_act = nd.get("y", nd.get("out")) if isinstance(nd, dict) else nd
                if out_act is not None:
                    self._ready[id(out_act)] = len(self.fwd)      # list position from which this activation is complete
                bwd_blocks[i] = blk
            self._forced = None
        self._build_pack_launches()
        # backward list: node blocks in reverse order; accumulate flags resolved in that order
        self.bwd_marks = []        # (end index in self.bwd, parameter names whose gradient is final there)
        if self.with_bwd:
            gcount = self._n_groups
            for item in reversed(items):
                gid = None
                if len(item) > 1:
                    gcount += 1
                    gid = gcount
                flush_lanes = []
                self._emit_group = len(item)
                self._forced = group_forced.get(item[0])          # the data gradients are tuned while the blocks are emitted
                for j, i in enumerate(item):
                    (kind, nd), blk, lane = self.nodes[i], bwd_blocks[i], self.node_lanes[i]
                    self._cur_lane, self._in_branch = lane, self.node_branch[i]
                    if self._forced is not None:
                        self._forced["member"] = j
                    if kind == "fork" and self.wgrad_group > 0:      # end of a branch region in backward order: every lane hands
                        for src in sorted(self._pend):                # its group over before the main stream joins
                            self._flush_wgrads(src)
                    n0 = len(self.bwd)
                    w0 = len(self._pending()["calls"]) if self.wgrad_group > 0 else 0
                    for emit in blk:
                        emit()
                    for k, c in enumerate(self.bwd[n0:]):
                        c.slane = lane
                        if gid is not None and isinstance(c, _Call):
                            c.mtag = (gid, "b", j, k)
                    if gid is not None and self.wgrad_group > 0:
                        for k, c in enumerate(self._pending()["calls"][w0:]):
                            if isinstance(c, _Call):
                                c.mtag = (gid, "w", j, k)
                    names = []
                    if kind in ("conv", "deconv"):
                        wnames = [nd["w"] + ".weight"] + ([nd["bias"]] if nd["bias"] else [])
                        if self.wgrad_group > 0:
                            p = self._pending()
                            p["names"] += wnames
                            p["layers"] += 1
                            p["bytes"] += sum(self.params[k].numel() * 4 for k in wnames)
                            # same rule as parallel.wgrad_group_cuts (tested on the CPU with the real parameter sizes)
                            if p["layers"] >= self.wgrad_group or (self.wgrad_bucket_bytes and p["bytes"] >= self.wgrad_bucket_bytes):
                                flush_lanes.append(lane)          # after the whole item: a batch group hands over together
                        else:
                            names += wnames
                    elif kind == "fuse":
                        for _, bn, _ in nd["terms"]:
                            if bn is not None:
                                names += [bn + ".weight", bn + ".bias"]
                    if names:
                        self.bwd_marks.append((len(self.bwd), names))
                self._forced = None
                for lane in dict.fromkeys(flush_lanes):
                    self._cur_lane = lane
                    self._flush_wgrads(lane)
            for src in sorted(self._pend):
                self._flush_wgrads(src, spread=self.opt.tail_spread)
            self.bwd_marks.sort(key=lambda m: m[0])
            # two workspaces: the weight-gradient chain may run concurrently with the BN-backward chain
            # (stream lanes run concurrently: each lane has its own pair)
            lanes = list(range(self.n_lanes if self.use_lanes else 1)) + ([-1 - i for i in range(self._w_lanes)] if self.wgrad_group > 0 else [])
            need_w = {L: max([nb for _, nb, l in self._ws_users if (l if self.use_lanes else 0) == L] + [256]) for L in lanes}
            ws_w = {L: self._alloc(need_w[L], dtype=torch.uint8) for L in lanes}      # ONE shared, cache-resident slab per stream
            ws_f = {L: self._alloc(max(self._ws_fuse, 256), dtype=torch.uint8) for L in lanes}
            for setter, nbytes, lane in self._ws_users:
                L = lane if self.use_lanes else 0
                setter(ws_w[L].data_ptr())
            for setter, lane in self._ws_users_fuse:
                setter(ws_f[lane if self.use_lanes else 0].data_ptr())
        self._attach_l2_touch()
        if self._n_groups:
            self._merge_groups()
        self._place_pack_markers()

    def _attach_l2_touch(self):
        """Training plans: an elementwise BatchNorm / ReLU pass (lh_fuse_fwd) that is followed on its stream by a tiled
        convolution warms that convolution's weight pack in L2 at its tail (lh_fuse_desc.l2_touch; bn_common.h lh_l2_touch).  Every
        workgroup of such a convolution walks the same weight slab stage by stage, at once: each stage waits for lines no XCD has
        seen yet (profiles/r05_ingest_ladder.txt, sitting 6: the complete K loop of the stage-3 3x3 takes 21.3 us, 19.1 us with the
        pack in L2).  Only where the pack fits beside the pass's own stream in the 4 MB L2 of an XCD (LH_L2_TOUCH_MAX_MB, default 3;
        LH_L2_TOUCH=0: off).  Not for members of HRNet's batch groups (measured slightly slower)."""
        if not self.opt.l2_touch or not self.training:
            return
        lim = self.opt.l2_touch_max_mb * (1 << 20)
        touch_all = self.opt.l2_touch == 2      # experiment: the persistent kernels' panels too
        lib, ig, n = self.lib, self._IG, 0

        def attach(lst, fuse_fn, look):
            nonlocal n
            for i, c in enumerate(lst):
                if not isinstance(c, _Call) or c.fn is not fuse_fn or c.lane or c.mtag is not None:
                    continue
                # the next convolution on this call's stream lane, right behind it
                nxt = None
                for d in lst[i + 1:i + 1 + look]:
                    if not isinstance(d, _Call) or d.lane or d.fn is lib.lh_bn_finalize:
                        continue
                    nxt = d
                    break
                if nxt is None or nxt.fn is not lib.lh_igemm or nxt.slane != c.slane or nxt.mtag is not None:
                    continue
                d = nxt.keep
                if (conv_kind(d.cfg[2]) in ("pointwise", "direct") and not touch_all) or not nxt.args[ig["pack"]]:    # pointwise / direct kernels fetch their panel once per workgroup
                    continue
                kstep = 128 // self.es
                nbytes = (d.cout + 127) // 128 * 128 * d.ntaps * ((d.k_run + kstep - 1) // kstep * kstep) * self.es
                if not 0 < nbytes <= lim:
                    continue
                fd = c.args[0]._obj
                fd.l2_touch, fd.l2_touch_bytes = nxt.args[ig["pack"]], nbytes
                n += 1
        attach(self.fwd, lib.lh_fuse_fwd, 3)
        # the same in the backward list: the BatchNorm / ReLU backward of a node (lh_fuse_bwd: its last apply pass) in front of the
        # data gradient that consumes the gradient it wrote
        attach(self.bwd, lib.lh_fuse_bwd, 2)
        self._n_l2_touch = n

    def _c_nop(self, nd, blk):
        pass

    def _c_fork(self, nd, blk):
        self.fwd.append(_Marker("fork"))
        self._regions.append([self.fwd[-1], None])
        blk.append(lambda: self.bwd.append(_Marker("join")))          # backward walks the region in reverse

    def _c_join(self, nd, blk):
        self.fwd.append(_Marker("join"))
        self._regions[-1][1] = self.fwd[-1]
        blk.append(lambda: self.bwd.append(_Marker("fork")))

    def _in_closed_region(self, call):
        """True when `call` sits inside a fork..join region that is already closed: work moved into it from a later node
        (eval-mode folding of a cross-branch sum) would read another lane's output unordered."""
        if not self.use_lanes:
            return False
        i = self.fwd.index(call)
        return any(r[1] is not None and self.fwd.index(r[0]) < i < self.fwd.index(r[1]) for r in self._regions)

    def _c_input(self, a, blk):
        pass        # the consumer (stem conv) owns the image transform

    def _c_input_act(self, a, blk):
        self.in_act = a
        self._act_buf(a)
        if self.with_bwd:
            self._act_grad(a)

    def _c_output(self, nd, blk):
        y = nd["y"]
        if self._head_fused:           # the fused head wrote the fp32 NCHW heat-map itself (_fuse_head)
            return
        self.out_nchw = self._alloc(y.n, y.c_valid, y.h, y.w, dtype=torch.float32)
        self.fwd.append(_Call(self.lib.lh_nhwc_to_nchw_f32, (y.buf.data_ptr(), self.out_nchw.data_ptr(), y.n, y.h, y.w, y.c_valid, y.c, self.dt), "output transform"))
        if self.with_bwd:
            self.dout_nchw = self._alloc(y.n, y.c_valid, y.h, y.w, dtype=torch.float32, zero=True)

            def emit():
                g = self._act_grad(y)
                self._first_write(y)
                self.bwd.append(_Call(self.lib.lh_nchw_f32_to_nhwc, (self.dout_nchw.data_ptr(), g.data_ptr(), y.n, y.h, y.w, y.c_valid, y.c, self.dt), "dheat transform"))
            blk.append(emit)

    # ---- convolution ---------------------------------------------------------------------------
    def _c_conv(self, nd, blk):
        x, y, k, s, p = nd["x"], nd["y"], nd["k"], nd["s"], nd["p"]
        wt = self.params[nd["w"] + ".weight"]
        cout, cin = wt.shape[0], wt.shape[1]
        ybuf = self._act_buf(y)
        bias = self._padded_bias(nd, y, cout)
        all_rs = [(r, q) for r in range(k) for q in range(k)]
        if x.is_image:
            self._c_stem(nd, blk, bias)
            return
        xbuf = self._act_buf(x)
        taps = [(r - p, q - p) for r, q in all_rs]
        d = _desc(x.n, x.h, x.w, x.c, cin, y.h, y.w, s, s, y.c, y.h, y.w, 1, 1, 0, 0, y.c, taps)
        pack = self._pack(wt, cout, cin, (cin * k * k, k * k, k, 1), all_rs, nd["w"] + " fwd pack")
        if self._fuse_head(nd, pack, bias):
            return
        stats_ptr = None
        self._tune([d], with_stats=id(y) in self._bn_inputs and self.training, role="fwd")
        if id(y) in self._bn_inputs and self.training:
            self._stats_for(y, [d])
            stats_ptr = y.stats
        flops = 2.0 * y.pixels * cout * cin * k * k
        self._igemm(self.fwd, d, xbuf, pack, ybuf, None, bias, stats_ptr, nd["w"] + " fwd", produces=y)
        self.profile_meta.append(("fwd", self.fwd[-1], self._kname(d, stats=stats_ptr is not None), flops, (x.pixels * x.c + y.pixels * y.c) * self.es))
        if not self.with_bwd:
            return
        # --- backward: weight gradient, then data gradient
        rs_arr = _taps_array(all_rs)
        gw = self.grads[nd["w"] + ".weight"]
        pad_out = y.c != cout
        gtmp = self._alloc(y.c, cin, k, k, dtype=torch.float32) if pad_out else gw

        def tune_launch(xp, dyp, ws, grad, sp):
            check(self.lib.lh_wgrad_fused(C.byref(d), 0, xp, dyp, y.c, y.c, cin, ws, grad, cin * k * k, k * k, k, 1, rs_arr, 0, self.dt, sp),
                  "autotune lh_wgrad_fused")
        self._tune_wgrad(d, y.c, cin, y.c, tune_launch, y.c * cin * k * k)
        slab_bytes = self.lib.lh_wgrad_workspace_bytes(C.byref(d), y.c, cin, self.dt)
        self._ws_wgrad = max(self._ws_wgrad, slab_bytes)
        dpacks, ddescs = [], []
        if x.needs_grad:
            for ph in range(s):
                for pw in range(s):
                    sub = [(r, q) for r, q in all_rs if (ph + p - r) % s == 0 and (pw + p - q) % s == 0]
                    tp = [((ph + p - r) // s, (pw + p - q) // s) for r, q in sub]
                    gh, gw_ = (x.h - ph + s - 1) // s, (x.w - pw + s - 1) // s
                    dd = _desc(y.n, y.h, y.w, y.c, y.c if pad_out else cout, gh, gw_, 1, 1, x.c, x.h, x.w, s, s, ph, pw, x.c, tp)
                    ddescs.append(dd)
                    dpacks.append(self._pack(wt, cin, cout, (k * k, cin * k * k, k, 1), sub, nd["w"] + " dgrad pack"))

        def emit():
            dy = self._act_grad(y)
            # weight gradient + fold of the pixel splits as ONE C-ABI call (wgrad kernel, then reduce kernel)
            a = [C.byref(d), 0, xbuf.data_ptr(), dy.data_ptr(), y.c, y.c, cin, 0, gtmp.data_ptr(), cin * k * k, k * k, k, 1, rs_arr, 0, self.dt]
            wl = self._wgrad_call(a, nd["w"] + " wgrad", slab_bytes, flops, (x.pixels * x.c + y.pixels * y.c) * self.es, wbufs=(xbuf, dy), keep_desc=d)
            if pad_out:
                wl.append(self._copy4(gw, gtmp[:cout].view_as(gw), "head grad crop", lane=1))
            if nd["bias"]:
                gb_ = self.grads[nd["bias"]]
                if y is self.out_act:      # the head: reduce the contiguous fp32 NCHW gradient instead of strided bf16
                    dn = self.dout_nchw
                    ws = self._alloc(self.lib.lh_channel_sum_workspace_bytes(dn.shape[1]), dtype=torch.uint8)
                    wl.append(_Call(self.lib.lh_channel_sum_nchw, (dn.data_ptr(), dn.shape[0], dn.shape[1], dn.shape[2] * dn.shape[3],
                                                                          gb_.data_ptr(), ws.data_ptr()), "head bias grad"))
                else:
                    wl.append(self._bias_grad(dy, y, cout, gb_))
            if x.needs_grad:
                for dd, ntaps in self._dgrad(ddescs, dy, dpacks, x, nd["w"] + " dgrad"):
                    batched = ntaps != dd.ntaps or (len(ddescs) > 1 and self.bwd[-1].ig is not None)
                    gname, gbytes = self._gate_meta(dd, x)
                    self.profile_meta.append(("bwd", self.bwd[-1], gname or self._kname(dd), 2.0 * dd.n * dd.ho * dd.wo * cin * cout * ntaps,
                                              gbytes + ((x.pixels * x.c + y.pixels * y.c) * self.es if batched else
                                                        (dd.n * dd.ho * dd.wo * x.c + y.pixels * y.c / (s * s)) * self.es)))
        blk.append(emit)

    def _c_stem(self, nd, blk, bias):
        """C_in = 3 convolution: the image is stored as zero-padded NHWC4 and every kernel ROW is
        one tap whose K run covers the k pixels x 4 channels that are contiguous in memory."""
        x, y, k, s, p = nd["x"], nd["y"], nd["k"], nd["s"], nd["p"]
        wt = self.params[nd["w"] + ".weight"]
        cout = wt.shape[0]
        kr = (k * 4 + 7) // 8 * 8
        hp, wp = x.h + 2 * p, x.w + 2 * p + 2
        assert (y.w - 1) * s * 4 + kr <= wp * 4
        self.img_nchw = self._alloc(x.n, 3, x.h, x.w, dtype=torch.float32)
        img = self._alloc(x.n, hp, wp, 4)
        self.img_nhwc4, self.img_pad, self.img_wp = img, p, wp
        self.fwd.append(_Call(self.lib.lh_image_to_nhwc4, (self.img_nchw.data_ptr(), img.data_ptr(), x.n, x.h, x.w, p, wp, self.dt), "image transform"))
        self._image_call_index = len(self.fwd) - 1
        # the flip test's second pass: the image launch of run_forward(mirrored=True), whichever input path wrote img
        self._mirror_call = _Call(self.lib.lh_nhwc4_mirror, (img.data_ptr(), x.n, x.h, x.w, p, wp, self.dt), "image mirror")
        stage = self._alloc(cout, k, kr // 4, 4, dtype=torch.float32, zero=True)
        self.packs.append(self._copy4(stage[:, :, :k, :3], wt.detach().permute(0, 2, 3, 1), "stem weight staging"))
        rows = [(r, 0) for r in range(k)]
        pack = self._pack(stage, cout, kr, (k * kr, 1, kr, 0), rows, nd["w"] + " stem pack")
        d = _desc(x.n, hp, wp, 4, kr, y.h, y.w, s, s, y.c, y.h, y.w, 1, 1, 0, 0, y.c, rows)
        ybuf = self._act_buf(y)
        stats_ptr = None
        flops = 2.0 * y.pixels * cout * 3 * k * k
        direct = (self.training and id(y) in self._bn_inputs and self.es == 2 and (k, s, p, cout, y.c) == (7, 2, 3, 64, 64) and bias is None
                  and self.opt.stem_direct)
        if direct:
            # training stem (pose_resnet.py:151-152) on the direct kernel: weights in registers, a tile's input patch in LDS,
            # raw convolution output + one statistics row per workgroup (stem_pool.hip, lh_stem_conv)
            rows_ = self.lib.lh_stem_conv_rows(x.n, y.h, y.w)
            self._alloc_stats(y, rows_)
            self.keep.append(d)
            c_ = _Call(self.lib.lh_stem_conv, (img.data_ptr(), x.n, hp, wp, pack.data_ptr(), ybuf.data_ptr(), y.stats.data_ptr(), y.h, y.w, self.dt),
                       nd["w"] + " stem fwd (direct)")
            self.fwd.append(c_)
            self._producers.setdefault(id(y), []).append(c_)
            self.profile_meta.append(("fwd", self.fwd[-1], "stem_conv_kernel", flops, (x.pixels * 4 + y.pixels * y.c) * self.es))
        else:
            self._tune([d], with_stats=id(y) in self._bn_inputs and self.training)
            if id(y) in self._bn_inputs and self.training:
                self._stats_for(y, [d])
                stats_ptr = y.stats
            self._igemm(self.fwd, d, img, pack, ybuf, None, bias, stats_ptr, nd["w"] + " stem fwd", produces=y)
            self.profile_meta.append(("fwd", self.fwd[-1], self._kname(d), flops, (x.pixels * 4 + y.pixels * y.c) * self.es))
        if not self.with_bwd:
            return
        # 16-bit runs: all k kernel rows in ONE pass (lh_wgrad_rowfold: dy is read once per input tile, not once per row);
        # the gradient index row*kr + j is gstage's [cout][k][kr] layout, so the fold is a plain sum over the splits
        bo, bi, ns, ring = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        self.lib.lh_wgrad_tile(C.byref(d), y.c, kr, self.dt, C.byref(bo), C.byref(bi), C.byref(ns), C.byref(ring))
        fold = bool(ring.value)
        dw = _desc(x.n, hp, wp, 4, k * kr, y.h, y.w, s, s, y.c, y.h, y.w, 1, 1, 0, 0, y.c, [(0, 0)]) if fold else d
        self.keep.append(dw)
        n_in_w = k * kr if fold else kr
        rs_arr = _taps_array([(0, 0)] if fold else rows)

        def tune_launch(xp, dyp, ws, grad, sp):
            if fold:
                check(self.lib.lh_wgrad_fused(C.byref(dw), k, xp, dyp, y.c, y.c, k * kr, ws, grad, k * kr, 1, 0, 0, rs_arr, 0, self.dt, sp),
                      "autotune lh_wgrad_fused")
            else:
                check(self.lib.lh_wgrad_fused(C.byref(d), 0, xp, dyp, y.c, y.c, kr, ws, grad, k * kr, 1, kr, 0, rs_arr, 0, self.dt, sp),
                      "autotune lh_wgrad_fused")
        self._tune_wgrad(dw, y.c, n_in_w, y.c, tune_launch, y.c * k * kr, tag=("fold", k if fold else 0))
        slab_bytes = self.lib.lh_wgrad_workspace_bytes(C.byref(dw), y.c, n_in_w, self.dt)
        self._ws_wgrad = max(self._ws_wgrad, slab_bytes)
        gstage = self._alloc(cout, k, kr // 4, 4, dtype=torch.float32)
        gw = self.grads[nd["w"] + ".weight"]

        def emit():
            dy = self._act_grad(y)
            if fold:
                a = [C.byref(dw), k, img.data_ptr(), dy.data_ptr(), y.c, y.c, k * kr, 0, gstage.data_ptr(), k * kr, 1, 0, 0, rs_arr, 0, self.dt]
            else:
                a = [C.byref(d), 0, img.data_ptr(), dy.data_ptr(), y.c, y.c, kr, 0, gstage.data_ptr(), k * kr, 1, kr, 0, rs_arr, 0, self.dt]
            wl = self._wgrad_call(a, "stem wgrad", slab_bytes, flops, (x.pixels * 4 + y.pixels * y.c) * self.es)
            wl.append(self._copy4(gw, gstage[:, :, :k, :3].permute(0, 3, 1, 2), "stem grad unstage", lane=1))
        blk.append(emit)

    # ---- transposed convolution ------------------------------------------------------------------
    def _c_deconv(self, nd, blk):
        x, y, k, p = nd["x"], nd["y"], nd["k"], nd["p"]
        wt = self.params[nd["w"] + ".weight"]          # [cin, cout, k, k]
        cin, cout = wt.shape[0], wt.shape[1]
        xbuf, ybuf = self._act_buf(x), self._act_buf(y)
        all_rs = [(r, q) for r in range(k) for q in range(k)]
        bias = self._padded_bias(nd, y, cout)
        descs, packs = [], []
        for ph in range(2):
            for pw in range(2):
                sub = [(r, q) for r, q in all_rs if (ph + p - r) % 2 == 0 and (pw + p - q) % 2 == 0]
                tp = [((ph + p - r) // 2, (pw + p - q) // 2) for r, q in sub]
                gh, gw_ = (y.h - ph + 1) // 2, (y.w - pw + 1) // 2
                descs.append(_desc(x.n, x.h, x.w, x.c, cin, gh, gw_, 1, 1, cout, y.h, y.w, 2, 2, ph, pw, y.c, tp))
                packs.append(self._pack(wt, cout, cin, (k * k, cout * k * k, k, 1), sub, nd["w"] + " deconv pack"))
        with_stats = id(y) in self._bn_inputs and self.training
        if self._phase_rows(descs) > 0:
            self._tune(descs, with_stats=with_stats)
        else:
            for dd in descs:
                self._tune([dd], with_stats=with_stats)
        prow = self._phase_rows(descs)
        if prow > 0:                          # the four sub-pixel phases as ONE launch
            stats = None
            if id(y) in self._bn_inputs and self.training:
                stats = self._alloc_stats(y, 4 * prow)
            self._igemm_phases(self.fwd, descs, xbuf, packs, ybuf, None, bias, stats, nd["w"] + " deconv fwd", produces=y)
            self.profile_meta.append(("fwd", self.fwd[-1], self._kname(descs[0]), 2.0 * x.pixels * cin * cout * k * k,
                                      (x.pixels * x.c + y.pixels * y.c) * self.es))
            descs = []
        offs = [None] * 4
        if descs and id(y) in self._bn_inputs and self.training:
            offs = self._stats_for(y, descs)
        for d, pk, off in zip(descs, packs, offs):
            st = 0 if off is None else y.stats.data_ptr() + off
            c = self._igemm(self.fwd, d, xbuf, pk, ybuf, None, bias, None, nd["w"] + " deconv fwd", produces=y)
            self._patch(c, stats=st)
            self.profile_meta.append(("fwd", self.fwd[-1], self._kname(d), 2.0 * d.n * d.ho * d.wo * cin * cout * d.ntaps,
                                      (x.pixels * x.c + y.pixels * y.c / 4) * self.es))
        if not self.with_bwd:
            return
        # data gradient = stride-2 convolution of dy; weight gradient gathers dy, dense operand is x
        taps = [(r - p, q - p) for r, q in all_rs]
        dg = _desc(y.n, y.h, y.w, y.c, cout, x.h, x.w, 2, 2, x.c, x.h, x.w, 1, 1, 0, 0, x.c, taps)
        self.keep.append(dg)
        gpack = self._pack(wt, cin, cout, (cout * k * k, k * k, k, 1), all_rs, nd["w"] + " deconv dgrad pack")
        rs_arr = _taps_array(all_rs)

        def tune_launch(xp, dyp, ws, grad, sp):            # dy is the gathered operand here, x the dense one
            check(self.lib.lh_wgrad_fused(C.byref(dg), 0, xp, dyp, x.c, cin, cout, ws, grad, cout * k * k, k * k, k, 1, rs_arr, 0, self.dt, sp),
                  "autotune lh_wgrad_fused")
        self._tune_wgrad(dg, cin, cout, x.c, tune_launch, cin * cout * k * k)
        slab_bytes = self.lib.lh_wgrad_workspace_bytes(C.byref(dg), cin, cout, self.dt)
        self._ws_wgrad = max(self._ws_wgrad, slab_bytes)
        gw = self.grads[nd["w"] + ".weight"]
        flops = 2.0 * x.pixels * cin * cout * k * k

        def emit():
            dy = self._act_grad(y)
            a = [C.byref(dg), 0, dy.data_ptr(), xbuf.data_ptr(), x.c, cin, cout, 0, gw.data_ptr(), cout * k * k, k * k, k, 1, rs_arr, 0, self.dt]
            wl = self._wgrad_call(a, nd["w"] + " wgrad", slab_bytes, flops, (x.pixels * x.c + y.pixels * y.c) * self.es, wbufs=(dy, xbuf))
            if nd["bias"]:
                gb_ = self.grads[nd["bias"]]
                wl.append(self._bias_grad(dy, y, cout, gb_))
            if x.needs_grad:
                for _dd, _nt in self._dgrad([dg], dy, [gpack], x, nd["w"] + " deconv dgrad"):
                    gname, gbytes = self._gate_meta(dg, x)
                    self.profile_meta.append(("bwd", self.bwd[-1], gname or self._kname(dg), flops, gbytes + (x.pixels * x.c + y.pixels * y.c) * self.es))
        blk.append(emit)

    # ---- BatchNorm + sum + ReLU ------------------------------------------------------------------
    def _c_fuse(self, nd, blk):
        terms, out, relu = nd["terms"], nd["out"], nd["relu"]
        obuf = self._act_buf(out)
        c = out.c
        fd = FuseDesc()
        fd.nterms, fd.relu = len(terms), int(relu)
        bn_state = []
        for i, (a, bn, l) in enumerate(terms):
            fd.x[i] = self._act_buf(a).data_ptr()
            fd.log2up[i] = l
            if bn is None:
                bn_state.append(None)
                continue
            st = {k: self._alloc(c, dtype=torch.float32) for k in ("scale", "shift", "mean", "invstd")}
            bn_state.append(st)
            fd.scale[i], fd.shift[i] = st["scale"].data_ptr(), st["shift"].data_ptr()
            P = self.params
            if self.training:
                assert a.stats is not None, f"BN {bn} input has no statistics slab"
                # the finalize (batch statistics -> scale / shift / saved mean, invstd / running statistics) travels WITH the
                # elementwise call (lh_fuse_desc.fin): small tensors run both as one launch, the others launch it first
                fin = _lib.BnFinalizeCall(
                    a.stats.data_ptr(), a.stats_rows, a.pixels, c, P[bn + ".weight"].data_ptr(), P[bn + ".bias"].data_ptr(),
                    P[bn + ".running_mean"].data_ptr(), P[bn + ".running_var"].data_ptr(),
                    _ptr(P.get(bn + ".num_batches_tracked")), BN_MOMENTUM, BN_EPS,
                    st["scale"].data_ptr(), st["shift"].data_ptr(), st["mean"].data_ptr(), st["invstd"].data_ptr())
                self.keep.append(fin)
                fd.fin[i] = C.pointer(fin)
            else:
                self.fwd.append(_Call(self.lib.lh_bn_eval_affine, (
                    P[bn + ".weight"].data_ptr(), P[bn + ".bias"].data_ptr(), P[bn + ".running_mean"].data_ptr(),
                    P[bn + ".running_var"].data_ptr(), BN_EPS, c, st["scale"].data_ptr(), st["shift"].data_ptr()), bn + " eval affine"))
        self.keep.append(fd)
        if not self.training and self._fold_eval_bn(terms, bn_state, out, relu):
            return
        # multi-term ReLU nodes (residual tails, HRNet fuse sums) keep the ReLU mask as one bit per element, so the
        # backward pass reads n*h*w*c/8 bytes instead of the stored activation (single-BN-term nodes recompute the
        # mask from x*scale+shift and need neither)
        relu_bits = None
        if relu and self.with_bwd and len(terms) > 1:
            relu_bits = self._alloc(out.pixels * c // (16 // self.es), dtype=torch.uint8)
            fd.relu_mask = relu_bits.data_ptr()
        if relu:
            self._note_gate(out, terms, bn_state, relu_bits)
        self.fwd.append(_Call(self.lib.lh_fuse_fwd, (C.byref(fd), obuf.data_ptr(), out.n, out.h, out.w, c, self.dt), "fuse fwd"))
        if self.training and relu and len(terms) == 1 and terms[0][1] is not None and terms[0][2] == 0 and relu_bits is None:
            # what a max-pool that follows needs to take this node's elementwise pass over (_c_maxpool)
            self._bnrelu_info[id(out)] = dict(raw=terms[0][0], st=bn_state[0], call=self.fwd[-1], fin=fd.fin[0])
        self.profile_meta.append(("fwd", self.fwd[-1], "fuse_fwd(all kernels)", 0.0, (sum(a.pixels for a, _, _ in terms) + out.pixels) * c * self.es))
        if not self.with_bwd:
            return
        self._ws_fuse = max(self._ws_fuse, self.lib.lh_fuse_bwd_workspace_bytes(out.n, out.h, out.w, c))
        def emit():
            bd = FuseBwdDesc()
            bd.dout = self._act_grad(out).data_ptr()
            bd.out = obuf.data_ptr() if relu else None
            bd.relu_mask = relu_bits.data_ptr() if relu_bits is not None else None
            bd.nterms, bd.relu = len(terms), int(relu)
            bd.strips_cap = 256 if self._emit_group > 1 else 0      # nodes of a batch group share their launches
            pre = self._gated.get(id(out))
            if pre is not None:                                     # dout was written by lh_igemm_gated: gated, with its partial sums
                bd.pre_partial, bd.pre_rows = pre[0].data_ptr(), pre[1]
                if len(pre) > 2 and pre[2] is not None:
                    bd.pre_partial2 = pre[2].data_ptr()
            for i, (a, bn, l) in enumerate(terms):
                bd.log2up[i] = l
                if not a.needs_grad:
                    continue
                if (bn is None and l == 0 and len(terms) == 2 and relu_bits is not None and a.c == out.c
                        and self._nwrites.get(id(a), 0) == 0 and self._next_writer_is_conv(a, nd)):
                    # identity shortcut whose gradient dout * mask would be the first write of a.grad, followed by a
                    # convolution's data gradient: that launch adds it from dout itself (lh_igemm addend_mask)
                    self._masked_addend[id(a)] = (self._act_grad(out), relu_bits)
                    continue
                bd.dx[i] = self._act_grad(a).data_ptr()
                bd.accumulate[i] = 0 if self._first_write(a) else 1
                if bn is not None:
                    st = bn_state[i]
                    bd.x[i] = a.buf.data_ptr()
                    bd.scale[i], bd.save_mean[i], bd.save_invstd[i] = st["scale"].data_ptr(), st["mean"].data_ptr(), st["invstd"].data_ptr()
                    bd.shift[i] = st["shift"].data_ptr()
                    bd.dgamma[i] = self.grads[bn + ".weight"].data_ptr()
                    bd.dbeta[i] = self.grads[bn + ".bias"].data_ptr()
            self.keep.append(bd)
            args = [C.byref(bd), out.n, out.h, out.w, c, 0, self.dt]
            call = _Call(self.lib.lh_fuse_bwd, None, "fuse bwd" + (" (reduce pass done by the gated data gradient)" if pre is not None else ""))

            def set_ws(ptr):
                args[5] = ptr
                call.args = tuple(args)
            self._ws_users_fuse.append((set_ws, self._cur_lane))
            self.bwd.append(call)
            # algorithmic bytes of the BN / ReLU backward of this node: the reduce pass reads dout and every BN term's x, the
            # apply pass reads them again and writes one gradient per term that takes one (5 tensor passes per BN)
            n_bn = sum(1 for _, bn, _ in terms if bn is not None)
            n_dx = sum(1 for i in range(len(terms)) if bd.dx[i])
            # (a node whose dout came from a gated data gradient has no reduce pass: that launch's epilogue read x -- charged to it, _gate_meta)
            passes = ((1 if pre is not None else 2) * (1 + n_bn) if n_bn else 1) + n_dx
            self.profile_meta.append(("bwd", self.bwd[-1], "fuse_bwd(all kernels)", 0.0, float(passes) * out.pixels * c * self.es))
            # what SURVEY 8(d)'s traffic model itself charges to the BatchNorm backward: ONE re-read of y per BatchNorm term
            self.bn_bwd_8d_bytes += float(n_bn) * out.pixels * c * self.es
        blk.append(emit)

    def _next_writer_is_conv(self, a, nd):
        """True when, walking backward from fuse node `nd`, the next writer of a.grad is a stride-1-output convolution /
        transposed convolution data gradient over a dense tensor (it can take a masked addend)."""
        uses = self._uses.get(id(a), [])
        idx = [i for i, (_, n) in enumerate(uses) if n is nd]
        if len(idx) != 1 or idx[0] == 0:
            return False
        kind, nxt = uses[idx[0] - 1]
        return kind in ("conv", "deconv") and a.c == a.c_valid

    def _c_maxpool(self, nd, blk):
        x, y = nd["x"], nd["y"]
        if self._fuse_stem_pool(nd):
            return
        xbuf, ybuf = self._act_buf(x), self._act_buf(y)
        idx = self._alloc(y.n, y.h, y.w, y.c, dtype=torch.uint8) if self.with_bwd else None     # window positions: only the backward pass reads them
        bi = self._bnrelu_info.get(id(x)) if self.opt.bn_pool else None
        nchunk = x.c * self.es // 16
        if bi is not None and len(self._uses.get(id(x), [])) == 1 and self.fwd and self.fwd[-1] is bi["call"] and x.c == x.c_valid \
                and nchunk & (nchunk - 1) == 0 and nchunk <= 256:            # (the flat BN-backward kernels: they take the mask from raw)
            # x = relu(BN(raw)) feeds this pool alone (the training stem, pose_resnet.py:153-156): the pool reads RAW, applies the
            # BatchNorm affine + ReLU per tap (rounded as the stored activation would be: bit-identical pooled values and
            # positions) and x -- the largest activation of the network -- is never written: the backward pass works from
            # idx (pool) and recomputes the ReLU mask from raw (lh_fuse_bwd), it never reads x
            self.fwd.pop()
            self.profile_meta = [m for m in self.profile_meta if m[1] is not bi["call"]]
            st = bi["st"]
            if bi["fin"]:                                           # the finalize that travelled with the elementwise call: a launch of its own
                arr = (_lib.BnFinalizeCall * 1)(bi["fin"].contents)
                self.keep.append(arr)
                self.fwd.append(_Call(self.lib.lh_bn_finalize_multi, (arr, 1), "bn finalize"))
            self.fwd.append(_Call(self.lib.lh_bn_relu_maxpool3x3s2_fwd, (bi["raw"].buf.data_ptr(), st["scale"].data_ptr(), st["shift"].data_ptr(),
                                                                          ybuf.data_ptr(), _ptr(idx), x.n, x.h, x.w, x.c, self.dt), "bn + relu + maxpool fwd"))
            self.profile_meta.append(("fwd", self.fwd[-1], "maxpool_fwd_kernel(bn)", 0.0, (x.pixels * x.c + y.pixels * y.c) * self.es))
        else:
            self.fwd.append(_Call(self.lib.lh_maxpool3x3s2_fwd, (xbuf.data_ptr(), ybuf.data_ptr(), _ptr(idx), x.n, x.h, x.w, x.c, self.dt), "maxpool fwd"))
        if not self.with_bwd:
            return

        def emit():
            dy, dx = self._act_grad(y), self._act_grad(x)
            assert self._first_write(x), "maxpool input gradient must be produced by the pool alone"
            gi = self._gate_info.get(id(x)) if (self.opt.bn_gate and self.n_lanes == 1 and self.es == 2 and self.opt.pool_gate) else None
            nch = x.c * self.es // 16
            if gi is not None and gi.get("mask") is None and len(self._uses.get(id(x), [])) == 1 and x.c == x.c_valid and nch & (nch - 1) == 0 and nch <= 256:
                # x = relu(BN(raw)) with the pool as its only reader: the pool's backward stores the ReLU-gated gradient and the
                # BatchNorm-backward partial sums (the node's backward skips its reduce pass), as lh_igemm_gated does for convolutions
                rows = self.lib.lh_maxpool3x3s2_bwd_gated_rows(x.n, x.h, x.w, x.c, self.dt)
                partial = self._alloc(rows * 2 * x.c, dtype=torch.float32)
                gate = self._make_gate(gi, partial)
                self.bwd.append(_Call(self.lib.lh_maxpool3x3s2_bwd_gated, (dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), C.byref(gate), x.n, x.h, x.w, x.c,
                                                                         self.dt), "maxpool bwd + BN-backward gate"))
                self._gated[id(x)] = (partial, rows)
            else:
                self.bwd.append(_Call(self.lib.lh_maxpool3x3s2_bwd, (dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), x.n, x.h, x.w, x.c, self.dt), "maxpool bwd"))
        blk.append(emit)

    def use_uint8_input(self, hs, ws, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), jitter=False, warp=False):
        """Switch the plan's input to raw uint8 HWC images [n][hs][ws][3]: ToTensor + bilinear Resize [+ ColorJitter] +
        Normalize (the reference's CPU transform chain, src/tools/dataset.py:128-159, defaults = its ImageNet
        constants) run fused on the device and write the stem's padded NHWC4 input.  With ``jitter`` the plan owns
        ``jitter_factors`` (fp32 [n][4]: brightness, contrast, saturation, hue) and ``jitter_order`` (int32 [n][4]: op
        ids, negative = skip) that the caller fills per batch (``sample_color_jitter``).  With ``warp`` it also owns
        ``warp_inv`` / ``warp_fwd`` (fp32 [n][6], identity until the caller draws: ``runtime.sample_affine``), read at every
        launch (replay), and the image launch is lh_image_u8_warp_to_nhwc4: a per-image affine warp in front of the resize.
        Returns the static uint8 input buffer."""
        self.img_u8 = self._alloc(self.n, hs, ws, 3, dtype=torch.uint8, zero=True)
        m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        self.keep += [m3, s3]
        if warp:
            eye = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float32, device=self.device)
            self.warp_inv = self._alloc(self.n, 6, dtype=torch.float32)
            self.warp_fwd = self._alloc(self.n, 6, dtype=torch.float32)
            self.warp_inv.copy_(eye.expand(self.n, 6))
            self.warp_fwd.copy_(eye.expand(self.n, 6))
        if jitter:
            self.jitter_factors = self._alloc(self.n, 4, dtype=torch.float32, zero=True)
            self.jitter_factors[:, :3] = 1.0                                    # identity until the caller draws
            self.jitter_order = torch.full((self.n, 4), -1, dtype=torch.int32, device=self.device)
            ws_j = self._alloc(self.lib.lh_image_jitter_workspace_bytes(self.n), dtype=torch.uint8)
            self.keep.append(self.jitter_order)
        # one launch: the plain pipeline, + ColorJitter, or + the affine warp (which takes the jitter operands too, null = none)
        jit = (self.jitter_factors.data_ptr(), self.jitter_order.data_ptr(), ws_j.data_ptr()) if jitter else (None, None, None)
        if warp:
            fn, extra, what = self.lib.lh_image_u8_warp_to_nhwc4, (self.warp_inv.data_ptr(),) + jit, "uint8 input pipeline + affine warp"
        elif jitter:
            fn, extra, what = self.lib.lh_image_u8_jitter_to_nhwc4, jit, "uint8 input pipeline"
        else:
            fn, extra, what = self.lib.lh_image_u8_to_nhwc4, (), "uint8 input pipeline"
        self.fwd[self._image_call_index] = _Call(fn, (
            self.img_u8.data_ptr(), self.img_nhwc4.data_ptr(), self.n, hs, ws, self.h, self.w, self.img_pad, self.img_wp,
            m3, s3) + extra + (self.dt,), what + (" + ColorJitter" if jitter else ""))
        return self.img_u8

    def use_frame_input(self, n_frames, hs, ws, padding=1.25, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), oriented=False,
                        max_taps=1, frame_format="rgb", yuv=("bt709", "limited"), chroma_siting="left", frame_layout=None, perturb=False,
                        jitter=False, surfaces=False):
        """Switch the plan's input to hand boxes on full camera frames (top-down inference; the sibling of ``use_uint8_input``): the
        plan owns ``frames_u8`` (uint8 [n_frames][hs][ws][3], shared by all n slots), ``boxes`` (fp32 [n][4] = x0 y0 x1 y1 in frame
        pixel-index coordinates, the whole frame until the caller writes them) and ``frame_index`` (int32 [n], arange % n_frames),
        all read at every launch (replay), and the image launch becomes two: lh_box_affine writes ``crop_mat`` (fp32 [n][6], crop
        pixel index -> frame pixel index of the box padded by ``padding`` at the crop's aspect ratio) and ``src_frame`` (int32 [n],
        -1 = empty slot), lh_frames_crop_to_nhwc4 samples the frames through them, normalises and writes the stem's padded NHWC4
        input.  run_forward(mirrored=True) still replaces only the launch that writes img_nhwc4.  ``oriented=True``: the plan also
        owns ``rot`` (fp32 [n][2], the frame direction of each crop's +x axis, (1, 0) = upright until the caller writes it) and
        ``mirror`` (int32 [n], 0), and lh_roi_affine writes ``crop_mat`` in lh_box_affine's place.  ``max_taps`` 2..8: the image
        launch is lh_frames_crop_area_to_nhwc4, which averages up to max_taps x max_taps samples over each crop pixel's footprint
        where a ROI is minified (topdown.crop_taps_host); 1: the launches above, unchanged.  ``frame_format="nv12"``: ``frames_u8``
        is a decoder's output, uint8 [n_frames][rows][pitch] in ``frame_layout`` (topdown.nv12_layout's tuple; None: the tight
        layout), and the image launch is lh_frames_crop_yuv_to_nhwc4 for every max_taps: ``yuv`` ((standard, range) or 12
        coefficients: topdown.yuv_matrix) and ``chroma_siting`` ("left" / "center") convert each sample; the zero-filled buffer
        decodes to a defined colour.  "rgb": the plan and its launches as above.  ``perturb=True`` (training on frames with ROI
        augmentation; implies the oriented launch, a turned ROI needs it): the plan also owns ``roi_aug`` (fp32 [n][6] = c, s, k, tx,
        ty, flip per slot, identity rows until the caller writes: ``runtime.sample_roi_aug``) and ``roi_boxes`` / ``roi_rot`` /
        ``roi_mirror``, the perturbed ROI; lh_roi_perturb runs in front of lh_roi_affine, which reads the perturbed ROI, and the
        caller's ``boxes`` / ``rot`` / ``mirror`` are never written.  False: the launch list as above.  ``jitter=True`` (training on
        frames with ColorJitter): the plan also owns ``jitter_factors`` (fp32 [n][4]) and ``jitter_order`` (int32 [n][4], identity
        factors and order -1 until the caller draws: ``runtime.sample_color_jitter``), as ``use_uint8_input(jitter=True)`` does, and
        the image launch is lh_frames_crop_jitter_to_nhwc4 for every ``frame_format`` and ``max_taps``: the grey-mean launch and the
        crop, one entry.  False: launches, buffers and bits as above.  ``frame_format`` "nv21" / "yuv420p" / "p010" (or "nv12" with
        a topdown.Yuv420Layout), and ``surfaces=True`` for every format: the image launch is lh_frames_crop_surfaces_to_nhwc4 (with
        ``jitter`` its two launches), which finds a sample through the plane descriptor ``frame_layout`` (topdown.frame_layout_of's
        rules; kept as ``self.frame_layout``).  Without ``surfaces`` ``frames_u8`` is uint8 [n_frames][frame_bytes]; with it the plan
        owns no frame buffer (``frames_u8`` is None) but ``surface_table`` (int64 [n_frames], zeros: every frame unbound), the device
        addresses of the frames, read by the launch at every replay.  Returns the frame buffer (None with ``surfaces``)."""
        from . import frame_formats, topdown
        if isinstance(max_taps, bool) or not isinstance(max_taps, int) or not 1 <= max_taps <= 8:
            raise ValueError(f"max_taps must be an integer 1..8, not {max_taps!r}")
        frame_formats.check_frame_format(frame_format)
        self.surface_table = self.frame_layout = None
        where = {}                                                # what crop_entry needs to find a sample: desc + source, or nv12
        if topdown.through_descriptor(frame_format, frame_layout, surfaces):
            self.frame_layout = frame_formats.frame_layout_of(frame_format, hs, ws, frame_layout)
            where["desc"] = frame_formats.frames_layout_struct(self.frame_layout, yuv, chroma_siting)
            self.keep.append(where["desc"])
            if surfaces:
                self.frames_u8 = None
                self.surface_table = self._alloc(n_frames, dtype=torch.int64, zero=True)
                where["table"] = self.surface_table.data_ptr()
            else:
                self.frames_u8 = self._alloc(n_frames, self.frame_layout.frame_bytes, dtype=torch.uint8, zero=True)
                where["frame_stride"] = self.frame_layout.frame_bytes
        elif frame_format == "nv12":
            pitch, uv_offset, frame_stride, rows = frame_formats.check_nv12_layout(hs, ws, frame_layout)
            csc, siting = (C.c_float * 12)(*frame_formats.csc12(yuv).tolist()), frame_formats.chroma_siting_code(chroma_siting)
            self.keep.append(csc)
            where["nv12"] = (pitch, uv_offset, frame_stride, siting, csc)
            self.frames_u8 = self._alloc(n_frames, rows, pitch, dtype=torch.uint8, zero=True)
        else:
            self.frames_u8 = self._alloc(n_frames, hs, ws, 3, dtype=torch.uint8, zero=True)
        self.boxes = self._alloc(self.n, 4, dtype=torch.float32)
        self.boxes.copy_(torch.tensor([-0.5, -0.5, ws - 0.5, hs - 0.5], dtype=torch.float32, device=self.device).expand(self.n, 4))
        self.frame_index = self._alloc(self.n, dtype=torch.int32)
        self.frame_index.copy_(torch.arange(self.n, dtype=torch.int32, device=self.device) % n_frames)
        self.crop_mat = self._alloc(self.n, 6, dtype=torch.float32, zero=True)
        self.src_frame = self._alloc(self.n, dtype=torch.int32)
        self.src_frame.fill_(-1)
        m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        self.keep += [m3, s3]
        i = self._image_call_index
        slane = self.fwd[i].slane
        if jitter:
            self.jitter_factors = self._alloc(self.n, 4, dtype=torch.float32, zero=True)
            self.jitter_factors[:, :3] = 1.0                                    # identity until the caller draws
            self.jitter_order = torch.full((self.n, 4), -1, dtype=torch.int32, device=self.device)
            ws_j = self._alloc(self.lib.lh_frames_crop_jitter_workspace_bytes(self.n), dtype=torch.uint8)
            self.keep.append(self.jitter_order)
            where["jit"] = (self.jitter_factors.data_ptr(), self.jitter_order.data_ptr(), ws_j.data_ptr())
        self.fwd[i] = _Call(*topdown.crop_entry(
            self.lib, frame_format, max_taps, None if surfaces else self.frames_u8.data_ptr(), self.img_nhwc4.data_ptr(), self.n, n_frames, hs, ws,
            self.h, self.w, self.img_pad, self.img_wp, m3, s3, self.crop_mat.data_ptr(), self.src_frame.data_ptr(), self.dt, plain=True, **where))
        self.rot = self.mirror = self.roi_aug = self.roi_boxes = self.roi_rot = self.roi_mirror = None
        if oriented or perturb:
            self.rot = self._alloc(self.n, 2, dtype=torch.float32)
            self.rot.copy_(torch.tensor([1.0, 0.0], dtype=torch.float32, device=self.device).expand(self.n, 2))
            self.mirror = self._alloc(self.n, dtype=torch.int32, zero=True)
            roi = (self.boxes, self.rot, self.mirror)
            if perturb:
                self.roi_aug = self._alloc(self.n, 6, dtype=torch.float32)
                self.roi_aug.copy_(torch.tensor(topdown.ROI_AUG_IDENTITY, dtype=torch.float32, device=self.device).expand(self.n, 6))
                self.roi_boxes = self._alloc(self.n, 4, dtype=torch.float32, zero=True)
                self.roi_rot = self._alloc(self.n, 2, dtype=torch.float32, zero=True)
                self.roi_mirror = self._alloc(self.n, dtype=torch.int32, zero=True)
                roi = (self.roi_boxes, self.roi_rot, self.roi_mirror)
            self.fwd.insert(i, _Call(self.lib.lh_roi_affine, (
                roi[0].data_ptr(), roi[1].data_ptr(), roi[2].data_ptr(), self.frame_index.data_ptr(), self.n, n_frames, self.h,
                self.w, float(padding), self.crop_mat.data_ptr(), self.src_frame.data_ptr()), "oriented hand ROI -> crop matrix"))
            if perturb:
                self.fwd.insert(i, _Call(self.lib.lh_roi_perturb, (
                    self.boxes.data_ptr(), self.rot.data_ptr(), self.mirror.data_ptr(), self.roi_aug.data_ptr(), self.n,
                    self.roi_boxes.data_ptr(), self.roi_rot.data_ptr(), self.roi_mirror.data_ptr()), "hand ROI augmentation"))
                self.fwd[i].slane = slane
                i += 1
        else:
            self.fwd.insert(i, _Call(self.lib.lh_box_affine, (
                self.boxes.data_ptr(), self.frame_index.data_ptr(), self.n, n_frames, self.h, self.w, float(padding),
                self.crop_mat.data_ptr(), self.src_frame.data_ptr()), "hand box -> crop matrix"))
        self.fwd[i].slane = self.fwd[i + 1].slane = slane
        self._image_call_index = i + 1                            # the launch that writes img_nhwc4 (what the flip test's mirror replaces)
        return self.frames_u8
