"""The device-side weight packs of a plan: the pack images and the launches that rebuild them from the parameter arena once per step (one
gather launch for the irregular ones, the tiled transposing kernel -- an early and a late group in training plans -- for the rest), the
'packjoin' / 'packfork2' / 'packjoin2' markers of the forward list and what a runner does at them.  A mixin of ``engine.Plan`` (split out
of engine.py in round 7).  The reference has no counterpart: its convolutions read the OIHW parameters directly."""
import ctypes as C

import torch

from . import _lib
from ._lib import check
from .graph import _Call, _Marker, _taps_array


def late_pack_split(sizes):
    """Which convolutions (in the order the forward pass first uses them, ``sizes`` = their weight elements) the LATE launch of the tiled
    pack takes: (cut, fork_conv) -- convs[cut:] are packed late, from the first use of convs[fork_conv] on -- or None for one launch.
    The late group is the longest tail that holds at most 0.8 of the elements; it must hold at least half of them and leave 8 layers
    in front of it (R50: stage 4 + the head's transposed convolutions, 75 % of the parameters)."""
    if len(sizes) < 16:
        return None
    total, acc, cut = sum(sizes), 0, len(sizes)
    while cut > 0 and acc + sizes[cut - 1] <= 0.8 * total:
        cut -= 1
        acc += sizes[cut]
    if not (8 <= cut < len(sizes) and acc >= 0.5 * total):
        return None
    return cut, max(1, cut - max(8, int(0.35 * len(sizes))))


def pack_chunk_table(items, chunk, kstep):
    """Work items of lh_pack_weights_multi: (item, start) for every ``chunk`` elements of the padded image
    [n_out pad 128][ntaps][n_in pad kstep] of each (n_out, n_in, ntaps) in ``items``."""
    table = []
    for i, (n_out, n_in, ntaps) in enumerate(items):
        total = (n_out + 127) // 128 * 128 * ntaps * ((n_in + kstep - 1) // kstep * kstep)
        table += [(i, s0) for s0 in range(0, total, chunk)]
    return table


def pack_tile_table(dims):
    """Work items of lh_pack_weights_tiled: (conv, t0, t1) for every 32 x 32 tile of each [d0][d1] weight matrix in ``dims``, row-major."""
    return [(i, a, b) for i, (d0, d1) in enumerate(dims) for a in range((d0 + 31) // 32) for b in range((d1 + 31) // 32)]


class WeightPacks:
    def _pack(self, wt, n_out, n_in, strides, taps_rs, what):
        """Allocate a pack image and register the launch that (re)builds it from ``wt``."""
        nbytes = C.c_size_t(0)
        arr = _taps_array(taps_rs)
        check(self.lib.lh_pack_weight(None, None, C.byref(nbytes), n_out, n_in, *strides, len(taps_rs), arr, self.dt, None), what)
        buf = self._alloc(max(nbytes.value, 16), dtype=torch.uint8, zero=True)     # padding stays zero for ever
        if taps_rs and self._pack_regular(wt, buf, n_out, n_in, strides, taps_rs):
            return buf
        if taps_rs:
            it = _lib.PackItem()
            it.w, it.out, it.n_out, it.n_in, it.ntaps = wt.data_ptr(), buf.data_ptr(), n_out, n_in, len(taps_rs)
            it.so, it.si, it.sr, it.ss = strides
            for i, (r, q) in enumerate(taps_rs):
                it.r[i], it.s[i] = r, q
            self._pack_items.append(it)
            self.keep.append(wt)
        return buf

    def _pack_regular(self, wt, buf, n_out, n_in, strides, taps_rs):
        """Queue a pack of a plain [d0][d1][kH][kW] weight tensor for the LDS-tiled transposing pack kernel.
        Returns False when the tensor / strides are not of that form (the stem's staged image, oversize taps)."""
        if wt.dim() != 4 or not wt.is_contiguous() or len(taps_rs) > 16:
            return False
        d0, d1, r, s = wt.shape
        rs = r * s
        if 32 * (32 * rs + 2) * self.es > 64 * 1024:
            return False
        if tuple(strides) == (d1 * rs, rs, s, 1) and (n_out, n_in) == (d0, d1):
            row_is_d1 = 0
        elif tuple(strides) == (rs, d1 * rs, s, 1) and (n_out, n_in) == (d1, d0):
            row_is_d1 = 1
        else:
            return False
        conv = self._pack_convs.get(id(wt))
        if conv is None:
            conv = _lib.PackConv()
            conv.w, conv.d0, conv.d1, conv.rs, conv.npacks = wt.data_ptr(), d0, d1, rs, 0
            self._pack_convs[id(wt)] = conv
            self.keep.append(wt)
        if conv.npacks >= 5:
            return False
        o = conv.packs[conv.npacks]
        kstep = 128 // self.es
        o.out, o.row_is_d1, o.ntaps, o.kpad = buf.data_ptr(), row_is_d1, len(taps_rs), (n_in + kstep - 1) // kstep * kstep
        for i, (rr, ss) in enumerate(taps_rs):
            o.taps[i] = rr * s + ss
        conv.npacks += 1
        return True

    def _pack_table(self, structs, columns, dtypes):
        """Upload an array of pack structs and the columns of its work-item table; returns the device tensors (kept alive by the plan)."""
        table = torch.frombuffer(bytearray(bytes(structs)), dtype=torch.uint8).to(self.device)
        tabs = [torch.tensor(list(v), dtype=t, device=self.device) for v, t in zip(columns, dtypes)]
        self.keep += [table] + tabs
        return table, tabs

    def _build_pack_launches(self):
        """The launches of self.packs that rebuild every pack image registered by _pack, once the forward list is complete."""
        if self._pack_items:       # every irregular weight pack of the model is rebuilt by ONE launch
            items = self._pack_items
            chunks = pack_chunk_table([(it.n_out, it.n_in, it.ntaps) for it in items], self.lib.lh_pack_chunk_elems(), 128 // self.es)
            table, (t_item, t_start) = self._pack_table((_lib.PackItem * len(items))(*items), zip(*chunks), (torch.int32, torch.int64))
            self.packs.append(_Call(self.lib.lh_pack_weights_multi,
                                    (table.data_ptr(), t_item.data_ptr(), t_start.data_ptr(), len(chunks), self.dt), "weight packs"))
        if not self._pack_convs:
            return
        convs = list(self._pack_convs.values())        # regular conv / deconv weights, in the order the forward pass first uses them
        # Training plans split the launch: the layers the forward pass reaches LATE and that hold most of the bytes
        # (R50: stage 4 + the head's transposed convolutions, 75 % of the parameters) are packed by a second launch that
        # runs under the latency-bound middle of the forward pass instead of beside the HBM-bound stem and stage 1.
        groups = [convs]
        split = late_pack_split([cv.d0 * cv.d1 * cv.rs for cv in convs]) if self.with_bwd and self.opt.late_pack else None
        if split is not None:
            cut, fork_conv = split
            groups = [convs[:cut], convs[cut:]]
            outs = lambda cvs: {cv.packs[k].out for cv in cvs for k in range(cv.npacks)}
            self._late_packs = (outs(convs[cut:]), outs([convs[fork_conv]]))
        for gi, grp in enumerate(groups):
            tiles = pack_tile_table([(cv.d0, cv.d1) for cv in grp])
            table, tabs = self._pack_table((_lib.PackConv * len(grp))(*grp), zip(*tiles), (torch.int32,) * 3)
            call = _Call(self.lib.lh_pack_weights_tiled,
                         (table.data_ptr(), tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), len(tiles),
                          max(cv.rs for cv in grp), self.dt), "weight packs (tiled)" + (", late group" if gi else ""))
            call.lane = gi           # 1 = the late group (refresh_packs(overlap=True) defers it to the 'packfork2' marker)
            self.packs.append(call)

    def _call_packs(self, c):
        """Pack buffers a forward convolution call reads (addresses)."""
        lib = self.lib
        if c.fn is lib.lh_igemm:
            return {c.args[2]}
        if c.fn is lib.lh_igemm_multi:
            return {c.args[0][i].wpack for i in range(c.args[1])}
        if c.fn is lib.lh_igemm_phases or c.fn is lib.lh_igemm_phases_head:
            return {c.args[3][i] for i in range(c.args[1])}
        return set()

    def _place_pack_markers(self):
        """Training plans: mark where the forward list first reads a pack written by the tiled pack launch ('packjoin') and, with a late
        group, where that group starts and where its first reader sits ('packfork2', 'packjoin2'): refresh_packs(overlap=True)."""
        if not (self.with_bwd and any(getattr(c, "fn", None) is self.lib.lh_pack_weights_tiled for c in self.packs)):
            return
        convs = (self.lib.lh_igemm, self.lib.lh_igemm_multi, self.lib.lh_igemm_phases, self.lib.lh_igemm_phases_head)
        for i, c in enumerate(self.fwd):
            if isinstance(c, _Call) and any(c.fn is f for f in convs) and not c.what.endswith("stem fwd"):
                self.fwd.insert(i, _Marker("packjoin"))
                self._packjoin_at = i
                self._pack_stream = torch.cuda.Stream(device=self.device)
                break
        if self._late_packs is not None and self._packjoin_at is not None:
            late, fork_at = self._late_packs
            first = lambda ptrs: next((i for i, c in enumerate(self.fwd) if isinstance(c, _Call) and self._call_packs(c) & ptrs), None)
            j, f = first(late), first(fork_at)
            if j is not None and f is not None and self._packjoin_at < f < j:
                self.fwd.insert(j, _Marker("packjoin2"))
                self.fwd.insert(f, _Marker("packfork2"))
            else:
                self._late_packs = None

    def refresh_packs(self, stream, overlap=False, side_work=None):
        """Rebuild the device-side weight packs from the parameter arena.  overlap=True (the captured training step): the
        one large launch -- the tiled transposing pack of every regular convolution, ~0.12 ms -- runs on a side stream
        under the image transform, the stem and the pool; the forward list waits for it at its 'packjoin' marker, just
        before the first launch that reads a regular pack.  side_work(stream): more work for that side stream that only
        depends on the step's inputs (the target render); returns True when it was run there."""
        side = self._pack_stream
        if not overlap or side is None or self._packjoin_at is None:
            for c in self.packs:
                c(stream)
            return False
        main = torch.cuda.current_stream()
        assert main.cuda_stream == stream
        side.wait_event(main.record_event())
        self._pack_late = None
        for c in self.packs:
            if c.fn is self.lib.lh_pack_weights_tiled:
                if c.lane == 1 and self._late_packs is not None:
                    self._pack_late = c          # launched when the forward list reaches its 'packfork2' marker
                else:
                    c(side.cuda_stream)
            else:
                c(stream)
        if side_work is not None:
            side_work(side.cuda_stream)
        self._pack_event = side.record_event()
        return side_work is not None

    def _pack_marker(self, kind, main, side):
        """What a runner does at marker ``kind`` of the forward list; False when it is no pack marker.  main: the stream the list runs on;
        side: the stream for the late pack group, None in a plan without side streams (it then runs in place: nothing to join)."""
        if kind == "packjoin" and self._pack_event is not None:
            main.wait_event(self._pack_event)
            self._pack_event = None
        elif kind == "packfork2" and self._pack_late is not None:
            if side is None:
                self._pack_late(main.cuda_stream)
            else:                            # the late pack group starts here, on the pack stream, under the launches that follow
                side.wait_event(main.record_event())
                self._pack_late(side.cuda_stream)
                self._pack_event2 = side.record_event()
            self._pack_late = None
        elif kind == "packjoin2" and self._pack_event2 is not None:
            main.wait_event(self._pack_event2)
            self._pack_event2 = None
        return kind in ("packjoin", "packfork2", "packjoin2")
