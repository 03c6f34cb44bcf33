"""The three weight-pack kernels of lighthand_amd/csrc/pack.hip (lh_pack_weight, lh_pack_weights_multi, lh_pack_weights_tiled), driven
through the C ABI without a Plan, and the packs a real training plan registers, BIT FOR BIT against ``pack_image_ref`` (a gather by
plain indexing on the CPU, tests/test_packs_host.py).  A pack is data movement plus one round-to-nearest-even conversion, so every
comparison is one of raw integers; every output image lies between two bands of sentinel bytes that must survive the launch."""
import ctypes as C

import pytest
import torch

from conftest import resnet_cfg
from test_packs_host import pack_image_ref, phase_taps

from lighthand_amd.weight_packs import late_pack_split, pack_chunk_table, pack_tile_table

pytestmark = pytest.mark.gpu

BAND = 256                    # guard bytes on either side of every output
SENT = 0xA5                   # their value: a non-zero bit pattern in every element type
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
INT_OF = {2: torch.int16, 4: torch.int32}


def _lib():
    from lighthand_amd import _lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """``nbytes`` of device memory at ``lead`` bytes past a 256-byte boundary, with at least BAND sentinel bytes before and after."""

    def __init__(self, nbytes, fill="sentinel", lead=0):
        self.nbytes, self.start = nbytes, BAND + lead
        self.buf = torch.full((self.start + nbytes + BAND,), SENT, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        if fill == "zero":
            self.buf[self.start:self.start + nbytes] = 0
        self.ptr = self.buf.data_ptr() + self.start

    def read(self, dtype):
        """(payload as integers of the width of ``dtype``, bands intact?) after the launch."""
        host = self.buf.cpu()
        lo, hi = host[:self.start], host[self.start + self.nbytes:]
        intact = bool((lo == SENT).all()) and bool((hi == SENT).all()) and hi.numel() == BAND
        return host[self.start:self.start + self.nbytes].view(INT_OF[_es(dtype)]), intact


def _es(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _ints(t):
    """A CPU tensor of a 2- or 4-byte type as raw integers."""
    return t.contiguous().view(INT_OF[t.element_size()])


def _sentinel_int(dtype):
    return int(torch.full((4,), SENT, dtype=torch.uint8).view(INT_OF[_es(dtype)])[0])


def values(shape, seed):
    """Finite fp32 values with magnitude in [2^-10, 2^4) (no 16-bit type goes subnormal or overflows), random signs.  Sixteen of
    them are made exact halfway cases: low half 0x8000 (between two bf16 values) or low 13 bits 0x1000 (between two fp16 values),
    with the last kept mantissa bit forced to 0 and to 1 in turn, so round-to-nearest-even goes down for some and up for others."""
    g = torch.Generator().manual_seed(seed)
    n = 1
    for s in shape:
        n *= s
    mag = torch.exp2(torch.rand(n, generator=g, dtype=torch.float64) * 13.999 - 10.0).float()
    v = torch.where(torch.rand(n, generator=g) < 0.5, -mag, mag)
    bits = v.view(torch.int32)
    for j in range(16):
        i = (j * 7919 + 3) % n
        b = int(bits[i])
        if j % 2 == 0:
            b = (b & ~0x1FFFF) | 0x8000 | ((j // 2 % 2) << 16)
        else:
            b = (b & ~0x3FFF) | 0x1000 | ((j // 2 % 2) << 13)
        bits[i] = b
    assert bool(torch.isfinite(v).all()) and float(v.abs().min()) >= 2.0 ** -10 and float(v.abs().max()) < 16.0
    return v.view(shape)


def source(shape, dtype, seed):
    """The weights of a case: index-coded for the fp32 run (element i holds i, exact in fp32, so a misplaced element cannot go
    unnoticed), ``values`` for the 16-bit runs."""
    n = 1
    for s in shape:
        n *= s
    if dtype == torch.float32:
        assert n < 1 << 24
        return torch.arange(n, dtype=torch.float32).view(shape)
    return values(shape, seed)


# ------------------------------------------------------------------------------------------------ lh_pack_weights_tiled
ALL = lambda k: list(range(k * k))
PH3 = [[r * 3 + q for r, q in sub] for _, _, sub, _ in phase_taps(3, 1, 2)]      # the stride-2 data-gradient phases of a 3 x 3
PH4 = [[r * 4 + q for r, q in sub] for _, _, sub, _ in phase_taps(4, 1, 2)]      # the four phases of a 4 x 4 / stride-2 deconvolution
assert PH3 == [[4], [3, 5], [1, 7], [0, 2, 6, 8]] and all(len(s) == 4 for s in PH4)

# (d0, d1, kH, kW) -> outputs (row_is_d1, taps)
TILED = {
    (64, 64, 1, 1): [(0, [0])],                                                  # every tile whole, rs = 1
    (80, 72, 3, 3): [(0, ALL(3))] + [(1, s) for s in PH3],                       # five outputs; whole tiles and ragged edges in both dims
    (40, 33, 3, 3): [(0, ALL(3)), (1, ALL(3))],                                  # d1 * rs odd: no tile may take the vector path
    (32, 96, 4, 4): [(1, s) for s in PH4] + [(0, ALL(4))],                       # deconvolution layout, rs = 16
    (21, 256, 1, 1): [(0, [0]), (1, [0])],                                       # fewer rows than one tile
    (32, 32, 5, 5): [(0, [t * 3 % 25 for t in range(16)]), (1, [t * 7 % 25 for t in range(16)])],   # 16 of 25 taps, out of order
}


def tiled_cases(dtype):
    """The cases a dtype can launch: the LDS tile [32][32 * rs + 4] must fit 64 KiB, which holds rs <= 31 for the 16-bit types and
    rs <= 15 for fp32 (the launcher refuses the rest: test_tiled_pack_refuses_a_tile_that_does_not_fit_lds)."""
    return [c for c in TILED if 32 * (32 * c[2] * c[3] + 4) * _es(dtype) <= 64 * 1024]


def out_geometry(case, row_is_d1, taps):
    """(n_out, n_in, strides, taps_rs) of one output of a regular tensor [d0][d1][kH][kW], as weight_packs._pack_regular reads them."""
    d0, d1, kh, kw = case
    rs = kh * kw
    taps_rs = [(t // kw, t % kw) for t in taps]
    if row_is_d1:
        return d1, d0, (rs, d1 * rs, kw, 1), taps_rs
    return d0, d1, (d1 * rs, rs, kw, 1), taps_rs


def run_tiled(cases, dtype, fill, srcs):
    """One lh_pack_weights_tiled launch over ``cases``; returns {(case, output index): (integers, bands intact)}."""
    L, lib = _lib()
    es = _es(dtype)
    kstep = 128 // es
    convs, outs, dev = (L.PackConv * len(cases))(), {}, []
    for ci, case in enumerate(cases):
        d0, d1, kh, kw = case
        w = srcs[case].cuda()
        dev.append(w)
        cv = convs[ci]
        cv.w, cv.d0, cv.d1, cv.rs, cv.npacks = w.data_ptr(), d0, d1, kh * kw, len(TILED[case])
        for oi, (row_is_d1, taps) in enumerate(TILED[case]):
            n_out, n_in, _, _ = out_geometry(case, row_is_d1, taps)
            kpad = -(-n_in // kstep) * kstep
            g = Guarded(-(-n_out // 128) * 128 * len(taps) * kpad * es, fill)
            o = cv.packs[oi]
            o.out, o.row_is_d1, o.ntaps, o.kpad = g.ptr, row_is_d1, len(taps), kpad
            for i, t in enumerate(taps):
                o.taps[i] = t
            outs[(case, oi)] = g
    tiles = pack_tile_table([(c[0], c[1]) for c in cases])
    table = torch.frombuffer(bytearray(bytes(convs)), dtype=torch.uint8).cuda()
    cols = [torch.tensor(list(col), dtype=torch.int32, device="cuda") for col in zip(*tiles)]
    torch.cuda.synchronize()
    rc = lib.lh_pack_weights_tiled(table.data_ptr(), cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), len(tiles),
                                   max(c[2] * c[3] for c in cases), L.dtype_code(dtype), _stream())
    assert rc == 0, lib.lh_last_error()
    torch.cuda.synchronize()
    return {key: g.read(dtype) for key, g in outs.items()}


def check_tiled(cases, dtype, fill, srcs, refs):
    got = run_tiled(cases, dtype, fill, srcs)
    sent = _sentinel_int(dtype)
    for case in cases:
        for oi, (row_is_d1, taps) in enumerate(TILED[case]):
            ints, intact = got[(case, oi)]
            n_out, n_in, _, _ = out_geometry(case, row_is_d1, taps)
            ref = _ints(refs[(case, oi)])
            ints = ints.view(ref.shape)
            what = (case, oi, row_is_d1, fill)
            assert intact, ("guard band written", what)
            if fill == "zero":                      # the whole image: payload placed and rounded, padding still zero
                assert torch.equal(ints, ref), (what, _first_diff(ints, ref))
                continue
            assert torch.equal(ints[:n_out, :, :n_in], ref[:n_out, :, :n_in]), (what, _first_diff(ints[:n_out, :, :n_in], ref[:n_out, :, :n_in]))
            pad = torch.ones(ref.shape, dtype=torch.bool)
            pad[:n_out, :, :n_in] = False
            assert bool(((ints == sent) | (ints == 0))[pad].all()), ("payload spilled into the padding", what)


def _first_diff(a, b):
    bad = (a != b).nonzero()
    return f"{len(bad)} elements differ, first at {bad[0].tolist()}: got {int(a[tuple(bad[0])])}, want {int(b[tuple(bad[0])])}" if len(bad) else ""


_TILED_DATA = {}


def tiled_data(dtype):
    """Sources and reference images of every tiled case of a dtype, computed once and shared (never modified)."""
    if dtype not in _TILED_DATA:
        srcs = {case: source(case, dtype, 100 + i) for i, case in enumerate(TILED)}
        refs = {}
        for case in tiled_cases(dtype):
            for oi, (row_is_d1, taps) in enumerate(TILED[case]):
                n_out, n_in, strides, taps_rs = out_geometry(case, row_is_d1, taps)
                refs[(case, oi)] = pack_image_ref(srcs[case], n_out, n_in, strides, taps_rs, dtype)
        _TILED_DATA[dtype] = (srcs, refs)
    return _TILED_DATA[dtype]


@pytest.mark.parametrize("fill", ["zero", "sentinel"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_tiled_pack_one_launch_holds_every_convolution(dt, fill):
    """All cases of the dtype in ONE launch, so max_rs (and the LDS row stride the launch is sized for) exceeds most members' rs."""
    dtype = DTYPES[dt]
    cases = tiled_cases(dtype)
    assert len(cases) == (4 if dt == "fp32" else 6) and max(c[2] * c[3] for c in cases) > min(c[2] * c[3] for c in cases)
    check_tiled(cases, dtype, fill, *tiled_data(dtype))


@pytest.mark.parametrize("fill", ["zero", "sentinel"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_tiled_pack_each_convolution_alone(dt, fill):
    dtype = DTYPES[dt]
    for case in tiled_cases(dtype):
        check_tiled([case], dtype, fill, *tiled_data(dtype))


def test_tiled_pack_refuses_a_tile_that_does_not_fit_lds():
    """No launch: a tile of 49 taps of a 2-byte type (and the 16 taps of the deconvolution case in fp32, 66 048 bytes) is larger
    than the 64 KiB the launcher sizes its tile within; it returns an error and names the reason."""
    L, lib = _lib()
    dummy = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = dummy.data_ptr()
    for max_rs, code in ((49, L.LH_BF16), (49, L.LH_F16), (16, L.LH_F32)):
        rc = lib.lh_pack_weights_tiled(p, p, p, p, 1, max_rs, code, _stream())
        assert rc < 0 and len(lib.lh_last_error()) > 0 and b"LDS" in lib.lh_last_error()
    assert lib.lh_pack_weights_tiled(p, p, p, p, 1, 50, L.LH_BF16, _stream()) < 0 and len(lib.lh_last_error()) > 0
    torch.cuda.synchronize()
    assert not dummy.any()


# ------------------------------------------------------------------------------------------------ lh_pack_weight(s_multi)
R3 = [(r, q) for r in range(3) for q in range(3)]
# name -> (source shape, n_out, n_in, strides, taps_rs, the tiled form (case, row_is_d1) of a regular tensor or None)
ITEMS = {
    "stem": ((64, 7, 8, 4), 64, 32, (7 * 32, 1, 32, 0), [(r, 0) for r in range(7)], None),      # staged stem image; n_in < kpad for 16 bits
    "oihw": ((96, 48, 3, 3), 96, 48, (48 * 9, 9, 3, 1), R3, ((96, 48, 3, 3), 0)),               # partial K step, rows 96 -> 128
    "dgrad": ((96, 48, 3, 3), 48, 96, (9, 48 * 9, 3, 1), R3, ((96, 48, 3, 3), 1)),              # the same tensor, transposed strides
    "short": ((21, 256, 1, 1), 21, 256, (256, 1, 1, 1), [(0, 0)], ((21, 256, 1, 1), 0)),
}
BIG = ((512, 512, 3, 3), 512, 512, (512 * 9, 9, 3, 1), R3, None)       # more elements (2.4 M) than lh_pack_weight launches threads (1 M)
_ITEM_DATA = {}


def item_data(dtype):
    if dtype not in _ITEM_DATA:
        shapes = {"stem": ITEMS["stem"][0], "oihw": ITEMS["oihw"][0], "short": ITEMS["short"][0]}
        srcs = {k: source(s, dtype, 200 + i) for i, (k, s) in enumerate(shapes.items())}
        srcs["dgrad"] = srcs["oihw"]
        refs = {k: pack_image_ref(srcs[k], *ITEMS[k][1:5], dtype) for k in ITEMS}
        _ITEM_DATA[dtype] = (srcs, refs)
    return _ITEM_DATA[dtype]


def image_bytes(item, dtype):
    _, n_out, n_in, _, taps_rs, _ = item
    es = _es(dtype)
    kstep = 128 // es
    return -(-n_out // 128) * 128 * len(taps_rs) * (-(-n_in // kstep) * kstep) * es


def run_single(item, w_dev, dtype):
    L, lib = _lib()
    _, n_out, n_in, strides, taps_rs, _ = item
    need = C.c_size_t(0)
    arr = (C.c_int * (2 * len(taps_rs)))(*[v for t in taps_rs for v in t])
    code = L.dtype_code(dtype)
    assert lib.lh_pack_weight(None, None, C.byref(need), n_out, n_in, *strides, len(taps_rs), arr, code, None) == 0
    assert need.value == image_bytes(item, dtype)
    g = Guarded(need.value)
    torch.cuda.synchronize()
    assert lib.lh_pack_weight(w_dev.data_ptr(), g.ptr, None, n_out, n_in, *strides, len(taps_rs), arr, code, _stream()) == 0, lib.lh_last_error()
    torch.cuda.synchronize()
    return g.read(dtype)


def run_multi(names, srcs_dev, dtype):
    L, lib = _lib()
    items, outs = (L.PackItem * len(names))(), {}
    for i, name in enumerate(names):
        _, n_out, n_in, strides, taps_rs, _ = ITEMS[name]
        g = outs[name] = Guarded(image_bytes(ITEMS[name], dtype))
        it = items[i]
        it.w, it.out, it.n_out, it.n_in, it.ntaps = srcs_dev[name].data_ptr(), g.ptr, n_out, n_in, len(taps_rs)
        it.so, it.si, it.sr, it.ss = strides
        for j, (r, q) in enumerate(taps_rs):
            it.r[j], it.s[j] = r, q
    chunks = pack_chunk_table([(ITEMS[n][1], ITEMS[n][2], len(ITEMS[n][4])) for n in names], lib.lh_pack_chunk_elems(), 128 // _es(dtype))
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()
    t_item = torch.tensor([c[0] for c in chunks], dtype=torch.int32, device="cuda")
    t_start = torch.tensor([c[1] for c in chunks], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = lib.lh_pack_weights_multi(table.data_ptr(), t_item.data_ptr(), t_start.data_ptr(), len(chunks), L.dtype_code(dtype), _stream())
    assert rc == 0, lib.lh_last_error()
    torch.cuda.synchronize()
    return {n: g.read(dtype) for n, g in outs.items()}


def _dev(srcs):
    dev = {k: v.cuda() for k, v in srcs.items() if k != "dgrad"}
    dev["dgrad"] = dev["oihw"]
    return dev


@pytest.mark.parametrize("dt", list(DTYPES))
def test_multi_pack_writes_whole_images_padding_included(dt):
    """lh_pack_weights_multi into sentinel-filled images: one launch with every item, then each item alone.  The kernel owns the
    padding: the whole image, zeros included, must equal the reference, and nothing outside it may change."""
    dtype = DTYPES[dt]
    srcs, refs = item_data(dtype)
    dev = _dev(srcs)
    for names in [list(ITEMS)] + [[n] for n in ITEMS]:
        got = run_multi(names, dev, dtype)
        for n in names:
            ints, intact = got[n]
            ref = _ints(refs[n]).flatten()
            assert intact, ("guard band written", n, names)
            assert torch.equal(ints, ref), (n, names, _first_diff(ints, ref))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_single_pack_writes_whole_images_and_strides_over_a_large_one(dt):
    """lh_pack_weight, one item per launch, into sentinel-filled images; the 512 x 512 x 3 x 3 tensor has more image elements than
    the launch has threads, so every thread goes round its grid-stride loop more than twice."""
    dtype = DTYPES[dt]
    srcs, refs = item_data(dtype)
    dev = _dev(srcs)
    for n in ITEMS:
        ints, intact = run_single(ITEMS[n], dev[n], dtype)
        ref = _ints(refs[n]).flatten()
        assert intact, ("guard band written", n)
        assert torch.equal(ints, ref), (n, _first_diff(ints, ref))
    big = source(BIG[0], dtype, 300)
    assert image_bytes(BIG, dtype) // _es(dtype) > 4096 * 256
    ints, intact = run_single(BIG, big.cuda(), dtype)
    ref = _ints(pack_image_ref(big, *BIG[1:5], dtype)).flatten()
    assert intact
    assert torch.equal(ints, ref), _first_diff(ints, ref)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_the_three_pack_kernels_write_identical_images(dt):
    """Every item through lh_pack_weight and lh_pack_weights_multi, and the regular tensors through lh_pack_weights_tiled as well
    (into zeroed images: that kernel leaves the padding alone): the same integers from each."""
    dtype = DTYPES[dt]
    L, lib = _lib()
    srcs, _ = item_data(dtype)
    dev = _dev(srcs)
    multi = run_multi(list(ITEMS), dev, dtype)
    for n, item in ITEMS.items():
        single, ok = run_single(item, dev[n], dtype)
        assert ok and multi[n][1]
        assert torch.equal(single, multi[n][0]), (n, _first_diff(single, multi[n][0]))
        if item[5] is None:
            continue
        case, row_is_d1 = item[5]
        d0, d1, kh, kw = case
        es = _es(dtype)
        convs = (L.PackConv * 1)()
        cv = convs[0]
        cv.w, cv.d0, cv.d1, cv.rs, cv.npacks = dev[n].data_ptr(), d0, d1, kh * kw, 1
        g = Guarded(image_bytes(item, dtype), "zero")
        o = cv.packs[0]
        o.out, o.row_is_d1, o.ntaps, o.kpad = g.ptr, row_is_d1, kh * kw, -(-item[2] // (128 // es)) * (128 // es)
        for t in range(kh * kw):
            o.taps[t] = t
        tiles = pack_tile_table([(d0, d1)])
        table = torch.frombuffer(bytearray(bytes(convs)), dtype=torch.uint8).cuda()
        cols = [torch.tensor(list(col), dtype=torch.int32, device="cuda") for col in zip(*tiles)]
        torch.cuda.synchronize()
        rc = lib.lh_pack_weights_tiled(table.data_ptr(), cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), len(tiles), kh * kw,
                                       L.dtype_code(dtype), _stream())
        assert rc == 0, lib.lh_last_error()
        torch.cuda.synchronize()
        tiled, ok = g.read(dtype)
        assert ok
        assert torch.equal(tiled, single), (n, "tiled", _first_diff(tiled, single))


# ------------------------------------------------------------------------------------------------ the packs of a real plan
def _plan_outputs(plan, tensors):
    """Every registered pack of a plan as (what, source tensor, destination tensor, n_out, n_in, strides, taps_rs)."""
    found = []
    for i, it in enumerate(plan._pack_items):
        taps_rs = [(it.r[j], it.s[j]) for j in range(it.ntaps)]
        found.append((f"item {i}", tensors[it.w], tensors[it.out], it.n_out, it.n_in, (it.so, it.si, it.sr, it.ss), taps_rs))
    for i, cv in enumerate(plan._pack_convs.values()):
        src = tensors[cv.w]
        assert src.dim() == 4 and tuple(src.shape[:2]) == (cv.d0, cv.d1) and src.shape[2] * src.shape[3] == cv.rs and src.is_contiguous()
        kw = src.shape[3]
        assert 1 <= cv.npacks <= 5
        for k in range(cv.npacks):
            o = cv.packs[k]
            taps_rs = [(o.taps[j] // kw, o.taps[j] % kw) for j in range(o.ntaps)]
            if o.row_is_d1:
                geo = (cv.d1, cv.d0, (cv.rs, cv.d1 * cv.rs, kw, 1))
            else:
                geo = (cv.d0, cv.d1, (cv.d1 * cv.rs, cv.rs, kw, 1))
            assert o.kpad == -(-geo[1] // 64) * 64
            found.append((f"conv {i} {tuple(src.shape)} output {k}", src, tensors[o.out], *geo, taps_rs))
    return found


def _check_plan_images(plan, outputs):
    torch.cuda.synchronize()
    host = {}
    for what, src, dst, n_out, n_in, strides, taps_rs in outputs:
        if src.data_ptr() not in host:
            host[src.data_ptr()] = src.detach().cpu().contiguous()
        ref = _ints(pack_image_ref(host[src.data_ptr()], n_out, n_in, strides, taps_rs, torch.bfloat16)).flatten()
        assert dst.dtype == torch.uint8 and dst.numel() == max(ref.numel() * 2, 16), what
        got = dst.cpu()[:ref.numel() * 2].view(torch.int16)
        assert torch.equal(got, ref), (what, _first_diff(got, ref))
    return host


def test_a_training_plan_rebuilds_every_registered_pack(monkeypatch):
    """ResNet-18 pose network, bf16 training plan with backward, 1 x 64 x 64: after refresh_packs every image the plan registered
    (the gather launch's items and every output of every tiled convolution) equals the reference of its source tensor, and
    follows the parameters when they change; the tiled launches cover every convolution once; a late group has its markers."""
    from lighthand_amd import _lib as L
    from lighthand_amd.graph import _Marker
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    monkeypatch.setenv("LH_AUTOTUNE", "0")           # static kernel choice: plan construction does not time candidates
    lib = L.load()
    torch.manual_seed(11)
    model = get_pose_net(resnet_cfg(18), True).cuda().set_precision("bf16").train()
    plan = model.plan(1, 64, 64, training=True, backward=True)
    flat = model.arena().flat
    tensors = {}
    for t in plan.keep:
        if isinstance(t, torch.Tensor) and t.numel() > 0:
            tensors.setdefault(t.data_ptr(), t)
    outputs = _plan_outputs(plan, tensors)
    assert len(plan._pack_items) >= 1 and len(plan._pack_convs) >= 20 and len(outputs) > len(plan._pack_convs)
    assert len({o[2].data_ptr() for o in outputs}) == len(outputs)               # one image per registered output
    stream = torch.cuda.current_stream().cuda_stream
    first = None
    for seed in (1, 2):
        flat.copy_(values((flat.numel(),), seed).cuda())
        plan.refresh_packs(stream)
        host = _check_plan_images(plan, outputs)
        if first is None:
            first = host
    assert any(not torch.equal(first[k], host[k]) for k in host)                 # the second round did see new parameters

    # the launches: one gather launch with every item, tiled launches that hold every registered convolution exactly once
    multi = [c for c in plan.packs if getattr(c, "fn", None) is lib.lh_pack_weights_multi]
    tiled = [c for c in plan.packs if getattr(c, "fn", None) is lib.lh_pack_weights_tiled]
    assert len(multi) == 1 and 1 <= len(tiled) <= 2
    tab = tensors[multi[0].args[0]].cpu().numpy().tobytes()
    items = (L.PackItem * (len(tab) // C.sizeof(L.PackItem))).from_buffer_copy(tab)
    assert [(it.w, it.out) for it in items] == [(it.w, it.out) for it in plan._pack_items]
    chunks = pack_chunk_table([(it.n_out, it.n_in, it.ntaps) for it in items], lib.lh_pack_chunk_elems(), 64)
    assert multi[0].args[3] == len(chunks)
    assert tensors[multi[0].args[1]].tolist() == [c[0] for c in chunks] and tensors[multi[0].args[2]].tolist() == [c[1] for c in chunks]
    launched = []
    for c in tiled:
        tab = tensors[c.args[0]].cpu().numpy().tobytes()
        grp = (L.PackConv * (len(tab) // C.sizeof(L.PackConv))).from_buffer_copy(tab)
        launched += [(cv.w, cv.npacks, tuple(cv.packs[k].out for k in range(cv.npacks))) for cv in grp]
        tiles = pack_tile_table([(cv.d0, cv.d1) for cv in grp])
        assert c.args[4] == len(tiles) and c.args[5] == max(cv.rs for cv in grp)
        assert [tensors[c.args[j]].tolist() for j in (1, 2, 3)] == [list(col) for col in zip(*tiles)]
    convs = list(plan._pack_convs.values())
    assert launched == [(cv.w, cv.npacks, tuple(cv.packs[k].out for k in range(cv.npacks))) for cv in convs]
    assert len({w for w, _, _ in launched}) == len(launched)

    kinds = [c.kind for c in plan.fwd if isinstance(c, _Marker)]
    assert kinds.count("packjoin") == 1
    split = late_pack_split([cv.d0 * cv.d1 * cv.rs for cv in convs])
    print(f"{len(plan._pack_items)} gathered + {len(outputs) - len(plan._pack_items)} tiled images of {len(convs)} convolutions in "
          f"{len(tiled)} tiled launch(es); late split {split}; markers {kinds}")
    if split is not None and plan.opt.late_pack:
        assert len(tiled) == 2 and [c.lane for c in tiled] == [0, 1]
        assert kinds.count("packfork2") == 1 and kinds.count("packjoin2") == 1
        assert kinds.index("packjoin") < kinds.index("packfork2") < kinds.index("packjoin2")
    else:
        assert len(tiled) == 1 and "packfork2" not in kinds and "packjoin2" not in kinds
