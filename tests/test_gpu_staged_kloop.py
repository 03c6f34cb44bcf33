"""The K loop of the register-staged fallback kernel (igemm_kernel, igemm_staged_kernel.h), exact, straight through lh_igemm.

The other GPU tests reach that kernel only through the zero-tap phases of the exact deconvolution tests, where no K step runs.  Here the
descriptor carries an irregular tap list -- the five taps of a "plus" -- which lh_tap_grid refuses, so cfg = 0 resolves to the fallback
although every row is 16-byte aligned (asserted with lh_igemm_tile: ring == 0).

Cases: batch 2, stride 1, same-size dense output; 24 -> 40, 40 -> 72 and 24 -> 72 channels (24 and 40 are ragged against the 64-byte K
step: one and two steps in 16 bits, two and three in fp32; 40 and 72 output channels select the 64- and the 128-row tile and fill
neither); 13 x 11 pixels (the 64-pixel tile, ragged last tile) and 160 x 160 (400 tiles of 128 pixels: the 128-pixel tile needs >= 384
workgroups; fp32 keeps 64 pixels beside 128 rows).  Together: the tiles 64 x 64, 64 x 128, 128 x 64 and 128 x 128, three of them in fp32.

Operands are integers (tests/exact_data.py: RANGES).  Five taps x 40 channels of products of at most 32 x 8 stay below 2^16: the fp32
accumulator is exact in any order (asserted on the host), a stored value is ONE rounding of exact_data.tap_conv's result and the
comparison is torch.equal.  Mode "stats" draws from the "exact_small" ranges: a slab row sums the stored values, and their squares, of one
pixel tile; wherever those sums of magnitudes stay below 2^24 (asserted per tile, on the host values) the row is exact, so the fp64 column
totals of the slab EQUAL those of the stored values.  The output stands between the sentinel margins of tests/test_gpu_epilogue_modes.py."""
import ctypes as C

import pytest
import torch

import exact_data as E
from test_gpu_epilogue_modes import MARGIN, SENTINEL

pytestmark = pytest.mark.gpu

PLUS = [(-1, 0), (0, -1), (0, 0), (0, 1), (1, 0)]
CHANNELS = [(24, 40), (40, 72), (24, 72)]
SIZES = {"13x11": (13, 11), "160x160": (160, 160)}
_DT = {"fp32": 0, "bf16": 1, "fp16": 2}
_SMALL = (4, 2)                                     # "exact_small" (exact_data.EPILOGUE_RANGES): a for x, a for w


def _desc(cin, cout, h, w):
    from lighthand_amd import _lib
    d = _lib.IgemmDesc()
    d.n, d.hi, d.wi, d.in_pix_stride, d.k_run = 2, h, w, cin, cin
    d.ho, d.wo, d.sh, d.sw, d.cout = h, w, 1, 1, cout
    d.OH, d.OW, d.osh, d.osw, d.ooh, d.oow, d.out_pix_stride = h, w, 1, 1, 0, 0, cout
    d.ntaps = len(PLUS)
    for t, (dh, dw) in enumerate(PLUS):
        d.dh[t], d.dw[t] = dh, dw
    return d


def _tile(d, precision):
    from lighthand_amd import _lib
    bm, bp, ring = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    _lib.check(_lib.load().lh_igemm_tile(C.byref(d), _DT[precision], C.byref(bm), C.byref(bp), C.byref(ring)), "lh_igemm_tile")
    return bm.value, bp.value, ring.value


def _want_tile(cout, size, precision):
    bm = 128 if cout > 64 else 64
    return bm, 128 if size == "160x160" and not (precision == "fp32" and bm == 128) else 64


def _data(cin, cout, size, precision, small):
    """(x, weight pack) on the device and the exact accumulator [pixels][cout] on the host (every case draws its own: none is used twice)."""
    h, w = SIZES[size]
    td = E.DTYPES[precision]
    ax, aw = _SMALL if small else E.RANGES[precision]
    g = torch.Generator().manual_seed(300 + cin + cout + h)
    x, wt = E.ints((2, h, w, cin), ax, g), E.ints((cout, len(PLUS), cin), aw, g)
    worst = float(E.tap_conv(x.abs(), wt.abs(), PLUS, h, w, torch.float64).max())
    assert worst < E.LIMIT and (precision != "fp16" or worst < E.FP16_MAX), worst
    es = torch.empty(0, dtype=td).element_size()
    pack = torch.zeros((cout + 127) // 128 * 128, len(PLUS), (cin * es + 127) // 128 * (128 // es), dtype=td)
    pack[:cout, :, :cin] = wt
    return x.to(td).cuda(), pack.cuda(), E.tap_conv(x, wt, PLUS, h, w).reshape(-1, cout)


def test_the_cases_run_the_fallback_on_every_tile():
    tiles = {p: set() for p in _DT}
    for cin, cout in CHANNELS:
        for size, (h, w) in SIZES.items():
            for p in _DT:
                bm, bp, ring = _tile(_desc(cin, cout, h, w), p)
                assert ring == 0 and (bm, bp) == _want_tile(cout, size, p), (cin, cout, size, p, bm, bp, ring)
                tiles[p].add((bm, bp))
    assert tiles["bf16"] == tiles["fp16"] == {(64, 64), (64, 128), (128, 64), (128, 128)}
    assert tiles["fp32"] == {(64, 64), (64, 128), (128, 64)}


@pytest.mark.parametrize("mode", ["plain", "stats"])
@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("channels", CHANNELS, ids=[f"{a}-{b}" for a, b in CHANNELS])
def test_staged_kernel_k_loop_is_exact(channels, size, precision, mode):
    from lighthand_amd import _lib
    lib = _lib.load()
    (cin, cout), (h, w), td = channels, SIZES[size], E.DTYPES[precision]
    d = _desc(cin, cout, h, w)
    bm, bp, ring = _tile(d, precision)
    assert ring == 0 and (bm, bp) == _want_tile(cout, size, precision)
    x, pack, acc = _data(cin, cout, size, precision, mode == "stats")
    want = E.expected_16(acc, td)
    M = 2 * h * w
    buf = torch.full((2 * MARGIN + M * cout,), SENTINEL, dtype=td, device="cuda")
    slab = None
    if mode == "stats":
        rows = lib.lh_igemm_stats_rows(C.byref(d), _DT[precision])
        assert rows == (M + bp - 1) // bp
        slab = torch.full((rows, 2, cout), float("nan"), device="cuda")
    rc = lib.lh_igemm(C.byref(d), x.data_ptr(), pack.data_ptr(), buf.data_ptr() + MARGIN * buf.element_size(), None, None, None, None, None,
                      slab.data_ptr() if slab is not None else None, _DT[precision], None)
    _lib.check(rc, f"lh_igemm {channels} {size} {precision} {mode}")
    torch.cuda.synchronize()
    buf = buf.cpu()
    assert bool((buf[:MARGIN].float() == SENTINEL).all()) and bool((buf[-MARGIN:].float() == SENTINEL).all()), "a margin of the output was written"
    got = buf[MARGIN:-MARGIN].view(M, cout)
    if not torch.equal(got, want):
        bad = got != want
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{int(bad.sum())} of {bad.numel()} stored values differ from the exact result, first at {i}: got {float(got[i])}, "
                             f"exact {float(acc[i])}, expected {float(want[i])}; tile {bm}x{bp}")
    if slab is not None:
        slab = slab.cpu()
        assert not bool(torch.isnan(slab).any()), "a statistics row was not written"
        sd = want.double()
        for which, term in ((0, sd), (1, sd * sd)):
            tiles = torch.zeros((M + bp - 1) // bp * bp, cout, dtype=torch.float64)
            tiles[:M] = term.abs()
            worst = float(tiles.view(-1, bp, cout).sum(1).max())
            assert worst < E.LIMIT, (which, worst)                    # every row of the slab is exact in fp32, in any order
            assert torch.equal(slab[:, which].double().sum(0), term.sum(0)), (which, "a statistics column differs from the sums of the stored values")
