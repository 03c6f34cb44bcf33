"""The pure-movement kernels a step depends on -- lh_copy_strided_f32, lh_nhwc_to_nchw_f32 / lh_nchw_f32_to_nhwc and
lh_image_to_nhwc4 -- BIT FOR BIT against torch indexing on the CPU.  Each moves data and converts at most once (round to nearest
even), so the expected bytes of the whole destination buffer are known: the buffer a kernel writes into is built on the host as
well, sentinel bands and untouched elements included, and compared as integers in one piece."""
import ctypes as C

import pytest
import torch

from test_gpu_packs import BAND, DTYPES, INT_OF, SENT, _es, _lib, _stream, values

pytestmark = pytest.mark.gpu

NAN_BITS = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01, torch.float32: 0x7FC00001}


def sentinel_buffer(nbytes, lead=0):
    """Host image of a destination: BAND + lead sentinel bytes, ``nbytes`` of sentinel payload, BAND sentinel bytes."""
    return torch.full((BAND + lead + nbytes + BAND,), SENT, dtype=torch.uint8)


def payload(buf, nbytes, dtype, lead=0):
    return buf[BAND + lead:BAND + lead + nbytes].view(dtype)


def same_bytes(dev, want):
    """The device buffer holds the bytes of the host buffer ``want``, compared as integers; names the first difference."""
    got = dev.cpu()
    assert got.dtype == want.dtype == torch.uint8 and got.shape == want.shape
    bad = (got != want).nonzero()
    assert len(bad) == 0, f"{len(bad)} bytes differ, first at {int(bad[0])} (payload starts at {BAND}): {int(got[bad[0]]):#x} != {int(want[bad[0]]):#x}"


# ------------------------------------------------------------------------------------------------ lh_copy_strided_f32
def copy4(dst, src):
    """dst.copy_(src) by lh_copy_strided_f32, with the argument arrays engine.Plan._copy4 builds (leading sizes 1, strides 0)."""
    _, lib = _lib()
    assert dst.dtype == src.dtype == torch.float32 and tuple(dst.shape) == tuple(src.shape) and dst.dim() <= 4
    pad = 4 - dst.dim()
    shape = (C.c_int * 4)(*([1] * pad + list(dst.shape)))
    ds = (C.c_long * 4)(*([0] * pad + list(dst.stride())))
    ss = (C.c_long * 4)(*([0] * pad + list(src.stride())))
    torch.cuda.synchronize()
    assert lib.lh_copy_strided_f32(dst.data_ptr(), src.data_ptr(), shape, ds, ss, _stream()) == 0, lib.lh_last_error()
    torch.cuda.synchronize()


def _copy_case(name):
    """(elements of the destination buffer, view of it the copy writes, source buffer on the host, view of it the copy reads)."""
    if name == "stem staging":           # engine.Plan._c_stem: stage[:, :, :k, :3] <- weight.permute(0, 2, 3, 1), k = 7
        return 64 * 7 * 8 * 4, lambda d: d.view(64, 7, 8, 4)[:, :, :7, :3], values((64, 3, 7, 7), 31), lambda s: s.permute(0, 2, 3, 1)
    if name == "crop":                   # a view with a storage offset and gaps between rows into a contiguous tensor
        return 21 * 10 * 3 * 3, lambda d: d.view(21, 10, 3, 3), values((32, 12, 3, 3), 32), lambda s: s[5:26, 1:11]
    if name == "2-d":                    # two dimensions: padded to four with sizes 1 and strides 0; transposed source, pitched destination
        return 13 * 9, lambda d: d.view(13, 9)[:, :7], values((7, 13), 33), lambda s: s.t()
    if name == "1-d":                    # the bias pad: bias[:cout] of a longer vector
        return 32, lambda d: d[:21], values((21,), 34), lambda s: s
    assert name == "large"               # 327 680 elements > the 262 144 threads the launch is capped at: the stride loop
    return 8 * 16 * 64 * 40, lambda d: d.view(8, 16, 64, 40), values((8, 64, 40, 16), 35), lambda s: s.permute(0, 3, 1, 2)


@pytest.mark.parametrize("name", ["stem staging", "crop", "2-d", "1-d", "large"])
def test_copy_strided_moves_exactly_the_view(name):
    numel, dview, src, sview = _copy_case(name)
    if name == "crop":
        assert sview(src).storage_offset() > 0 and not sview(src).is_contiguous()
    if name == "large":
        assert numel > 1024 * 256
    want = sentinel_buffer(numel * 4)
    dev = want.cuda()
    src_dev = src.cuda()
    dview(payload(want, numel * 4, torch.float32)).copy_(sview(src))
    copy4(dview(payload(dev, numel * 4, torch.float32)), sview(src_dev))
    same_bytes(dev, want)                # the view, the elements of the buffer outside the view (still sentinel) and both bands
    assert torch.equal(src_dev.cpu().view(torch.int32), src.view(torch.int32))


# ------------------------------------------------------------------------------------------------ NHWC <-> NCHW
N, H, W = 2, 7, 9
# (c, c_stride, elements the base pointer is advanced by)
LAYOUTS = [
    (21, 32, 0),          # vector path
    (21, 24, 0),          # vector path, last 16-byte chunk partly valid (16-bit types: 8 channels per chunk)
    (21, 21, 0),          # scalar path: the pixel stride is no multiple of a 16-byte chunk
    (17, 64, 4),          # base pointer advanced by 4 channels: 8 bytes off alignment for the 16-bit types -> scalar path
]


def _layouts(dtype):
    return [l for l in LAYOUTS if not (l[:2] == (21, 24) and dtype == torch.float32)]


@pytest.mark.parametrize("dt", list(DTYPES))
def test_nhwc_to_nchw_reads_valid_channels_only(dt):
    """NHWC (run dtype, pixel stride c_stride) -> NCHW fp32: the padding channels of the source hold NaN bit patterns and none of
    them reaches the output; the conversion to fp32 is exact, so the output is the source, bit for bit."""
    L, lib = _lib()
    dtype = DTYPES[dt]
    es = _es(dtype)
    for c, cs, adv in _layouts(dtype):
        nhwc = values((N * H * W, cs), 40 + c + cs).to(dtype)
        nhwc.view(INT_OF[es])[:, c:] = NAN_BITS[dtype]
        assert bool(torch.isnan(nhwc[:, c:].float()).all()) and bool(torch.isfinite(nhwc[:, :c].float()).all())
        src = sentinel_buffer(nhwc.numel() * es, adv * es)
        payload(src, nhwc.numel() * es, dtype, adv * es).copy_(nhwc.flatten())
        src_dev = src.cuda()
        base = src_dev.data_ptr() + BAND + adv * es
        assert (base % 16 != 0) == (adv * es % 16 != 0)
        nout = N * c * H * W
        want = sentinel_buffer(nout * 4)
        dev = want.cuda()
        payload(want, nout * 4, torch.float32).view(N, c, H, W).copy_(nhwc.view(N, H, W, cs)[..., :c].permute(0, 3, 1, 2).float())
        torch.cuda.synchronize()
        assert lib.lh_nhwc_to_nchw_f32(base, dev.data_ptr() + BAND, N, H, W, c, cs, L.dtype_code(dtype), _stream()) == 0, lib.lh_last_error()
        torch.cuda.synchronize()
        same_bytes(dev, want)
        same_bytes(src_dev, src)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_nchw_to_nhwc_rounds_once_and_zeroes_the_padding_channels(dt):
    """NCHW fp32 -> NHWC (run dtype) into a sentinel-filled destination: channels below c are the source rounded to nearest even
    (halfway cases among the inputs), channels c <= ch < c_stride of every pixel come out zero, nothing else is written."""
    L, lib = _lib()
    dtype = DTYPES[dt]
    es = _es(dtype)
    for c, cs, adv in _layouts(dtype):
        nchw = values((N, c, H, W), 50 + c + cs)
        nbytes = N * H * W * cs * es
        want = sentinel_buffer(nbytes, adv * es)
        dev = want.cuda()
        img = payload(want, nbytes, dtype, adv * es).view(N, H, W, cs)
        img.view(INT_OF[es]).zero_()
        img[..., :c] = nchw.permute(0, 2, 3, 1).to(dtype)
        src_dev = nchw.cuda()
        torch.cuda.synchronize()
        rc = lib.lh_nchw_f32_to_nhwc(src_dev.data_ptr(), dev.data_ptr() + BAND + adv * es, N, H, W, c, cs, L.dtype_code(dtype), _stream())
        assert rc == 0, lib.lh_last_error()
        torch.cuda.synchronize()
        same_bytes(dev, want)


# ------------------------------------------------------------------------------------------------ lh_image_to_nhwc4
@pytest.mark.parametrize("dt", list(DTYPES))
def test_image_to_nhwc4_pads_with_zeros(dt):
    """NCHW fp32 image -> zero-padded NHWC4 in the run dtype, row pitch wider than the padded image: the interior is the converted
    source, the border pixels, the pitch columns and the fourth channel are zero, the bands on either side are intact."""
    L, lib = _lib()
    dtype = DTYPES[dt]
    es = _es(dtype)
    n, h, w, pad = 2, 5, 7, 3
    wp, hp = w + 2 * pad + 3, h + 2 * pad
    x = values((n, 3, h, w), 60)
    nbytes = n * hp * wp * 4 * es
    want = sentinel_buffer(nbytes)
    dev = want.cuda()
    img = payload(want, nbytes, dtype).view(n, hp, wp, 4)
    img.view(INT_OF[es]).zero_()
    img[:, pad:pad + h, pad:pad + w, :3] = x.permute(0, 2, 3, 1).to(dtype)
    x_dev = x.cuda()
    torch.cuda.synchronize()
    assert lib.lh_image_to_nhwc4(x_dev.data_ptr(), dev.data_ptr() + BAND, n, h, w, pad, wp, L.dtype_code(dtype), _stream()) == 0, lib.lh_last_error()
    torch.cuda.synchronize()
    same_bytes(dev, want)
