"""CPU: decoder surfaces and the 4:2:0 flavours of the frame crop (lh_frames_crop_surfaces_to_nhwc4) -- the plane descriptor
(topdown.yuv420_layout / surface_bytes), the numpy restatement frames_crop_yuv420_host anchored to frames_crop_nv12_host bit for bit,
nv21 / yuv420p / p010 against NV12 on the same samples, true 10-bit data against a closed form, the test encoder, the entry's argument
validation without a device, the constructors' refusals and the kernel table.  The inputs are tests/surfaces_data.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import surfaces_data as D
from conftest import ROOT

F = np.float32
ENTRY = "lh_frames_crop_surfaces_to_nhwc4"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


# ------------------------------------------------------------------------------------------------ 1. layouts
def test_tight_layouts_and_their_closed_forms():
    from lighthand_amd.topdown import nv12_layout, surface_bytes, yuv420_layout
    hs, ws = D.HS, D.WS
    hc, wc = hs // 2, ws // 2
    want = {  # (sample_bytes, shift, pitch, c_pitch, cb_offset, cr_offset, c_step, frame_bytes)
        "nv12": (1, 0, ws, ws, hs * ws, hs * ws + 1, 2, hs * ws * 3 // 2),
        "nv21": (1, 0, ws, ws, hs * ws + 1, hs * ws, 2, hs * ws * 3 // 2),
        "yuv420p": (1, 0, ws, wc, hs * ws, hs * ws + hc * wc, 1, hs * ws * 3 // 2),
        "p010": (2, 6, 2 * ws, 2 * ws, 2 * hs * ws, 2 * hs * ws + 2, 4, hs * ws * 3)}
    for code, fmt in enumerate(D.FORMATS, 1):
        L = yuv420_layout(fmt, hs, ws)
        assert L.code == code and tuple(L)[1:9] == want[fmt] and (L.hs, L.ws) == (hs, ws), fmt
        assert surface_bytes(L) == L.frame_bytes                   # tight: the last sample is the last byte
    assert tuple(yuv420_layout("nv12", hs, ws))[3:9:5] == nv12_layout(hs, ws)[:3:2]          # pitch and frame_stride agree


def test_pitched_layouts_and_surface_bytes():
    from lighthand_amd.topdown import nv12_layout, surface_bytes, yuv420_layout
    hs, ws, hc, wc = D.HS, D.WS, D.HS // 2, D.WS // 2
    Ls = D.layouts()
    L = Ls["nv12"]
    assert (L.pitch, L.cb_offset, L.frame_bytes) == nv12_layout(hs, ws, D.PITCH, D.LUMA_ROWS)[:3] and L.cr_offset == L.cb_offset + 1
    assert surface_bytes(L) == L.cb_offset + (hc - 1) * 64 + ws
    L = Ls["nv21"]
    assert (L.pitch, L.c_pitch, L.cr_offset, L.cb_offset) == (64, 80, 64 * 40, 64 * 40 + 1) and L.frame_bytes == 64 * 40 + 80 * hc
    assert surface_bytes(L) == 64 * 40 + (hc - 1) * 80 + ws
    L = Ls["yuv420p"]
    assert (L.c_pitch, L.cb_offset, L.cr_offset, L.frame_bytes) == (30, 64 * 38, 64 * 38 + 30 * hc, 64 * 38 + 60 * hc)
    assert surface_bytes(L) == L.cr_offset + (hc - 1) * 30 + wc
    yv12 = L._replace(cb_offset=L.cr_offset, cr_offset=L.cb_offset)          # swapped offsets: YV12, the same bytes
    assert surface_bytes(yv12) == surface_bytes(L)
    L = Ls["p010"]
    assert (L.pitch, L.c_pitch, L.cb_offset, L.cr_offset) == (128, 120, 128 * 37, 128 * 37 + 2) and L.frame_bytes == 128 * 37 + 120 * hc
    assert surface_bytes(L) == L.cb_offset + (hc - 1) * 120 + (wc - 1) * 4 + 4
    assert yuv420_layout("yuv420p", hs, ws, 53).c_pitch == 27      # the default chroma pitch: half the luma pitch, rounded up


def test_layouts_that_cannot_be_read_are_refused():
    from lighthand_amd.topdown import check_yuv420_layout, surface_bytes, yuv420_layout
    hs, ws = D.HS, D.WS
    for fmt in D.FORMATS:
        sb = 2 if fmt == "p010" else 1
        for kw in (dict(hs=hs + 1), dict(ws=ws - 1), dict(hs=0), dict(pitch=ws * sb - sb), dict(luma_rows=hs - 1),
                   dict(chroma_pitch=(ws // 2 if fmt == "yuv420p" else ws * sb) - sb), dict(pitch=1 << 20, luma_rows=1 << 11)):
            args = dict(hs=hs, ws=ws)
            args.update(kw)
            with pytest.raises(ValueError, match="yuv420_layout"):
                yuv420_layout(fmt, **args)
    with pytest.raises(ValueError, match="even"):
        yuv420_layout("p010", hs, ws, 2 * ws + 1)                  # an odd p010 pitch
    with pytest.raises(ValueError, match="even"):
        yuv420_layout("p010", hs, ws, 2 * ws + 2, None, 2 * ws + 3)
    for bad in ("i420", "yuv420", "rgb", "NV12", None):
        with pytest.raises(ValueError, match="frame_format"):
            yuv420_layout(bad, hs, ws)
    L = yuv420_layout("yuv420p", hs, ws)
    for edit in (dict(cr_offset=L.cb_offset + 5), dict(cb_offset=hs * ws - 1), dict(cr_offset=L.cb_offset), dict(frame_bytes=L.frame_bytes - 1),
                 dict(c_step=2), dict(sample_bytes=2), dict(code=7)):
        with pytest.raises(ValueError, match="layout"):
            check_yuv420_layout(L._replace(**edit))
    with pytest.raises(ValueError, match="cr_offset"):
        check_yuv420_layout(yuv420_layout("nv12", hs, ws)._replace(cr_offset=hs * ws + 3))
    with pytest.raises(ValueError, match="layout"):
        surface_bytes((ws, hs * ws, hs * ws * 3 // 2, hs * 3 // 2))          # nv12_layout's tuple is no descriptor


# ------------------------------------------------------------------------------------------------ 2. anchored to the NV12 restatement
_NV12 = {}


def nv12_reference(siting, dtype):
    """frames_crop_nv12_host on the shared samples in the pitched NV12 layout: computed once per (siting, dtype), read-only."""
    key = (siting, np.dtype(dtype).name)
    if key not in _NV12:
        from lighthand_amd.topdown import frames_crop_nv12_host, nv12_layout
        luma, chroma = D.samples()
        frames = D.pack(D.layouts()["nv12"], luma, chroma)
        lay = nv12_layout(D.HS, D.WS, D.PITCH, D.LUMA_ROWS)
        want = frames_crop_nv12_host(frames.reshape(D.NF, lay[3], lay[0]), (D.HS, D.WS), D.MAT, D.SRC, (D.H, D.W), chroma_siting=siting,
                                     max_taps=D.MAX_TAPS, layout=lay, dtype=dtype)
        want.setflags(write=False)
        _NV12[key] = want
    return _NV12[key]


def test_the_slots_take_every_path():
    from lighthand_amd.topdown import crop_taps_host
    taps = crop_taps_host(D.MAT, D.MAX_TAPS).tolist()
    assert taps[:5] == [[1, 1], [2, 2], [2, 3], [1, 1], [1, 1]]
    want = nv12_reference("left", np.float32)
    black = ((F(0) - F([0.485, 0.456, 0.406])) * (F(1) / F([0.229, 0.224, 0.225]))).astype(np.float32)
    for s in D.DARK_SLOTS:
        assert (want[s] == black[:, None, None]).all()
    lit = (want != black[None, :, None, None]).any(1)              # (a sample inside the frame may still convert to black: noise)
    assert lit[[0, 1, 4]].mean() > 0.95 and lit[[2, 3]].mean() > 0.5 and 0.3 < lit[5].mean() < 0.7          # the half-outside slot is half black


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("siting", ["left", "center"])
def test_nv12_input_gives_the_nv12_restatement_bit_for_bit(siting, dtype):
    from lighthand_amd.topdown import frames_crop_yuv420_host, nv12_layout
    luma, chroma = D.samples()
    L = D.layouts()["nv12"]
    frames = D.pack(L, luma, chroma)
    want = nv12_reference(siting, dtype)
    for layout in (L, nv12_layout(D.HS, D.WS, D.PITCH, D.LUMA_ROWS)):          # the descriptor, or nv12_layout's tuple
        for source in (frames, list(frames)):                                  # one array, or a list of per-frame byte arrays
            got = frames_crop_yuv420_host(source, (D.HS, D.WS), D.MAT, D.SRC, (D.H, D.W), "nv12", layout, chroma_siting=siting,
                                          max_taps=D.MAX_TAPS, dtype=dtype)
            assert got.dtype == np.dtype(dtype) and np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(nv12_reference("left", dtype), nv12_reference("center", dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("siting", ["left", "center"])
def test_nv12_restatements_reproduce_the_recorded_crops_bit_for_bit(siting, dtype):
    """frames_crop_nv12_host and frames_crop_yuv420_host share one sampler, so the test above compares a function with itself; this one
    holds both to tests/golden/nv12_crop_host.npz, the outputs of frames_crop_nv12_host while it still had a sampler of its own.  The
    recording (inputs included: ``frames``, ``mat``, ``src``; outputs ``{siting}_{fp32|fp64}_taps{1|4}``): layout = nv12_layout(12,
    16, 24, 14), frames = RandomState(11).randint(0, 256, (2, 20, 24)) as uint8, c, s = cos, sin of pi / 6, mat fp32 = (1, 0, 2.25, 0,
    1, 1.5) upright at scale 1, (3, 0, -3.5, 0, 3, -5.5) minified by 3, (c, -s, 9, s, c, -2) turned and partly outside, zeros with
    src = -1 empty; src = (0, 1, 0, -1); frames_crop_nv12_host(frames, (12, 16), mat, src, (8, 8), chroma_siting=siting, max_taps=taps,
    layout=layout, dtype=dtype) with the default yuv, mean and std."""
    from lighthand_amd.topdown import frames_crop_nv12_host, frames_crop_yuv420_host, nv12_layout
    rec = np.load(os.path.join(ROOT, "tests", "golden", "nv12_crop_host.npz"))
    layout = nv12_layout(12, 16, 24, 14)
    frames, mat, src = rec["frames"], rec["mat"], rec["src"]
    assert frames.shape == (2, layout[3], layout[0]) and frames.dtype == np.uint8 and list(src) == [0, 1, 0, -1]
    for taps in (1, 4):
        want = rec[f"{siting}_{'fp32' if dtype is np.float32 else 'fp64'}_taps{taps}"]
        assert want.dtype == np.dtype(dtype) and want.shape == (4, 3, 8, 8)
        nv12 = frames_crop_nv12_host(frames, (12, 16), mat, src, (8, 8), chroma_siting=siting, max_taps=taps, layout=layout, dtype=dtype)
        y420 = frames_crop_yuv420_host(frames, (12, 16), mat, src, (8, 8), "nv12", layout, chroma_siting=siting, max_taps=taps, dtype=dtype)
        assert nv12.dtype == y420.dtype == want.dtype
        assert np.array_equal(_bits(nv12), _bits(want)) and np.array_equal(_bits(y420), _bits(want)), taps
    assert not np.array_equal(rec[f"{siting}_fp32_taps1"][1], rec[f"{siting}_fp32_taps4"][1])          # the minified slot takes the taps


@pytest.mark.parametrize("siting", ["left", "center"])
@pytest.mark.parametrize("fmt,low", [("nv21", None), ("yuv420p", None), ("yv12", None), ("p010", "zero"), ("p010", "random")])
def test_formats_give_the_nv12_bits_on_the_same_samples(fmt, low, siting):
    """The same luma and chroma samples laid out as each format (p010: u16 = v8 << 8, once with the 6 low bits zero and once random)."""
    from lighthand_amd.topdown import frames_crop_yuv420_host
    luma, chroma = D.samples()
    Ls = D.layouts()
    L = Ls["yuv420p"]._replace(cb_offset=Ls["yuv420p"].cr_offset, cr_offset=Ls["yuv420p"].cb_offset) if fmt == "yv12" else Ls[fmt]
    lowbits = np.random.RandomState(8).randint(0, 64, luma.shape) if low == "random" else None
    frames = D.pack(L, luma, chroma, lowbits)
    name = "yuv420p" if fmt == "yv12" else fmt
    for dtype in (np.float32, np.float64):
        got = frames_crop_yuv420_host(list(frames), (D.HS, D.WS), D.MAT, D.SRC, (D.H, D.W), name, L, chroma_siting=siting, max_taps=D.MAX_TAPS,
                                      dtype=dtype)
        assert np.array_equal(_bits(got), _bits(nv12_reference(siting, dtype))), (fmt, low, dtype)
    if fmt == "nv21":                                              # ... and the comparison can fail: nv21 bytes read as nv12 swap Cb and Cr
        wrong = frames_crop_yuv420_host(frames, (D.HS, D.WS), D.MAT, D.SRC, (D.H, D.W), "nv12",
                                        L._replace(code=1, cb_offset=L.cr_offset, cr_offset=L.cb_offset), chroma_siting=siting, max_taps=D.MAX_TAPS)
        assert not np.array_equal(wrong, nv12_reference(siting, np.float32))


def test_an_unbound_surface_is_an_empty_slot():
    from lighthand_amd.topdown import frames_crop_host, frames_crop_yuv420_host, surface_bytes
    luma, chroma = D.samples()
    L = D.layouts()["yuv420p"]
    frames = list(D.pack(L, luma, chroma))
    all_bound = frames_crop_yuv420_host(frames, (D.HS, D.WS), D.MAT, D.SRC, (D.H, D.W), "yuv420p", L, max_taps=D.MAX_TAPS)
    frames[1] = None
    got = frames_crop_yuv420_host(frames, (D.HS, D.WS), D.MAT, D.SRC, (D.H, D.W), "yuv420p", L, max_taps=D.MAX_TAPS)
    unbound = D.SRC == 1
    assert np.array_equal(got[~unbound], all_bound[~unbound]) and np.array_equal(got[unbound], np.broadcast_to(got[7], got[unbound].shape))
    with pytest.raises(ValueError, match="bytes"):
        frames_crop_yuv420_host([frames[0][:surface_bytes(L) - 1]] * 3, (D.HS, D.WS), D.MAT, D.SRC, (D.H, D.W), "yuv420p", L)   # a byte short
    rgb = D.rgb_frames()                                           # packed RGB surfaces follow the RGB rule
    flat = [f.reshape(-1) for f in rgb]
    src = np.where(D.SRC == 3, -1, D.SRC)
    assert np.array_equal(frames_crop_yuv420_host(flat, (D.HS, D.WS), D.MAT, D.SRC, (D.H, D.W), "rgb", max_taps=D.MAX_TAPS),
                          frames_crop_host(rgb, D.MAT, src, (D.H, D.W), D.MAX_TAPS))


# ------------------------------------------------------------------------------------------------ 3. true 10-bit data
def test_ten_bit_grey_frames_follow_the_closed_form():
    """Y10 = 4g + r with r in 0..3, Cb = Cr = 512, full range: the texel is g + r/4 exactly, the chroma terms are 0 and the pixel is
    min(max((k0 * Y + k1 * 0) + k2 * 0, 0), 255) * (1/255), then Normalize -- every operation in the rule's fp32 order."""
    from lighthand_amd.topdown import MEAN, STD, frames_crop_yuv420_host, yuv420_layout, yuv_matrix
    L = yuv420_layout("p010", D.HS, D.WS, 2 * D.WS + 6, D.HS + 1)
    greys = [(17, 1), (200, 3), (255, 3)]                          # the last one is code 1023
    frames = np.zeros((3, L.frame_bytes), np.uint8)
    y, x = np.meshgrid(np.arange(D.HS), np.arange(D.WS), indexing="ij")
    cy, cx = np.meshgrid(np.arange(D.HS // 2), np.arange(D.WS // 2), indexing="ij")
    for f, (g, r) in enumerate(greys):
        for at, code in ((y * L.pitch + 2 * x, 4 * g + r), (L.cb_offset + cy * L.c_pitch + 4 * cx, 512), (L.cr_offset + cy * L.c_pitch + 4 * cx, 512)):
            u16 = (code << 6) | 0x2A                               # low bits that are not data
            frames[f, at], frames[f, at + 1] = u16 & 255, u16 >> 8
    csc = yuv_matrix("bt709", "full", bits=10)
    eight = yuv_matrix("bt709", "full")
    k64 = np.array([[1.0, 0.0, 1.5748], [1.0, -0.1873242729, -0.4681242729], [1.0, 1.8556, 0.0]]) * (255.0 / 255.75)
    assert csc.dtype == np.float32 and np.array_equal(csc[9:], F([0, 128, 128])) and np.allclose(csc[:9].reshape(3, 3), k64, rtol=0, atol=2e-7)
    assert np.array_equal(yuv_matrix("bt601", "limited", bits=10), yuv_matrix("bt601", "limited")) and not np.array_equal(csc, eight)
    mat = np.array([[1, 0, 0.25, 0, 1, 0.5]] * 3, np.float32)       # between the pixels: a blend of equal texels is the texel
    got = frames_crop_yuv420_host(frames, (D.HS, D.WS), mat, [0, 1, 2], (8, 8), "p010", L, yuv=("bt709", "full"))
    assert np.array_equal(got, frames_crop_yuv420_host(list(frames), (D.HS, D.WS), mat, [0, 1, 2], (8, 8), "p010", L, yuv=csc))
    for f, (g, r) in enumerate(greys):
        texel = F(4 * g + r) * F(0.25)
        e0, zero = texel - csc[9], F(128) - csc[10]
        for c in range(3):
            s = np.minimum(np.maximum((csc[3 * c] * e0 + csc[3 * c + 1] * zero) + csc[3 * c + 2] * zero, F(0)), F(255))
            want = (s * (F(1) / F(255)) - F(MEAN[c])) * (F(1) / F(STD[c]))
            assert want.dtype == np.float32 and (_bits(got[f, c, :7, :7]) == _bits(F(want))).all(), (f, c)
    assert got[2, 0, 0, 0] == (F(1) - F(MEAN[0])) * (F(1) / F(STD[0]))          # code 1023 is white


# ------------------------------------------------------------------------------------------------ 4. the encoder
def test_encoder_gives_the_nv12_encoders_bytes_and_round_trips():
    from lighthand_amd.topdown import frames_crop_nv12_host, frames_crop_yuv420_host, nv12_layout, rgb_to_nv12_host, rgb_to_yuv420_host, yuv420_layout
    rgb = D.rgb_frames()
    lay = nv12_layout(D.HS, D.WS, D.PITCH, D.LUMA_ROWS)
    for args in ((), ("bt601", "full")):
        assert np.array_equal(rgb_to_yuv420_host(rgb, "nv12", *args), rgb_to_nv12_host(rgb, *args))
        assert np.array_equal(rgb_to_yuv420_host(rgb, "nv12", *args, layout=lay), rgb_to_nv12_host(rgb, *args, layout=lay))
    tight = rgb_to_nv12_host(rgb)
    ident = np.array([[1, 0, 0, 0, 1, 0]], np.float32)
    want = frames_crop_nv12_host(tight, (D.HS, D.WS), ident, [1], (D.HS, D.WS))
    for fmt in ("nv12", "nv21", "yuv420p"):                        # the same roundings behind another layout
        enc = rgb_to_yuv420_host(rgb, fmt, layout=D.layouts()[fmt])
        assert enc.shape == (D.NF, D.layouts()[fmt].frame_bytes)
        assert np.array_equal(frames_crop_yuv420_host(enc, (D.HS, D.WS), ident, [1], (D.HS, D.WS), fmt, D.layouts()[fmt]), want)
    ten = rgb_to_yuv420_host(rgb, "p010")
    L = yuv420_layout("p010", D.HS, D.WS)
    u16 = ten.reshape(D.NF, -1, 2).astype(np.int32)
    u16 = u16[..., 0] | (u16[..., 1] << 8)
    assert (u16 & 63 == 0).all() and (u16[:, :D.HS * D.WS] >> 6).max() <= 940 and (u16[:, :D.HS * D.WS] >> 6).min() >= 64
    got = frames_crop_yuv420_host(ten, (D.HS, D.WS), ident, [1], (D.HS, D.WS), "p010", L)
    # each of Y, Cb, Cr differs from its 8-bit rounding by at most 0.5 + 0.125 of an 8-bit step, the blends are convex, the largest
    # absolute row sum of the BT.709 limited matrix is 1.1644 + 2.1124 (blue), and the smallest std is 0.224
    assert np.abs(got - want).max() < 0.625 * (1.1644 + 2.1124) / 255 / 0.224
    with pytest.raises(ValueError):
        rgb_to_yuv420_host(rgb, "rgb")
    with pytest.raises(ValueError, match="frame_format"):
        rgb_to_yuv420_host(rgb, "i420")


def test_jitter_restatement_takes_the_new_formats():
    from lighthand_amd.topdown import frames_crop_jitter_host, frames_crop_yuv420_host
    luma, chroma = D.samples()
    L = D.layouts()["yuv420p"]
    frames = D.pack(L, luma, chroma)
    b = len(D.SRC)
    off = dict(factors=np.ones((b, 4), np.float32), order=np.full((b, 4), -1, np.int32))
    kw = dict(max_taps=D.MAX_TAPS, frame_format="yuv420p", frame_size=(D.HS, D.WS), layout=L)
    plain = frames_crop_jitter_host(list(frames), D.MAT, D.SRC, (D.H, D.W), **off, **kw)
    assert np.array_equal(_bits(plain), _bits(frames_crop_yuv420_host(frames, (D.HS, D.WS), D.MAT, D.SRC, (D.H, D.W), "yuv420p", L, max_taps=D.MAX_TAPS)))
    factors = np.tile(F([[1.2, 0.7, 1.4, 0.1]]), (b, 1))
    order = np.tile(np.int32([[2, 0, 3, 1]]), (b, 1))
    jit = frames_crop_jitter_host(frames, D.MAT, D.SRC, (D.H, D.W), factors, order, **kw)
    nv12 = frames_crop_jitter_host(D.pack(D.layouts()["nv12"], luma, chroma), D.MAT, D.SRC, (D.H, D.W), factors, order, max_taps=D.MAX_TAPS,
                                   frame_format="nv12", frame_size=(D.HS, D.WS), layout=D.layouts()["nv12"])
    assert np.array_equal(_bits(jit), _bits(nv12)) and not np.array_equal(jit[:6], plain[:6])


# ------------------------------------------------------------------------------------------------ 5. the C ABI without a device
def test_entry_is_declared_bound_and_validates_without_a_device():
    from lighthand_amd import _lib
    from lighthand_amd.topdown import _frames_layout_struct, yuv420_layout
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lighthand_hip.h")).read(), flags=re.S)
    decl = re.search(r"\b" + ENTRY + r"\s*\(([^)]*)\)", text)
    assert hasattr(lib, ENTRY) and decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES[ENTRY][1]) == 23
    fields = re.search(r"typedef struct lh_frames_layout \{(.*?)\} lh_frames_layout;", text, flags=re.S).group(1)
    names = [n.strip().split("[")[0] for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f for f, _ in _lib.FramesLayout._fields_] and C.sizeof(_lib.FramesLayout) == 7 * 4 + 12 * 4
    assert [_lib.LH_FRAMES_FMT[k] for k in ("rgb", "nv12", "nv21", "yuv420p", "p010")] == [0, 1, 2, 3, 4]
    p = [C.c_void_p(0x1000 * i) for i in range(1, 9)]             # never dereferenced: validation fails before any launch
    m3, s3 = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25)
    hs, ws = 96, 128

    def layout(fmt="nv12", **edit):
        s = _frames_layout_struct(yuv420_layout(fmt, hs, ws), ("bt709", "limited"), "left")
        for k, v in edit.items():
            if k.startswith("csc"):
                s.csc12[int(k[3:])] = v
            else:
                setattr(s, k, v)
        return s

    def crop(frames=p[0], stride=hs * ws * 3, table=None, lay=None, out=p[1], b=4, n=2, hs_=hs, ws_=ws, h=64, w=64, pad=1, wp=66, mat=p[2],
             src=p[3], taps=1, jit=(None, None, None), dtype=0):
        lay = lay or layout()
        return lib.lh_frames_crop_surfaces_to_nhwc4(frames, out, stride, table, C.byref(lay), b, n, hs_, ws_, h, w, pad, wp, m3, s3, mat, src, taps,
                                                    *jit, dtype, None)
    inf, nan = float("inf"), float("nan")
    cases = [  # (arguments, a word of the error text)
        (dict(frames=None), b"no frame source"), (dict(table=p[4]), b"two frame sources"),
        (dict(lay=layout(format=5)), b"unknown format"), (dict(lay=layout(format=-1)), b"unknown format"),
        (dict(lay=layout(cb_offset=hs * ws - 2, cr_offset=hs * ws - 1)), b"inside the luma plane"),
        (dict(lay=layout("yuv420p", cb_offset=100)), b"inside the luma plane"),
        (dict(lay=layout("yuv420p", cr_offset=hs * ws + 7)), b"overlap"),
        (dict(lay=layout("p010", pitch=2 * ws + 1)), b"even"), (dict(lay=layout("p010", c_pitch=2 * ws + 3)), b"even"),
        (dict(lay=layout("p010"), frames=C.c_void_p(0x1001), stride=hs * ws * 3), b"even"),
        (dict(lay=layout("p010"), stride=hs * ws * 3 + 1), b"even"),
        (dict(lay=layout(csc0=nan)), b"csc12[0]"), (dict(lay=layout(csc7=inf)), b"csc12[7]"), (dict(lay=layout(csc11=-inf)), b"csc12[11]"),
        (dict(hs_=95), b"even"), (dict(ws_=127), b"even"), (dict(lay=layout(pitch=ws - 1)), b"pitch"), (dict(lay=layout(c_pitch=ws - 1)), b"c_pitch"),
        (dict(lay=layout(cr_offset=hs * ws + 2)), b"nv12"), (dict(lay=layout("nv21", cb_offset=hs * ws + 3)), b"nv21"),
        (dict(lay=layout(frame_bytes=hs * ws * 3 // 2 - 1)), b"frame_bytes"), (dict(stride=hs * ws * 3 // 2 - 1), b"frame_stride"),
        (dict(lay=layout(chroma_siting=2)), b"chroma_siting"), (dict(lay=layout(format=0), stride=hs * ws * 3 - 1), b"frame_stride"),
        (dict(jit=(p[5], None, p[7])), b"order_dev"), (dict(jit=(p[5], p[6], C.c_void_p(0x7004))), b"8-byte"),
        (dict(frames=None, table=C.c_void_p(0x5004)), b"8-byte"), (dict(taps=0), b"max_taps"), (dict(taps=9), b"max_taps"), (dict(dtype=3), b"dtype"),
        (dict(out=C.c_void_p(0x2004)), b"aligned"), (dict(mat=None), b"bad arguments"), (dict(b=0), b"bad arguments"), (dict(b=1 << 16), b"bad arguments"),
        (dict(wp=65), b"bad arguments"), (dict(h=30000, w=30000, wp=30006), b"too large")]
    for kw, word in cases:
        assert crop(**kw) == -1, kw
        err = lib.lh_last_error()
        assert ENTRY.encode() in err and word in err, (kw, err)
    null = lib.lh_frames_crop_surfaces_to_nhwc4(p[0], p[1], 0, None, None, 4, 2, hs, ws, 64, 64, 1, 66, m3, s3, p[2], p[3], 1, None, None, None, 0, None)
    assert null == -1 and b"bad arguments" in lib.lh_last_error()


@pytest.mark.parametrize("plain", [False, True], ids=["eager", "plan"])
def test_the_choice_of_crop_entry(plain):
    """topdown.crop_entry, the one place that picks among the five C crop entries, over formats x buffer / surfaces x jitter x max_taps:
    the descriptor path first (with or without jitter), then jitter, NV12, the area entry; what is left is lh_frames_crop_to_nhwc4 for
    the plan (``plain``) at max_taps = 1 and the area entry for the eager launch.  The arguments are the entry's but for the stream.
    Nothing is called: the pointers are dummies."""
    from lighthand_amd import _lib
    from lighthand_amd.topdown import FRAME_FORMATS, crop_entry, frame_layout_of, frames_layout_struct, nv12_layout, through_descriptor
    lib = _lib.load()
    hs, ws = 96, 128
    m3, s3, csc = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 12)()
    seen = set()
    taps_at = {"lh_frames_crop_surfaces_to_nhwc4": -5, "lh_frames_crop_jitter_to_nhwc4": -5, "lh_frames_crop_yuv_to_nhwc4": -2,
               "lh_frames_crop_area_to_nhwc4": -2}                 # max_taps from the end: in front of (jitter triple,) dtype
    cases = [(fmt, None, surfaces) for fmt in FRAME_FORMATS for surfaces in (False, True)] + [("nv12", frame_layout_of("nv12", hs, ws), False)]
    for fmt, layout, surfaces in cases:
        for jitter in (False, True):
            for taps in (1, 4):
                where = {}
                if through_descriptor(fmt, layout, surfaces):
                    assert surfaces or fmt in ("nv21", "yuv420p", "p010") or layout is not None
                    where["desc"] = frames_layout_struct(frame_layout_of(fmt, hs, ws, layout), ("bt709", "limited"), "left")
                    where.update(dict(table=0x9000) if surfaces else dict(frame_stride=hs * ws * 3))
                    want = "lh_frames_crop_surfaces_to_nhwc4"
                else:
                    assert fmt in ("rgb", "nv12")
                    if fmt == "nv12":
                        where["nv12"] = nv12_layout(hs, ws)[:3] + (0, csc)
                    want = ("lh_frames_crop_jitter_to_nhwc4" if jitter else "lh_frames_crop_yuv_to_nhwc4" if fmt == "nv12" else
                            "lh_frames_crop_area_to_nhwc4" if taps > 1 or not plain else "lh_frames_crop_to_nhwc4")
                if jitter:
                    where["jit"] = (0x5000, 0x6000, 0x7000)
                fn, args, what = crop_entry(lib, fmt, taps, None if surfaces else 0x1000, 0x2000, 4, 2, hs, ws, 64, 64, 1, 66, m3, s3, 0x3000, 0x4000,
                                            0, plain=plain, **where)
                assert fn.__name__ == want and fn is getattr(lib, want), (fmt, surfaces, jitter, taps, fn.__name__)
                assert len(args) == len(_lib.SIGNATURES[want][1]) - 1, (want, len(args))
                assert args[1] == 0x2000 and args[-1] == 0 and ("ColorJitter" in what) == jitter and ("antialiased" in what) == (taps > 1)
                assert want not in taps_at or args[taps_at[want]] == taps
                assert ("surface table" in what) == surfaces
                seen.add(want)
    assert len(seen) == (5 if plain else 4)


# ------------------------------------------------------------------------------------------------ 6. the constructors' refusals
def test_constructors_refuse_before_any_device_work():
    from lighthand_amd.runtime import InferPipeline, InferStep, TrainStep
    from lighthand_amd.topdown import nv12_layout, yuv420_layout
    fr = dict(frames=(2, 96, 128))
    for cls in (InferStep, InferPipeline, TrainStep):
        with pytest.raises(ValueError, match="surfaces=True"):      # surfaces without frames
            cls(object(), 2, 64, 64, surfaces=True)
        with pytest.raises(ValueError, match="surfaces"):
            cls(object(), 2, 64, 64, surfaces=1, **fr)
        for fmt, lay in (("nv21", yuv420_layout("yuv420p", 96, 128)), ("p010", yuv420_layout("nv12", 96, 128)), ("yuv420p", nv12_layout(96, 128)),
                         ("nv12", yuv420_layout("nv21", 96, 128)), ("yuv420p", yuv420_layout("yuv420p", 96, 130)), ("rgb", yuv420_layout("nv12", 96, 128))):
            with pytest.raises(ValueError, match="layout"):         # a layout of the wrong format or size
                cls(object(), 2, 64, 64, frame_format=fmt, frame_layout=lay, **fr)
        for bad in ("i420", "yuv420", "YUV420P", "p016"):
            with pytest.raises(ValueError, match="frame_format"):
                cls(object(), 2, 64, 64, frame_format=bad, **fr)
        for fmt in ("nv21", "yuv420p", "p010"):
            with pytest.raises(ValueError, match="frames="):        # a format without frames
                cls(object(), 2, 64, 64, frame_format=fmt)
            with pytest.raises(ValueError, match="even"):
                cls(object(), 2, 64, 64, frame_format=fmt, frames=(2, 96, 127))
    from lighthand_amd.tools import track_frames as T
    parse = T.build_parser().parse_args
    a = parse(["--synthetic", "3", "--frame_format", "p010", "--surfaces"])
    assert a.frame_format == "p010" and a.surfaces is True and parse(["--synthetic", "3"]).surfaces is False
    for bad in ("i420", "yuv420"):
        with pytest.raises(SystemExit):
            parse(["--synthetic", "3", "--frame_format", bad])


def test_train_cli_options():
    from lighthand_amd.tools import train as T
    base = ["--synthetic", "8", "--frame_size", "96x128"]
    assert T.frame_options(T.parse_args(base)) == dict(oriented=False)          # the new options off: today's dict
    a = T.parse_args(base + ["--frame_format", "nv21", "--surfaces"])
    assert T.frame_options(a) == dict(oriented=False, frame_format="nv21", yuv=("bt709", "limited"), chroma_siting="left", surfaces=True)
    for bad in (["--surfaces"], ["--synthetic", "8", "--frame_size", "96x127", "--frame_format", "p010"], base + ["--frame_format", "i420"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)
    ds = T.SyntheticFrames(2, (96, 128), 3, nv12=("bt709", "limited"), frame_format="yuv420p")
    assert tuple(ds[0][0].shape) == (96 * 128 * 3 // 2,)


# ------------------------------------------------------------------------------------------------ 7. the kernel table
def test_the_feature_adds_no_kernel_symbol_and_keeps_the_crop_out_of_scratch():
    """The surface table and the plane descriptor live inside frames_crop_kernel: every kernel of the built library is in the table in
    force (tests/golden/kernel_ceilings_roi.json, as committed), and the three instantiations of the crop read [0, 0] scratch bytes
    and spilled VGPRs."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    with open(kr.GOLDEN) as f:
        table = json.load(f)
    crops = ["_Z18frames_crop_kernelIfEv8CropArgs", "_Z18frames_crop_kernelIDF16bEv8CropArgs", "_Z18frames_crop_kernelIDF16_Ev8CropArgs"]
    assert all(table[k] == [0, 0] for k in crops) and not [k for k in table if "surface" in k]
    if not os.path.exists(kr.LIB) or not kr.tools_present():
        pytest.skip("the library is not built, or the tools that read its kernels are missing")
    built = kr.read_resources()
    assert not [k for k in built if k not in table]
    assert all(built[k] == [0, 0] for k in crops)
