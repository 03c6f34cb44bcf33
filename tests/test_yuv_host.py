"""CPU: the host side of top-down inference on NV12 frames -- yuv_matrix / nv12_layout / rgb_to_nv12_host and the numpy restatement
frames_crop_nv12_host of lighthand_amd.topdown (the rule of lh_frames_crop_yuv_to_nhwc4: csrc/frames_crop_kernel.h, above crop_sample_nv12) against
the standards' colour bars, the RGB restatement on grey frames and the chroma siting formed by hand; the entry's argument checks and
the refusals of InferStep / InferPipeline without a GPU.  The kernel is checked against frames_crop_nv12_host in tests/test_gpu_yuv_crop.py."""
import ctypes as C

import numpy as np
import pytest

F = np.float32
IDENT = [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]]
PLAIN = dict(mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))


# ------------------------------------------------------------------------------------------------ 1. the matrix
@pytest.mark.parametrize("standard,kr,kb", [("bt601", 0.299, 0.114), ("bt709", 0.2126, 0.0722)])
@pytest.mark.parametrize("rng,ys,cs,o0", [("limited", 255 / 219, 255 / 224, 16.0), ("full", 1.0, 1.0, 0.0)])
def test_yuv_matrix_gives_the_values_of_the_formula(standard, kr, kb, rng, ys, cs, o0):
    from lighthand_amd.topdown import yuv_matrix
    kg = 1 - kr - kb
    want = [ys, 0.0, 2 * (1 - kr) * cs, ys, -2 * (1 - kb) * kb / kg * cs, -2 * (1 - kr) * kr / kg * cs, ys, 2 * (1 - kb) * cs, 0.0, o0, 128.0, 128.0]
    got = yuv_matrix(standard, rng)
    assert got.dtype == np.float32 and got.shape == (12,)
    assert np.array_equal(got, np.asarray(want, np.float64).astype(np.float32))          # fp64, rounded once
    if (standard, rng) == ("bt709", "limited"):
        assert np.array_equal(yuv_matrix(), got)                   # the defaults
        assert np.allclose(got[:9], [1.16438, 0, 1.79274, 1.16438, -0.21325, -0.53291, 1.16438, 2.11240, 0], atol=1e-5)  # the familiar figures


def test_yuv_matrix_and_layout_refuse_anything_else():
    from lighthand_amd.topdown import chroma_siting_code, nv12_layout, yuv_matrix
    for bad in (("bt2020", "limited"), ("bt709", "video"), ("BT709", "full"), (709, "full"), ("bt601", None)):
        with pytest.raises(ValueError, match="yuv_matrix"):
            yuv_matrix(*bad)
    assert (chroma_siting_code("left"), chroma_siting_code("center")) == (0, 1)
    for bad in ("centre", 0, None, "LEFT"):
        with pytest.raises(ValueError, match="chroma_siting"):
            chroma_siting_code(bad)
    assert nv12_layout(150, 210) == (210, 150 * 210, 150 * 210 * 3 // 2, 225)           # tight
    assert nv12_layout(150, 210, pitch=232, luma_rows=156) == (232, 232 * 156, 232 * 231, 231)
    assert nv12_layout(1080, 1920, 2048, 1088) == (2048, 2048 * 1088, 2048 * 1628, 1628)  # a decoder's 1080p surface
    for bad in ((151, 210), (150, 211), (0, 210), (150, 2.0), (150, 210, 209), (150, 210, 210, 149), (True, 210)):
        with pytest.raises(ValueError, match="nv12_layout"):
            nv12_layout(*bad)
    with pytest.raises(ValueError, match="32-bit"):
        nv12_layout(40000, 40000)


# ------------------------------------------------------------------------------------------------ 2. colour bars
def _bars():
    """The eight 0/255 colour bars, 4 x 4 pixels each, side by side: uint8 [1][4][32][3] and the colours [8][3]."""
    colours = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    return np.repeat(np.repeat(colours[None, None], 4, 1), 4, 2), colours


def test_red_encodes_as_the_standards_say():
    from lighthand_amd.topdown import rgb_to_nv12_host
    frames, colours = _bars()
    red = int(np.flatnonzero((colours == [255, 0, 0]).all(1))[0])
    for standard, want in (("bt601", (81, 90, 240)), ("bt709", (63, 102, 240))):
        nv = rgb_to_nv12_host(frames, standard, "limited")
        assert nv.shape == (1, 6, 32) and nv.dtype == np.uint8
        assert (nv[0, :4, 4 * red:4 * red + 4] == want[0]).all()
        assert (nv[0, 4:, 4 * red:4 * red + 4:2] == want[1]).all() and (nv[0, 4:, 4 * red + 1:4 * red + 4:2] == want[2]).all()
    for standard in ("bt601", "bt709"):                             # black and white: the ends of the limited and the full range
        lim, full = rgb_to_nv12_host(frames, standard, "limited"), rgb_to_nv12_host(frames, standard, "full")
        assert (lim[0, :4, :4] == 16).all() and (lim[0, :4, 28:] == 235).all() and (full[0, :4, :4] == 0).all() and (full[0, :4, 28:] == 255).all()
        assert (lim[0, 4:, :4] == 128).all() and (lim[0, 4:, 28:] == 128).all()


@pytest.mark.parametrize("standard", ["bt601", "bt709"])
@pytest.mark.parametrize("rng", ["limited", "full"])
def test_colour_bars_come_back_within_the_rounding_of_three_bytes(standard, rng):
    """Bars -> rgb_to_nv12_host -> frames_crop_nv12_host at the centre of every bar (a 1:4 crop: sample x = 4*ox + 1.5, y = 1.5, where
    luma and both sitings' chroma are constant): within 1.5 of 255 levels, the rounding of the three bytes Y, Cb, Cr (worst over the
    bars in fp64: 1.34 levels, BT.709 full)."""
    from lighthand_amd.topdown import frames_crop_nv12_host, rgb_to_nv12_host
    frames, colours = _bars()
    nv = rgb_to_nv12_host(frames, standard, rng)
    mat = [[4.0, 0.0, 1.5, 0.0, 4.0, 1.5]]
    for siting in ("left", "center"):
        for dtype in (np.float32, np.float64):
            got = frames_crop_nv12_host(nv, (4, 32), mat, [0], (1, 8), (standard, rng), siting, dtype=dtype, **PLAIN)
            assert got.dtype == dtype and got.shape == (1, 3, 1, 8)
            err = np.abs(got[0, :, 0, :].T.astype(np.float64) * 255 - colours)
            print(f"{standard} {rng} {siting} {np.dtype(dtype).name}: worst {err.max():.3f} of 255 levels")
            assert err.max() <= 1.5


# ------------------------------------------------------------------------------------------------ 3. grey anchor
def _grey(seed, n=3, hs=150, ws=210, layout=None):
    """Random luma, CbCr = 128 -> (NV12 frames, the same frames as grey RGB)."""
    from lighthand_amd.topdown import nv12_layout
    pitch, uv_offset, _, rows = layout or nv12_layout(hs, ws)
    luma = np.random.RandomState(seed).randint(0, 256, size=(n, hs, ws)).astype(np.uint8)
    nv = np.zeros((n, rows, pitch), np.uint8)
    nv[:, :hs, :ws] = luma
    nv[:, uv_offset // pitch:, :ws] = 128
    return nv, np.repeat(luma[..., None], 3, 3)


@pytest.mark.parametrize("standard", ["bt601", "bt709"])
@pytest.mark.parametrize("max_taps", [1, 8])
def test_grey_frames_give_the_rgb_restatement_bit_for_bit(standard, max_taps):
    """CbCr = 128 at full range: k * 0 is +-0, Y + 0 is Y, a blend of equal bytes is exact -- frames_crop_host's bits on the grey RGB
    frames, for 24 slots in the recipe of tests/test_gpu_area_crop.py (boxes up to 8x minified and turned, mirrored ROIs, empty slots)."""
    from lighthand_amd.topdown import box_affine_host, crop_taps_host, frames_crop_host, frames_crop_nv12_host, roi_affine_host
    nv, rgb = _grey(5)
    rs = np.random.RandomState(21)
    c = np.stack([rs.uniform(-20, 230, size=12), rs.uniform(-20, 170, size=12)], 1)
    half = np.exp(rs.uniform(np.log(8), np.log(220), size=(12, 2)))
    boxes = np.concatenate([c - half, c + half], 1).astype(np.float32)
    index = rs.randint(0, 3, size=12).astype(np.int32)
    boxes[5, 0], index[7] = np.nan, -1
    mb, sb = box_affine_host(boxes, index, 3, (24, 40), 1.25)
    mr, sr = roi_affine_host(boxes, rs.normal(size=(12, 2)), rs.randint(0, 2, size=12), index, 3, (24, 40), 1.25)
    mat, src = np.concatenate([mb, mr]), np.concatenate([sb, sr])
    assert (src < 0).sum() == 4 and crop_taps_host(mat, 8).max() == 8
    want = frames_crop_host(rgb, mat, src, (24, 40), max_taps=max_taps)
    for siting in ("left", "center"):
        got = frames_crop_nv12_host(nv, (150, 210), mat, src, (24, 40), (standard, "full"), siting, max_taps=max_taps)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    limited = frames_crop_nv12_host(nv, (150, 210), mat, src, (24, 40), (standard, "limited"), max_taps=max_taps)
    assert not np.array_equal(limited, want)                        # the anchor is not vacuous: another matrix, other values


def test_pitched_layout_gives_the_tight_layouts_values():
    """pitch = ws + 22, 6 more luma rows, the gap bytes 0xFF: nothing beside a plane is read."""
    from lighthand_amd.topdown import frames_crop_nv12_host, nv12_layout
    rs = np.random.RandomState(3)
    hs, ws = 20, 26
    tight_l, wide_l = nv12_layout(hs, ws), nv12_layout(hs, ws, ws + 22, hs + 6)
    tight = rs.randint(0, 256, size=(2, tight_l[3], ws)).astype(np.uint8)
    wide = np.full((2, wide_l[3], wide_l[0]), 0xFF, np.uint8)
    wide[:, :hs, :ws], wide[:, hs + 6:, :ws] = tight[:, :hs], tight[:, hs:]
    mat = [[0.8, 0.1, -2.0, -0.1, 0.8, -1.0], [2.6, 0.0, -3.0, 0.0, 2.6, -4.0]]
    for taps in (1, 8):
        a = frames_crop_nv12_host(tight, (hs, ws), mat, [0, 1], (12, 14), max_taps=taps)
        b = frames_crop_nv12_host(wide, (hs, ws), mat, [0, 1], (12, 14), max_taps=taps, layout=wide_l)
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    with pytest.raises(ValueError, match="nv12_layout"):
        frames_crop_nv12_host(wide, (hs, ws), mat, [0, 1], (12, 14), layout=(ws + 22, 5, 7, 9))


# ------------------------------------------------------------------------------------------------ 4. siting
def test_chroma_siting_left_and_center_see_the_chroma_the_rule_says():
    """Constant luma 200 (blue stays inside 0..255), Cb = 16 + 4*cx, Cr = 128, a whole-frame 1:1 crop, BT.601 full: at luma column x "left" samples the chroma
    plane at x/2 (U = 16 + 2x), "center" at (x - 0.5)/2 (U = 16 + 2x - 1), exactly; blue is formed from that U by the rule in fp32
    scalars and compared bit for bit."""
    from lighthand_amd.topdown import frames_crop_nv12_host, yuv_matrix
    hs, ws = 8, 40
    nv = np.zeros((1, hs * 3 // 2, ws), np.uint8)
    nv[0, :hs] = 200
    nv[0, hs:, 0::2] = 16 + 4 * np.arange(ws // 2)
    nv[0, hs:, 1::2] = 128
    csc = yuv_matrix("bt601", "full")
    k, o = csc[:9].reshape(3, 3), csc[9:]
    for siting, shift in (("left", 0), ("center", -1)):
        got = frames_crop_nv12_host(nv, (hs, ws), IDENT, [0], (hs, ws), ("bt601", "full"), siting, **PLAIN)
        for x in range(1, ws - 2):                                  # interior columns: the chroma clamp is not in play
            u = F(16 + 2 * x + shift)
            e0, e1, e2 = F(200) - o[0], u - o[1], F(128) - o[2]
            blue = np.minimum(np.maximum((k[2, 0] * e0 + k[2, 1] * e1) + k[2, 2] * e2, F(0)), F(255)) * (F(1) / F(255))
            assert blue.dtype == np.float32
            assert (got[0, 2, :, x].view(np.int32) == blue.view(np.int32)).all(), (siting, x)
        assert not np.array_equal(got[0, 2, :, 0], got[0, 2, :, 20])


# ------------------------------------------------------------------------------------------------ 5. argument checks
def test_yuv_entry_is_exported_declared_and_validates_arguments_without_gpu():
    import os
    import re
    from conftest import ROOT
    from lighthand_amd import _lib
    from lighthand_amd.topdown import yuv_matrix
    lib = _lib.load()
    name = "lh_frames_crop_yuv_to_nhwc4"
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lighthand_hip.h")).read(), flags=re.S)
    decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
    assert hasattr(lib, name) and name in _lib.SIGNATURES and decl
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES["lh_frames_crop_area_to_nhwc4"][1]) + 5
    assert "int pitch, int uv_offset, long frame_stride, int chroma_siting, const float* csc12" in " ".join(decl.group(1).split())

    fake = C.c_void_p(0x1000)                                      # never dereferenced: validation fails before any launch
    m3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    good = dict(frames=fake, out=fake, b=4, n=2, hs=48, ws=56, pitch=64, uv=64 * 48, stride=64 * 72, siting=0,
                csc=(C.c_float * 12)(*yuv_matrix().tolist()), h=24, w=40, pad=3, wp=48, mean=m3, std=m3, mat=fake, src=fake, max_taps=8,
                dtype=_lib.LH_BF16)

    def crop(**kw):
        a = dict(good, **kw)
        return lib.lh_frames_crop_yuv_to_nhwc4(a["frames"], a["out"], a["b"], a["n"], a["hs"], a["ws"], a["pitch"], a["uv"], a["stride"],
                                               a["siting"], a["csc"], a["h"], a["w"], a["pad"], a["wp"], a["mean"], a["std"], a["mat"],
                                               a["src"], a["max_taps"], a["dtype"], None)

    def bad_csc(i, v):
        c = yuv_matrix().tolist()
        c[i] = v
        return (C.c_float * 12)(*c)
    inf, nan = float("inf"), float("nan")
    cases = [  # (arguments, a word of the error text)
        (dict(hs=47), b"even"), (dict(ws=55), b"even"), (dict(hs=0), b"bad arguments"), (dict(hs=1, ws=56), b"even"),
        (dict(pitch=55), b"pitch"), (dict(pitch=0), b"pitch"),
        (dict(uv=64 * 48 - 1), b"uv_offset"), (dict(uv=0), b"uv_offset"),
        (dict(stride=64 * 48 + 23 * 64 + 55), b"frame_stride"), (dict(stride=0), b"frame_stride"),
        (dict(stride=1 << 31), b"32-bit"), (dict(stride=1 << 40), b"32-bit"),
        (dict(siting=2), b"chroma_siting"), (dict(siting=-1), b"chroma_siting"),
        (dict(csc=bad_csc(0, nan)), b"csc12[0]"), (dict(csc=bad_csc(7, inf)), b"csc12[7]"), (dict(csc=bad_csc(11, -inf)), b"csc12[11]"),
        (dict(csc=None), b"bad arguments"),
        (dict(max_taps=0), b"max_taps"), (dict(max_taps=9), b"max_taps"), (dict(dtype=3), b"dtype"), (dict(out=C.c_void_p(0x1004)), b"aligned"),
        (dict(frames=None), b"bad arguments"), (dict(mat=None), b"bad arguments"), (dict(src=None), b"bad arguments"), (dict(b=0), b"bad arguments"),
        (dict(b=1 << 16), b"bad arguments"), (dict(wp=45), b"bad arguments"), (dict(h=30000, w=30000, wp=30006), b"too large")]
    for kw, word in cases:
        assert crop(**kw) == -1, kw
        err = lib.lh_last_error()
        assert name.encode() in err and word in err, (kw, err)


def test_frame_format_is_refused_without_frames_and_for_unknown_values():
    """Refused with ValueError before the model is looked at (and so before any device work)."""
    from lighthand_amd.runtime import InferPipeline, InferStep
    from lighthand_amd.topdown import nv12_layout
    fr = dict(frames=(2, 96, 128))
    for cls in (InferStep, InferPipeline):
        for kw in (dict(frame_format="nv12"), dict(yuv=("bt601", "full")), dict(chroma_siting="center"), dict(frame_layout=nv12_layout(96, 128, 160))):
            with pytest.raises(ValueError, match="frames="):
                cls(object(), 2, 64, 64, **kw)
            with pytest.raises(ValueError, match="frames"):
                cls(object(), 2, 64, 64, input_u8=(96, 128), **kw)
        for kw in (dict(yuv=("bt601", "full")), dict(chroma_siting="center"), dict(frame_layout=nv12_layout(96, 128, 160))):
            with pytest.raises(ValueError, match="frame_format='nv12'"):     # NV12's options on RGB frames
                cls(object(), 2, 64, 64, **fr, **kw)
        for bad in ("yuv420", "NV12", None, 12):
            with pytest.raises(ValueError, match="frame_format"):
                cls(object(), 2, 64, 64, frame_format=bad, **fr)
        for bad in (("bt2020", "limited"), ("bt709",), "bt709", [1.0] * 11, [float("nan")] * 12):
            with pytest.raises(ValueError, match="yuv"):
                cls(object(), 2, 64, 64, frame_format="nv12", yuv=bad, **fr)
        for bad in ("centre", 1, None):
            with pytest.raises(ValueError, match="chroma_siting"):
                cls(object(), 2, 64, 64, frame_format="nv12", chroma_siting=bad, **fr)
        for bad in ((128, 96 * 128, 96 * 128 * 3 // 2), (100, 9600, 14400, 144), "tight", nv12_layout(98, 128)):
            with pytest.raises(ValueError, match="layout"):
                cls(object(), 2, 64, 64, frame_format="nv12", frame_layout=bad, **fr)
        with pytest.raises(ValueError, match="even"):               # odd frame sides have no 4:2:0 chroma plane
            cls(object(), 2, 64, 64, frame_format="nv12", frames=(2, 97, 128))
    from lighthand_amd.tools import track_frames as T
    parse = T.build_parser().parse_args
    a = parse(["--synthetic", "3"])
    assert (a.frame_format, a.yuv_matrix, a.yuv_range, a.chroma_siting) == ("rgb", "bt709", "limited", "left")
    a = parse(["--synthetic", "3", "--frame_format", "nv12", "--yuv_matrix", "bt601", "--yuv_range", "full", "--chroma_siting", "center"])
    assert (a.frame_format, a.yuv_matrix, a.yuv_range, a.chroma_siting) == ("nv12", "bt601", "full", "center")
    with pytest.raises(SystemExit):
        parse(["--synthetic", "3", "--frame_format", "i420"])
