"""The pixel formats of full frames: what the frame crop (topdown.py, csrc/frames_crop.hip) reads, described without a crop matrix and
without a device.  topdown.py imports every public name here, so ``topdown.yuv_matrix`` and the rest are the same objects.

NV12 frames (lh_frames_crop_yuv_to_nhwc4, InferStep(frames=..., frame_format="nv12")): ``yuv_matrix`` gives the conversion's 12
coefficients (``csc12`` also takes them ready made), ``nv12_layout`` the buffer of a pitched surface (``check_nv12_layout`` checks
one) and ``rgb_to_nv12_host`` is an encoder for the tools and tests.

Decoder surfaces in place and the other 4:2:0 flavours (lh_frames_crop_surfaces_to_nhwc4, InferStep / TrainStep(frames=...,
surfaces=True, frame_format="nv21" | "yuv420p" | "p010")): ``yuv420_layout`` gives the plane descriptor of a format (``Yuv420Layout``),
``frame_layout_of`` the one a step or a launch uses, ``surface_bytes`` what a surface must hold, ``frames_layout_struct`` the C
structure of a descriptor, ``yuv_matrix(..., bits=10)`` the matrix of p010's texels and ``rgb_to_yuv420_host`` an encoder for the
tools and tests."""
import collections

import numpy as np

_range = range          # several functions below take a parameter named ``range`` (the YUV range)

_YUV_K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}          # (Kr, Kb)
_YUV_RANGE = {"limited": (255.0 / 219.0, 255.0 / 224.0, 16.0), "full": (1.0, 1.0, 0.0)}          # (luma scale, chroma scale, luma offset)
_SITING = {"left": 0, "center": 1}


def _yuv_matrix64(standard, range, bits=8):
    if not (isinstance(standard, str) and isinstance(range, str)) or standard not in _YUV_K or range not in _YUV_RANGE:
        raise ValueError(f"yuv_matrix: standard is one of {sorted(_YUV_K)} and range one of {sorted(_YUV_RANGE)}, not {standard!r} / {range!r}")
    if isinstance(bits, bool) or bits not in (8, 10):
        raise ValueError(f"yuv_matrix: bits is 8 or 10, not {bits!r}")
    kr, kb = _YUV_K[standard]
    kg = 1.0 - kr - kb
    ys, cs, o0 = _YUV_RANGE[range]
    k = np.array([[ys, 0.0, 2 * (1 - kr) * cs], [ys, -2 * (1 - kb) * kb / kg * cs, -2 * (1 - kr) * kr / kg * cs], [ys, 2 * (1 - kb) * cs, 0.0]])
    if bits == 10 and range == "full":                                 # 0..1023 on the v/4 scale is 0..255.75
        k = k * (255.0 / 255.75)
    return k, np.array([o0, 128.0, 128.0])


def yuv_matrix(standard="bt709", range="limited", bits=8):
    """float32 [12] = k[3][3] row-major then o[3], lh_frames_crop_yuv_to_nhwc4's csc12: rgb = k (yuv - o) on 8-bit values, for the
    luma coefficients of ``standard`` ("bt601": Kr, Kb = 0.299, 0.114; "bt709": 0.2126, 0.0722; Kg = 1 - Kr - Kb) and ``range``
    ("limited": Y in 16..235, CbCr in 16..240; "full": 0..255).  Computed in fp64 and rounded once.  ``bits=10``: for 10-bit samples on
    the v/4 scale a p010 texel has -- "limited" is the 8-bit matrix unchanged (64..940 is 4 x 16..235), "full" the 8-bit full-range
    matrix times 255/255.75 with offsets (0, 128, 128)."""
    k, o = _yuv_matrix64(standard, range, bits)
    return np.concatenate([k.ravel(), o]).astype(np.float32)


def chroma_siting_code(chroma_siting):
    """"left" (chroma co-sited with the even luma columns: H.264 / HEVC) -> 0, "center" (between them: JPEG / MPEG-1) -> 1."""
    if not isinstance(chroma_siting, str) or chroma_siting not in _SITING:
        raise ValueError(f"chroma_siting is 'left' or 'center', not {chroma_siting!r}")
    return _SITING[chroma_siting]


def csc12(yuv, bits=8):
    """yuv = (standard, range) or 12 numbers -> float32 [12]; ``bits`` is the samples' (10: p010), for the (standard, range) form."""
    if isinstance(yuv, (tuple, list)) and len(yuv) == 2 and all(isinstance(v, str) for v in yuv):
        return yuv_matrix(*yuv, bits=bits)
    if isinstance(yuv, str):
        raise ValueError(f"yuv is (standard, range) or 12 coefficients, not {yuv!r}")
    try:
        csc = np.asarray(yuv, np.float32).reshape(-1)
    except (TypeError, ValueError):
        csc = np.zeros(0, np.float32)
    if csc.shape != (12,) or not np.isfinite(csc).all():
        raise ValueError(f"yuv is (standard, range) or 12 finite coefficients (k[3][3] row-major, then o[3]), not {yuv!r}")
    return csc


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def nv12_layout(hs, ws, pitch=None, luma_rows=None):
    """The NV12 buffer of hs x ws frames -> (pitch, uv_offset, frame_stride, rows): uint8 [n][rows][pitch] per frame, ``luma_rows``
    (>= hs, default hs) rows of luma on a row pitch of ``pitch`` (>= ws, default ws) bytes, then hs/2 rows of interleaved CbCr on the
    same pitch: uv_offset = pitch * luma_rows, rows = luma_rows + hs/2, frame_stride = pitch * rows.  The defaults are the tight layout
    (ws, hs*ws, hs*ws*3/2, hs*3/2); a decoder's surface passes its pitch and its aligned height."""
    pitch = ws if pitch is None else pitch
    luma_rows = hs if luma_rows is None else luma_rows
    if not all(_is_int(v) for v in (hs, ws, pitch, luma_rows)) or hs < 2 or ws < 2 or hs % 2 or ws % 2:
        raise ValueError(f"nv12_layout: NV12 frames have even integer sides >= 2, not {hs!r} x {ws!r} (pitch {pitch!r}, luma_rows {luma_rows!r})")
    if pitch < ws or luma_rows < hs:
        raise ValueError(f"nv12_layout: pitch {pitch} / luma_rows {luma_rows} are below the frame's {ws} / {hs}")
    rows = int(luma_rows) + int(hs) // 2
    if int(pitch) * rows >= 1 << 31:
        raise ValueError(f"nv12_layout: a frame of {rows} rows of {pitch} bytes does not fit 32-bit byte indices")
    return int(pitch), int(pitch) * int(luma_rows), int(pitch) * rows, rows


def check_nv12_layout(hs, ws, layout):
    """layout = None (tight) or nv12_layout's tuple for hs x ws frames -> the tuple."""
    if layout is None:
        return nv12_layout(hs, ws)
    ok = isinstance(layout, (tuple, list)) and len(layout) == 4 and all(_is_int(v) for v in layout)
    if not ok or tuple(layout) != nv12_layout(hs, ws, layout[0], layout[3] - hs // 2):
        raise ValueError(f"frame layout must be topdown.nv12_layout({hs}, {ws}, pitch, luma_rows)'s (pitch, uv_offset, frame_stride, rows), "
                         f"not {layout!r}")
    return tuple(int(v) for v in layout)


def rgb_to_nv12_host(frames_rgb, standard="bt709", range="limited", layout=None):
    """uint8 RGB frames [n][hs][ws][3] (even hs, ws) -> uint8 NV12 [n][rows][pitch] in ``layout`` (nv12_layout's tuple; None: tight),
    what an encoder of ``standard`` / ``range`` followed by a decoder would hand over: yuv = k^-1 rgb + o of yuv_matrix's fp64 matrix,
    Y = rint per pixel, Cb and Cr = rint of the mean over each 2 x 2 block, clipped to 0..255.  The bytes between the planes and beside
    the rows are 0.  For the tools and the tests."""
    frames = np.asarray(frames_rgb)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3:
        raise ValueError(f"rgb_to_nv12_host: frames uint8 [n][hs][ws][3], not {frames.shape} {frames.dtype}")
    n, hs, ws = frames.shape[:3]
    pitch, uv_offset, _, rows = check_nv12_layout(hs, ws, layout)
    k, o = _yuv_matrix64(standard, range)
    yuv = frames.astype(np.float64) @ np.linalg.inv(k).T + o
    out = np.zeros((n, rows, pitch), np.uint8)
    out[:, :hs, :ws] = np.clip(np.rint(yuv[..., 0]), 0, 255).astype(np.uint8)
    chroma = yuv[..., 1:].reshape(n, hs // 2, 2, ws // 2, 2, 2).mean((2, 4))
    out[:, uv_offset // pitch:, :ws] = np.clip(np.rint(chroma), 0, 255).astype(np.uint8).reshape(n, hs // 2, ws)
    return out


# ---- decoder surfaces and the 4:2:0 flavours (lh_frames_crop_surfaces_to_nhwc4): one plane descriptor for nv12 / nv21 / yuv420p / p010
FRAME_FORMATS = ("rgb", "nv12", "nv21", "yuv420p", "p010")          # the decoders' own pixel-format names
_FMT_CODE = {"rgb": 0, "nv12": 1, "nv21": 2, "yuv420p": 3, "p010": 4}          # LH_FRAMES_FMT_* of the header

Yuv420Layout = collections.namedtuple("Yuv420Layout", "code sample_bytes shift pitch c_pitch cb_offset cr_offset c_step frame_bytes hs ws")
Yuv420Layout.__doc__ = """Where the samples of one hs x ws frame are, from its first byte (yuv420_layout builds it): ``code`` the format
(LH_FRAMES_FMT_*), ``sample_bytes`` 1 or 2 (little-endian), ``shift`` the low bits of a sample that are not data (6 for p010: the
texel is (u16 >> 6) * 0.25), luma (x, y) at y*pitch + x*sample_bytes, Cb / Cr of chroma sample (cx, cy) at cb_offset / cr_offset +
cy*c_pitch + cx*c_step, ``frame_bytes`` what one frame occupies."""


def check_frame_format(frame_format):
    if not isinstance(frame_format, str) or frame_format not in FRAME_FORMATS:
        raise ValueError(f"frame_format is one of {', '.join(repr(f) for f in FRAME_FORMATS)}, not {frame_format!r}")
    return frame_format


def _plane_ends(L):
    """(luma end, one chroma plane's extent from its offset) of a Yuv420Layout: the closed forms surface_bytes and the checks share."""
    hc, wc = L.hs // 2, L.ws // 2
    luma = (L.hs - 1) * L.pitch + L.ws * L.sample_bytes
    plane = (hc - 1) * L.c_pitch + (wc if L.code == 3 else (wc - 1) * L.c_step + L.sample_bytes)
    return luma, plane


def check_yuv420_layout(layout, hs=None, ws=None, frame_format=None):
    """A Yuv420Layout (yuv420_layout's, or one edited with ``_replace``: yuv420p with cb_offset and cr_offset swapped is YV12) ->
    the layout, or ValueError: what lh_frames_crop_surfaces_to_nhwc4 refuses, and a layout of another size or format than asked for."""
    L = layout
    if not isinstance(L, Yuv420Layout) or not all(_is_int(v) for v in L) or L.code not in (1, 2, 3, 4):
        raise ValueError(f"frame layout must be topdown.yuv420_layout(...)'s named tuple, not {layout!r}")
    name = FRAME_FORMATS[L.code]
    if frame_format is not None and name != frame_format:
        raise ValueError(f"frame layout is a {name!r} layout, the frames are {frame_format!r}")
    if (hs is not None and L.hs != hs) or (ws is not None and L.ws != ws):
        raise ValueError(f"frame layout describes {L.hs} x {L.ws} frames, not {hs} x {ws}")
    sb = 2 if L.code == 4 else 1
    if L.hs < 2 or L.ws < 2 or L.hs % 2 or L.ws % 2:
        raise ValueError(f"yuv420_layout: 4:2:0 frames have even integer sides >= 2, not {L.hs!r} x {L.ws!r}")
    if L.sample_bytes != sb or L.shift != (6 if sb == 2 else 0) or L.c_step != (1 if L.code == 3 else 2 * sb):
        raise ValueError(f"yuv420_layout: {name} has sample_bytes {sb}, shift {6 if sb == 2 else 0} and c_step {1 if L.code == 3 else 2 * sb}, not "
                         f"{L.sample_bytes} / {L.shift} / {L.c_step}")
    wc = L.ws // 2
    if L.pitch < L.ws * sb or L.c_pitch < (wc if L.code == 3 else wc * 2 * sb):
        raise ValueError(f"yuv420_layout: pitch {L.pitch} / c_pitch {L.c_pitch} are below a row's bytes ({L.ws * sb} luma, "
                         f"{wc if L.code == 3 else wc * 2 * sb} chroma)")
    if sb == 2 and (L.pitch % 2 or L.c_pitch % 2 or L.cb_offset % 2 or L.cr_offset % 2):
        raise ValueError(f"yuv420_layout: p010 samples are 16-bit: pitch {L.pitch}, c_pitch {L.c_pitch} and the offsets must be even")
    delta = {1: 1, 2: -1, 4: 2}.get(L.code)
    if delta is not None and L.cr_offset - L.cb_offset != delta:
        raise ValueError(f"yuv420_layout: {name} has cr_offset - cb_offset = {delta}, not {L.cr_offset - L.cb_offset}")
    luma, plane = _plane_ends(L)
    lo, hi = min(L.cb_offset, L.cr_offset), max(L.cb_offset, L.cr_offset)
    if lo < luma or (L.code == 3 and hi < lo + plane):
        raise ValueError(f"yuv420_layout: the planes overlap (luma ends at byte {luma}, cb_offset {L.cb_offset}, cr_offset {L.cr_offset}, "
                         f"{plane} bytes a chroma plane)")
    if L.frame_bytes < hi + plane or L.frame_bytes >= 1 << 31:
        raise ValueError(f"yuv420_layout: a frame of {L.frame_bytes} bytes does not hold its planes (they end at byte {hi + plane}) or does "
                         f"not fit 32-bit byte indices")
    return L


def yuv420_layout(frame_format, hs, ws, pitch=None, luma_rows=None, chroma_pitch=None):
    """The layout of hs x ws frames of ``frame_format`` ("nv12", "nv21", "yuv420p", "p010") as a Yuv420Layout: ``luma_rows`` (>= hs,
    default hs) rows of luma on a row pitch of ``pitch`` bytes (default: the row's own bytes), then the chroma: hs/2 rows of
    interleaved pairs on ``chroma_pitch`` (default ``pitch``) for nv12 (Cb first), nv21 (Cr first) and p010 (16-bit samples, Cb
    first), or a Cb plane and then a Cr plane of hs/2 rows on ``chroma_pitch`` (default pitch/2, rounded up) for yuv420p.  The defaults
    are the tight layout; a decoder's surface passes its pitch and aligned height.  (YV12 is yuv420p with the two offsets swapped:
    ``layout._replace(cb_offset=layout.cr_offset, cr_offset=layout.cb_offset)``.)"""
    if not isinstance(frame_format, str) or frame_format not in FRAME_FORMATS[1:]:
        raise ValueError(f"yuv420_layout: frame_format is one of {FRAME_FORMATS[1:]}, not {frame_format!r}")
    code = _FMT_CODE[frame_format]
    sb = 2 if code == 4 else 1
    if not all(_is_int(v) for v in (hs, ws)) or hs < 2 or ws < 2 or hs % 2 or ws % 2:
        raise ValueError(f"yuv420_layout: 4:2:0 frames have even integer sides >= 2, not {hs!r} x {ws!r}")
    pitch = ws * sb if pitch is None else pitch
    luma_rows = hs if luma_rows is None else luma_rows
    chroma_pitch = ((pitch + 1) // 2 if code == 3 else pitch) if chroma_pitch is None and _is_int(pitch) else chroma_pitch
    if not all(_is_int(v) for v in (pitch, luma_rows, chroma_pitch)):
        raise ValueError(f"yuv420_layout: pitch, luma_rows and chroma_pitch are integers, not {pitch!r} / {luma_rows!r} / {chroma_pitch!r}")
    hc = hs // 2
    cb = pitch * luma_rows
    if code == 3:
        cr, frame_bytes = cb + chroma_pitch * hc, cb + 2 * chroma_pitch * hc
    else:
        cb, cr = (cb + 1, cb) if code == 2 else (cb, cb + sb)
        frame_bytes = pitch * luma_rows + chroma_pitch * hc
    return check_yuv420_layout(Yuv420Layout(code, sb, 6 if sb == 2 else 0, int(pitch), int(chroma_pitch), int(cb), int(cr),
                                            1 if code == 3 else 2 * sb, int(frame_bytes), int(hs), int(ws)))


def _rgb_layout(hs, ws):
    if hs * ws * 3 >= 1 << 31:
        raise ValueError(f"a packed RGB frame of {hs} x {ws} does not fit 32-bit byte indices")
    return Yuv420Layout(0, 1, 0, ws * 3, 0, 0, 0, 0, hs * ws * 3, int(hs), int(ws))


def frame_layout_of(frame_format, hs, ws, layout=None):
    """The Yuv420Layout a step or a launch uses for hs x ws frames of ``frame_format``: ``layout`` None is the tight one; "nv12" also
    takes nv12_layout's 4-tuple; "rgb" has no layout to pass (packed [hs][ws][3])."""
    check_frame_format(frame_format)
    if frame_format == "rgb":
        if layout is not None:
            raise ValueError(f"frame_layout={layout!r} describes 4:2:0 frames: packed RGB frames have none")
        return _rgb_layout(hs, ws)
    if frame_format == "nv12" and not isinstance(layout, Yuv420Layout):          # nv12_layout's rules and error texts, as they were
        pitch, _, _, rows = check_nv12_layout(hs, ws, layout)
        return yuv420_layout("nv12", hs, ws, pitch, rows - hs // 2)
    if layout is None:
        return yuv420_layout(frame_format, hs, ws)
    return check_yuv420_layout(layout, hs, ws, frame_format)


def surface_bytes(layout):
    """The bytes a surface of ``layout`` (a Yuv420Layout) must hold: the highest byte a sample can touch, plus one."""
    if isinstance(layout, Yuv420Layout) and layout.code == 0:
        return layout.frame_bytes
    L = check_yuv420_layout(layout)
    return max(L.cb_offset, L.cr_offset) + _plane_ends(L)[1]


def frames_layout_struct(L, yuv, chroma_siting):
    """The lh_frames_layout of a Yuv420Layout (``yuv`` and ``chroma_siting`` as frames_crop's)."""
    from . import _lib
    s = _lib.FramesLayout()
    s.format = L.code
    if L.code:
        s.pitch, s.c_pitch, s.cb_offset, s.cr_offset, s.frame_bytes = L.pitch, L.c_pitch, L.cb_offset, L.cr_offset, L.frame_bytes
        s.chroma_siting = chroma_siting_code(chroma_siting)
        s.csc12[:] = csc12(yuv, 10 if L.code == 4 else 8).tolist()
    return s


def rgb_to_yuv420_host(frames_rgb, frame_format="nv12", standard="bt709", range="limited", layout=None):
    """uint8 RGB frames [n][hs][ws][3] (even hs, ws) -> the frames as ``frame_format`` in ``layout``, uint8 [n][frame_bytes] (for
    "nv12" with ``layout`` None or nv12_layout's tuple: rgb_to_nv12_host's array, [n][rows][pitch]): rgb_to_nv12_host's rounding --
    Y = rint per pixel, Cb and Cr = rint of the mean over each 2 x 2 block, clipped -- laid out through the plane descriptor.  "p010"
    rounds to 10 bits (the code value is 4 x the 8-bit scale's through yuv_matrix(..., bits=10)) and stores them shifted left by 6,
    little-endian.  The bytes between the planes and beside the rows are 0.  For the tools and the tests."""
    check_frame_format(frame_format)
    if frame_format == "nv12" and not isinstance(layout, Yuv420Layout):
        return rgb_to_nv12_host(frames_rgb, standard, range, layout)
    frames = np.asarray(frames_rgb)
    if frame_format == "rgb" or frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3:
        raise ValueError(f"rgb_to_yuv420_host: frames uint8 [n][hs][ws][3] to a 4:2:0 format, not {frames.shape} {frames.dtype} to {frame_format!r}")
    n, hs, ws = frames.shape[:3]
    L = frame_layout_of(frame_format, hs, ws, layout)
    bits = 10 if L.code == 4 else 8
    k, o = _yuv_matrix64(standard, range, bits)
    yuv = frames.astype(np.float64) @ np.linalg.inv(k).T + o
    scale, top = (4.0, 1023) if bits == 10 else (1.0, 255)
    luma = np.clip(np.rint(yuv[..., 0] * scale), 0, top).astype(np.int64) << L.shift
    chroma = np.clip(np.rint(yuv[..., 1:].reshape(n, hs // 2, 2, ws // 2, 2, 2).mean((2, 4)) * scale), 0, top).astype(np.int64) << L.shift
    out = np.zeros((n, L.frame_bytes), np.uint8)
    y, x = np.meshgrid(np.arange(hs), np.arange(ws), indexing="ij")
    cy, cx = np.meshgrid(np.arange(hs // 2), np.arange(ws // 2), indexing="ij")
    for byte in _range(L.sample_bytes):                    # little-endian
        out[:, y * L.pitch + x * L.sample_bytes + byte] = (luma >> (8 * byte)) & 255
        out[:, L.cb_offset + cy * L.c_pitch + cx * L.c_step + byte] = (chroma[..., 0] >> (8 * byte)) & 255
        out[:, L.cr_offset + cy * L.c_pitch + cx * L.c_step + byte] = (chroma[..., 1] >> (8 * byte)) & 255
    return out
