"""Top-down inference on full frames: hand box -> crop matrix and keypoints -> next box, eagerly on device tensors (the C-ABI
entries lh_box_affine / lh_keypoints_to_boxes that runtime.InferStep(frames=...) captures into its graph) and restated in numpy.

Coordinates are pixel indices (pixel centres on the integers, an image spans [-0.5, size-0.5]); a box is (x0, y0, x1, y1) in them,
the box that encloses pixels i0..i1 is (i0-0.5, i1+0.5).  The matrix of a box takes a CROP pixel index to a FRAME pixel index: the
crop kernel (lh_frames_crop_to_nhwc4) samples through it and lh_affine_points takes the decoded keypoints back to the frame through
it.  The ``*_host`` functions follow the kernels operation by operation in fp32 (the library is built with -ffp-contract=off): the CPU
tests check the geometry on them, the GPU tests check the kernels against them.

Oriented, mirrored ROIs and the One-Euro filter (lh_roi_affine / lh_keypoints_to_rois / lh_one_euro, InferStep(oriented=True, smooth=...))
follow the same pattern: ``roi_affine`` / ``rois_from_keypoints`` / ``one_euro`` on device tensors, ``*_host`` in numpy, ``one_euro_host64``
the filter's recurrence in fp64.  An orientation is a direction vector -- the frame direction of the crop's +x axis, (1, 0) = upright --
never an angle: the kernels use + - * /, sqrt, abs and comparisons only, which numpy rounds as the device does.

The antialiased crop of minified ROIs (lh_frames_crop_area_to_nhwc4, InferStep(antialias=...)): ``frames_crop`` on device tensors,
``crop_taps_host`` / ``frames_crop_host`` in numpy -- with ``max_taps=1`` the plain crop's sampling rule.

NV12 frames (lh_frames_crop_yuv_to_nhwc4, InferStep(frames=..., frame_format="nv12")): ``frames_crop(..., frame_format="nv12")`` is the
launch, ``frames_crop_nv12_host`` its rule in numpy (fp32, or fp64 with ``dtype=np.float64``).  The pixel formats themselves -- the
conversion matrix, the layouts, the encoders -- are frame_formats.py's; every public name there is imported here.

Training on frames (lh_roi_perturb / lh_affine_points_inv, runtime.TrainStep(frames=..., roi_aug=...)): ``roi_perturb`` turns the
caller's ROI and a drawn row (c, s, k, tx, ty, flip) into the ROI the crop uses, ``affine_points_inv`` takes frame coordinates into
the crop through the inverse of the crop matrix (``POINT_OFF`` for a slot that has none); ``roi_perturb_host`` /
``affine_points_inv_host`` restate them in numpy, in fp32 or, as the yardstick, in fp64.

ColorJitter on the crop (lh_frames_crop_jitter_to_nhwc4, runtime.TrainStep(frames=..., crop_jitter=...)): ``frames_crop(...,
jitter=(factors, order))`` is the launch, ``frames_crop_jitter_host`` its rule in numpy -- the host crop stopped in front of
Normalize, csrc/color_jitter.h's four ops (``color_jitter_host``), Normalize -- in fp32 or, as the yardstick, in fp64.

Decoder surfaces in place and the other 4:2:0 flavours (lh_frames_crop_surfaces_to_nhwc4, InferStep / TrainStep(frames=...,
surfaces=True, frame_format="nv21" | "yuv420p" | "p010")): ``check_surface`` / ``surface_table`` are the host checks and the table of
addresses, ``frames_crop(..., surfaces=[...])`` the launch, ``frames_crop_yuv420_host`` its rule in numpy -- the NV12 rule behind
another texel fetch (frame_formats.py: the plane descriptor ``Yuv420Layout`` and what builds and checks one).

Motion-aware tracking (lh_rois_predict / lh_one_euro_gated, runtime.ManagedInferStep(motion=..., smooth_gate=...)): ``rois_predict``
shifts the next ROIs along their low-passed velocity and coasts lost ones, ``one_euro_gated`` is the One-Euro filter gated per joint
by confidence with its speed in hand sizes; ``rois_predict_host`` / ``one_euro_gated_host`` restate them in numpy, fp32 or fp64.

The skeleton overlay (lh_draw_hands, runtime.ManagedInferStep(frames=..., overlay=...)): ``draw_hands`` draws the tracked hands into the
frames in place, ``draw_hands_host`` restates it in numpy, ``overlay_palette`` converts an RGB palette into the frames' plane space;
``HAND_PARENTS`` / ``HAND_GROUPS`` / ``OVERLAY_DEFAULTS`` hold the defaults.  All of it is overlay.py's; every public name there is
imported here."""
import numpy as np

from .frame_formats import (FRAME_FORMATS, Yuv420Layout, check_frame_format, check_nv12_layout, check_yuv420_layout,  # noqa: F401
                            chroma_siting_code, csc12, frame_layout_of, frames_layout_struct, nv12_layout, rgb_to_nv12_host,
                            rgb_to_yuv420_host, surface_bytes, yuv420_layout, yuv_matrix)

from .overlay import (HAND_GROUPS, HAND_PALETTE_RGB, HAND_PARENTS, OVERLAY_DEFAULTS, draw_hands, draw_hands_host,  # noqa: F401
                      overlay_palette, overlay_tables)

F = np.float32
_frames_layout_struct = frames_layout_struct          # the name tests/test_surfaces_host.py imports


def box_affine_host(boxes, frame_index, n_frames, size, padding):
    """boxes [b][4], frame_index [b], size = (h, w) of the crop -> (mat fp32 [b][6], src_frame int32 [b]); lh_box_affine in numpy."""
    h, w = F(size[0]), F(size[1])
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    fi = np.asarray(frame_index, np.int32).reshape(-1)
    pad = F(padding)
    x0, y0, x1, y1 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    with np.errstate(all="ignore"):
        bw, bh = x1 - x0, y1 - y0
        ok = (fi >= 0) & (fi < n_frames) & np.isfinite(boxes).all(1) & (bw > 0) & (bh > 0)
        cx, cy = (x0 + x1) * F(0.5), (y0 + y1) * F(0.5)
        sw = pad * np.maximum(bw, bh * w / h)
        sh = sw * h / w
        a = sw / w
        zero = np.zeros_like(a)
        mat = np.stack([a, zero, (cx - sw * F(0.5)) + a * F(0.5), zero, a, (cy - sh * F(0.5)) + a * F(0.5)], 1).astype(np.float32)
    mat[~ok] = 0
    return mat, np.where(ok, fi, -1).astype(np.int32)


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def crop_taps_host(mat, max_taps=8):
    """mat [b][6] -> int32 [b][2] = (kx, ky), the samples lh_frames_crop_area_to_nhwc4 averages per crop pixel along the crop's x and y
    axes: sx = sqrt(m0*m0 + m3*m3) frame pixels per crop pixel, kx = min(max_taps, ceil(min(sx, 64))) where sx > 1 + 1/64 and is
    finite, otherwise 1 (not minified, NaN, or a matrix that samples nothing); ky likewise from (m1, m4)."""
    if not 1 <= int(max_taps) <= 8:
        raise ValueError(f"max_taps must be 1..8, not {max_taps!r}")
    m = np.asarray(mat, np.float32).reshape(-1, 6)
    out = np.ones((m.shape[0], 2), np.int32)
    with np.errstate(all="ignore"):
        for axis, (a, b) in enumerate(((m[:, 0], m[:, 3]), (m[:, 1], m[:, 4]))):
            s = np.sqrt(a * a + b * b)
            many = (s > F(1.015625)) & np.isfinite(s)
            k = np.minimum(int(max_taps), np.ceil(np.minimum(np.where(many, s, F(1)), F(64))).astype(np.int32))
            out[:, axis] = np.where(many, k, 1)
    return out


def _sample_host(img, hs, ws, fx, fy):
    """One bilinear sample per element of fx / fy on the raw 0..255 values of img fp32 [3][hs][ws], the crop kernel's: -> (fp32
    [3][...], inside mask); outside the frame (NaN included) the sample is 0."""
    with np.errstate(all="ignore"):
        inside = (fx >= F(-0.5)) & (fx <= F(ws) - F(0.5)) & (fy >= F(-0.5)) & (fy <= F(hs) - F(0.5))
    cy = np.where(inside, np.maximum(fy, F(0)), F(0)).astype(np.float32)
    cx = np.where(inside, np.maximum(fx, F(0)), F(0)).astype(np.float32)
    y0, x0 = np.minimum(cy.astype(np.int32), hs - 1), np.minimum(cx.astype(np.int32), ws - 1)
    y1, x1 = np.minimum(y0 + 1, hs - 1), np.minimum(x0 + 1, ws - 1)
    wy, wx = cy - y0.astype(np.float32), cx - x0.astype(np.float32)
    a00, a01, a10, a11 = img[:, y0, x0], img[:, y0, x1], img[:, y1, x0], img[:, y1, x1]
    top, bot = a00 + (a01 - a00) * wx, a10 + (a11 - a10) * wx
    return np.where(inside, top + (bot - top) * wy, F(0)).astype(np.float32), inside


def _normalise_host(c, mean, std, dtype=np.float32):
    """(c - mean) * (1 / std) per channel on [b][3][h][w], the crop kernels' Normalize (1 / std is formed in fp32)."""
    mean = np.asarray(mean, np.float32).astype(dtype)[None, :, None, None]
    istd = (F(1) / np.asarray(std, np.float32)).astype(dtype)[None, :, None, None]
    return ((c - mean) * istd).astype(dtype)


def frames_crop_host(frames, mat, src_frame, size, max_taps=1, mean=MEAN, std=STD):
    """uint8 frames [n][hs][ws][3], mat [b][6], src_frame [b], size = (h, w) of the crop -> normalised fp32 [b][3][h][w];
    lh_frames_crop_area_to_nhwc4 in numpy (``max_taps=1``: lh_frames_crop_to_nhwc4), fp32 in the kernel's order: per slot
    (kx, ky) = crop_taps_host, per pixel the kx * ky samples at ux = ox + (2*i + 1 - kx) / (2*kx), uy likewise (j outside, i inside)
    are summed on the raw 0..255 values, a sample outside the frame adding 0, then (acc * (1 / (kx*ky))) * (1/255) and Normalize."""
    return _normalise_host(_crop_unit_host(frames, mat, src_frame, size, max_taps), mean, std)


def _tap_loop_host(sample_of, mat, src_frame, size, max_taps, dtype=np.float32):
    """The tap loop of every host crop, stopped in front of Normalize: the pixels' c in 0..1, [b][3][h][w] of ``dtype``, every operation
    in it.  ``sample_of(f)`` gives frame f's sample, a callable (fx, fy) -> [3][h][w] on 0..255, or None where the slot's frame number
    names no frame: an empty slot, black."""
    T = np.dtype(dtype).type
    h, w = int(size[0]), int(size[1])
    mat = np.asarray(mat, np.float32).reshape(-1, 6)
    src = np.asarray(src_frame, np.int32).reshape(-1)
    taps = crop_taps_host(mat, max_taps)
    oy, ox = np.meshgrid(np.arange(h, dtype=dtype), np.arange(w, dtype=dtype), indexing="ij")
    out = np.empty((len(src), 3, h, w), dtype)
    for s in range(len(src)):
        acc = np.zeros((3, h, w), dtype)
        kx, ky = int(taps[s, 0]), int(taps[s, 1])
        sample = sample_of(int(src[s]))
        if sample is not None:
            m0, m1, m2, m3, m4, m5 = mat[s].astype(dtype)
            with np.errstate(all="ignore"):
                for j in range(ky):
                    uy = oy + T(2 * j + 1 - ky) / T(2 * ky)
                    for i in range(kx):
                        ux = ox + T(2 * i + 1 - kx) / T(2 * kx)
                        acc += sample((m0 * ux + m1 * uy) + m2, (m3 * ux + m4 * uy) + m5)
        else:
            kx = ky = 1
        out[s] = (acc * (T(1) / T(kx * ky))) * (T(1) / T(255))
    return out


def _crop_unit_host(frames, mat, src_frame, size, max_taps=1):
    """frames_crop_host stopped in front of Normalize: the pixels' c in 0..1, fp32 [b][3][h][w]."""
    frames = np.asarray(frames)
    n, hs, ws = frames.shape[:3]

    def sample_of(f):
        if not 0 <= f < n:
            return None
        img = np.transpose(frames[f].astype(np.float32), (2, 0, 1))
        return lambda fx, fy: _sample_host(img, hs, ws, fx, fy)[0]
    return _tap_loop_host(sample_of, mat, src_frame, size, max_taps)


def frames_crop_nv12_host(frames_nv12, frame_size, mat, src_frame, size, yuv=("bt709", "limited"), chroma_siting="left", max_taps=1,
                          layout=None, mean=MEAN, std=STD, dtype=np.float32):
    """uint8 NV12 frames [n][rows][pitch] of ``frame_size`` = (hs, ws) in ``layout`` (nv12_layout's tuple; None: tight), mat [b][6],
    src_frame [b], size = (h, w) of the crop -> normalised [b][3][h][w]; lh_frames_crop_yuv_to_nhwc4 in numpy, fp32 in the kernel's order:
    frames_crop_host's tap loop with the NV12 sample (the rule: csrc/frames_crop_kernel.h, above crop_sample_nv12) in the RGB one's place.  ``yuv`` is
    (standard, range) or the 12 coefficients, ``chroma_siting`` "left" or "center".  ``dtype=np.float64``: the same operations in fp64
    on the same fp32 matrices and coefficients (the tap counts stay crop_taps_host's) -- what the fp32 order is measured against."""
    return _normalise_host(_crop_unit_nv12_host(frames_nv12, frame_size, mat, src_frame, size, yuv, chroma_siting, max_taps, layout, dtype),
                           mean, std, dtype)


def _crop_unit_nv12_host(frames_nv12, frame_size, mat, src_frame, size, yuv=("bt709", "limited"), chroma_siting="left", max_taps=1,
                         layout=None, dtype=np.float32):
    """frames_crop_nv12_host stopped in front of Normalize: the pixels' c in 0..1, [b][3][h][w] of ``dtype``."""
    hs, ws = int(frame_size[0]), int(frame_size[1])
    pitch, _, _, rows = check_nv12_layout(hs, ws, layout)
    frames = np.asarray(frames_nv12)
    if frames.dtype != np.uint8 or frames.ndim != 3 or frames.shape[1:] != (rows, pitch):
        raise ValueError(f"frames_crop_nv12_host: frames uint8 [n][{rows}][{pitch}], not {frames.shape} {frames.dtype}")
    # the same bytes through the plane descriptor: c_pitch = pitch, cb_offset = uv_offset, cr_offset = uv_offset + 1, c_step = 2
    L = yuv420_layout("nv12", hs, ws, pitch, rows - hs // 2)
    return _crop_unit_420_host([f.reshape(-1) for f in frames], L, mat, src_frame, size, yuv, chroma_siting, max_taps, dtype)


def _crop_unit_420_host(frames, L, mat, src_frame, size, yuv, chroma_siting, max_taps, dtype):
    """The tap loop on 4:2:0 frames: ``frames`` a list of flat uint8 arrays (None: an unbound surface, an empty slot) in the layout L."""
    T = np.dtype(dtype).type
    csc = csc12(yuv, 10 if L.code == 4 else 8).astype(dtype)
    k, o = csc[:9].reshape(3, 3), csc[9:]
    siting = chroma_siting_code(chroma_siting)

    def sample_of(f):
        if not 0 <= f < len(frames) or frames[f] is None:
            return None
        return lambda fx, fy: _sample_420_host(frames[f], L, siting, k, o, fx, fy, T)[0]
    return _tap_loop_host(sample_of, mat, src_frame, size, max_taps, dtype)


def _sample_420_host(flat, L, siting, k, o, fx, fy, T):
    """One sample per element of fx / fy of one 4:2:0 frame (``flat``: its bytes, uint8) through the plane descriptor ``L``,
    lh_frames_crop_surfaces_to_nhwc4's and, for an NV12 buffer, lh_frames_crop_yuv_to_nhwc4's -> (RGB on 0..255, type T [3][...], inside
    mask); outside the frame (NaN included) the sample is 0."""
    hs, ws = L.hs, L.ws
    with np.errstate(all="ignore"):
        inside = (fx >= T(-0.5)) & (fx <= T(ws) - T(0.5)) & (fy >= T(-0.5)) & (fy <= T(hs) - T(0.5))
    cy = np.where(inside, np.maximum(fy, T(0)), T(0)).astype(T)
    cx = np.where(inside, np.maximum(fx, T(0)), T(0)).astype(T)

    def tex(off):
        if L.sample_bytes == 2:
            u16 = flat[off].astype(np.int32) | (flat[off + 1].astype(np.int32) << 8)
            return (u16 >> L.shift).astype(T) * T(0.25)
        return flat[off].astype(T)

    def blend(at, x0, x1, y0, y1, wx, wy):
        a00, a01, a10, a11 = tex(at(x0, y0)), tex(at(x1, y0)), tex(at(x0, y1)), tex(at(x1, y1))
        top, bot = a00 + (a01 - a00) * wx, a10 + (a11 - a10) * wx
        return top + (bot - top) * wy

    y0, x0 = np.minimum(cy.astype(np.int32), hs - 1), np.minimum(cx.astype(np.int32), ws - 1)
    y1, x1 = np.minimum(y0 + 1, hs - 1), np.minimum(x0 + 1, ws - 1)
    lum = blend(lambda x, y: y * L.pitch + x * L.sample_bytes, x0, x1, y0, y1, cx - x0.astype(T), cy - y0.astype(T))
    hc, wc = hs // 2, ws // 2
    gx = cx * T(0.5) if siting == 0 else (cx - T(0.5)) * T(0.5)
    gy = (cy - T(0.5)) * T(0.5)
    gx, gy = np.minimum(np.maximum(gx, T(0)), T(wc - 1)), np.minimum(np.maximum(gy, T(0)), T(hc - 1))
    v0, u0 = np.minimum(gy.astype(np.int32), hc - 1), np.minimum(gx.astype(np.int32), wc - 1)
    v1, u1 = np.minimum(v0 + 1, hc - 1), np.minimum(u0 + 1, wc - 1)
    wx, wy = gx - u0.astype(T), gy - v0.astype(T)
    cb = blend(lambda x, y: L.cb_offset + y * L.c_pitch + x * L.c_step, u0, u1, v0, v1, wx, wy)
    cr = blend(lambda x, y: L.cr_offset + y * L.c_pitch + x * L.c_step, u0, u1, v0, v1, wx, wy)
    e0, e1, e2 = lum - o[0], cb - o[1], cr - o[2]
    rgb = np.stack([np.minimum(np.maximum((k[c, 0] * e0 + k[c, 1] * e1) + k[c, 2] * e2, T(0)), T(255)) for c in (0, 1, 2)])
    return np.where(inside, rgb, T(0)).astype(T), inside


def _frame_bytes_host(frames_or_surfaces, need, who):
    """One array [n][...] or a sequence of per-frame byte arrays (None: an unbound surface) -> a list of flat uint8 arrays / None."""
    seq = list(frames_or_surfaces) if isinstance(frames_or_surfaces, (list, tuple)) else list(np.asarray(frames_or_surfaces))
    out = []
    for f in seq:
        if f is None:
            out.append(None)
            continue
        f = np.asarray(f)
        if f.dtype != np.uint8 or f.size < need:
            raise ValueError(f"{who}: a frame is uint8 with at least {need} bytes, not {f.shape} {f.dtype}")
        out.append(f.reshape(-1))
    return out


def _crop_unit_yuv420_host(frames_or_surfaces, frame_size, mat, src_frame, size, frame_format="nv12", layout=None, yuv=("bt709", "limited"),
                           chroma_siting="left", max_taps=1, dtype=np.float32):
    """frames_crop_yuv420_host stopped in front of Normalize: the pixels' c in 0..1, [b][3][h][w] of ``dtype``."""
    hs, ws = int(frame_size[0]), int(frame_size[1])
    L = frame_layout_of(frame_format, hs, ws, layout)
    frames = _frame_bytes_host(frames_or_surfaces, surface_bytes(L), "frames_crop_yuv420_host")
    n = len(frames)
    if L.code == 0:                                                # packed RGB surfaces: the RGB rule, an unbound surface is an empty slot
        src = np.asarray(src_frame, np.int32).reshape(-1)
        live = np.array([0 <= s < n and frames[s] is not None for s in src])
        rgb = np.stack([np.zeros(hs * ws * 3, np.uint8) if f is None else f[:hs * ws * 3] for f in frames]).reshape(n, hs, ws, 3)
        return _crop_unit_host(rgb, mat, np.where(live, src, -1), size, max_taps).astype(dtype)
    return _crop_unit_420_host(frames, L, mat, src_frame, size, yuv, chroma_siting, max_taps, dtype)


def frames_crop_yuv420_host(frames_or_surfaces, frame_size, mat, src_frame, size, frame_format="nv12", layout=None, yuv=("bt709", "limited"),
                            chroma_siting="left", max_taps=1, mean=MEAN, std=STD, dtype=np.float32):
    """lh_frames_crop_surfaces_to_nhwc4 in numpy: ``frames_or_surfaces`` is one uint8 array [n][...] or a sequence of per-frame byte
    arrays (None: an unbound surface, the slot is black), each at least surface_bytes(layout) long, of ``frame_size`` = (hs, ws) frames
    of ``frame_format`` in ``layout`` (frame_layout_of's rules; None: tight) -> normalised [b][3][h][w].  frames_crop_nv12_host's
    operations in its order, the texels through the plane descriptor (a p010 texel is (u16 >> 6) * 0.25); on NV12 input its bits.
    fp32 in the kernel's order, or with ``dtype=np.float64`` the same operations in fp64 on the same fp32 matrices and coefficients.
    ``yuv`` = (standard, range) means yuv_matrix(standard, range, bits=10) for p010."""
    return _normalise_host(_crop_unit_yuv420_host(frames_or_surfaces, frame_size, mat, src_frame, size, frame_format, layout, yuv,
                                                  chroma_siting, max_taps, dtype), mean, std, dtype)


# ---- ColorJitter on the crop: csrc/color_jitter.h's four ops in numpy, in the kernel's order of operations (T = the evaluation type)
def _cj_clamp01(v, T):
    return np.minimum(np.maximum(v, T(0)), T(1))


def _cj_gray(c, T):
    return (T(F(0.2989)) * c[0] + T(F(0.587)) * c[1]) + T(F(0.114)) * c[2]


def _cj_blend(c, o, r, T):
    """clamp(r * c + (1 - r) * o) per channel; ``o`` is a scalar or one plane."""
    return np.stack([_cj_clamp01(r * c[ch] + (T(1) - r) * o, T) for ch in range(3)])


def _cj_hue(c, f, T):
    r, g, b = c
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    eq = maxc == minc
    cr = maxc - minc
    s = cr / np.where(eq, T(1), maxc)
    div = np.where(eq, T(1), cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    h = np.where(maxc == r, bc - gc, np.where(maxc == g, (T(2) + rc) - bc, (T(4) + gc) - rc))
    h = np.fmod(h / T(6) + T(1), T(1))
    h = np.fmod(h + f, T(1))
    h = np.where(h < T(0), h + T(1), h)
    h6 = h * T(6)
    fl = np.floor(h6)
    fr = h6 - fl
    i = fl.astype(np.int32) % 6
    v = maxc
    p = _cj_clamp01(v * (T(1) - s), T)
    q = _cj_clamp01(v * (T(1) - s * fr), T)
    t = _cj_clamp01(v * (T(1) - s * (T(1) - fr)), T)
    return np.stack([np.choose(i, [v, q, p, p, t, v]), np.choose(i, [t, v, v, q, p, p]), np.choose(i, [p, p, t, v, v, q])])


def color_jitter_host(c, factors, order, dtype=np.float32):
    """One crop c [3][h][w] in 0..1 through the ops of ``order`` (ids 0..3 = brightness, contrast, saturation, hue; negative = skip)
    with ``factors`` [4]: cj_apply of csrc/color_jitter.h on every pixel, the contrast op's mean = the crop's grey mean when the op
    runs, summed in fp64 and rounded once ((float)(sum / (h*w)); the kernels sum partials, so the last bit of the mean may differ)."""
    T = np.dtype(dtype).type
    c = np.asarray(c, dtype)
    f = np.asarray(factors, np.float32).astype(dtype)
    with np.errstate(all="ignore"):
        for op in (int(v) for v in order):
            if op == 0:
                c = _cj_blend(c, T(0), f[0], T)
            elif op == 1:
                mean = T(np.float32(_cj_gray(c, T).astype(np.float64).sum() / (c.shape[1] * c.shape[2]))) if T is np.float32 else \
                    T(_cj_gray(c, T).sum() / (c.shape[1] * c.shape[2]))
                c = _cj_blend(c, mean, f[1], T)
            elif op == 2:
                c = _cj_blend(c, _cj_gray(c, T), f[2], T)
            elif op == 3:
                c = _cj_hue(c, f[3], T)
    return c.astype(dtype)


def frames_crop_jitter_host(frames, mat, src_frame, size, factors, order, max_taps=1, mean=MEAN, std=STD, frame_format="rgb",
                            frame_size=None, yuv=("bt709", "limited"), chroma_siting="left", layout=None, dtype=np.float32):
    """lh_frames_crop_jitter_to_nhwc4 in numpy: frames_crop_host (``frame_format="nv12"``: frames_crop_nv12_host, with ``frame_size``,
    ``yuv``, ``chroma_siting`` and ``layout`` as there) stopped in front of Normalize, then per slot the ops of ``order`` int [b][4]
    with ``factors`` fp32 [b][4] (color_jitter_host), then Normalize -> [b][3][h][w].  fp32 in the kernel's order; a slot whose order
    is all negative is the un-jittered host crop bit for bit.  ``dtype=np.float64``: the jitter and Normalize (and, for NV12, the
    sampling) evaluated in fp64 on the same inputs -- what the fp32 order is measured against.  ``frame_format`` "nv21" / "yuv420p" /
    "p010", a Yuv420Layout, or ``frames`` as a list of per-frame byte arrays (surfaces; None: unbound): frames_crop_yuv420_host's crop."""
    check_frame_format(frame_format)
    if frame_format == "nv12" and not isinstance(layout, Yuv420Layout) and not isinstance(frames, (list, tuple)):
        c = _crop_unit_nv12_host(frames, frame_size, mat, src_frame, size, yuv, chroma_siting, max_taps, layout, dtype)
    elif frame_format != "rgb" or isinstance(frames, (list, tuple)):          # the plane descriptor's formats, or a list of surfaces
        if frame_size is None:
            frame_size = np.asarray(frames).shape[1:3]
        c = _crop_unit_yuv420_host(frames, frame_size, mat, src_frame, size, frame_format, layout, yuv, chroma_siting, max_taps, dtype)
    else:
        c = _crop_unit_host(frames, mat, src_frame, size, max_taps).astype(dtype)
    factors = np.asarray(factors, np.float32).reshape(c.shape[0], 4)
    order = np.asarray(order, np.int32).reshape(c.shape[0], 4)
    c = np.stack([color_jitter_host(c[s], factors[s], order[s], dtype) for s in range(c.shape[0])])
    return _normalise_host(c, mean, std, dtype)


def boxes_from_keypoints_host(preds, maxvals, boxes, src_frame, min_score=0.1, min_joints=8, min_side=16.0):
    """preds [b][j][2] (frame coordinates), maxvals [b][j] or [b][j][1], boxes [b][4], src_frame [b] -> (next_boxes fp32 [b][4],
    lost int32 [b]); lh_keypoints_to_boxes in numpy: the joints are walked in order with the kernel's comparisons."""
    preds = np.asarray(preds, np.float32)
    b, j = preds.shape[:2]
    mv = np.asarray(maxvals, np.float32).reshape(b, j)
    boxes = np.asarray(boxes, np.float32).reshape(b, 4)
    src = np.asarray(src_frame, np.int32).reshape(b)
    lo_x, lo_y, hi_x, hi_y = (np.zeros(b, np.float32) for _ in range(4))
    n = np.zeros(b, np.int64)
    with np.errstate(all="ignore"):
        for k in range(j):
            take = mv[:, k] >= F(min_score)
            x, y = preds[:, k, 0], preds[:, k, 1]
            first = take & (n == 0)
            lo_x, hi_x = np.where(first, x, lo_x), np.where(first, x, hi_x)
            lo_y, hi_y = np.where(first, y, lo_y), np.where(first, y, hi_y)
            lo_x, hi_x = np.where(take & (x < lo_x), x, lo_x), np.where(take & (x > hi_x), x, hi_x)
            lo_y, hi_y = np.where(take & (y < lo_y), y, lo_y), np.where(take & (y > hi_y), y, hi_y)
            n += take
        half = F(min_side) * F(0.5)
        for lo, hi in ((lo_x, hi_x), (lo_y, hi_y)):
            narrow = hi - lo < F(min_side)
            c = (lo + hi) * F(0.5)
            lo[:], hi[:] = np.where(narrow, c - half, lo), np.where(narrow, c + half, hi)
    lost = (n < min_joints) | (src < 0)
    out = np.stack([lo_x, lo_y, hi_x, hi_y], 1).astype(np.float32)
    out[lost] = boxes[lost]
    return out, lost.astype(np.int32)


def _over_host(a, b, t):
    """lh_tracks_manage's overlap test on two boxes of fp32 scalars: intersection over the smaller area > t, by comparisons and products."""
    ix1, ix0 = (a[2] if a[2] < b[2] else b[2]), (a[0] if a[0] > b[0] else b[0])
    iy1, iy0 = (a[3] if a[3] < b[3] else b[3]), (a[1] if a[1] > b[1] else b[1])
    iw, ih = ix1 - ix0, iy1 - iy0
    if not (iw > 0 and ih > 0):
        return False
    aa, ab = (a[2] - a[0]) * (a[3] - a[1]), (b[2] - b[0]) * (b[3] - b[1])
    return bool(iw * ih > t * (aa if aa < ab else ab))


MANAGE_TRACKS_DEFAULTS = dict(dup_overlap=0.5, match_overlap=0.5, det_min_score=0.0, max_lost=0)


def manage_tracks_host(preds, maxvals, src_frame, frame_index, n_frames, next_boxes, next_rot, lost, lost_count, det_boxes, det_frame, det_score,
                       min_score=0.1, min_side=16.0, dup_overlap=0.5, match_overlap=0.5, det_min_score=0.0, max_lost=0, dup_of=None,
                       seeded=None):
    """lh_tracks_manage in numpy, fp32 in the kernel's order: preds [b][j][2] (frame coordinates), maxvals [b][j] or [b][j][1], src_frame /
    frame_index / lost / lost_count [b], next_boxes [b][4], next_rot [b][2] or None, the detection list det_boxes [k][4], det_frame [k],
    det_score [k] -> (next_boxes, next_rot, lost, lost_count, dup_of, seeded, det_state), new arrays: the inputs are not modified.
    ``dup_of`` / ``seeded`` [b] are what the outputs of those names hold before the call (None: -1), which a slot of no frame keeps.
    Per frame f (the slots with frame_index == f, 0 <= f < n_frames):
    kb = the bounds lh_keypoints_to_boxes takes of the joints with maxval >= min_score, score = the sum of those maxvals; the live slots
    (lost == 0) are walked in descending score, ties to the lower index, and one is kept unless it overlaps (``_over_host`` at
    dup_overlap) a slot kept before it -- then dup_of names the first such slot, lost = 1, its next box is 0 0 0 0 and lost_count 0.
    lost_count is 0 for a kept slot and for an empty one (src_frame < 0) and counts up (to 1 << 30) for every other slot; with max_lost > 0
    a count >= max_lost empties the slot (next box 0 0 0 0, count 0).  The valid detections (finite box with x1 > x0, y1 > y0, finite
    score >= det_min_score) are walked in descending score, ties to the lower index: det_state = -2 when one overlaps (match_overlap) a
    kept slot, else -3 when it overlaps a detection accepted before it, else -4 when every slot that was not kept is taken, else the
    lowest such slot i: seeded[i] = d, its next box is the detection's, next_rot (1, 0), lost_count 0, lost as it was.  -1 for every
    other entry of the list."""
    preds = np.asarray(preds, np.float32)
    b, j = preds.shape[:2]
    mv = np.asarray(maxvals, np.float32).reshape(b, j)
    src, fidx = np.asarray(src_frame, np.int32).reshape(b), np.asarray(frame_index, np.int32).reshape(b)
    nbox = np.array(next_boxes, np.float32).reshape(b, 4)
    nrot = None if next_rot is None else np.array(next_rot, np.float32).reshape(b, 2)
    lost, count = np.array(lost, np.int32).reshape(b), np.array(lost_count, np.int32).reshape(b)
    dbox = np.asarray(det_boxes, np.float32).reshape(-1, 4)
    k = dbox.shape[0]
    dfr, dsc = np.asarray(det_frame, np.int32).reshape(k), np.asarray(det_score, np.float32).reshape(k)
    dup_of = np.full(b, -1, np.int32) if dup_of is None else np.array(dup_of, np.int32).reshape(b)
    seeded = np.full(b, -1, np.int32) if seeded is None else np.array(seeded, np.int32).reshape(b)
    det_state = np.full(k, -1, np.int32)
    kb, _ = boxes_from_keypoints_host(preds, mv, np.zeros((b, 4), np.float32), np.zeros(b, np.int32), min_score, 0, min_side)
    score = np.zeros(b, np.float32)
    for q in range(j):
        score = np.where(mv[:, q] >= F(min_score), score + mv[:, q], score).astype(np.float32)
    dup_t, match_t = F(dup_overlap), F(match_overlap)
    with np.errstate(all="ignore"):
        valid = ((dfr >= 0) & (dfr < n_frames) & np.isfinite(dbox).all(1) & (dbox[:, 2] > dbox[:, 0]) & (dbox[:, 3] > dbox[:, 1])
                 & np.isfinite(dsc) & (dsc >= F(det_min_score)))
        for f in range(int(n_frames)):
            members = [int(i) for i in np.nonzero(fidx == f)[0]]
            kept, suppressed = [], set()
            for i in sorted((i for i in members if lost[i] == 0), key=lambda i: (-score[i], i)):
                hit = next((q for q in kept if _over_host(kb[i], kb[q], dup_t)), None)
                if hit is None:
                    kept.append(i)
                else:
                    suppressed.add(i)
                    dup_of[i], lost[i], nbox[i], count[i] = hit, 1, 0, 0
            for i in members:
                seeded[i] = -1
                if i in kept:
                    dup_of[i], count[i] = -1, 0
                elif i in suppressed:
                    pass
                elif src[i] < 0:
                    dup_of[i], count[i] = -1, 0
                else:
                    dup_of[i] = -1
                    count[i] = count[i] + 1 if count[i] < (1 << 30) else (1 << 30)
                    if max_lost > 0 and count[i] >= max_lost:
                        nbox[i], count[i] = 0, 0
            free = [i for i in members if i not in kept]
            accepted = []
            for d in sorted((int(d) for d in np.nonzero(valid & (dfr == f))[0]), key=lambda d: (-dsc[d], d)):
                if any(_over_host(dbox[d], kb[i], match_t) for i in kept):
                    det_state[d] = -2
                elif any(_over_host(dbox[d], dbox[e], match_t) for e in accepted):
                    det_state[d] = -3
                elif len(accepted) >= len(free):
                    det_state[d] = -4
                else:
                    i = free[len(accepted)]
                    accepted.append(d)
                    det_state[d], seeded[i], nbox[i], count[i] = i, d, dbox[d], 0
                    if nrot is not None:
                        nrot[i] = (1, 0)
    return nbox, nrot, lost, count, dup_of, seeded, det_state


def rot_from_angle(radians):
    """The orientation (cos, sin) of a crop turned by ``radians`` in the image plane (x to the right, y down: a positive angle turns
    the crop's +x axis towards the frame's +y).  The kernels take the direction, never the angle."""
    import math
    return (math.cos(radians), math.sin(radians))


def roi_affine_host(boxes, rot, mirror, frame_index, n_frames, size, padding):
    """boxes [b][4], rot [b][2] (frame direction of the crop's +x axis, any length), mirror [b], frame_index [b], size = (h, w) of the
    crop -> (mat fp32 [b][6], src_frame int32 [b]); lh_roi_affine in numpy."""
    h, w = F(size[0]), F(size[1])
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    rot = np.asarray(rot, np.float32).reshape(-1, 2)
    g = np.where(np.asarray(mirror).reshape(-1) != 0, F(-1), F(1)).astype(np.float32)
    fi = np.asarray(frame_index, np.int32).reshape(-1)
    pad = F(padding)
    x0, y0, x1, y1 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    rx, ry = rot[:, 0], rot[:, 1]
    with np.errstate(all="ignore"):
        bw, bh = x1 - x0, y1 - y0
        n = np.sqrt(rx * rx + ry * ry)
        ok = (fi >= 0) & (fi < n_frames) & np.isfinite(boxes).all(1) & (bw > 0) & (bh > 0) & np.isfinite(rot).all(1) & (n > 0)
        cx, cy = (x0 + x1) * F(0.5), (y0 + y1) * F(0.5)
        sw = pad * np.maximum(bw, bh * w / h)
        a = sw / w
        c, s = rx / n, ry / n
        ac, as_ = a * c, a * s
        m0, m1, m3, m4 = g * ac, -as_, g * as_, ac
        hx, hy = (w - F(1)) * F(0.5), (h - F(1)) * F(0.5)
        mat = np.stack([m0, m1, cx - (m0 * hx + m1 * hy), m3, m4, cy - (m3 * hx + m4 * hy)], 1).astype(np.float32)
    mat[~ok] = 0
    return mat, np.where(ok, fi, -1).astype(np.int32)


POINT_OFF = -65536.0          # LH_POINT_OFF: where lh_affine_points_inv puts the points of a slot it cannot map
ROI_AUG_IDENTITY = (1.0, 0.0, 1.0, 0.0, 0.0, 0.0)          # (c, s, k, tx, ty, flip): lh_roi_perturb copies such a slot bit for bit


def roi_perturb_host(boxes, rot, mirror, aug, dtype=np.float32):
    """boxes [b][4], rot [b][2] (None: (1, 0)), mirror [b] (None: 0), aug [b][6] = (c, s, k, tx, ty, flip) -> (boxes' [b][4], rot'
    [b][2], mirror' int32 [b]); lh_roi_perturb in numpy, fp32 in the kernel's order.  ``dtype=np.float64``: the same operations in fp64
    on the same fp32 inputs (the yardstick of the fp32 order); the copied slots are the same in both."""
    T = np.dtype(dtype).type
    boxes32 = np.asarray(boxes, np.float32).reshape(-1, 4)
    b = boxes32.shape[0]
    rot32 = np.tile(np.array([1, 0], np.float32), (b, 1)) if rot is None else np.asarray(rot, np.float32).reshape(b, 2)
    mir = np.zeros(b, np.int32) if mirror is None else np.asarray(mirror, np.int32).reshape(b)
    aug32 = np.asarray(aug, np.float32).reshape(b, 6)
    bx, rt, ag = boxes32.astype(dtype), rot32.astype(dtype), aug32.astype(dtype)
    x0, y0, x1, y1 = bx[:, 0], bx[:, 1], bx[:, 2], bx[:, 3]
    rx, ry = rt[:, 0], rt[:, 1]
    c, s, k, tx, ty, flip = (ag[:, i] for i in range(6))
    with np.errstate(all="ignore"):
        n32 = np.sqrt(rot32[:, 0] * rot32[:, 0] + rot32[:, 1] * rot32[:, 1])          # the decision is the kernel's, in fp32
        same = (aug32 == np.asarray(ROI_AUG_IDENTITY, np.float32)).all(1)
        ok = np.isfinite(boxes32).all(1) & np.isfinite(rot32).all(1) & (n32 > 0) & np.isfinite(aug32).all(1)
        bw, bh = x1 - x0, y1 - y0
        cx, cy = (x0 + x1) * T(0.5), (y0 + y1) * T(0.5)
        n = np.sqrt(rx * rx + ry * ry)
        ux, uy = rx / n, ry / n
        dx, dy = tx * bw, ty * bh
        ncx, ncy = cx + (dx * ux - dy * uy), cy + (dx * uy + dy * ux)
        hw, hh = (bw * k) * T(0.5), (bh * k) * T(0.5)
        nbox = np.stack([ncx - hw, ncy - hh, ncx + hw, ncy + hh], 1).astype(dtype)
        nrot = np.stack([ux * c - uy * s, ux * s + uy * c], 1).astype(dtype)
    nmir = ((mir != 0) != (aug32[:, 5] != 0)).astype(np.int32)
    keep = same | ~ok
    nbox[keep], nrot[keep], nmir[keep] = bx[keep], rt[keep], mir[keep]
    return nbox, nrot, nmir


def affine_points_inv_host(pts, mat, src_frame, dtype=np.float32):
    """pts [b][j][>=2] (frame coordinates), mat [b][6] (crop -> frame), src_frame [b] -> crop coordinates [b][j][2];
    lh_affine_points_inv in numpy, fp32 in the kernel's order.  A slot with src_frame < 0, or whose determinant (in fp32, the kernel's)
    is not finite or 0, gives POINT_OFF.  ``dtype=np.float64``: the same operations in fp64 on the same fp32 inputs."""
    T = np.dtype(dtype).type
    pts32 = np.asarray(pts, np.float32)
    b = pts32.shape[0]
    m32 = np.asarray(mat, np.float32).reshape(b, 6)
    src = np.asarray(src_frame, np.int32).reshape(b)
    p, m = pts32.astype(dtype), m32.astype(dtype)[:, None, :]
    with np.errstate(all="ignore"):
        det32 = m32[:, 0] * m32[:, 4] - m32[:, 1] * m32[:, 3]
        ok = (src >= 0) & np.isfinite(det32) & (det32 != 0)
        det = m[..., 0] * m[..., 4] - m[..., 1] * m[..., 3]
        qx, qy = p[..., 0] - m[..., 2], p[..., 1] - m[..., 5]
        out = np.stack([(m[..., 4] * qx - m[..., 1] * qy) / det, (m[..., 0] * qy - m[..., 3] * qx) / det], -1).astype(dtype)
    out[~ok] = T(POINT_OFF)
    return out


def rois_from_keypoints_host(preds, maxvals, boxes, rot, src_frame, axis=(0, 9), min_score=0.1, min_joints=8, min_side=16.0, min_axis=4.0):
    """preds [b][j][2] (frame coordinates), maxvals [b][j] or [b][j][1], boxes [b][4], rot [b][2], src_frame [b] -> (next_boxes fp32
    [b][4], next_rot fp32 [b][2], lost int32 [b]); lh_keypoints_to_rois in numpy, the joints walked in order."""
    preds = np.asarray(preds, np.float32)
    b, j = preds.shape[:2]
    mv = np.asarray(maxvals, np.float32).reshape(b, j)
    boxes = np.asarray(boxes, np.float32).reshape(b, 4)
    rot = np.asarray(rot, np.float32).reshape(b, 2)
    src = np.asarray(src_frame, np.int32).reshape(b)
    k0, k1 = axis
    score, side = F(min_score), F(min_side)
    with np.errstate(all="ignore"):
        rx, ry = rot[:, 0], rot[:, 1]
        rn = np.sqrt(rx * rx + ry * ry)
        c, s = rx / rn, ry / rn
        dx, dy = preds[:, k1, 0] - preds[:, k0, 0], preds[:, k1, 1] - preds[:, k0, 1]
        d = np.sqrt(dx * dx + dy * dy)
        turn = (mv[:, k0] >= score) & (mv[:, k1] >= score) & (d >= F(min_axis))
        c, s = np.where(turn, -(dy / d), c).astype(np.float32), np.where(turn, dx / d, s).astype(np.float32)
        lo_p, lo_q, hi_p, hi_q = (np.zeros(b, np.float32) for _ in range(4))
        n = np.zeros(b, np.int64)
        for k in range(j):
            take = mv[:, k] >= score
            x, y = preds[:, k, 0], preds[:, k, 1]
            u, v = x * c + y * s, y * c - x * s
            first = take & (n == 0)
            lo_p, hi_p = np.where(first, u, lo_p), np.where(first, u, hi_p)
            lo_q, hi_q = np.where(first, v, lo_q), np.where(first, v, hi_q)
            lo_p, hi_p = np.where(take & (u < lo_p), u, lo_p), np.where(take & (u > hi_p), u, hi_p)
            lo_q, hi_q = np.where(take & (v < lo_q), v, lo_q), np.where(take & (v > hi_q), v, hi_q)
            n += take
        half = side * F(0.5)
        for lo, hi in ((lo_p, hi_p), (lo_q, hi_q)):
            narrow = hi - lo < side
            m = (lo + hi) * F(0.5)
            lo[:], hi[:] = np.where(narrow, m - half, lo), np.where(narrow, m + half, hi)
        cp, cq, hp, hq = (lo_p + hi_p) * F(0.5), (lo_q + hi_q) * F(0.5), (hi_p - lo_p) * F(0.5), (hi_q - lo_q) * F(0.5)
        fx, fy = cp * c - cq * s, cp * s + cq * c
        out = np.stack([fx - hp, fy - hq, fx + hp, fy + hq], 1).astype(np.float32)
    lost = (n < min_joints) | (src < 0) | ~(np.isfinite(c) & np.isfinite(s))
    nrot = np.stack([c, s], 1).astype(np.float32)
    out[lost], nrot[lost] = boxes[lost], rot[lost]
    return out, nrot, lost.astype(np.int32)


TWO_PI = F(6.2831855)


def one_euro_host(x, dt, state=None, src_frame=None, lost=None, min_cutoff=1.0, beta=0.007, d_cutoff=1.0, dtype=np.float32):
    """One frame of the One-Euro filter, lh_one_euro in numpy: x [b][j][2], dt [b] (or a scalar) in seconds, state = (xhat, dxhat, init)
    of the previous frame (None: nothing seen yet), src_frame / lost [b] (None: every slot is live) -> (out [b][j][2], new state).
    The inputs are not modified."""
    T = np.dtype(dtype).type
    x = np.asarray(x, dtype)
    b = x.shape[0]
    dt = np.broadcast_to(np.asarray(dt, dtype), (b,)).reshape((b,) + (1,) * (x.ndim - 1))
    if state is None:
        state = (np.zeros_like(x), np.zeros_like(x), np.zeros(b, np.int32))
    xhat, dxhat, init = np.asarray(state[0], dtype), np.asarray(state[1], dtype), np.asarray(state[2], np.int32).reshape(b)
    away = np.zeros(b, bool)
    if src_frame is not None:
        away |= np.asarray(src_frame).reshape(b) < 0
    if lost is not None:
        away |= np.asarray(lost).reshape(b) != 0
    shape = (b,) + (1,) * (x.ndim - 1)
    with np.errstate(all="ignore"):
        fresh = ((init == 0).reshape(shape) | ~(dt > 0) | ~np.isfinite(dt))
        rd = (T(TWO_PI) * T(d_cutoff)) * dt
        ad = rd / (rd + T(1))
        dx = (x - xhat) / dt
        dxh = ad * dx + (T(1) - ad) * dxhat
        fc = T(min_cutoff) + T(beta) * np.abs(dxh)
        r = (T(TWO_PI) * fc) * dt
        al = r / (r + T(1))
        nx = al * x + (T(1) - al) * xhat
    aw = away.reshape(shape)
    new_xhat = np.where(aw, xhat, np.where(fresh, x, nx)).astype(dtype)
    new_dxhat = np.where(aw, dxhat, np.where(fresh, T(0), dxh)).astype(dtype)
    out = np.where(aw | fresh, x, nx).astype(dtype)
    return out, (new_xhat, new_dxhat, np.where(away, 0, 1).astype(np.int32))


def one_euro_host64(x, dt, state=None, src_frame=None, lost=None, min_cutoff=1.0, beta=0.007, d_cutoff=1.0):
    """one_euro_host's recurrence in fp64: what the fp32 order of operations is measured against."""
    return one_euro_host(x, dt, state, src_frame, lost, min_cutoff, beta, d_cutoff, dtype=np.float64)


GATE_OPEN = -3.0e38                  # gate_min_score that every finite maxval passes: lh_one_euro_gated is then lh_one_euro


def one_euro_gated_host(x, maxvals, dt, state=None, src_frame=None, lost=None, next_boxes=None, min_cutoff=1.0, beta=0.007, d_cutoff=1.0,
                        gate_min_score=GATE_OPEN, by_size=False, dtype=np.float32):
    """One frame of the gated One-Euro filter, lh_one_euro_gated in numpy (``dtype=np.float64``: the same recurrence in fp64): x
    [b][j][2], maxvals [b][j] or [b][j][1], dt [b] (or a scalar), state = (xhat, dxhat [b][j][2], seen_j int32 [b][j], gap [b][j]) of
    the previous frame (None: nothing seen yet), src_frame / lost [b] (None: every slot is live), next_boxes [b][4] (read with
    ``by_size``) -> (out [b][j][2], new state).  A joint with ``!(maxval >= gate_min_score)`` holds its filtered position and counts
    the seconds in ``gap``; on its return the update runs over T = gap + dt.  The inputs are not modified."""
    T = np.dtype(dtype).type
    x = np.asarray(x, dtype)
    b, j = x.shape[:2]
    mv = np.asarray(maxvals, dtype).reshape(b, j)
    dt = np.broadcast_to(np.asarray(dt, dtype), (b,)).reshape(b, 1)
    if state is None:
        state = (np.zeros_like(x), np.zeros_like(x), np.zeros((b, j), np.int32), np.zeros((b, j), dtype))
    xhat, dxhat = np.asarray(state[0], dtype), np.asarray(state[1], dtype)
    seen, gap = np.asarray(state[2], np.int32).reshape(b, j) != 0, np.asarray(state[3], dtype).reshape(b, j)
    away = np.zeros(b, bool)
    if src_frame is not None:
        away |= np.asarray(src_frame).reshape(b) < 0
    if lost is not None:
        away |= np.asarray(lost).reshape(b) != 0
    away = away.reshape(b, 1)
    size = T(1)
    if by_size:
        box = np.asarray(next_boxes, dtype).reshape(b, 4)
        size = np.fmax(np.fmax(box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]), T(1)).reshape(b, 1, 1)
    with np.errstate(all="ignore"):
        gin = mv >= T(gate_min_score)
        span = gap + dt
        fresh = ~seen | ~(span > 0) | ~np.isfinite(span)
        s3 = span[:, :, None]
        rd = (T(TWO_PI) * T(d_cutoff)) * s3
        ad = rd / (rd + T(1))
        dx = (x - xhat) / s3
        dxh = ad * dx + (T(1) - ad) * dxhat
        speed = np.abs(dxh) / size if by_size else np.abs(dxh)
        fc = T(min_cutoff) + T(beta) * speed
        r = (T(TWO_PI) * fc) * s3
        al = r / (r + T(1))
        nx = al * x + (T(1) - al) * xhat
        okdt = (dt > 0) & np.isfinite(dt)
        grown = np.where(okdt, gap + dt, gap)
    upd, start, hold = (~away & gin & ~fresh)[:, :, None], (~away & gin & fresh)[:, :, None], (~away & ~gin & seen)[:, :, None]
    new_xhat = np.where(upd, nx, np.where(start, x, xhat)).astype(dtype)
    new_dxhat = np.where(upd, dxh, np.where(start, T(0), dxhat)).astype(dtype)
    out = np.where(upd, nx, np.where(hold, xhat, x)).astype(dtype)
    new_seen = np.where(away, 0, np.where(gin, 1, seen)).astype(np.int32)
    new_gap = np.where(away | gin, T(0), grown).astype(dtype)
    return out, (new_xhat, new_dxhat, new_seen, new_gap)


MOTION_DEFAULTS = dict(cutoff=10.0, lead=1.0, max_shift=0.5, coast=0)


def rois_predict_host(next_boxes, lost, src_frame, seeded, dt, state=None, cutoff=10.0, lead=1.0, max_shift=0.5, coast=0, dtype=np.float32):
    """ROI velocity prediction and coasting, lh_rois_predict in numpy (``dtype=np.float64``: the same rule in fp64): next_boxes [b][4]
    as lh_keypoints_to_boxes / lh_keypoints_to_rois (and lh_tracks_manage) left them, lost / src_frame [b], seeded [b] or None, dt [b]
    (or a scalar), state = (centre [b][2], vel [b][2], seen int32 [b], coasted int32 [b]) of the previous frame (None: nothing seen
    yet) -> (the shifted boxes [b][4], new state).  The rule, clause by clause, is in include/lighthand_hip.h.  The inputs are not
    modified."""
    T = np.dtype(dtype).type
    box = np.asarray(next_boxes, dtype).reshape(-1, 4)
    b = box.shape[0]
    lost = np.asarray(lost).reshape(b) != 0
    dt = np.broadcast_to(np.asarray(dt, dtype), (b,)).reshape(b, 1)
    if state is None:
        state = (np.zeros((b, 2), dtype), np.zeros((b, 2), dtype), np.zeros(b, np.int32), np.zeros(b, np.int32))
    centre, vel = np.asarray(state[0], dtype).reshape(b, 2), np.asarray(state[1], dtype).reshape(b, 2)
    seen, coasted = np.asarray(state[2], np.int32).reshape(b) != 0, np.asarray(state[3], np.int32).reshape(b)
    bw, bh = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    reset = (np.asarray(src_frame).reshape(b) < 0) | ~((bw > 0) & (bh > 0))
    if seeded is not None:
        reset |= np.asarray(seeded).reshape(b) >= 0
    with np.errstate(all="ignore"):
        okdt = ((dt > 0) & np.isfinite(dt)).reshape(b)
        lim = (T(max_shift) * np.fmax(bw, bh)).reshape(b, 1)
        coasting = ~reset & lost & seen & okdt & (coasted < int(coast))
        forget = ~reset & lost & ~coasting
        found = ~reset & ~lost
        fresh = found & (~seen | ~okdt)
        c = np.stack([(box[:, 0] + box[:, 2]) * T(0.5), (box[:, 1] + box[:, 3]) * T(0.5)], 1)
        vm = (c - centre) / dt
        r = (T(TWO_PI) * T(cutoff)) * dt
        al = r / (r + T(1))
        nv = al * vm + (T(1) - al) * vel
        bad = found & ~fresh & ~np.isfinite(nv).all(1)
        good = found & ~fresh & ~bad
        s_coast = np.fmin(np.fmax(vel * dt, -lim), lim)
        s_lead = np.fmin(np.fmax((T(lead) * nv) * dt, -lim), lim)
        s = np.where(coasting[:, None], s_coast, s_lead)
        moved = (coasting | good)[:, None]
        out = np.where(np.tile(moved, (1, 4)), box + np.tile(s, (1, 2)), box).astype(dtype)
        new_centre = np.where(coasting[:, None], centre + s_coast, np.where(found[:, None], c, centre)).astype(dtype)
    new_vel = np.where((reset | forget | fresh | bad)[:, None], T(0), np.where(good[:, None], nv, vel)).astype(dtype)
    new_seen = np.where(reset | forget, 0, np.where(found, 1, seen)).astype(np.int32)
    new_coasted = np.where(reset | found, 0, np.where(coasting, coasted + 1, coasted)).astype(np.int32)
    return out, (new_centre, new_vel, new_seen, new_coasted)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def box_affine(boxes, frame_index, n_frames, size, padding=1.25):
    """Device tensors boxes fp32 [b][4], frame_index int32 [b] -> (mat fp32 [b][6], src_frame int32 [b]) for an h x w = ``size`` crop
    (one lh_box_affine launch on the current stream)."""
    import torch
    from . import _lib
    if not padding > 0:
        raise ValueError(f"padding must be > 0, not {padding!r}")
    boxes = boxes.to(torch.float32).contiguous()
    frame_index = frame_index.to(torch.int32).contiguous()
    b = boxes.shape[0]
    if tuple(boxes.shape) != (b, 4) or tuple(frame_index.shape) != (b,) or not boxes.is_cuda or frame_index.device != boxes.device:
        raise _lib.LightHandError(f"box_affine: boxes [b, 4] and frame_index [b] on one device, got {tuple(boxes.shape)} / {tuple(frame_index.shape)}")
    mat = torch.empty(b, 6, dtype=torch.float32, device=boxes.device)
    src = torch.empty(b, dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        _lib.check(_lib.load().lh_box_affine(boxes.data_ptr(), frame_index.data_ptr(), b, int(n_frames), int(size[0]), int(size[1]),
                                             float(padding), mat.data_ptr(), src.data_ptr(), _stream()), "lh_box_affine")
    return mat, src


def check_surface(t, device, layout):
    """One surface of a step or launch on ``device`` whose frames have ``layout`` (a Yuv420Layout): a contiguous uint8 device tensor of
    at least surface_bytes(layout) bytes, 2-byte aligned where the samples are 16-bit -> its address; ValueError otherwise."""
    import torch
    need = surface_bytes(layout)
    if not torch.is_tensor(t) or not t.is_cuda or t.device != torch.device(device):
        raise ValueError(f"a surface is a uint8 tensor on {device}, not {type(t).__name__ if not torch.is_tensor(t) else t.device}")
    if t.dtype != torch.uint8 or not t.is_contiguous():
        raise ValueError(f"a surface is a contiguous uint8 tensor, not {t.dtype} with strides {tuple(t.stride())}")
    if t.numel() < need:
        raise ValueError(f"a surface holds at least {need} bytes (topdown.surface_bytes), not {t.numel()}")
    if layout.sample_bytes == 2 and t.data_ptr() % 2:
        raise ValueError("a surface of 16-bit samples must be 2-byte aligned")
    return t.data_ptr()


def surface_table(surfaces, layout, device):
    """A sequence of surfaces (check_surface's rules; None: an unbound frame, entry 0), or one tensor [k][...] taken row by row ->
    (int64 device tensor [k] of their addresses, the list of tensors to keep alive): the table lh_frames_crop_surfaces_to_nhwc4 reads."""
    import torch
    seq = list(surfaces.unbind(0)) if torch.is_tensor(surfaces) else list(surfaces)
    if not seq:
        raise ValueError("surfaces is empty")
    addresses = [0 if t is None else check_surface(t, device, layout) for t in seq]
    return torch.tensor(addresses, dtype=torch.int64).to(device), [t for t in seq if t is not None]


def through_descriptor(frame_format, layout, surfaces):
    """Whether a crop finds its samples through the plane descriptor (crop_entry's ``desc``): surfaces in place of a frame buffer, the
    formats only the descriptor covers, or "nv12" with a Yuv420Layout."""
    return bool(surfaces) or frame_format not in ("rgb", "nv12") or isinstance(layout, Yuv420Layout)


def crop_entry(lib, frame_format, max_taps, frames, out, b, n_frames, hs, ws, h, w, pad, wp, m3, s3, mat, src_frame, dtype_code, desc=None,
               frame_stride=0, table=None, nv12=None, jit=None, plain=False):
    """Which of the five C crop entries a launch is -> (the function of ``lib``, its arguments without the stream, a description): the
    choice frames_crop and engine.Plan.use_frame_input share.  Pointers are addresses (or None), m3 / s3 the float[3] of Normalize.
    The first match wins: ``desc`` (an lh_frames_layout: the descriptor path -- surfaces, nv21 / yuv420p / p010, or a Yuv420Layout;
    ``frames`` + ``frame_stride`` or ``table`` is its source) -> lh_frames_crop_surfaces_to_nhwc4, with or without jitter; ``jit`` =
    (factors, order, workspace) -> lh_frames_crop_jitter_to_nhwc4; ``nv12`` = (pitch, uv_offset, frame_stride, siting, csc12) ->
    lh_frames_crop_yuv_to_nhwc4; ``max_taps`` > 1 -> lh_frames_crop_area_to_nhwc4; otherwise the area entry again, or with ``plain``
    (the plan's rule) lh_frames_crop_to_nhwc4."""
    import ctypes as C
    geometry = (h, w, pad, wp, m3, s3, mat, src_frame)
    taps = ", antialiased" if max_taps > 1 else ""
    if desc is not None:
        return (lib.lh_frames_crop_surfaces_to_nhwc4,
                (frames, out, frame_stride, table, C.byref(desc), b, n_frames, hs, ws) + geometry + (max_taps,) + (jit or (None, None, None))
                + (dtype_code,),
                f"{frame_format} frame crop input pipeline" + (", surface table" if table is not None else "") + taps
                + (" + ColorJitter" if jit else ""))
    head = (frames, out, b, n_frames, hs, ws)
    what = "NV12 frame crop input pipeline" if nv12 else "frame crop input pipeline"
    if jit:
        return (lib.lh_frames_crop_jitter_to_nhwc4, head + (nv12 or (0, 0, 0, 0, None)) + geometry + (max_taps,) + jit + (dtype_code,),
                what + taps + " + ColorJitter")
    if nv12:
        return lib.lh_frames_crop_yuv_to_nhwc4, head + nv12 + geometry + (max_taps, dtype_code), what + taps
    if max_taps > 1 or not plain:
        return lib.lh_frames_crop_area_to_nhwc4, head + geometry + (max_taps, dtype_code), ("antialiased " if max_taps > 1 else "") + what
    return lib.lh_frames_crop_to_nhwc4, head + geometry + (dtype_code,), what


def frames_crop(frames, mat, src_frame, size, max_taps=1, dtype=None, mean=MEAN, std=STD, frame_format="rgb", frame_size=None,
                yuv=("bt709", "limited"), chroma_siting="left", layout=None, jitter=None, surfaces=None):
    """Device tensors frames uint8 [n][hs][ws][3], mat fp32 [b][6], src_frame int32 [b] -> the normalised crops as NHWC4
    [b][h][w][4] of ``dtype`` (torch.float32 by default; no padding, channel 3 is 0) for an h x w = ``size`` crop: one
    lh_frames_crop_area_to_nhwc4 launch on the current stream.  ``max_taps`` 1..8: the most samples per crop pixel and axis that a
    minified ROI averages (crop_taps_host); 1 is the plain crop.  ``frame_format="nv12"``: frames uint8 [n][rows][pitch] of
    ``frame_size`` = (hs, ws) in ``layout`` (nv12_layout's tuple; None: tight), converted per sample with ``yuv`` ((standard, range)
    or 12 coefficients) and ``chroma_siting`` ("left" / "center"): one lh_frames_crop_yuv_to_nhwc4 launch.  ``jitter=(factors, order)``
    (device tensors fp32 [b][4] and int32 [b][4], runtime.sample_color_jitter's draw): ColorJitter between the sample and Normalize,
    lh_frames_crop_jitter_to_nhwc4 for either format (the grey-mean launch, then the crop).
    ``frame_format`` "nv21" / "yuv420p" / "p010" (or "nv12" with a Yuv420Layout): frames uint8 [n][frame_bytes] in ``layout``
    (frame_layout_of's rules), one lh_frames_crop_surfaces_to_nhwc4 launch, with or without ``jitter``.  ``surfaces=`` in place of
    ``frames`` (which is then None), for every format: a sequence of uint8 device tensors, one per frame and each a frame in place
    (None: an unbound frame, its slots are black), read through a surface table by the same entry; ``frame_size`` is needed."""
    import ctypes as C
    import torch
    from . import _lib
    if isinstance(max_taps, bool) or not isinstance(max_taps, int) or not 1 <= max_taps <= 8:
        raise ValueError(f"max_taps must be an integer 1..8, not {max_taps!r}")
    check_frame_format(frame_format)
    dtype = dtype or torch.float32
    descriptor = through_descriptor(frame_format, layout, surfaces is not None)
    if (frames is None) == (surfaces is None):
        raise ValueError("frames_crop: pass frames (one buffer) or surfaces= (one tensor per frame), one of the two")
    if not descriptor:
        frames = frames.contiguous()
    mat = mat.to(torch.float32).contiguous()
    src_frame = src_frame.to(torch.int32).contiguous()
    b = mat.shape[0]
    jit = None
    if jitter is not None:
        factors, order = (t.contiguous() for t in jitter)
        if (factors.dtype != torch.float32 or order.dtype != torch.int32 or tuple(factors.shape) != (b, 4) or tuple(order.shape) != (b, 4)
                or factors.device != mat.device or order.device != mat.device or not mat.is_cuda):
            raise _lib.LightHandError(f"frames_crop: jitter = (factors fp32 [b, 4], order int32 [b, 4]) on the crop's device, got "
                                      f"{tuple(factors.shape)} {factors.dtype} / {tuple(order.shape)} {order.dtype}")
        ws_j = torch.empty(max(1, _lib.load().lh_frames_crop_jitter_workspace_bytes(b) // 8), dtype=torch.float64, device=mat.device)
        jit = (factors.data_ptr(), order.data_ptr(), ws_j.data_ptr())
    desc = table = nv12 = None
    frame_stride, keep = 0, ()
    if descriptor:
        if tuple(mat.shape) != (b, 6) or tuple(src_frame.shape) != (b,) or not mat.is_cuda or src_frame.device != mat.device:
            raise _lib.LightHandError(f"frames_crop: mat [b, 6] and src_frame [b] on one device, got {tuple(mat.shape)} / {tuple(src_frame.shape)}")
        if surfaces is None and frame_format == "rgb" and frame_size is None and frames.dim() == 4:
            frame_size = tuple(frames.shape[1:3])
        if not (isinstance(frame_size, (tuple, list)) and len(frame_size) == 2):
            raise ValueError(f"frames_crop: frame_size=(hs, ws) is needed, not {frame_size!r}")
        hs, ws = int(frame_size[0]), int(frame_size[1])
        L = frame_layout_of(frame_format, hs, ws, layout)
        desc = frames_layout_struct(L, yuv, chroma_siting)
        device = mat.device
        if surfaces is not None:
            table_dev, keep = surface_table(surfaces, L, device)
            table, n = table_dev.data_ptr(), table_dev.shape[0]
        else:
            if not frames.is_cuda or frames.device != mat.device or frames.dtype != torch.uint8 or frames.dim() < 2 or not frames.is_contiguous():
                raise _lib.LightHandError(f"frames_crop: frames contiguous uint8 [n, ...] on the crop's device, got {tuple(frames.shape)} {frames.dtype}")
            n, frame_stride = frames.shape[0], frames.stride(0)
    elif frame_format == "nv12":
        if not (isinstance(frame_size, (tuple, list)) and len(frame_size) == 2):
            raise ValueError(f"frame_format='nv12' needs frame_size=(hs, ws), not {frame_size!r}")
        hs, ws = int(frame_size[0]), int(frame_size[1])
        pitch, uv_offset, stride, rows = check_nv12_layout(hs, ws, layout)
        nv12 = (pitch, uv_offset, stride, chroma_siting_code(chroma_siting), (C.c_float * 12)(*csc12(yuv).tolist()))
        if (frames.dtype != torch.uint8 or tuple(frames.shape[1:]) != (rows, pitch) or frames.dim() != 3 or tuple(mat.shape) != (b, 6)
                or tuple(src_frame.shape) != (b,) or not frames.is_cuda or mat.device != frames.device or src_frame.device != frames.device):
            raise _lib.LightHandError(f"frames_crop: NV12 frames uint8 [n, {rows}, {pitch}], mat [b, 6] and src_frame [b] on one device, got "
                                      f"{tuple(frames.shape)} {frames.dtype} / {tuple(mat.shape)} / {tuple(src_frame.shape)}")
        n, device = frames.shape[0], frames.device
    else:
        if (frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or tuple(mat.shape) != (b, 6) or tuple(src_frame.shape) != (b,)
                or not frames.is_cuda or mat.device != frames.device or src_frame.device != frames.device):
            raise _lib.LightHandError(f"frames_crop: frames uint8 [n, hs, ws, 3], mat [b, 6] and src_frame [b] on one device, got "
                                      f"{tuple(frames.shape)} {frames.dtype} / {tuple(mat.shape)} / {tuple(src_frame.shape)}")
        (n, hs, ws), device = frames.shape[:3], frames.device
    h, w = int(size[0]), int(size[1])
    out = torch.empty(b, h, w, 4, dtype=dtype, device=device)
    m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    fn, args, _ = crop_entry(_lib.load(), frame_format, max_taps, None if surfaces is not None else frames.data_ptr(), out.data_ptr(), b, n, hs, ws,
                             h, w, 0, w, m3, s3, mat.data_ptr(), src_frame.data_ptr(), _lib.dtype_code(dtype), desc=desc,
                             frame_stride=frame_stride, table=table, nv12=nv12, jit=jit)
    with torch.cuda.device(device):
        _lib.check(fn(*args, _stream()), fn.__name__)
    for t in keep:                                                 # the launch is queued: the allocator must not hand the surfaces out before it ran
        t.record_stream(torch.cuda.current_stream())
    return out


def boxes_from_keypoints(preds, maxvals, boxes, src_frame, min_score=0.1, min_joints=8, min_side=16.0):
    """Device tensors preds fp32 [b][j][2] (frame coordinates), maxvals [b][j] or [b][j][1], boxes [b][4], src_frame int32 [b] ->
    (next_boxes fp32 [b][4], lost int32 [b]) (one lh_keypoints_to_boxes launch on the current stream)."""
    import torch
    from . import _lib
    preds = preds.to(torch.float32).contiguous()
    b, j = preds.shape[:2]
    maxvals = maxvals.to(torch.float32).reshape(b, j).contiguous()
    boxes = boxes.to(torch.float32).contiguous()
    src_frame = src_frame.to(torch.int32).contiguous()
    if tuple(preds.shape) != (b, j, 2) or tuple(boxes.shape) != (b, 4) or tuple(src_frame.shape) != (b,) or not preds.is_cuda:
        raise _lib.LightHandError(f"boxes_from_keypoints: preds [b, j, 2], boxes [b, 4], src_frame [b] on the device, got "
                                  f"{tuple(preds.shape)} / {tuple(boxes.shape)} / {tuple(src_frame.shape)}")
    nxt = torch.empty(b, 4, dtype=torch.float32, device=preds.device)
    lost = torch.empty(b, dtype=torch.int32, device=preds.device)
    with torch.cuda.device(preds.device):
        _lib.check(_lib.load().lh_keypoints_to_boxes(preds.data_ptr(), maxvals.data_ptr(), boxes.data_ptr(), src_frame.data_ptr(), b, j,
                                                     float(min_score), int(min_joints), float(min_side), nxt.data_ptr(), lost.data_ptr(),
                                                     _stream()), "lh_keypoints_to_boxes")
    return nxt, lost


def roi_affine(boxes, rot, mirror, frame_index, n_frames, size, padding=1.25):
    """Device tensors boxes fp32 [b][4], rot fp32 [b][2], mirror int32 [b], frame_index int32 [b] -> (mat fp32 [b][6], src_frame int32
    [b]) for an h x w = ``size`` crop (one lh_roi_affine launch on the current stream)."""
    import torch
    from . import _lib
    if not padding > 0:
        raise ValueError(f"padding must be > 0, not {padding!r}")
    boxes = boxes.to(torch.float32).contiguous()
    rot = rot.to(torch.float32).contiguous()
    mirror = mirror.to(torch.int32).contiguous()
    frame_index = frame_index.to(torch.int32).contiguous()
    b = boxes.shape[0]
    if (tuple(boxes.shape) != (b, 4) or tuple(rot.shape) != (b, 2) or tuple(mirror.shape) != (b,) or tuple(frame_index.shape) != (b,)
            or not boxes.is_cuda or any(t.device != boxes.device for t in (rot, mirror, frame_index))):
        raise _lib.LightHandError(f"roi_affine: boxes [b, 4], rot [b, 2], mirror [b] and frame_index [b] on one device, got "
                                  f"{tuple(boxes.shape)} / {tuple(rot.shape)} / {tuple(mirror.shape)} / {tuple(frame_index.shape)}")
    mat = torch.empty(b, 6, dtype=torch.float32, device=boxes.device)
    src = torch.empty(b, dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        _lib.check(_lib.load().lh_roi_affine(boxes.data_ptr(), rot.data_ptr(), mirror.data_ptr(), frame_index.data_ptr(), b, int(n_frames),
                                             int(size[0]), int(size[1]), float(padding), mat.data_ptr(), src.data_ptr(), _stream()),
                   "lh_roi_affine")
    return mat, src


def roi_perturb(boxes, rot, mirror, aug):
    """Device tensors boxes fp32 [b][4], rot fp32 [b][2] or None (= (1, 0)), mirror int32 [b] or None (= 0), aug fp32 [b][6] =
    (c, s, k, tx, ty, flip) (runtime.sample_roi_aug) -> (boxes' fp32 [b][4], rot' fp32 [b][2], mirror' int32 [b]), the ROI the crop of
    an augmented training step uses (one lh_roi_perturb launch on the current stream)."""
    import torch
    from . import _lib
    boxes = boxes.to(torch.float32).contiguous()
    aug = aug.to(torch.float32).contiguous()
    rot = None if rot is None else rot.to(torch.float32).contiguous()
    mirror = None if mirror is None else mirror.to(torch.int32).contiguous()
    b = boxes.shape[0]
    if (tuple(boxes.shape) != (b, 4) or tuple(aug.shape) != (b, 6) or (rot is not None and tuple(rot.shape) != (b, 2))
            or (mirror is not None and tuple(mirror.shape) != (b,)) or not boxes.is_cuda
            or any(t is not None and t.device != boxes.device for t in (rot, mirror, aug))):
        raise _lib.LightHandError(f"roi_perturb: boxes [b, 4], rot [b, 2] or None, mirror [b] or None and aug [b, 6] on one device, got "
                                  f"{tuple(boxes.shape)} / {None if rot is None else tuple(rot.shape)} / "
                                  f"{None if mirror is None else tuple(mirror.shape)} / {tuple(aug.shape)}")
    nbox = torch.empty(b, 4, dtype=torch.float32, device=boxes.device)
    nrot = torch.empty(b, 2, dtype=torch.float32, device=boxes.device)
    nmir = torch.empty(b, dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        _lib.check(_lib.load().lh_roi_perturb(boxes.data_ptr(), None if rot is None else rot.data_ptr(),
                                              None if mirror is None else mirror.data_ptr(), aug.data_ptr(), b, nbox.data_ptr(),
                                              nrot.data_ptr(), nmir.data_ptr(), _stream()), "lh_roi_perturb")
    return nbox, nrot, nmir


def affine_points_inv(pts, mat, src_frame):
    """Device tensors pts fp32 [b][j][>=2] (frame coordinates; further columns are ignored), mat fp32 [b][6] (crop -> frame), src_frame
    int32 [b] -> crop coordinates fp32 [b][j][2] (one lh_affine_points_inv launch on the current stream); POINT_OFF for the points of a
    slot that is empty or whose matrix has no inverse."""
    import torch
    from . import _lib
    pts = pts.to(torch.float32).contiguous()
    mat = mat.to(torch.float32).contiguous()
    src_frame = src_frame.to(torch.int32).contiguous()
    if pts.dim() != 3 or pts.shape[2] < 2 or pts.shape[0] < 1 or pts.shape[1] < 1:
        raise _lib.LightHandError(f"affine_points_inv: pts [b, j, >= 2], got {tuple(pts.shape)}")
    b, j, stride = pts.shape
    if tuple(mat.shape) != (b, 6) or tuple(src_frame.shape) != (b,) or not pts.is_cuda or mat.device != pts.device or src_frame.device != pts.device:
        raise _lib.LightHandError(f"affine_points_inv: pts [b, j, >= 2], mat [b, 6] and src_frame [b] on one device, got "
                                  f"{tuple(pts.shape)} / {tuple(mat.shape)} / {tuple(src_frame.shape)}")
    out = torch.empty(b, j, 2, dtype=torch.float32, device=pts.device)
    with torch.cuda.device(pts.device):
        _lib.check(_lib.load().lh_affine_points_inv(pts.data_ptr(), stride, mat.data_ptr(), src_frame.data_ptr(), out.data_ptr(), 2, b, j,
                                                    _stream()), "lh_affine_points_inv")
    return out


def rois_from_keypoints(preds, maxvals, boxes, rot, src_frame, axis=(0, 9), min_score=0.1, min_joints=8, min_side=16.0, min_axis=4.0):
    """Device tensors preds fp32 [b][j][2] (frame coordinates), maxvals [b][j] or [b][j][1], boxes [b][4], rot [b][2], src_frame int32
    [b] -> (next_boxes fp32 [b][4], next_rot fp32 [b][2], lost int32 [b]) (one lh_keypoints_to_rois launch on the current stream)."""
    import torch
    from . import _lib
    preds = preds.to(torch.float32).contiguous()
    b, j = preds.shape[:2]
    maxvals = maxvals.to(torch.float32).reshape(b, j).contiguous()
    boxes = boxes.to(torch.float32).contiguous()
    rot = rot.to(torch.float32).contiguous()
    src_frame = src_frame.to(torch.int32).contiguous()
    if (tuple(preds.shape) != (b, j, 2) or tuple(boxes.shape) != (b, 4) or tuple(rot.shape) != (b, 2) or tuple(src_frame.shape) != (b,)
            or not preds.is_cuda):
        raise _lib.LightHandError(f"rois_from_keypoints: preds [b, j, 2], boxes [b, 4], rot [b, 2], src_frame [b] on the device, got "
                                  f"{tuple(preds.shape)} / {tuple(boxes.shape)} / {tuple(rot.shape)} / {tuple(src_frame.shape)}")
    nxt = torch.empty(b, 4, dtype=torch.float32, device=preds.device)
    nrot = torch.empty(b, 2, dtype=torch.float32, device=preds.device)
    lost = torch.empty(b, dtype=torch.int32, device=preds.device)
    with torch.cuda.device(preds.device):
        _lib.check(_lib.load().lh_keypoints_to_rois(preds.data_ptr(), maxvals.data_ptr(), boxes.data_ptr(), rot.data_ptr(), src_frame.data_ptr(),
                                                    b, j, int(axis[0]), int(axis[1]), float(min_score), int(min_joints), float(min_side),
                                                    float(min_axis), nxt.data_ptr(), nrot.data_ptr(), lost.data_ptr(), _stream()),
                   "lh_keypoints_to_rois")
    return nxt, nrot, lost


def one_euro(x, dt, state, src_frame, lost=None, min_cutoff=1.0, beta=0.007, d_cutoff=1.0, out=None):
    """One frame of the One-Euro filter on device tensors: x fp32 [b][j][2], dt fp32 [b], state = (xhat, dxhat fp32 [b][j][2], init int32
    [b]) UPDATED IN PLACE (fresh state: zeros), src_frame int32 [b], lost int32 [b] or None -> out fp32 [b][j][2] (one lh_one_euro
    launch on the current stream)."""
    import torch
    from . import _lib
    xhat, dxhat, init = state
    b, j = x.shape[:2]
    good = (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (b, j, 2)
            and all(t.dtype == torch.float32 and t.is_contiguous() and t.shape == x.shape and t.device == x.device for t in (xhat, dxhat))
            and all(t is None or (t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (b,) and t.device == x.device)
                    for t in (init, src_frame, lost))
            and dt.dtype == torch.float32 and dt.is_contiguous() and tuple(dt.shape) == (b,) and dt.device == x.device)
    if not good or init is None or src_frame is None:
        raise _lib.LightHandError("one_euro: x, xhat, dxhat contiguous fp32 [b, j, 2], dt fp32 [b], init / src_frame / lost int32 [b], on one device")
    if out is None:
        out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().lh_one_euro(x.data_ptr(), src_frame.data_ptr(), lost.data_ptr() if lost is not None else None, dt.data_ptr(),
                                           b, j, float(min_cutoff), float(beta), float(d_cutoff), xhat.data_ptr(), dxhat.data_ptr(),
                                           init.data_ptr(), out.data_ptr(), _stream()), "lh_one_euro")
    return out


def manage_tracks(preds, maxvals, src_frame, frame_index, n_frames, next_boxes, next_rot, lost, lost_count, det_boxes, det_frame, det_score,
                  dup_of, seeded, det_state, min_score=0.1, min_side=16.0, dup_overlap=0.5, match_overlap=0.5, det_min_score=0.0, max_lost=0):
    """One lh_tracks_manage launch on the current stream, on contiguous device tensors: preds fp32 [b][j][2], maxvals fp32 [b][j] or
    [b][j][1], src_frame / frame_index int32 [b], the detection list det_boxes fp32 [k][4], det_frame int32 [k], det_score fp32 [k];
    next_boxes fp32 [b][4], next_rot fp32 [b][2] or None, lost / lost_count int32 [b] are UPDATED IN PLACE, dup_of / seeded int32 [b] and
    det_state int32 [k] are written (a slot of no frame keeps what they held).  The rule: manage_tracks_host."""
    import torch
    from . import _lib
    b, j = preds.shape[:2]
    k = det_boxes.shape[0]
    f32 = [(preds, (b, j, 2)), (next_boxes, (b, 4)), (det_boxes, (k, 4)), (det_score, (k,))] + ([(next_rot, (b, 2))] if next_rot is not None else [])
    i32 = [(t, (b,)) for t in (src_frame, frame_index, lost, lost_count, dup_of, seeded)] + [(det_frame, (k,)), (det_state, (k,))]
    good = (preds.is_cuda and maxvals.dtype == torch.float32 and maxvals.is_contiguous() and maxvals.numel() == b * j and maxvals.device == preds.device
            and all(t.dtype == torch.float32 and tuple(t.shape) == shape for t, shape in f32)
            and all(t.dtype == torch.int32 and tuple(t.shape) == shape for t, shape in i32)
            and all(t.is_contiguous() and t.device == preds.device for t, _ in f32 + i32))
    if not good:
        raise _lib.LightHandError("manage_tracks: contiguous tensors on one device -- fp32 preds [b, j, 2], maxvals [b, j], next_boxes [b, 4], "
                                  "next_rot [b, 2] or None, det_boxes [k, 4], det_score [k]; int32 src_frame, frame_index, lost, lost_count, "
                                  "dup_of, seeded [b], det_frame, det_state [k]")
    with torch.cuda.device(preds.device):
        _lib.check(_lib.load().lh_tracks_manage(preds.data_ptr(), maxvals.data_ptr(), src_frame.data_ptr(), frame_index.data_ptr(), b, j,
                                                int(n_frames), det_boxes.data_ptr(), det_frame.data_ptr(), det_score.data_ptr(), k,
                                                float(min_score), float(min_side), float(dup_overlap), float(match_overlap),
                                                float(det_min_score), int(max_lost), next_boxes.data_ptr(),
                                                None if next_rot is None else next_rot.data_ptr(), lost.data_ptr(), lost_count.data_ptr(),
                                                dup_of.data_ptr(), seeded.data_ptr(), det_state.data_ptr(), _stream()), "lh_tracks_manage")
    return next_boxes, next_rot, lost, lost_count, dup_of, seeded, det_state


def rois_predict(next_boxes, lost, src_frame, seeded, dt, state, cutoff=10.0, lead=1.0, max_shift=0.5, coast=0):
    """One lh_rois_predict launch on the current stream, on contiguous device tensors: next_boxes fp32 [b][4] and state = (centre fp32
    [b][2], vel fp32 [b][2], seen int32 [b], coasted int32 [b]) are UPDATED IN PLACE (fresh state: zeros); lost / src_frame int32 [b],
    seeded int32 [b] or None and dt fp32 [b] are read.  The rule: rois_predict_host."""
    import torch
    from . import _lib
    centre, vel, seen, coasted = state
    b = next_boxes.shape[0]
    f32 = [(next_boxes, (b, 4)), (centre, (b, 2)), (vel, (b, 2)), (dt, (b,))]
    i32 = [(t, (b,)) for t in (lost, src_frame, seen, coasted) + ((seeded,) if seeded is not None else ())]
    good = (next_boxes.is_cuda and all(torch.is_tensor(t) and t.dtype == torch.float32 and tuple(t.shape) == shape for t, shape in f32)
            and all(torch.is_tensor(t) and t.dtype == torch.int32 and tuple(t.shape) == shape for t, shape in i32)
            and all(t.is_contiguous() and t.device == next_boxes.device for t, _ in f32 + i32))
    if not good:
        raise _lib.LightHandError("rois_predict: contiguous tensors on one device -- fp32 next_boxes [b, 4], centre, vel [b, 2], dt [b]; int32 lost, "
                                  "src_frame, seen, coasted [b], seeded [b] or None")
    with torch.cuda.device(next_boxes.device):
        _lib.check(_lib.load().lh_rois_predict(next_boxes.data_ptr(), lost.data_ptr(), src_frame.data_ptr(),
                                               None if seeded is None else seeded.data_ptr(), dt.data_ptr(), b, float(cutoff), float(lead),
                                               float(max_shift), int(coast), centre.data_ptr(), vel.data_ptr(), seen.data_ptr(),
                                               coasted.data_ptr(), _stream()), "lh_rois_predict")
    return next_boxes


def one_euro_gated(x, maxvals, dt, state, src_frame, lost=None, next_boxes=None, min_cutoff=1.0, beta=0.007, d_cutoff=1.0,
                   gate_min_score=GATE_OPEN, by_size=False, out=None):
    """One frame of the gated One-Euro filter on device tensors: x fp32 [b][j][2], maxvals fp32 [b][j] or [b][j][1], dt fp32 [b], state =
    (xhat, dxhat fp32 [b][j][2], seen_j int32 [b][j], gap fp32 [b][j]) UPDATED IN PLACE (fresh state: zeros), src_frame int32 [b], lost
    int32 [b] or None, next_boxes fp32 [b][4] (needed with ``by_size``) -> out fp32 [b][j][2] (one lh_one_euro_gated launch on the current
    stream).  The rule: one_euro_gated_host."""
    import torch
    from . import _lib
    xhat, dxhat, seen_j, gap = state
    b, j = x.shape[:2]
    f32 = [(x, (b, j, 2)), (xhat, (b, j, 2)), (dxhat, (b, j, 2)), (gap, (b, j)), (dt, (b,))] + ([(next_boxes, (b, 4))] if next_boxes is not None else [])
    i32 = [(seen_j, (b, j)), (src_frame, (b,))] + ([(lost, (b,))] if lost is not None else [])
    good = (x.is_cuda and torch.is_tensor(maxvals) and maxvals.dtype == torch.float32 and maxvals.is_contiguous() and maxvals.numel() == b * j
            and maxvals.device == x.device and (next_boxes is not None or not by_size)
            and all(torch.is_tensor(t) and t.dtype == torch.float32 and tuple(t.shape) == shape for t, shape in f32)
            and all(torch.is_tensor(t) and t.dtype == torch.int32 and tuple(t.shape) == shape for t, shape in i32)
            and all(t.is_contiguous() and t.device == x.device for t, _ in f32 + i32))
    if not good:
        raise _lib.LightHandError("one_euro_gated: contiguous tensors on one device -- fp32 x, xhat, dxhat [b, j, 2], maxvals, gap [b, j], dt [b], "
                                  "next_boxes [b, 4] (needed with by_size); int32 seen_j [b, j], src_frame [b], lost [b] or None")
    if out is None:
        out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().lh_one_euro_gated(x.data_ptr(), maxvals.data_ptr(), None if next_boxes is None else next_boxes.data_ptr(),
                                                 src_frame.data_ptr(), None if lost is None else lost.data_ptr(), dt.data_ptr(), b, j,
                                                 float(min_cutoff), float(beta), float(d_cutoff), float(gate_min_score), int(bool(by_size)),
                                                 xhat.data_ptr(), dxhat.data_ptr(), seen_j.data_ptr(), gap.data_ptr(), out.data_ptr(), _stream()),
                   "lh_one_euro_gated")
    return out
