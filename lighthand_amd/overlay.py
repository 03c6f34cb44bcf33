"""The skeleton overlay of the tracked top-down step (lh_draw_hands, runtime.ManagedInferStep(frames=..., overlay=...)): the tracked
hands -- ROI outline, bones, joint discs -- drawn into the frames in place, on the pixels around each hand only.  ``draw_hands`` is the
launch on device tensors, ``draw_hands_host`` its rule in numpy (fp32 in the kernel's order, or fp64 with ``dtype=np.float64``),
``overlay_palette`` the host conversion of an RGB palette into the frames' own plane space, ``HAND_PARENTS`` / ``HAND_GROUPS`` /
``HAND_PALETTE_RGB`` / ``OVERLAY_DEFAULTS`` the defaults.  topdown.py imports every public name here.

The topology is data: ``parents`` int32 [j] (-1: no bone) and ``groups`` int32 [j] (the palette row of joint i and of the bone that ends
in i); the palette is fp32 [n_groups + 2][3], its last two rows the ROI outline of a live and of a lost slot.  Chroma siting is
ignored: a chroma texel takes the mean coverage of the 2 x 2 luma block it spans."""
import numpy as np

from .frame_formats import _yuv_matrix64, check_frame_format, csc12, frame_layout_of, frames_layout_struct, surface_bytes

HAND_PARENTS = (-1, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15, 0, 17, 18, 19)          # wrist, then four joints per finger
HAND_GROUPS = (0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5)
# wrist, thumb .. little finger, then the ROI outline of a live and of a lost slot
HAND_PALETTE_RGB = ((255, 255, 255), (255, 128, 0), (255, 220, 0), (0, 200, 80), (0, 160, 255), (200, 80, 255), (0, 255, 0), (255, 0, 0))
OVERLAY_DEFAULTS = dict(min_score=0.1, line_radius=1.0, joint_radius=2.5, by_size=0.0, opacity=1.0, draw_roi=True, source="raw",
                        target="inplace", parents=None, groups=None, palette=None)
_NUMBERS = ("min_score", "line_radius", "joint_radius", "by_size", "opacity")


def overlay_palette(rgb_rows=HAND_PALETTE_RGB, frame_format="rgb", yuv=("bt709", "limited")):
    """RGB rows on 0..255 -> float32 [rows][3] in the plane space of ``frame_format``: the rows themselves for "rgb", Y Cb Cr on the
    8-bit scale for the 4:2:0 formats and on the 10-bit scale for "p010" -- yuv = k^-1 rgb + o of ``yuv``'s matrix ((standard, range)
    or 12 coefficients), the forward matrix of rgb_to_yuv420_host, in fp64 and rounded once.  The kernel never converts colours."""
    check_frame_format(frame_format)
    try:
        rgb = np.asarray(rgb_rows, np.float64)
    except (TypeError, ValueError):
        rgb = np.zeros(0)
    if rgb.ndim != 2 or rgb.shape[1:] != (3,) or rgb.shape[0] < 1 or not np.isfinite(rgb).all():
        raise ValueError(f"overlay_palette: rgb_rows is [rows][3] finite numbers, not {rgb_rows!r}")
    if frame_format == "rgb":
        return rgb.astype(np.float32)
    bits = 10 if frame_format == "p010" else 8
    if isinstance(yuv, (tuple, list)) and len(yuv) == 2 and all(isinstance(v, str) for v in yuv):
        k, o = _yuv_matrix64(yuv[0], yuv[1], bits)
    else:
        c = csc12(yuv, bits).astype(np.float64)
        k, o = c[:9].reshape(3, 3), c[9:]
    out = rgb @ np.linalg.inv(k).T + o
    return (out * (4.0 if bits == 10 else 1.0)).astype(np.float32)


def overlay_tables(j, parents=None, groups=None, palette=None, frame_format="rgb", yuv=("bt709", "limited")):
    """The checked topology and palette of a j-joint overlay -> (parents int32 [j], groups int32 [j], palette float32 [n_groups + 2][3]).
    None: the hand tree (j = 21 only), HAND_GROUPS, HAND_PALETTE_RGB through overlay_palette.  ``palette`` is in the frames' own plane
    space (overlay_palette converts RGB rows)."""
    j = int(j)
    if parents is None or groups is None:
        if j != len(HAND_PARENTS):
            raise ValueError(f"overlay: the default topology has {len(HAND_PARENTS)} joints, the model has {j}: pass parents= and groups=")
    par = np.asarray(HAND_PARENTS if parents is None else parents)
    grp = np.asarray(HAND_GROUPS if groups is None else groups)
    for name, v in (("parents", par), ("groups", grp)):
        if v.shape != (j,) or v.dtype.kind not in "iu":
            raise ValueError(f"overlay: {name} is {j} integers (one per joint), not {v.shape} {v.dtype}")
    if ((par < -1) | (par >= j)).any():
        raise ValueError(f"overlay: parents are -1 (no bone) or joints 0..{j - 1}, not {par.tolist()}")
    pal = overlay_palette(frame_format=frame_format, yuv=yuv) if palette is None else np.asarray(palette, np.float32)
    if pal.ndim != 2 or pal.shape[1:] != (3,) or pal.shape[0] < 3 or not np.isfinite(pal).all():
        raise ValueError(f"overlay: palette is finite fp32 [n_groups + 2][3], not {getattr(pal, 'shape', None)}")
    if ((grp < 0) | (grp >= pal.shape[0] - 2)).any():
        raise ValueError(f"overlay: groups are palette rows 0..{pal.shape[0] - 3} (the last two rows are the ROI outline's), not {grp.tolist()}")
    return par.astype(np.int32), grp.astype(np.int32), np.ascontiguousarray(pal, np.float32)


def check_overlay_numbers(min_score, line_radius, joint_radius, by_size, opacity):
    """What lh_draw_hands refuses of its five numbers, as ValueError -> the five floats."""
    v = [float(x) for x in (min_score, line_radius, joint_radius, by_size, opacity)]
    if not all(np.isfinite(v)) or min(v[1:4]) < 0 or not 0.0 <= v[4] <= 1.0:
        raise ValueError(f"overlay: min_score finite, line_radius / joint_radius / by_size finite and >= 0, 0 <= opacity <= 1, not "
                         f"{dict(zip(_NUMBERS, v))}")
    return v


def resolve_overlay(overlay, j, track_min_score, frame_format, yuv, smooth):
    """ManagedInferStep's ``overlay=`` (None / False: off, True, or a dict of OVERLAY_DEFAULTS' keys) -> None or the resolved options
    (numpy ``parents`` / ``groups`` / ``palette`` included); ValueError for unknown keys and bad values."""
    if overlay is None or overlay is False:
        return None
    if overlay is not True and not isinstance(overlay, dict):
        raise ValueError(f"overlay is None, True or a dict of {sorted(OVERLAY_DEFAULTS)}, not {overlay!r}")
    given = {} if overlay is True else dict(overlay)
    unknown = sorted(set(given) - set(OVERLAY_DEFAULTS))
    if unknown:
        raise ValueError(f"overlay: unknown keys {unknown}; the keys are {sorted(OVERLAY_DEFAULTS)}")
    o = dict(OVERLAY_DEFAULTS, min_score=track_min_score)
    o.update(given)
    for k, v in zip(_NUMBERS, check_overlay_numbers(*(o[k] for k in _NUMBERS))):
        o[k] = v
    o["draw_roi"] = bool(o["draw_roi"])
    if o["source"] not in ("raw", "smooth") or o["target"] not in ("inplace", "surfaces"):
        raise ValueError(f"overlay: source is 'raw' or 'smooth' and target 'inplace' or 'surfaces', not {o['source']!r} / {o['target']!r}")
    if o["source"] == "smooth" and not smooth:
        raise ValueError("overlay: source='smooth' draws smooth_preds: pass smooth=(min_cutoff, beta)")
    o["parents"], o["groups"], o["palette"] = overlay_tables(j, o["parents"], o["groups"], o["palette"], frame_format, yuv)
    return o


# ---- the rule in numpy
def _slot_prims_host(T, t, preds, maxvals, lost, mat, crop_size, boxes, parents, groups, n_groups, min_score, line_radius, joint_radius,
                     by_size, draw_roi):
    """The primitives of slot t in drawing order: (ax, ay, bx, by, r, row) of type T, those lh_draw_hands skips left out."""
    j = preds.shape[1]
    is_lost = lost is not None and lost[t] != 0
    s = T(0)
    if by_size != T(0):
        bw, bh = boxes[t, 2] - boxes[t, 0], boxes[t, 3] - boxes[t, 1]
        s = bw if bw > bh else bh
    r_line, r_joint = line_radius + by_size * s, joint_radius + by_size * s
    out = []

    def emit(ax, ay, bx, by, r, row):
        if all(np.isfinite(v) for v in (ax, ay, bx, by, r)) and 0 <= row < n_groups + 2:
            out.append((ax, ay, bx, by, r, int(row)))
    if mat is not None and draw_roi:
        m = mat[t]
        u1, v1 = T(crop_size[1]) - T(0.5), T(crop_size[0]) - T(0.5)
        lo = T(-0.5)
        c = [((m[0] * u + m[1] * v) + m[2], (m[3] * u + m[4] * v) + m[5]) for u, v in ((lo, lo), (u1, lo), (u1, v1), (lo, v1))]
        for e in range(4):
            emit(c[e][0], c[e][1], c[(e + 1) & 3][0], c[(e + 1) & 3][1], r_line, n_groups + (1 if is_lost else 0))
    if is_lost:
        return out
    p, mv = preds[t], maxvals[t]
    for i in range(j):
        pi = int(parents[i])
        if 0 <= pi < j and mv[pi] >= min_score and mv[i] >= min_score:
            emit(p[pi, 0], p[pi, 1], p[i, 0], p[i, 1], r_line, groups[i])
    for i in range(j):
        if mv[i] >= min_score:
            emit(p[i, 0], p[i, 1], p[i, 0], p[i, 1], r_joint, groups[i])
    return out


def _cov_host(T, px, py, ax, ay, bx, by, r):
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    qx, qy = px - ax, py - ay
    ex, ey = qx, qy
    if l2 > T(0):
        t = (qx * dx + qy * dy) * (T(1) / l2)
        t = np.where(t < T(0), T(0), np.where(t > T(1), T(1), t)).astype(T)
        ex, ey = qx - t * dx, qy - t * dy
    v = (r + T(0.5)) - np.sqrt(ex * ex + ey * ey)
    return np.where(v < T(0), T(0), np.where(v > T(1), T(1), v)).astype(T)


def _code_host(c, top, T):
    v = np.floor(c + T(0.5))
    return np.where(~(v >= T(0)), T(0), np.where(v > T(top), T(top), v)).astype(np.int64)


def _region(prim, hs, ws, even):
    """The pixels a primitive can cover, inclusive, or None: its bounds grown by r + 2 and clipped (outside them the coverage is 0)."""
    ax, ay, bx, by, r, _ = (float(v) for v in prim)
    g = r + 2.0
    lo_x, hi_x, lo_y, hi_y = min(ax, bx) - g, max(ax, bx) + g, min(ay, by) - g, max(ay, by) + g
    if not (lo_x <= ws - 1 and hi_x >= 0 and lo_y <= hs - 1 and hi_y >= 0):
        return None
    x0, x1 = int(max(np.floor(lo_x), 0)), int(min(np.ceil(hi_x), ws - 1))
    y0, y1 = int(max(np.floor(lo_y), 0)), int(min(np.ceil(hi_y), hs - 1))
    if even:
        x0, y0, x1, y1 = x0 & ~1, y0 & ~1, x1 | 1, y1 | 1
    return x0, y0, x1, y1


def draw_hands_host(frames, preds, maxvals, src_frame, lost=None, crop_mat=None, crop_size=None, boxes=None, frame_format="rgb",
                    frame_size=None, layout=None, parents=None, groups=None, palette=None, yuv=("bt709", "limited"), min_score=0.1,
                    line_radius=1.0, joint_radius=2.5, by_size=0.0, opacity=1.0, draw_roi=True, dtype=np.float32):
    """lh_draw_hands in numpy -> a drawn COPY of ``frames``: one uint8 array [n][...] (the copy has its shape) or a sequence of per-frame
    byte arrays (None: an unbound surface, skipped; the copy is a list), of ``frame_size`` = (hs, ws) frames of ``frame_format`` in
    ``layout`` (frame_layout_of's rules; packed RGB [n][hs][ws][3] needs neither).  preds [b][j][2] frame coordinates, maxvals [b][j] or
    [b][j][1], src_frame [b], lost [b] or None, crop_mat [b][6] or None (no ROI outline) for an h x w = ``crop_size`` crop, boxes [b][4]
    (read with ``by_size`` only).  ``parents`` / ``groups`` / ``palette``: overlay_tables' (the palette in the frames' plane space).
    Per slot, in index order: the four edges of the crop's quad (a lost slot: those alone, in the last palette row), the bones whose
    two maxvals are >= ``min_score``, the joints with maxval >= ``min_score``; coverage k = clamp(r + 0.5 - d, 0, 1) of a pixel at
    distance d, c += (opacity * k) * (colour - c) wherever that factor is > 0, floor(c + 0.5) clamped at the end, and a texel no
    primitive covers keeps its bytes.  A chroma texel takes (opacity * ((k00 + k01) + (k10 + k11))) * 0.25 over its 2 x 2 luma block
    (chroma siting is ignored); p010 blends u16 >> 6 on the 10-bit scale.  fp32 in the kernel's order of operations, or with
    ``dtype=np.float64`` the same operations in fp64 on the same fp32 inputs."""
    from .topdown import _frame_bytes_host
    T = np.dtype(dtype).type
    preds = np.asarray(preds, np.float32)
    b, j = preds.shape[:2]
    maxvals = np.asarray(maxvals, np.float32).reshape(b, j)
    src_frame = np.asarray(src_frame, np.int32).reshape(b)
    lost = None if lost is None else np.asarray(lost, np.int32).reshape(b)
    mat = None if crop_mat is None else np.asarray(crop_mat, np.float32).reshape(b, 6).astype(T)
    if mat is not None and draw_roi and not (isinstance(crop_size, (tuple, list)) and len(crop_size) == 2):
        raise ValueError(f"draw_hands: crop_size=(h, w) is needed with crop_mat, not {crop_size!r}")
    min_score, line_radius, joint_radius, by_size, opacity = (T(np.float32(v)) for v in
                                                              check_overlay_numbers(min_score, line_radius, joint_radius, by_size, opacity))
    if by_size != T(0) and boxes is None:
        raise ValueError("draw_hands: by_size needs boxes")
    boxes = None if boxes is None else np.asarray(boxes, np.float32).reshape(b, 4).astype(T)
    par, grp, pal = overlay_tables(j, parents, groups, palette, frame_format, yuv)
    pal, n_groups = pal.astype(T), pal.shape[0] - 2
    is_array = not isinstance(frames, (list, tuple))
    if is_array and frame_format == "rgb" and frame_size is None and np.ndim(frames) == 4:
        frame_size = np.shape(frames)[1:3]
    if not (isinstance(frame_size, (tuple, list)) and len(frame_size) == 2):
        raise ValueError(f"draw_hands: frame_size=(hs, ws) is needed, not {frame_size!r}")
    hs, ws = int(frame_size[0]), int(frame_size[1])
    L = frame_layout_of(frame_format, hs, ws, layout)
    flats = [None if f is None else f.copy() for f in _frame_bytes_host(frames, surface_bytes(L), "draw_hands_host")]
    n = len(flats)
    pT, mT = preds.astype(T), maxvals.astype(T)
    even = L.code != 0
    top, shift, sb = (1023, 6, 2) if L.code == 4 else (255, 0, 1)
    yy, xx = np.meshgrid(np.arange(hs), np.arange(ws), indexing="ij")
    for f in range(n):
        flat = flats[f]
        slots = [t for t in range(b) if src_frame[t] == f]
        if flat is None or not slots:
            continue

        def tex(off):
            if sb == 2:
                return ((flat[off].astype(np.int64) | (flat[off + 1].astype(np.int64) << 8)) >> shift).astype(T)
            return flat[off].astype(T)

        def put(off, code, hit):
            code = code << shift
            for byte in range(sb):
                flat[off[hit] + byte] = ((code[hit] >> (8 * byte)) & 255).astype(np.uint8)
        if even:
            cy_, cx_ = np.meshgrid(np.arange(hs // 2), np.arange(ws // 2), indexing="ij")
            offs = [yy * L.pitch + xx * sb, L.cb_offset + cy_ * L.c_pitch + cx_ * L.c_step, L.cr_offset + cy_ * L.c_pitch + cx_ * L.c_step]
            planes = [tex(o) for o in offs]
        else:
            offs = [(yy * ws + xx) * 3 + ch for ch in range(3)]
            planes = [tex(o) for o in offs]
        hits = [np.zeros(p.shape, bool) for p in planes]
        with np.errstate(all="ignore"):
            for t in slots:
                for prim in _slot_prims_host(T, t, pT, mT, lost, mat, crop_size, boxes, par, grp, n_groups, min_score, line_radius,
                                             joint_radius, by_size, draw_roi):
                    reg = _region(prim, hs, ws, even)
                    if reg is None:
                        continue
                    x0, y0, x1, y1 = reg
                    px, py = np.arange(x0, x1 + 1).astype(T)[None, :], np.arange(y0, y1 + 1).astype(T)[:, None]
                    k = _cov_host(T, px, py, *prim[:5])
                    col = pal[prim[5]]
                    full = (slice(y0, y1 + 1), slice(x0, x1 + 1))
                    if even:
                        k4 = k.reshape((y1 - y0 + 1) // 2, 2, (x1 - x0 + 1) // 2, 2)
                        kc = (opacity * ((k4[:, 0, :, 0] + k4[:, 0, :, 1]) + (k4[:, 1, :, 0] + k4[:, 1, :, 1]))) * T(0.25)
                        half = (slice(y0 // 2, y1 // 2 + 1), slice(x0 // 2, x1 // 2 + 1))
                        work = [(0, full, opacity * k), (1, half, kc), (2, half, kc)]
                    else:
                        work = [(ch, full, opacity * k) for ch in range(3)]
                    for ch, sl, al in work:
                        m = al > T(0)
                        c = planes[ch][sl]
                        planes[ch][sl] = np.where(m, c + al * (col[ch] - c), c).astype(T)
                        hits[ch][sl] |= m
        for ch in range(3):
            put(offs[ch], _code_host(planes[ch], top, T), hits[ch])
    if is_array:
        src = np.asarray(frames)
        return np.stack([fl.reshape(src.shape[1:]) for fl in flats])
    return flats


# ---- the launch
def draw_hands(frames, preds, maxvals, src_frame, lost=None, crop_mat=None, crop_size=None, boxes=None, frame_format="rgb", frame_size=None,
               layout=None, parents=None, groups=None, palette=None, yuv=("bt709", "limited"), min_score=0.1, line_radius=1.0,
               joint_radius=2.5, by_size=0.0, opacity=1.0, draw_roi=True):
    """One lh_draw_hands launch on the current stream, IN PLACE: ``frames`` is one contiguous uint8 device tensor [n][...] (frame f at
    row f) or a sequence of surfaces (one uint8 device tensor per frame, None: unbound, skipped), drawn through a surface table; the
    other arguments are draw_hands_host's, the per-slot ones as contiguous device tensors (preds fp32 [b][j][2], maxvals fp32 [b][j] or
    [b][j][1], src_frame / lost int32 [b], crop_mat fp32 [b][6], boxes fp32 [b][4]).  Returns ``frames``."""
    import torch
    from . import _lib
    from .topdown import _stream, surface_table
    check_frame_format(frame_format)
    numbers = check_overlay_numbers(min_score, line_radius, joint_radius, by_size, opacity)
    if not torch.is_tensor(preds) or preds.dim() != 3:
        raise _lib.LightHandError("draw_hands: preds is a device tensor fp32 [b, j, 2]")
    b, j = preds.shape[:2]
    dev = preds.device
    par, grp, pal = overlay_tables(j, parents, groups, palette, frame_format, yuv)
    f32 = [(preds, (b, j, 2))] + [(t, s) for t, s in ((crop_mat, (b, 6)), (boxes, (b, 4))) if t is not None]
    i32 = [(t, (b,)) for t in (src_frame, lost) if t is not None]
    good = (preds.is_cuda and torch.is_tensor(maxvals) and maxvals.dtype == torch.float32 and maxvals.is_contiguous() and maxvals.numel() == b * j
            and maxvals.device == dev and src_frame is not None
            and all(torch.is_tensor(t) and t.dtype == torch.float32 and tuple(t.shape) == s for t, s in f32)
            and all(torch.is_tensor(t) and t.dtype == torch.int32 and tuple(t.shape) == s for t, s in i32)
            and all(t.is_contiguous() and t.device == dev for t, _ in f32 + i32))
    if not good:
        raise _lib.LightHandError("draw_hands: contiguous tensors on one device -- fp32 preds [b, j, 2], maxvals [b, j], crop_mat [b, 6] or None, "
                                  "boxes [b, 4] or None; int32 src_frame [b], lost [b] or None")
    if crop_mat is not None and draw_roi and not (isinstance(crop_size, (tuple, list)) and len(crop_size) == 2):
        raise ValueError(f"draw_hands: crop_size=(h, w) is needed with crop_mat, not {crop_size!r}")
    if numbers[3] != 0.0 and boxes is None:
        raise ValueError("draw_hands: by_size needs boxes")
    is_table = isinstance(frames, (list, tuple))
    if not is_table and frame_format == "rgb" and frame_size is None and torch.is_tensor(frames) and frames.dim() == 4:
        frame_size = tuple(frames.shape[1:3])
    if not (isinstance(frame_size, (tuple, list)) and len(frame_size) == 2):
        raise ValueError(f"draw_hands: frame_size=(hs, ws) is needed, not {frame_size!r}")
    hs, ws = int(frame_size[0]), int(frame_size[1])
    L = frame_layout_of(frame_format, hs, ws, layout)
    desc = frames_layout_struct(L, yuv, "left")
    keep, table, base, stride = (), None, None, 0
    if is_table:
        table_dev, keep = surface_table(frames, L, dev)
        table, n = table_dev.data_ptr(), table_dev.shape[0]
    else:
        if (not torch.is_tensor(frames) or not frames.is_cuda or frames.device != dev or frames.dtype != torch.uint8 or frames.dim() < 2
                or not frames.is_contiguous() or frames.stride(0) < surface_bytes(L)):
            raise _lib.LightHandError(f"draw_hands: frames contiguous uint8 [n, >= {surface_bytes(L)} bytes] on the keypoints' device, or a sequence "
                                      "of surfaces")
        base, n, stride = frames.data_ptr(), frames.shape[0], frames.stride(0)
    tabs = [torch.from_numpy(a).to(dev) for a in (par, grp, pal)]
    ch, cw = (int(crop_size[0]), int(crop_size[1])) if crop_mat is not None and crop_size is not None else (1, 1)
    import ctypes as C
    with torch.cuda.device(dev):
        _lib.check(_lib.load().lh_draw_hands(base, stride, table, C.byref(desc), n, hs, ws, preds.data_ptr(), maxvals.data_ptr(), src_frame.data_ptr(),
                                             None if lost is None else lost.data_ptr(), None if crop_mat is None else crop_mat.data_ptr(),
                                             None if boxes is None else boxes.data_ptr(), b, j, ch, cw, tabs[0].data_ptr(), tabs[1].data_ptr(),
                                             tabs[2].data_ptr(), pal.shape[0] - 2, *numbers, int(bool(draw_roi)), _stream()), "lh_draw_hands")
    for t in list(keep) + tabs:                                    # the launch is queued: the allocator must not hand these out before it ran
        t.record_stream(torch.cuda.current_stream())
    return frames
