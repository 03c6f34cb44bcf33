"""Shared inputs of tests/test_surfaces_host.py and tests/test_gpu_surfaces.py: 3 frames of 36 x 52 (NV12: pitch 64, 40 luma rows), a
24 x 40 crop, and the slots that take every path of the frame crop -- one sample, 2 and 3 taps, a ROI turned 30 degrees, a mirrored
one, one half outside the frame, one wholly outside, an empty slot (src_frame = -1) and one that names frame 3: past the end of a
3-frame buffer, or an unbound entry of a 4-entry surface table."""
import numpy as np

HS, WS, H, W, NF = 36, 52, 24, 40, 3
PITCH, LUMA_ROWS = 64, 40
MAX_TAPS = 3
FORMATS = ("nv12", "nv21", "yuv420p", "p010")
C30, S30 = 0.8 * np.cos(np.pi / 6), 0.8 * np.sin(np.pi / 6)
MAT = np.array([[0.9, 0.0, 3.2, 0.0, 0.9, 2.7],                    # magnified: one sample
                [1.3, 0.0, 0.5, 0.0, 1.3, 0.4],                     # 2 x 2 taps
                [1.3, 0.0, 0.25, 0.0, 2.2, -8.0],                   # 2 x 3 taps
                [C30, -S30, 20.0, S30, C30, 2.0],                   # turned 30 degrees
                [-1.0, 0.0, 45.0, 0.0, 1.0, 5.0],                   # mirrored
                [1.0, 0.0, -20.25, 0.0, 1.0, 6.5],                  # half outside
                [1.0, 0.0, 500.0, 0.0, 1.0, 500.0],                 # wholly outside
                [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],                     # empty
                [1.0, 0.0, 2.0, 0.0, 1.0, 3.0]], np.float32)        # frame 3: no such frame / an unbound surface
SRC = np.array([0, 1, 2, 0, 1, 2, 0, -1, 3], np.int32)
DARK_SLOTS = (6, 7, 8)                                              # exactly black, whatever the frames hold


def layouts():
    """One pitched layout per format: the pitch above the row's bytes, more luma rows than hs, a chroma pitch of its own."""
    from lighthand_amd.topdown import yuv420_layout
    return {"nv12": yuv420_layout("nv12", HS, WS, PITCH, LUMA_ROWS),
            "nv21": yuv420_layout("nv21", HS, WS, PITCH, LUMA_ROWS, 80),
            "yuv420p": yuv420_layout("yuv420p", HS, WS, PITCH, LUMA_ROWS - 2, 30),
            "p010": yuv420_layout("p010", HS, WS, 2 * PITCH, LUMA_ROWS - 3, 120)}


def samples(seed=3):
    """Random 8-bit samples: luma [NF][HS][WS], chroma [NF][HS/2][WS/2][2] (Cb, Cr)."""
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (NF, HS, WS)).astype(np.uint8), rng.randint(0, 256, (NF, HS // 2, WS // 2, 2)).astype(np.uint8)


def pack(layout, luma, chroma, low=None, gap=0xA5):
    """The samples laid out by ``layout`` (a Yuv420Layout) -> uint8 [n][frame_bytes]; every byte that is no sample is ``gap``.  16-bit
    samples are u16 = v8 << 8 | low, ``low`` (None: 0) an array of luma's shape with values below 64: the 6 bits that are not data."""
    n = luma.shape[0]
    out = np.full((n, layout.frame_bytes), gap, np.uint8)
    y, x = np.meshgrid(np.arange(luma.shape[1]), np.arange(luma.shape[2]), indexing="ij")
    cy, cx = np.meshgrid(np.arange(chroma.shape[1]), np.arange(chroma.shape[2]), indexing="ij")
    top = layout.sample_bytes - 1                                   # little-endian: the 8 data bits of v8 << 8 are the high byte
    out[:, y * layout.pitch + x * layout.sample_bytes + top] = luma
    out[:, layout.cb_offset + cy * layout.c_pitch + cx * layout.c_step + top] = chroma[..., 0]
    out[:, layout.cr_offset + cy * layout.c_pitch + cx * layout.c_step + top] = chroma[..., 1]
    if layout.sample_bytes == 2:
        low = np.zeros(luma.shape, np.uint8) if low is None else np.asarray(low, np.uint8)
        assert low.max() < 64
        out[:, y * layout.pitch + 2 * x] = low
        out[:, layout.cb_offset + cy * layout.c_pitch + cx * layout.c_step] = low[:, ::2, ::2]
        out[:, layout.cr_offset + cy * layout.c_pitch + cx * layout.c_step] = low[:, 1::2, 1::2]
    return out


def rgb_frames(seed=4):
    return np.random.RandomState(seed).randint(0, 256, (NF, HS, WS, 3)).astype(np.uint8)
