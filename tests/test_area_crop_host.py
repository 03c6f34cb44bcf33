"""CPU: the host side of the antialiased frame crop -- the numpy restatements crop_taps_host / frames_crop_host of
lighthand_amd.topdown (the sampling rule of lh_frames_crop_area_to_nhwc4: csrc/frames_crop_kernel.h, above crop_taps) against a hand-written
table, the exact block mean, the plain crop's reference and a white-noise property; the entry's argument validation and the refusals
of InferStep / InferPipeline(antialias=) without a GPU.  The kernel is checked against frames_crop_host in tests/test_gpu_area_crop.py."""
import ctypes as C

import numpy as np
import pytest

F = np.float32
NAN, INF = float("nan"), float("inf")


def _scale(sx, sy=None):
    sy = sx if sy is None else sy
    return [sx, 0.0, 3.25, 0.0, sy, -7.5]


TAPS = [  # (matrix, max_taps, (kx, ky))
    ([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], 8, (1, 1)),                   # identity
    (_scale(0.125), 8, (1, 1)),                                    # x8 magnification
    (_scale(1.015625), 8, (1, 1)),                                 # 1 + 1/64 exactly: still the single sample
    (_scale(1.02), 8, (2, 2)),
    (_scale(2.0), 8, (2, 2)),
    (_scale(2.0001), 8, (3, 3)),
    (_scale(7.5), 8, (8, 8)),
    (_scale(16.0), 8, (8, 8)),
    (_scale(1000.0), 8, (8, 8)),
    (_scale(7.5), 4, (4, 4)),
    (_scale(2.0), 1, (1, 1)),
    (_scale(NAN), 8, (1, 1)),
    (_scale(INF), 8, (1, 1)),
    (_scale(-INF), 8, (1, 1)),
    ([NAN] * 6, 8, (1, 1)),
    ([2.0, NAN, 0.0, 0.0, 2.0, 0.0], 8, (2, 1)),                   # one axis is NaN, the other is not
    ([0.0] * 6, 8, (1, 1)),                                        # an empty slot's matrix
    (_scale(3.3, 0.9), 8, (4, 1)),
    (_scale(0.9, 3.3), 8, (1, 4)),
    ([2.0, -1.5, 10.0, 1.5, 2.0, 20.0], 8, (3, 3)),                # the direction (0.8, 0.6) at scale 2.5
    ([-2.0, -1.5, 10.0, -1.5, 2.0, 20.0], 8, (3, 3)),              # ... mirrored
    ([2.0, -1.5, 10.0, 1.5, 2.0, 20.0], 2, (2, 2)),
]


def test_crop_taps_host_against_a_hand_written_table():
    from lighthand_amd.topdown import crop_taps_host
    for mat, max_taps, want in TAPS:
        got = crop_taps_host([mat], max_taps)
        assert got.dtype == np.int32 and got.shape == (1, 2)
        assert tuple(got[0]) == want, (mat, max_taps, got)
    by_cap = {}
    for mat, max_taps, want in TAPS:
        by_cap.setdefault(max_taps, []).append((mat, want))
    for max_taps, rows in by_cap.items():                         # the same answers in one call
        assert crop_taps_host([m for m, _ in rows], max_taps).tolist() == [list(w) for _, w in rows]
    assert crop_taps_host([_scale(7.5)]).tolist() == [[8, 8]]      # the default cap is 8
    for bad in (0, 9, -1):
        with pytest.raises(ValueError, match="max_taps"):
            crop_taps_host([_scale(2.0)], bad)


def _normalise(val, mean, std):
    m, s = np.asarray(mean, np.float32)[:, None, None], np.asarray(std, np.float32)[:, None, None]
    return ((val - m) * (F(1) / s)).astype(np.float32)


def block_mean(frame, s, mean, std):
    """The expectation of an aligned minification by s: (sum of each s x s block) * (1.f / (s*s)) * (1.f / 255.f) in fp32 (a sum of at
    most 64 bytes is exact), then Normalize; frame uint8 [hs][ws][3] -> fp32 [3][hs/s][ws/s]."""
    hs, ws = frame.shape[:2]
    sums = frame.astype(np.int64).reshape(hs // s, s, ws // s, s, 3).sum((1, 3))
    assert sums.max() <= 255 * 64
    val = (np.transpose(sums, (2, 0, 1)).astype(np.float32) * (F(1) / F(s * s))) * (F(1) / F(255))
    return _normalise(val, mean, std)


@pytest.mark.parametrize("s", [2, 3, 4, 6, 8])
def test_aligned_integer_minification_is_the_exact_block_mean(s):
    from lighthand_amd.topdown import MEAN, STD, box_affine_host, crop_taps_host, frames_crop_host
    # seed 13: bytes on which s = 3 misses the block mean by one unit in the last place in the crop's first row and column if the
    # tap offset is formed as (i + 0.5f) / k - 0.5f (-0.33333331: the sample lands 6e-8 beside its pixel) instead of rounded once
    frames = np.random.RandomState(13).randint(0, 256, size=(2, 96, 96, 3)).astype(np.uint8)
    c = 96 // s
    mat, src = box_affine_host([[-0.5, -0.5, 95.5, 95.5]] * 2, [1, 0], 2, (c, c), 1.0)
    assert mat.tolist() == [[s, 0.0, (s - 1) / 2, 0.0, s, (s - 1) / 2]] * 2 and src.tolist() == [1, 0]
    assert crop_taps_host(mat).tolist() == [[s, s]] * 2
    got = frames_crop_host(frames, mat, src, (c, c), max_taps=8)
    assert got.dtype == np.float32 and got.shape == (2, 3, c, c)
    for i, f in enumerate((1, 0)):
        assert np.array_equal(got[i].view(np.int32), block_mean(frames[f], s, MEAN, STD).view(np.int32))
    # fewer taps than the minification: not the block mean any more (s = 2 is left out: its single sample sits between the four
    # pixels of the block with weights 1/2, which is their mean)
    if s > 2:
        assert not np.array_equal(frames_crop_host(frames, mat, src, (c, c), max_taps=1), got)
        assert not np.array_equal(frames_crop_host(frames, mat, src, (c, c), max_taps=s - 1), got)


def topdown_slots():
    """The 32 slots of tests/test_gpu_topdown.py::test_crops_match_the_numpy_sampling_rule: (frames, mat, src)."""
    from lighthand_amd.topdown import box_affine_host
    from test_gpu_topdown import BOXES, FRAME_INDEX, H, HS, W, WS, _frames, _random_boxes
    frames = _frames(3, HS, WS, 5)
    rb, ri = _random_boxes(18, 21)
    mat = np.concatenate([box_affine_host(BOXES, FRAME_INDEX, 3, (H, W), 1.0)[0], box_affine_host(BOXES, FRAME_INDEX, 3, (H, W), 1.25)[0],
                          box_affine_host(rb, ri, 3, (H, W), 1.25)[0]])
    src = np.concatenate([box_affine_host(BOXES, FRAME_INDEX, 3, (H, W), 1.0)[1]] * 2 + [ri]).astype(np.int32)
    return frames, mat, src


def test_one_tap_is_the_plain_crop_and_unminified_slots_never_change():
    from lighthand_amd.topdown import crop_taps_host, frames_crop_host
    from test_gpu_topdown import H, W, crop_reference
    frames, mat, src = topdown_slots()
    assert len(src) == 32
    one = frames_crop_host(frames, mat, src, (H, W), max_taps=1)
    for i in range(32):
        want = crop_reference(frames, mat[i], int(src[i]), H, W)[0]
        assert np.array_equal(one[i].view(np.int32), want.view(np.int32)), i
    assert np.array_equal(frames_crop_host(frames, mat, src, (H, W)), one)       # max_taps defaults to 1
    eight = frames_crop_host(frames, mat, src, (H, W), max_taps=8)
    taps = crop_taps_host(mat, 8)
    small = mat[:, 0] <= 1                                          # upright boxes: one scale on both axes
    assert 5 < small.sum() < 27 and (taps[small] == 1).all() and (taps[~small & (mat[:, 0] > 1.02)] > 1).all()
    assert np.array_equal(eight[small].view(np.int32), one[small].view(np.int32))
    changed = [i for i in range(32) if not np.array_equal(eight[i], one[i])]
    assert changed and all(taps[i].max() > 1 and src[i] >= 0 for i in changed)


@pytest.mark.parametrize("turned", [False, True], ids=["upright", "turned"])
@pytest.mark.parametrize("s", [2.1, 2.9, 3.9, 5.6])
def test_white_noise_is_averaged_down(s, turned):
    """A 200 x 200 frame of iid bytes minified by s into a 32 x 32 crop, inner 16 x 16: an ideal box over s^2 iid pixels has
    std_frame / s, one bilinear sample (2/3) std_frame (the mean of (1-w)^2 + w^2 over w is 2/3, on both axes: (2/3)^2 of the
    variance), so the ideal ratio is 1.5 / s.  Required: std(area) / std(single sample) in [1.0 / s, 1.6 / s]."""
    from lighthand_amd.topdown import crop_taps_host, frames_crop_host
    frames = np.random.RandomState(7).randint(0, 256, size=(1, 200, 200, 3)).astype(np.uint8)
    c, sn = (0.8, 0.6) if turned else (1.0, 0.0)
    m0, m1, m3, m4 = s * c, -s * sn, s * sn, s * c
    mat = np.array([[m0, m1, 99.5 - (m0 + m1) * 15.5, m3, m4, 99.5 - (m3 + m4) * 15.5]], np.float32)
    k = int(np.ceil(s))
    assert crop_taps_host(mat).tolist() == [[k, k]]
    plain = dict(mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))         # one distribution for the three channels
    area = frames_crop_host(frames, mat, [0], (32, 32), max_taps=8, **plain)[0, :, 8:24, 8:24]
    single = frames_crop_host(frames, mat, [0], (32, 32), max_taps=1, **plain)[0, :, 8:24, 8:24]
    ratio = float(area.astype(np.float64).std() / single.astype(np.float64).std())
    print(f"white noise, scale {s} {'turned' if turned else 'upright'}: std ratio {ratio:.4f} = {ratio * s:.3f} / s")
    assert 1.0 / s <= ratio <= 1.6 / s, ratio * s


def test_area_entry_is_exported_declared_and_validates_arguments_without_gpu():
    import os
    import re
    from conftest import ROOT
    from lighthand_amd import _lib
    lib = _lib.load()
    name = "lh_frames_crop_area_to_nhwc4"
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lighthand_hip.h")).read(), flags=re.S)
    decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
    assert hasattr(lib, name) and name in _lib.SIGNATURES and decl
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES["lh_frames_crop_to_nhwc4"][1]) + 1
    assert "int max_taps, int dtype" in " ".join(decl.group(1).split())

    fake = C.c_void_p(0x1000)                                      # never dereferenced: validation fails before any launch
    m3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    good = dict(frames=fake, out=fake, b=4, n=2, hs=48, ws=56, h=24, w=40, pad=3, wp=48, mean=m3, std=m3, mat=fake, src=fake, max_taps=8,
                dtype=_lib.LH_BF16)

    def crop(**kw):
        a = dict(good, **kw)
        return lib.lh_frames_crop_area_to_nhwc4(a["frames"], a["out"], a["b"], a["n"], a["hs"], a["ws"], a["h"], a["w"], a["pad"], a["wp"],
                                                a["mean"], a["std"], a["mat"], a["src"], a["max_taps"], a["dtype"], None)
    for rc in (crop(frames=None), crop(out=None), crop(mean=None), crop(std=None), crop(mat=None), crop(src=None), crop(b=0),
               crop(b=1 << 16), crop(n=0), crop(hs=0), crop(ws=0), crop(h=0), crop(w=0), crop(pad=-1), crop(wp=45), crop(dtype=3),
               crop(out=C.c_void_p(0x1004)), crop(hs=40000, ws=40000), crop(h=30000, w=30000, wp=30006)):
        assert rc == -1 and name.encode() in lib.lh_last_error()
    for bad in (0, 9, -1, 64, 1 << 30):
        assert crop(max_taps=bad) == -1
        assert name.encode() in lib.lh_last_error() and b"max_taps" in lib.lh_last_error()


def test_antialias_is_refused_without_frames_and_outside_1_to_8():
    """Refused with ValueError before the model is looked at (and so before any device work)."""
    from lighthand_amd.runtime import InferPipeline, InferStep, _antialias_taps
    assert [_antialias_taps(v) for v in (False, True, 1, 3, 8)] == [1, 8, 1, 3, 8]
    for cls in (InferStep, InferPipeline):
        for value in (True, 1, 4):
            with pytest.raises(ValueError, match="frames"):
                cls(object(), 2, 64, 64, antialias=value)
            with pytest.raises(ValueError, match="frames"):
                cls(object(), 2, 64, 64, input_u8=(96, 128), antialias=value)
        for bad in (0, 9, -1, 2.0, "8", None):
            with pytest.raises(ValueError, match="antialias"):
                cls(object(), 2, 64, 64, frames=(2, 96, 128), antialias=bad)
    from lighthand_amd.tools import track_frames as T
    parse = T.build_parser().parse_args
    assert parse(["--synthetic", "3"]).antialias is None
    assert parse(["--synthetic", "3", "--antialias"]).antialias == 8
    assert parse(["--synthetic", "3", "--antialias", "4", "--oriented"]).antialias == 4
