"""CPU: the host side of top-down inference on full frames -- the numpy restatements of lh_box_affine / lh_keypoints_to_boxes
(lighthand_amd.topdown: the geometry is checked here, the kernels against them in tests/test_gpu_topdown.py), the three C-ABI
entries (exported, declared, arguments validated without a GPU) and InferStep's / InferPipeline's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

F = np.float32
NEW = ("lh_box_affine", "lh_frames_crop_to_nhwc4", "lh_keypoints_to_boxes")


def _apply(m, x, y):
    m = m.astype(np.float32)
    return (m[0] * F(x) + m[1] * F(y)) + m[2], (m[3] * F(x) + m[4] * F(y)) + m[5]


@pytest.mark.parametrize("size", [(64, 64), (24, 40), (256, 192)])
@pytest.mark.parametrize("padding", [1.0, 1.25, 2.0])
def test_crop_corners_land_on_the_padded_box(size, padding):
    """The crop's extent [-0.5, w-0.5] x [-0.5, h-0.5] maps onto the padded box: centred on the box, padding * the box's larger
    side (at the crop's aspect ratio) wide, within 4 fp32 spacings of the coordinates involved."""
    from lighthand_amd.topdown import box_affine_host
    h, w = size
    rng = np.random.RandomState(h + w)
    boxes = np.concatenate([rng.uniform(-50, 900, size=(16, 2)), rng.uniform(950, 1900, size=(16, 2))], 1).astype(np.float32)
    mat, src = box_affine_host(boxes, np.zeros(16, np.int32), 1, size, padding)
    assert (src == 0).all()
    for bx, m in zip(boxes.astype(np.float64), mat):
        bw, bh = bx[2] - bx[0], bx[3] - bx[1]
        sw = padding * max(bw, bh * w / h)
        sh = sw * h / w
        cx, cy = (bx[0] + bx[2]) / 2, (bx[1] + bx[3]) / 2
        lo, hi = _apply(m, -0.5, -0.5), _apply(m, w - 0.5, h - 0.5)
        tol = 4 * np.spacing(F(max(abs(cx) + sw, abs(cy) + sh)))
        assert abs(lo[0] - (cx - sw / 2)) <= tol and abs(hi[0] - (cx + sw / 2)) <= tol
        assert abs(lo[1] - (cy - sh / 2)) <= tol and abs(hi[1] - (cy + sh / 2)) <= tol
        assert m[1] == 0 and m[3] == 0


def test_whole_frame_box_is_the_exact_identity():
    from lighthand_amd.topdown import box_affine_host
    for h, w in ((256, 256), (37, 53), (1080, 1920)):
        mat, src = box_affine_host([[-0.5, -0.5, w - 0.5, h - 0.5]], [0], 1, (h, w), 1.0)
        assert mat.dtype == np.float32 and src.dtype == np.int32
        assert mat.tolist() == [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]] and src.tolist() == [0]


def test_non_square_crop_keeps_the_aspect_ratio():
    """24 x 40 crop: one scale on both axes, whichever side of the box decides the size."""
    from lighthand_amd.topdown import box_affine_host
    boxes = np.array([[10, 10, 20, 90], [10, 10, 200, 30], [5.5, 7.25, 45.5, 31.25]], np.float32)       # tall, wide, the crop's own shape
    mat, _ = box_affine_host(boxes, [0, 0, 0], 1, (24, 40), 1.5)
    assert (mat[:, 0] == mat[:, 4]).all() and (mat[:, 0] > 0).all()
    assert mat[0, 0] == F(1.5) * (F(80) * F(40) / F(24)) / F(40)                 # the tall box: its height decides
    assert mat[1, 0] == F(1.5) * F(190) / F(40)                                  # the wide box: its width
    assert mat[2, 0] == F(1.5)                                                   # 40 x 24 box: one source pixel per crop pixel, * padding


def test_empty_slots():
    from lighthand_amd.topdown import box_affine_host
    good = [4.0, 4.0, 30.0, 30.0]
    boxes = np.array([good, good, good, [np.nan, 4, 30, 30], [4, 4, np.inf, 30], [30, 4, 30, 30], [31, 4, 30, 30], [4, 30, 30, 4], good],
                     np.float32)
    index = np.array([0, 3, -1, 0, 0, 0, 0, 0, 2], np.int32)
    mat, src = box_affine_host(boxes, index, 3, (64, 64), 1.25)
    assert src.tolist() == [0, -1, -1, -1, -1, -1, -1, -1, 2]
    assert (mat[src < 0] == 0).all() and (mat[src >= 0][:, 0] > 0).all()
    assert np.isfinite(mat).all()


def test_boxes_from_keypoints_host():
    from lighthand_amd.topdown import boxes_from_keypoints_host
    j = 21
    rng = np.random.RandomState(0)
    preds = rng.uniform(100, 400, size=(5, j, 2)).astype(np.float32)
    mv = np.full((5, j, 1), 0.9, np.float32)
    old = rng.uniform(0, 50, size=(5, 4)).astype(np.float32)
    src = np.array([0, 0, 0, 0, -1], np.int32)
    mv[0, 5:] = 0.05                                             # slot 0: five confident joints, the others (far away) must not count
    preds[0, 5:] += 1000
    preds[1] = preds[1, :1] + rng.uniform(-2, 2, size=(j, 2)).astype(np.float32)     # slot 1: a 4 px cluster -> widened to min_side
    mv[2, 7:] = 0.0                                              # slot 2: seven joints, one short of min_joints
    mv[3, 0] = 0.1                                               # slot 3: maxval == min_score counts
    preds[3, 0] = (-30.0, 700.0)
    nxt, lost = boxes_from_keypoints_host(preds, mv, old, src, min_score=0.1, min_joints=5, min_side=16.0)
    assert nxt.dtype == np.float32 and lost.dtype == np.int32
    assert lost.tolist() == [0, 0, 0, 0, 1]
    c = preds[0, :5]
    assert nxt[0].tolist() == [c[:, 0].min(), c[:, 1].min(), c[:, 0].max(), c[:, 1].max()]
    assert abs((nxt[1, 2] - nxt[1, 0]) - 16.0) <= 1e-4 and abs((nxt[1, 3] - nxt[1, 1]) - 16.0) <= 1e-4
    lo, hi = preds[1].min(0), preds[1].max(0)
    assert np.allclose((nxt[1, :2] + nxt[1, 2:]) / 2, (lo + hi) / 2, atol=1e-4)      # widened about its centre
    assert nxt[3, 0] == F(-30.0) and nxt[3, 3] == F(700.0)
    assert nxt[4].tolist() == old[4].tolist()                                      # the empty slot keeps its box
    nxt, lost = boxes_from_keypoints_host(preds, mv, old, src, min_score=0.1, min_joints=8, min_side=16.0)
    assert lost.tolist() == [1, 0, 1, 0, 1]                      # 5 and 7 joints < 8
    assert nxt[0].tolist() == old[0].tolist() and nxt[2].tolist() == old[2].tolist()
    assert nxt[3, 0] == F(-30.0)


def test_topdown_entries_are_exported_and_declared():
    from lighthand_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lighthand_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_topdown_entries_validate_arguments_without_gpu():
    from lighthand_amd import _lib
    lib = _lib.load()
    fake, fake2 = C.c_void_p(0x1000), C.c_void_p(0x2000)          # never dereferenced: validation fails before any launch
    m3 = (C.c_float * 3)(0.5, 0.5, 0.5)

    def affine(boxes=fake, index=fake, b=4, n=2, h=64, w=64, padding=1.25, mat=fake, src=fake):
        return lib.lh_box_affine(boxes, index, b, n, h, w, padding, mat, src, None)
    for rc in (affine(boxes=None), affine(index=None), affine(mat=None), affine(src=None), affine(b=0), affine(n=0), affine(h=0),
               affine(w=-1), affine(padding=0.0), affine(padding=-1.0), affine(padding=float("nan")), affine(padding=float("inf"))):
        assert rc == -1 and b"lh_box_affine" in lib.lh_last_error()

    good = dict(frames=fake, out=fake, b=4, n=2, hs=48, ws=56, h=24, w=40, pad=3, wp=48, mean=m3, std=m3, mat=fake, src=fake,
                dtype=_lib.LH_BF16)

    def crop(**kw):
        a = dict(good, **kw)
        return lib.lh_frames_crop_to_nhwc4(a["frames"], a["out"], a["b"], a["n"], a["hs"], a["ws"], a["h"], a["w"], a["pad"], a["wp"],
                                           a["mean"], a["std"], a["mat"], a["src"], a["dtype"], None)
    for rc in (crop(frames=None), crop(out=None), crop(mean=None), crop(std=None), crop(mat=None), crop(src=None), crop(b=0),
               crop(b=1 << 16), crop(n=0), crop(hs=0), crop(ws=0), crop(h=0), crop(w=0), crop(pad=-1), crop(wp=45), crop(dtype=3),
               crop(out=C.c_void_p(0x1004)), crop(hs=40000, ws=40000), crop(h=30000, w=30000, wp=30006)):
        assert rc == -1 and b"lh_frames_crop_to_nhwc4" in lib.lh_last_error()

    def k2b(preds=fake, mv=fake, boxes=fake, src=fake, b=4, j=21, score=0.1, joints=8, side=16.0, nxt=fake2, lost=fake):
        return lib.lh_keypoints_to_boxes(preds, mv, boxes, src, b, j, score, joints, side, nxt, lost, None)
    for rc in (k2b(preds=None), k2b(mv=None), k2b(boxes=None), k2b(src=None), k2b(nxt=None), k2b(lost=None), k2b(b=0), k2b(j=0),
               k2b(joints=0), k2b(side=-1.0), k2b(side=float("inf")), k2b(score=float("nan")), k2b(nxt=fake)):
        assert rc == -1 and b"lh_keypoints_to_boxes" in lib.lh_last_error()


def test_infer_step_refuses_bad_frame_arguments():
    """Refused with ValueError before the model is looked at (and so before any device work)."""
    from lighthand_amd.runtime import InferPipeline, InferStep
    for cls in (InferStep, InferPipeline):
        with pytest.raises(ValueError, match="input_u8"):
            cls(object(), 2, 64, 64, frames=(2, 96, 128), input_u8=(96, 128))
        with pytest.raises(ValueError, match="box_padding"):
            cls(object(), 2, 64, 64, frames=(2, 96, 128), box_padding=0)
        with pytest.raises(ValueError, match="box_padding"):
            cls(object(), 2, 64, 64, frames=(2, 96, 128), box_padding=float("nan"))
        for bad in ((2, 96), (2, 96, 0), (2.0, 96, 128), "2x96x128", 7):
            with pytest.raises(ValueError, match="frames"):
                cls(object(), 2, 64, 64, frames=bad)
        with pytest.raises(ValueError, match="frames"):
            cls(object(), 2, 64, 64, track=True)
        with pytest.raises(ValueError, match="track_min_joints"):
            cls(object(), 2, 64, 64, frames=(2, 96, 128), track=True, track_min_joints=0)


def test_track_frames_cli_flags():
    from lighthand_amd.tools import track_frames as T
    args = T.build_parser().parse_args(["--synthetic", "8", "--frame_size", "96x128"])
    assert (args.synthetic, args.frame_size, args.hands, args.flip_test, args.dark_decode) == (8, (96, 128), 2, False, False)
    args = T.build_parser().parse_args(["--synthetic", "4", "--frame_size", "1080x1920", "--hands", "1", "--flip_test", "--dark_decode"])
    assert (args.frame_size, args.hands, args.flip_test, args.dark_decode) == ((1080, 1920), 1, True, True)
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--synthetic", "4", "--frame_size", "96"])
    frames, boxes = T.synthetic_sequence(3, 96, 128, 2, seed=1)
    again, _ = T.synthetic_sequence(3, 96, 128, 2, seed=1)
    assert frames.shape == (3, 96, 128, 3) and frames.dtype == np.uint8 and boxes.shape == (2, 4) and boxes.dtype == np.float32
    assert (frames == again).all() and frames.max() > 0
