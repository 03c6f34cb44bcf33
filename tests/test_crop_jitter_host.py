"""CPU: ColorJitter on the frame crop, the host side -- topdown.frames_crop_jitter_host (the numpy restatement the GPU tests hold
lh_frames_crop_jitter_to_nhwc4 to, tests/test_gpu_crop_jitter.py) against the un-jittered host crop, against oracle/color.py and on a
closed-form case; TrainStep's crop_jitter rules through the device-free validation function; the two C-ABI entries (declared, bound,
arguments validated without a GPU); and the kernel table, which the feature must not extend."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import crop_jitter_data as D
from conftest import ROOT

F = np.float32
NEW = ("lh_frames_crop_jitter_workspace_bytes", "lh_frames_crop_jitter_to_nhwc4")
ZERO, ONE = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)          # mean / std that make Normalize the identity: (c - 0) * (1 / 1) = c


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _mats(scale=(0.4, 1.1), padding=1.0):
    from lighthand_amd.topdown import roi_affine_host
    boxes, rot, mirror, index = D.rois(scale=scale)
    return roi_affine_host(boxes, rot, mirror, index, D.N_FRAMES, (D.SIZE, D.SIZE), padding)


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("case", ["rgb", "antialias", "nv12"])
def test_no_op_orders_are_the_plain_host_crop_bit_for_bit(case):
    from lighthand_amd import topdown as T
    frames = D.frames()
    mat, src = _mats((2.5, 3.2) if case == "antialias" else (0.4, 1.1))
    factors, _ = D.draw()
    order = np.full((D.B, 4), -1, np.int32)
    if case == "nv12":
        nv = T.rgb_to_nv12_host(frames)
        want = T.frames_crop_nv12_host(nv, (D.HS, D.WS), mat, src, (D.SIZE, D.SIZE), max_taps=2)
        got = T.frames_crop_jitter_host(nv, mat, src, (D.SIZE, D.SIZE), factors, order, max_taps=2, frame_format="nv12", frame_size=(D.HS, D.WS))
    else:
        taps = 4 if case == "antialias" else 1
        if taps > 1:
            assert (T.crop_taps_host(mat, taps)[src >= 0] > 1).all()
        want = T.frames_crop_host(frames, mat, src, (D.SIZE, D.SIZE), max_taps=taps)
        got = T.frames_crop_jitter_host(frames, mat, src, (D.SIZE, D.SIZE), factors, order, max_taps=taps)
    assert got.dtype == np.float32 and got.shape == (D.B, 3, D.SIZE, D.SIZE) and np.array_equal(_bits(got), _bits(want))
    assert np.abs(want).max() > 1 and src[5] == -1


def test_restatement_agrees_with_the_oracle_and_with_its_own_fp64_evaluation():
    """frames_crop_jitter_host against oracle.color.color_jitter (the independent statement of torchvision's published arithmetic)
    applied to the un-normalised host crop, on the 28 slots of crop_jitter_data (seed 20: two noise frames and a grey one, ROIs of
    0.4 .. 1.1 frame pixels per crop pixel reaching past the frame, all 24 op orders, no op, skips, both range ends), under the
    criterion of test_color_jitter_input_pipeline_matches_oracle: per slot fewer than 1e-3 of the values differ by more than 1e-4 and
    the median difference is below 1e-6.  The share is a cap on what rounding may flip (a hue sector, a clamp): the same restatement
    evaluated in fp64 on the same samples must leave at most half of it, 5e-4, to the fp32 order of operations itself -- that is what
    the seed was checked for; both shares are printed."""
    from lighthand_amd import topdown as T
    from oracle import color as oc
    frames = D.frames()
    mat, src = _mats()
    factors, order = D.draw()
    size = (D.SIZE, D.SIZE)
    unit = T.frames_crop_host(frames, mat, src, size, mean=ZERO, std=ONE)
    assert unit.min() == 0 and 0.9 < unit.max() <= 1 and not unit[5].any()
    outside = (unit == 0).all(1).mean((1, 2))
    assert (outside[src >= 0] > 0.05).sum() >= 8                                     # many crops do reach past the frame
    m, s = F(T.MEAN)[:, None, None], F(T.STD)[:, None, None]
    want = np.stack([((oc.color_jitter(unit[i], factors[i], [int(v) for v in order[i]]) - m) / s).astype(np.float32) for i in range(D.B)])
    got = T.frames_crop_jitter_host(frames, mat, src, size, factors, order)
    got64 = T.frames_crop_jitter_host(frames, mat, src, size, factors, order, dtype=np.float64)
    assert got.dtype == np.float32 and got64.dtype == np.float64
    share64, med64 = D.mismatch(got, got64)
    share, med = D.mismatch(got, want)
    print(f"fp32 restatement vs its fp64 evaluation: share {share64:.2e} (cap 5e-4), median {med64:.2e}; vs oracle.color: share {share:.2e} "
          f"(cap 1e-3), median {med:.2e}")
    assert share64 <= 5e-4 and med64 < 1e-6
    assert share < 1e-3 and med < 1e-6
    changed = np.abs(got - T.frames_crop_host(frames, mat, src, size)).reshape(D.B, -1).max(1)
    assert changed[24] == 0 and changed[5] == 0 and (np.delete(changed, [5, 24]) > 0.05).all()          # the draw does something everywhere else


def test_empty_slot_stays_black_and_grey_pixels_ignore_hue():
    from lighthand_amd import topdown as T
    frames = D.frames()
    mat, src = _mats()
    factors, order = D.draw()
    order[5] = (1, 3, 0, 2)
    size = (D.SIZE, D.SIZE)
    got = T.frames_crop_jitter_host(frames, mat, src, size, factors, order, mean=ZERO, std=ONE)
    assert not got[5].any()                                                          # every op maps black with mean 0 to black
    grey = np.flatnonzero((src == 1))
    assert len(grey) >= 8 and all(np.array_equal(got[i, 0], got[i, 1]) and np.array_equal(got[i, 0], got[i, 2]) for i in grey)
    only_hue = np.tile(np.int32([3, -1, -1, -1]), (D.B, 1))
    hue = T.frames_crop_jitter_host(frames, mat, src, size, factors, only_hue, mean=ZERO, std=ONE)
    plain = T.frames_crop_host(frames, mat, src, size, mean=ZERO, std=ONE)
    assert np.abs(hue[grey] - plain[grey]).max() <= 2.0 ** -23 and np.abs(hue[src == 0] - plain[src == 0]).max() > 0.1


@pytest.mark.parametrize("f", [0.6, 1.3])
def test_contrast_mean_counts_the_black_outside_closed_form(f):
    from lighthand_amd import topdown as T
    fr, boxes, want = D.half_outside_case(f=f)
    mat, src = T.box_affine_host(boxes, [0], 1, (D.SIZE, D.SIZE), 1.0)
    assert np.array_equal(mat, F([[1, 0, -32, 0, 1, 10]])) and src[0] == 0
    got = T.frames_crop_jitter_host(fr, mat, src, (D.SIZE, D.SIZE), F([[1, f, 1, 0]]), np.int32([[1, -1, -1, -1]]), mean=ZERO, std=ONE)
    assert np.array_equal(_bits(got[0]), _bits(want))
    if f < 1:                                                  # neither side clamps: the outside is (1 - f) * mean, not 0
        assert 0 < want[0, 0, 0] < want[0, 0, 63] < 1
    else:                                                      # (1 - f) * mean < 0 clamps to black; the inside is brighter than c
        assert want[0, 0, 0] == 0 and F(150) * (F(1) / F(255)) < want[0, 0, 63] < 1


# ------------------------------------------------------------------------------------------------ 2. TrainStep's rules
def test_crop_jitter_rules_before_any_device_work():
    from lighthand_amd.runtime import TrainStep, _check_train_frames as check
    fr = (4, 96, 128)
    got = check(None, fr, crop_jitter=(0.5, 0.5, 0.5, 0.5))
    assert got == (fr, None, (0.5, 0.5, 0.5, 0.5)) and all(isinstance(v, float) for v in got[2])
    assert check(None, fr, roi_aug=(30, 0.25, 0.1, 0.5), crop_jitter=[0.4, 0, 0.2, 0.1])[2] == (0.4, 0.0, 0.2, 0.1)
    assert check(None, fr) == (fr, None, None)                                       # without the option: the same three values
    with pytest.raises(ValueError, match="crop_jitter"):
        check(None, None, crop_jitter=(0.5, 0.5, 0.5, 0.5))
    for bad in ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5, 0.5, 0.5), (0.5, -0.5, 0.5, 0.5), (0.5, 0.5, 0.5, -0.1), (0.5, 0.5, 0.5, 0.6), 0.5, "0.5",
                (0.5, 0.5, float("nan"), 0.5), (True, 0.5, 0.5, 0.5)):
        with pytest.raises(ValueError, match="crop_jitter"):
            check(None, fr, crop_jitter=bad)
    with pytest.raises(ValueError, match="color_jitter") as e:
        check(None, fr, color_jitter=(0.5, 0.5, 0.5, 0.5))
    assert "crop_jitter" in str(e.value)                                             # the refusal names the option that does it
    with pytest.raises(ValueError, match="crop_jitter"):
        TrainStep(object(), 2, 64, 64, crop_jitter=(0.5, 0.5, 0.5, 0.5))
    with pytest.raises(ValueError, match="crop_jitter"):
        TrainStep(object(), 2, 64, 64, frames=fr, crop_jitter=(0.5, 0.5))


def test_train_cli_turns_ratio_of_aug_into_crop_jitter():
    import torch
    from lighthand_amd.tools import train as T
    ds = T._FramesWithAugFlag(T.SyntheticFrames(5, (96, 128), 3), 0.6)
    assert len(ds) == 5 and [ds[i][3] for i in range(5)] == [True, True, True, False, False]
    frame, jt, box, _ = ds[2]
    assert frame.dtype == torch.uint8 and tuple(jt.shape) == (21, 2) and tuple(box.shape) == (4,)


# ------------------------------------------------------------------------------------------------ 3. the C ABI and the kernel table
def test_entries_are_declared_bound_and_validate_arguments_without_gpu():
    from lighthand_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lighthand_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.lh_frames_crop_jitter_workspace_bytes(28) == 28 * 32 * 8 == lib.lh_image_jitter_workspace_bytes(28)
    assert lib.lh_frames_crop_jitter_workspace_bytes(0) == 0
    p = [C.c_void_p(0x1000 * i) for i in range(1, 8)]          # never dereferenced: validation fails before any launch
    m3, s3, csc = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25), (C.c_float * 12)(*([1.0] * 12))

    def crop(frames=p[0], out=p[1], b=4, n=2, hs=96, ws=128, pitch=128, uv=96 * 128, stride=96 * 128 * 3 // 2, siting=0, csc12=None, h=64, w=64,
             pad=1, wp=66, mat=p[2], src=p[3], taps=1, factors=p[4], order=p[5], workspace=p[6], dtype=0):
        return lib.lh_frames_crop_jitter_to_nhwc4(frames, out, b, n, hs, ws, pitch, uv, stride, siting, csc12, h, w, pad, wp, m3, s3, mat, src,
                                                  taps, factors, order, workspace, dtype, None)
    for rc in (crop(factors=None), crop(order=None), crop(workspace=None), crop(workspace=C.c_void_p(0x7004)), crop(frames=None), crop(out=None),
               crop(mat=None), crop(src=None), crop(b=0), crop(b=65536), crop(wp=65), crop(taps=0), crop(taps=9), crop(dtype=7),
               crop(out=C.c_void_p(0x2004)),
               # NV12 (csc12 given): the layout rules of the entry it extends
               crop(csc12=csc, hs=95), crop(csc12=csc, pitch=127), crop(csc12=csc, uv=96 * 128 - 1), crop(csc12=csc, stride=96 * 128),
               crop(csc12=csc, siting=2)):
        assert rc == -1 and b"lh_frames_crop_jitter_to_nhwc4" in lib.lh_last_error(), lib.lh_last_error()


def test_the_feature_adds_no_kernel_symbol_and_keeps_the_crop_out_of_scratch():
    """The grey-mean reduction and the jitter run as modes of frames_crop_kernel: the table in force (kernel_ceilings_roi.json, entry for
    entry as committed) lists every kernel of the built library, and the three instantiations of the crop stay at [0, 0] scratch
    bytes and spilled VGPRs."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    assert os.path.basename(kr.GOLDEN) == "kernel_ceilings_roi.json"
    with open(kr.GOLDEN) as f:
        table = json.load(f)
    crops = ["_Z18frames_crop_kernelIfEv8CropArgs", "_Z18frames_crop_kernelIDF16bEv8CropArgs", "_Z18frames_crop_kernelIDF16_Ev8CropArgs"]
    assert all(table[k] == [0, 0] for k in crops) and not [k for k in table if "jitter" in k and "crop" in k]
    if not os.path.exists(kr.LIB) or not kr.tools_present():
        return
    built = kr.read_resources()
    assert not [k for k in built if k not in table]
    assert all(built[k] == [0, 0] for k in crops)
    for k in (k for k in built if "image_u8_kernel" in k or "jitter_mean_kernel" in k):          # the uint8 kernels that share the helpers
        assert built[k][0] <= table[k][0] and built[k][1] <= table[k][1], k
