"""CPU: the host side of the sub-pixel heat-map coding -- the C-ABI entries lh_gaussian_target_sub / lh_heatmap_dark (exported,
declared, arguments validated before any launch), the option checks of the Python surface and the CLI flags."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT


def test_entries_are_exported_declared_and_bound_with_the_header_arity():
    from lighthand_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lighthand_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(lh_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S))
    for name, arity in (("lh_gaussian_target_sub", 12), ("lh_heatmap_dark", 10)):
        assert name in protos, f"{name} is not declared in the header"
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert len(protos[name].split(",")) == len(_lib.SIGNATURES[name][1]) == arity, name


def test_dark_validates_arguments_without_gpu():
    from lighthand_amd import _lib
    lib = _lib.load()
    hm, idx, mv, p = (C.c_void_p(a) for a in (0x100000, 0x200000, 0x300000, 0x400000))    # never dereferenced

    def dark(hm=hm, idx=idx, mv=mv, bj=21, h=64, w=64, k=11, p=p):
        return lib.lh_heatmap_dark(hm, idx, mv, bj, h, w, k, 4.0, p, None)
    for rc in (dark(hm=None), dark(idx=None), dark(mv=None), dark(p=None), dark(bj=0), dark(bj=-2), dark(h=0), dark(w=-1)):
        assert rc == -1 and b"lh_heatmap_dark" in lib.lh_last_error()
    for k in (10, 4, 2, 1, 0, -3, 19, 21):                           # even, below 3, above 17
        assert dark(k=k) == -1 and b"blur_kernel" in lib.lh_last_error(), k
    for h, w in ((96, 97), (97, 96), (128, 128), (1, 96 * 96 + 1), (1 << 16, 1 << 16)):
        assert dark(h=h, w=w) == -1 and b"lh_heatmap_dark" in lib.lh_last_error(), (h, w)


def test_target_sub_validates_arguments_without_gpu():
    from lighthand_amd import _lib
    lib = _lib.load()
    j, t, wt, vis = (C.c_void_p(a) for a in (0x100000, 0x200000, 0x300000, 0x400000))

    def sub(j=j, jstride=2, vis=None, vstride=0, radius=6, sigma=2.0, t=t, wt=wt, b=2, nj=21, size=64):
        return lib.lh_gaussian_target_sub(j, jstride, vis, vstride, radius, sigma, t, wt, b, nj, size, None)
    for rc in (sub(j=None), sub(t=None), sub(jstride=1), sub(vis=vis, vstride=0), sub(radius=-1), sub(sigma=0.0), sub(sigma=-2.0),
               sub(sigma=float("nan")), sub(b=0), sub(nj=0), sub(size=0)):
        assert rc == -1 and b"lh_gaussian_target_sub" in lib.lh_last_error()


def test_invalid_decode_and_encoding_options_raise():
    from lighthand_amd import heatmap
    from lighthand_amd._lib import LightHandError
    from lighthand_amd.runtime import InferPipeline, InferStep, TrainStep
    assert [heatmap.decode_mode(v) for v in (False, None, True, "quarter", "dark")] == [None, None, "quarter", "quarter", "dark"]
    maps = torch.zeros(1, 1, 8, 8)
    for bad in ("Dark", "taylor", "", 2, 0.5, b"dark"):
        with pytest.raises(ValueError, match="post_process"):
            heatmap.max_preds_device(maps, post_process=bad)
        with pytest.raises(ValueError, match="post_process"):
            heatmap.get_max_preds(maps.numpy(), post_process=bad)
        with pytest.raises(ValueError, match="post_process"):
            InferStep(object(), 2, 64, 64, post_process=bad)
        with pytest.raises(ValueError, match="post_process"):
            InferPipeline(object(), 2, 64, 64, post_process=bad)
    for bad in ("dark", "subpixel", None, True):
        with pytest.raises(ValueError, match="target_encoding"):
            TrainStep(object(), 2, 64, 64, target_encoding=bad)
    with pytest.raises(LightHandError, match="targets_from_joints"):
        TrainStep(object(), 2, 64, 64, target_encoding="unbiased", targets_from_joints=False)


def test_defaults_keep_the_present_behaviour():
    from lighthand_amd import heatmap
    from lighthand_amd.runtime import InferPipeline, InferStep, TrainStep
    from lighthand_amd.tools import wearable_eval_2d as E
    for fn in (heatmap.render_targets, heatmap.generate_target):
        assert inspect.signature(fn).parameters["unbiased"].default is False
    for fn in (heatmap.max_preds_device, heatmap.get_max_preds, InferStep.__init__, InferPipeline.__init__, E._Steps.__init__,
               E.pred_store, E.pred_store_test, E.device_eval):
        p = inspect.signature(fn).parameters
        assert p["post_process"].default is False and p["blur_kernel"].default == 11, fn
    assert inspect.signature(TrainStep.__init__).parameters["target_encoding"].default == "quantised"


def test_cli_flags():
    from lighthand_amd.tools import train as T
    from lighthand_amd.tools import wearable_eval_2d as E
    a = T.parse_args([])
    assert a.unbiased_target is False and a.dark_decode is False
    a = T.parse_args(["--unbiased_target", "--dark_decode"])
    assert a.unbiased_target is True and a.dark_decode is True
    e = E.build_parser().parse_args([])
    assert (e.dark_decode, e.blur_kernel, e.post_process) == (False, 11, False)
    e = E.build_parser().parse_args(["--dark_decode", "--blur_kernel", "7"])
    assert (e.dark_decode, e.blur_kernel, e.post_process) == (True, 7, False)
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(["--blur_kernel", "wide"])
    with pytest.raises(SystemExit) as err:
        E.main(["--synthetic", "4", "--post_process", "--dark_decode"])
    assert err.value.code == 2                                       # argparse's error exit, before any model is built
