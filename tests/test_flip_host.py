"""CPU: the host side of the flip test -- the C-ABI entries lh_nhwc4_mirror / lh_heatmap_flip_merge (exported, declared,
arguments validated without a GPU), InferStep's refusal of shift_heatmap=False without flip_test, and the evaluation CLI's
flags."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NEW = ("lh_nhwc4_mirror", "lh_heatmap_flip_merge")


def test_flip_entries_are_exported_and_declared():
    from lighthand_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lighthand_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", text), name


def test_mirror_validates_arguments_without_gpu():
    from lighthand_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x1000)                                     # never dereferenced: validation fails before any launch
    good = dict(n=2, h=8, w=8, pad=3, wp=16, dtype=_lib.LH_BF16)

    def mirror(img=fake, **kw):
        a = dict(good, **kw)
        return lib.lh_nhwc4_mirror(img, a["n"], a["h"], a["w"], a["pad"], a["wp"], a["dtype"], None)
    for rc in (mirror(img=None), mirror(n=0), mirror(n=-1), mirror(h=0), mirror(w=0), mirror(pad=-1),
               mirror(wp=8 + 2 * 3 - 1), mirror(pad=5), mirror(dtype=3), mirror(n=1 << 20, h=1024, w=1024, pad=0, wp=1024)):
        assert rc == -1 and b"lh_nhwc4_mirror" in lib.lh_last_error()


def test_flip_merge_validates_arguments_without_gpu():
    from lighthand_amd import _lib
    lib = _lib.load()
    a, m, out = C.c_void_p(0x100000), C.c_void_p(0x200000), C.c_void_p(0x300000)     # 21 maps of 64 x 64 fp32: 344 KB each, 1 MB apart
    p, mv, idx = C.c_void_p(0x400000), C.c_void_p(0x500000), C.c_void_p(0x600000)

    def merge(a=a, m=m, bj=21, h=64, w=64, merged=out, preds=p, maxvals=mv):
        return lib.lh_heatmap_flip_merge(a, m, bj, h, w, 1, 4.0, merged, preds, maxvals, idx, None)
    for rc in (merge(a=None), merge(m=None), merge(merged=None), merge(preds=None), merge(maxvals=None), merge(bj=0),
               merge(bj=-3), merge(h=0), merge(w=0), merge(merged=m), merge(merged=C.c_void_p(0x100000 + 4096)),
               merge(m=C.c_void_p(0x300000 - 4))):
        assert rc == -1 and b"lh_heatmap_flip_merge" in lib.lh_last_error()


def test_infer_step_refuses_unshifted_merge_without_flip_test():
    from lighthand_amd.runtime import InferStep
    with pytest.raises(ValueError, match="flip_test"):
        InferStep(object(), 2, 64, 64, shift_heatmap=False)


def test_eval_cli_test_flags():
    from lighthand_amd.tools import wearable_eval_2d as E
    args = E.build_parser().parse_args([])
    assert (args.flip_test, args.post_process, args.shift_heatmap) == (False, False, True)
    args = E.build_parser().parse_args(["--flip_test", "--no_shift_heatmap", "--post_process"])
    assert (args.flip_test, args.post_process, args.shift_heatmap) == (True, True, False)
    with pytest.raises(SystemExit):
        E.main(["--synthetic", "4", "--no_shift_heatmap"])
