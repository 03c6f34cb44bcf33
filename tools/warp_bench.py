"""Times the uint8 input kernels on the benchmark batch (64 frames 224 x 224 -> padded NHWC4 256 x 256 bf16): the plain pipeline,
the affine warp (rotation +-20 degrees, scale 0.75-1.25, shift +-10 %) and warp + ColorJitter.  ``--step``: instead, a captured
R50 bs64 bf16 TrainStep on uint8 input, without and with geometric_aug (fresh draws every step).
usage (GPU box): python tools/warp_bench.py [--step [--geo]]"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lighthand_amd import _lib  # noqa: E402
from lighthand_amd.runtime import sample_affine, sample_color_jitter  # noqa: E402


def _median_us(f, reps=50):
    f()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def kernels():
    lib = _lib.load()
    n, hs, ws, h, w, pad = 64, 224, 224, 256, 256, 3
    wp = w + 2 * pad + 2
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (n, hs, ws, 3), dtype=torch.uint8, generator=g).cuda()
    out = torch.empty(n, h + 2 * pad, wp, 4, dtype=torch.bfloat16, device="cuda")
    m3, s3 = (C.c_float * 3)(0.485, 0.456, 0.406), (C.c_float * 3)(0.229, 0.224, 0.225)
    inv, _ = sample_affine(n, 20.0, 0.25, 0.1, generator=g, size=(h, w))
    inv = inv.cuda()
    factors, order = (t.cuda() for t in sample_color_jitter(n, generator=g))
    wsp = torch.empty(lib.lh_image_jitter_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    base = (src.data_ptr(), out.data_ptr(), n, hs, ws, h, w, pad, wp, m3, s3)
    runs = {
        "u8 plain": lambda: _lib.check(lib.lh_image_u8_to_nhwc4(*base, _lib.LH_BF16, s), "plain"),
        "u8 jitter": lambda: _lib.check(lib.lh_image_u8_jitter_to_nhwc4(*base, factors.data_ptr(), order.data_ptr(), wsp.data_ptr(),
                                                                        _lib.LH_BF16, s), "jitter"),
        "u8 warp": lambda: _lib.check(lib.lh_image_u8_warp_to_nhwc4(*base, inv.data_ptr(), None, None, None, _lib.LH_BF16, s), "warp"),
        "u8 warp + jitter": lambda: _lib.check(lib.lh_image_u8_warp_to_nhwc4(*base, inv.data_ptr(), factors.data_ptr(), order.data_ptr(),
                                                                             wsp.data_ptr(), _lib.LH_BF16, s), "warp + jitter"),
    }
    for name, f in runs.items():
        print(f"{name:18s} {_median_us(f):7.1f} us, checksum {float(out.float().sum()):.4f}")


def step(geo):
    from lighthand_amd.modeling.simplebaseline.config import default_config
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    from lighthand_amd.runtime import TrainStep
    torch.manual_seed(0)
    model = get_pose_net(default_config(50), is_train=True).cuda().set_precision("bf16")
    st = TrainStep(model, 64, 256, 256, input_u8=(224, 224), geometric_aug=(20.0, 0.25, 0.1) if geo else None)
    x = torch.randint(0, 256, (64, 224, 224, 3), dtype=torch.uint8, device="cuda")
    j = torch.rand(64, 21, 2, device="cuda") * 200 + 28
    st(x, j)
    for _ in range(10):
        st()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            st()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / 20)
    ts.sort()
    print(f"R50 bs64 u8 step {'with' if geo else 'without'} geometric_aug: median {ts[2]:.3f} ms (min {ts[0]:.3f}), loss {float(st.loss):.6f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--geo", action="store_true")
    a = ap.parse_args()
    step(a.geo) if a.step else kernels()
