"""Cost of the flip test on the evaluation workload: R50, 64 x 256 x 256, bf16, eval-mode InferStep (captured graph).

Default: step times of the plain step, the flip-test step and the flip-test step with post_process, alternated in one process
(device events around 20 replays, median and min of ``--rounds`` windows per variant), then the new kernels on their own at the
step's shapes, with device events: hot (back to back) and cold (a 512 MB write between launches evicts the Infinity Cache),
against their byte bounds at 6.3 TB/s.  ``--trace``: a short run for ``rocprofv3 --kernel-trace --stats`` (a few flip-test
replays and the standalone kernels), no timing.
usage (GPU box): python tools/flip_bench.py [--rounds 7] [--trace]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lighthand_amd import _lib  # noqa: E402

HBM = 6.3e12                      # achievable HBM bytes/s (float4 copy), MI355X
B, S, J, HM = 64, 256, 21, 64


def _events(f, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def steps(rounds):
    from lighthand_amd.modeling.simplebaseline.config import default_config
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    from lighthand_amd.runtime import InferStep
    torch.manual_seed(0)
    model = get_pose_net(default_config(50), is_train=True).cuda().set_precision("bf16").eval()
    x = torch.randn(B, 3, S, S, device="cuda")
    variants = {"plain": InferStep(model, B, S, S), "flip_test": InferStep(model, B, S, S, flip_test=True),
                "flip_test + post_process": InferStep(model, B, S, S, flip_test=True, post_process=True)}
    for st in variants.values():
        st(x)
        for _ in range(10):
            st()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(rounds):
        for k, st in variants.items():
            ts[k].append(_events(st, 20))
    med = {}
    for k, v in ts.items():
        v.sort()
        med[k] = v[len(v) // 2]
        print(f"R50 bs{B} {S}^2 bf16 eval InferStep {k:26s} median {med[k]:.3f} ms  min {v[0]:.3f}  max {v[-1]:.3f}")
    aim = 2 * med["plain"] + 0.08
    print(f"flip_test - 2 x plain = {med['flip_test'] - 2 * med['plain']:+.3f} ms (aim: <= +0.080; flip_test <= {aim:.3f} ms)")
    print(f"post_process adds {med['flip_test + post_process'] - med['flip_test']:+.3f} ms")
    p = variants["flip_test"]
    print(f"checksum preds {float(p.preds.sum()):.1f} maxvals {float(p.maxvals.sum()):.6f}")


def _kernel_calls():
    lib = _lib.load()
    pad = 3
    wp = S + 2 * pad + 2
    img = torch.randn(B, S + 2 * pad, wp, 4, device="cuda").to(torch.bfloat16)
    a = torch.randn(B, J, HM, HM, device="cuda")
    m = torch.randn(B, J, HM, HM, device="cuda")
    out = torch.empty_like(a)
    preds = torch.empty(B, J, 2, device="cuda")
    maxvals = torch.empty(B, J, 1, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    bj = B * J
    return {
        "lh_nhwc4_mirror": (lambda: _lib.check(lib.lh_nhwc4_mirror(img.data_ptr(), B, S, S, pad, wp, _lib.LH_BF16, s), "mirror"),
                            2.0 * B * S * S * 8),
        "lh_heatmap_flip_merge": (lambda: _lib.check(lib.lh_heatmap_flip_merge(a.data_ptr(), m.data_ptr(), bj, HM, HM, 1, 4.0, a.data_ptr(),
                                                                               preds.data_ptr(), maxvals.data_ptr(), None, s), "merge"),
                                  3.0 * bj * HM * HM * 4),
        "heat-map copy": (lambda: out.copy_(m), 2.0 * bj * HM * HM * 4),
    }


def kernels():
    calls = _kernel_calls()
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    for name, (f, nbytes) in calls.items():
        for _ in range(5):
            f()
        hot = _events(f, 50)
        cold = []
        for _ in range(20):
            flush.fill_(1)
            cold.append(_events(f, 1))
        cold.sort()
        bound = nbytes / HBM * 1e3
        print(f"{name:22s} {nbytes / 1e6:5.1f} MB  bound {bound * 1e3:5.1f} us  hot {hot * 1e3:6.1f} us ({bound / hot:4.0%})  "
              f"cold median {cold[10] * 1e3:6.1f} us ({bound / cold[10]:4.0%})")


def trace():
    from lighthand_amd.modeling.simplebaseline.config import default_config
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    from lighthand_amd.runtime import InferStep
    torch.manual_seed(0)
    model = get_pose_net(default_config(50), is_train=True).cuda().set_precision("bf16").eval()
    st = InferStep(model, B, S, S, flip_test=True, use_graph=False)
    x = torch.randn(B, 3, S, S, device="cuda")
    st(x)
    for _ in range(10):
        st()
    for f, _ in _kernel_calls().values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    print("trace run done")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if args.trace:
        trace()
    else:
        steps(args.rounds)
        kernels()
