"""Scratch memory and register spills of every kernel in the built library, held to a committed table (VERDICT E2).

Round 6 put the BatchNorm-backward gate behind run-time switches in the tiled convolution kernel's shared epilogue; every 256-pixel tile
went into scratch memory (208 B, 110 spilled VGPRs) and nothing noticed.  tests/golden/kernel_resources.json lists, per kernel symbol of
the gfx950 code objects, [.private_segment_fixed_size, .vgpr_spill_count] as the committed sources compile (tools/kernel_resources.py
--write regenerates it).  A kernel above its entry, or missing from the table, fails; a kernel below its entry passes (lower the entry
with the change that earned it).  The plain tiled kernels (igemm_ring_kernel, igemm_ring_multi_kernel) must read 0 / 0 whatever the table
says.  Reads the metadata notes only (llvm-objcopy, llvm-readelf): no GPU."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def resources():
    kr = _tool()
    if not os.path.exists(kr.LIB):
        pytest.skip("lighthand_amd/liblighthand_hip.so is not built")
    if not kr.tools_present():
        pytest.skip("llvm-readelf / llvm-objcopy of the ROCm installation are not on this machine")
    with open(kr.GOLDEN) as f:
        return kr.read_resources(), json.load(f)


def test_no_kernel_exceeds_its_committed_scratch_and_spill_figures(resources):
    built, table = resources
    assert len(built) > 500, f"only {len(built)} kernels found in the library's code objects"
    missing = sorted(k for k in built if k not in table)
    assert not missing, f"{len(missing)} kernels have no entry in tests/golden/kernel_resources.json (tools/kernel_resources.py --write): {missing[:5]}"
    worse = {k: (v, table[k]) for k, v in built.items() if v[0] > table[k][0] or v[1] > table[k][1]}
    assert not worse, f"[scratch bytes, spilled VGPRs] (built, committed ceiling) of {len(worse)} kernels: {dict(list(worse.items())[:8])}"


def test_plain_tiled_convolution_kernels_use_no_scratch(resources):
    built, table = resources
    plain = [k for k in built if "igemm_ring_kernel" in k or "igemm_ring_multi_kernel" in k]
    gated = [k for k in built if "igemm_ring_gated_kernel" in k]
    assert len(plain) >= 60 and len(gated) >= 60, (len(plain), len(gated))
    for src in (built, table):
        bad = {k: src[k] for k in plain if src.get(k, [1, 1]) != [0, 0]}
        assert not bad, f"plain tiled kernels with scratch memory or spills: {bad}"
    # the gated 256-pixel tiles may keep scratch, but no more than they had inside the shared epilogue (208 B / 200 B)
    for k in gated:
        assert built[k][0] <= (208 if "Li256ELi256E" in k else 200), (k, built[k])
