"""The table in force (tests/golden/kernel_ceilings.json, what tests/test_kernel_resources.py holds every built kernel to) only extends
the first table, tests/golden/kernel_resources.json, which stays frozen as committed: every entry of the frozen table is in the table in
force with [scratch bytes, spilled VGPRs] no higher.  A change that adds kernels adds entries; no entry rises.  The kernels of top-down
inference on full frames (csrc/roi_track.hip, csrc/frames_crop.hip) are listed, with no scratch memory and no spills.  Reads the two JSON files only: no GPU."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPDOWN = ("box_affine_kernel", "frames_crop_kernel", "keypoints_to_boxes_kernel")


def _tables():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    assert kr.GOLDEN != kr.FROZEN
    with open(kr.FROZEN) as f, open(kr.GOLDEN) as g:
        return json.load(f), json.load(g)


def test_table_in_force_only_extends_the_frozen_table():
    frozen, table = _tables()
    assert len(frozen) > 500
    missing = sorted(k for k in frozen if k not in table)
    assert not missing, f"{len(missing)} kernels of kernel_resources.json left kernel_ceilings.json: {missing[:5]}"
    higher = {k: (table[k], v) for k, v in frozen.items() if table[k][0] > v[0] or table[k][1] > v[1]}
    assert not higher, f"(in force, frozen) ceilings that rose: {dict(list(higher.items())[:8])}"


def test_topdown_kernels_are_listed_without_scratch_or_spills():
    frozen, table = _tables()
    for name in TOPDOWN:
        hits = {k: v for k, v in table.items() if name in k}
        assert hits and not any(k in frozen for k in hits), name
        assert all(v == [0, 0] for v in hits.values()), hits
    assert len([k for k in table if "frames_crop_kernel" in k]) == 3          # fp32, bf16, fp16
