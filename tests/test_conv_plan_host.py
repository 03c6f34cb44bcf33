"""CPU: which kernel and configuration a convolution launch resolves to, pinned to tests/golden/conv_plan.json.

The fixture was recorded (tools/conv_plan_dump.py --write) from the library as it stood BEFORE the host layer of the forward /
data-gradient convolution was split by role and given one kernel-kind rule and one resolver; it is never regenerated from refactored
code.  Per descriptor, element type and configuration (the default, cfg = 0, and every candidate the library offers): the status and
result of lh_igemm_config, what lh_igemm_tile reports, the candidate count and a CRC of the candidate list IN ORDER (the tuner breaks
ties by order), lh_igemm_stats_rows, lh_igemm_gated_rows for one and two terms, lh_igemm_phases_rows of the two phase sets, and the
refusals with the words of lh_last_error().  The rows of pointwise configurations come from an occupancy query that answers differently
with and without a device: for those the test asserts what tests/test_cabi.py does, a multiple of 8 in 8..512.

lighthand_amd._lib.conv_kind is the Python copy of the library's kind rule (lh_conv_kind, csrc/igemm_args.h): it names every configuration
the library offers and none of the codes the library refuses."""
import ctypes as C
import importlib.util
import json
import os

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("conv_plan_dump", os.path.join(ROOT, "tools", "conv_plan_dump.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden(tool):
    with open(tool.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dumped(tool):
    from lighthand_amd import _lib
    saved = os.environ.get("LH_DENSE_TILES")
    try:
        return tool.dump(_lib.load())               # (deletes LH_DENSE_TILES: the dense-wave forms are offered)
    finally:
        if saved is not None:
            os.environ["LH_DENSE_TILES"] = saved


def test_the_fixture_covers_every_kind_and_refusal(tool, golden):
    from lighthand_amd._lib import conv_kind
    assert os.path.getsize(tool.GOLDEN) < 256 * 1024
    assert golden["fields"] == tool.FIELDS
    rows = [r for v in golden["cases"].values() for r in v["rows"]]
    ok = [r for r in rows if r[4] == 0]
    assert len(ok) == len(rows) > 500, "a default or an offered candidate did not resolve when the fixture was recorded"
    assert {conv_kind(r[7]) for r in ok} == {"staged", "tiled", "dense", "pointwise", "direct"}
    assert any(r[5:7] == [256, 256] for r in ok), "no 256 x 256 tile"
    assert all(r[14:17] == [None] * 3 for r in ok if r[7] == 1) and all(None not in r[14:17] for r in ok if r[7] != 1)
    assert {r[8] for r in golden["refusals"]} == {-1, -3} and all(r[3] for r in golden["refusals"])
    assert sorted(golden["phases_rows"]) == sorted(f"{s} {t}" for s in tool.PHASE_SETS for t in tool.DTYPES)


def test_resolver_answers_are_pinned(tool, golden, dumped):
    assert sorted(dumped["cases"]) == sorted(golden["cases"])
    for case, want in golden["cases"].items():
        got = dumped["cases"][case]
        assert got["candidates"] == want["candidates"], (case, "candidate count / CRC of the list in order")
        assert len(got["rows"]) == len(want["rows"])
        for g, w in zip(got["rows"], want["rows"]):
            if w[7] == 1 and w[4] == 0:             # pointwise: everything but the row counts
                assert g[:14] == w[:14] and g[14:17] == [None] * 3, (case, dict(zip(tool.FIELDS, zip(g, w))))
            else:
                assert g == w, (case, dict(zip(tool.FIELDS, zip(g, w))))
    assert dumped["phases_rows"] == golden["phases_rows"]


def test_pointwise_rows_are_whole_groups_of_eight(tool, golden):
    from lighthand_amd import _lib
    lib = _lib.load()
    descs, seen = tool.descriptors(), 0
    for case, want in golden["cases"].items():
        name, tname = case.rsplit(" ", 1)
        for w in want["rows"]:
            if w[7] != 1:
                continue
            d, dt = descs[name], tool.DTYPES[tname]
            tool.set_cfg(d, w[:4])
            rows = [lib.lh_igemm_stats_rows(C.byref(d), dt), lib.lh_igemm_gated_rows(C.byref(d), dt, 1), lib.lh_igemm_gated_rows(C.byref(d), dt, 2)]
            tool.set_cfg(d, (0, 0, 0, 0))
            assert all(8 <= r <= 512 and r % 8 == 0 for r in rows), (case, w[:4], rows)
            seen += 1
    assert seen >= 8                                # two 1x1 descriptors, two 16-bit types, two or more panels each


def test_refusals_are_pinned(tool, golden):
    from lighthand_amd import _lib
    lib = _lib.load()
    descs = tool.descriptors()
    assert [r[:3] + r[4:8] for r in golden["refusals"]] == [[n, t, s] + list(c) for n, t, c, s in tool.REFUSALS]
    for name, tname, text, _, *want in golden["refusals"]:
        d, dt = descs[name], tool.DTYPES[tname]
        assert tool.record(lib, d, dt, want[:4]) == want, (name, tname, want[:4])
        tool.set_cfg(d, want[:4])
        assert lib.lh_igemm_config(C.byref(d), dt, (C.c_int * 5)()) == want[4] and text.encode() in lib.lh_last_error(), (name, want[:4], text)
        # the launch answers as lh_igemm_config does, before it looks at a pointer it would use
        assert lib.lh_igemm(C.byref(d), 16, 16, 16, None, None, None, None, None, None, dt, None) == want[4]
        assert text.encode() in lib.lh_last_error()
        tool.set_cfg(d, (0, 0, 0, 0))


def test_python_kind_rule_agrees_with_the_library(tool, golden):
    from lighthand_amd import _lib
    lib = _lib.load()
    for case, want in golden["cases"].items():
        for w in want["rows"]:
            assert _lib.conv_kind(w[7]) is not None, (case, w)
            assert (_lib.conv_kind(w[7]) == "staged") == (w[13] == 0), (case, w)      # lh_igemm_tile's ring = 0: the register-staged kernel
    d = tool.descriptors()["3x3 256->128 16x16"]
    for depth in list(range(10, 20)) + list(range(30, 100)):
        assert _lib.conv_kind(depth) is None, depth
        tool.set_cfg(d, (128, 128, depth, 128))
        assert lib.lh_igemm_config(C.byref(d), _lib.LH_BF16, (C.c_int * 5)()) == -3 and b"not compiled in" in lib.lh_last_error(), depth
    assert [_lib.conv_kind(v) for v in (0, 1, 2, 9, 20, 29, 100)] == ["staged", "pointwise", "tiled", "tiled", "dense", "dense", "direct"]


def test_gate_aware_choice_follows_the_kind_rule():
    """BnGate._cfg_gateable (the tuner's "does this candidate take the gate"): with the default switches, one BatchNorm term is gated by
    every kernel but the register-staged one, two terms by the pointwise kernel alone -- what lh_igemm_gated accepts (lh_kind_gated,
    lh_kind_gates_two in csrc/igemm_args.h) -- and by no code that names no kernel."""
    import types
    from lighthand_amd.bn_gate import BnGate
    from lighthand_amd.options import PlanOptions
    me = types.SimpleNamespace(opt=PlanOptions.from_env({}))
    for depth, one, two in ((0, False, False), (1, True, True), (3, True, False), (22, True, False), (100, True, False), (12, False, False),
                            (32, False, False)):
        cfg = (128, 128, depth, 128)
        assert [BnGate._cfg_gateable(me, cfg, k, 1 << 20) for k in ("x", "mask", "mask2")] == [one, one, two], depth
