"""Every epilogue mode of the two PERSISTENT convolution kernels -- pointwise (igemm_pw_kernel.h, all 14 compiled configurations) and direct
3x3 (conv3x3_direct_kernel.h, 32 and 64 input channels) -- straight through the C ABI with the configuration forced in lh_igemm_desc.cfg
(cfg[2] == 1 / == 100).  Their epilogue is igemm_wave_epilogue.h, not the tiled kernel's, and STATS / GATE are template parameters that
change the kernels' structure (the pointwise kernel's double-buffered operand path depends on STATS): each of plain, statistics, one-term
gate and two-term gate is an instantiation of its own.  Helpers, host model and assertions are those of tests/test_gpu_epilogue_modes.py
(see there for the data flavours and what is compared bit for bit); the cases are in tests/exact_data.py, their preconditions are proved on
the CPU by tests/test_exact_host.py.

Short cases (every configuration x every mode, three flavours).  Pointwise: one tap, 2 x 13 x 11 = 286 pixels (ragged against 16, 32 and 64
pixels per wave step), 136 output channels (a part-filled 256-channel panel, a second 128-channel block of 8 channels, a third 64-channel
block of 8), one K run per panel K, ragged against it: 40 (panel 64), 72 (128), 136 (256: the fourth 64-element sub-panel comes from the
zero page), 264 (512).  The K = 72 case has operand rows of 80 elements whose slack is NaN, the K = 136 case output rows of 144 elements
whose slack must keep the sentinel (not in the modes with mask bits, which need a dense output); the K = 40 case also runs on the tiled
64 x 64 form, which must store the same bits.  Direct: nine taps, 2 x 21 x 19 (ragged against the 16 x 16 tiles, every border), 136 channels.

Long cases (one per configuration): the grids of these kernels are capped, but by the number of tiles as well, so a launch of a few
hundred pixels ends after ONE trip of the tile loop.  Here every wave of a pointwise launch / workgroup of a direct launch takes at least
two tiles and some take three, at any occupancy the library may pick (exact_data.py has the arithmetic; the test asserts it from the rows
the library reports): the B0 / B1 alternation, the operand loads issued under the previous tile's stores, the direct kernel's patch double
buffer, its staging area aliased onto the finished patch, its counted waits, and the statistics carried in registers across tiles all run.
"exact_small" data: the stored bits are compared in full and the sums row of the slab equals the fp64 sums of the stored values."""
import ctypes as C

import pytest

import exact_data as E
import test_gpu_epilogue_modes as T

pytestmark = pytest.mark.gpu

PW_SHORT = [f"pw{k}" for k in E.PW_K.values()]
D3_SHORT = ["d32", "d64"]
LONG_MODES = ["plain", "stats", "addend_mask", "gate_x", "gate_mask"]
# (long case, precision): the cases of one K class and precision follow each other, so their shared data is made once
LONG_PW = [(c, p) for k in E.PW_K.values() for p in ("bf16", "fp16") for c, b in E.EPILOGUE_BASE.items() if b == f"long_pw{k}"]
LONG_D3 = [(c, p) for c in ("long_d32", "long_d64") for p in ("bf16", "fp16")]


def test_the_forms_are_the_compiled_pointwise_configurations():
    """Every case's forms are exactly the pointwise configurations lh_igemm_candidates offers it, all 14 are covered, and the direct cases
    are offered the direct kernel."""
    from lighthand_amd import _lib
    lib = _lib.load()
    seen = set()
    for case in PW_SHORT + D3_SHORT:
        d = T._desc(case, T.CASES[case][14][0])
        buf = (C.c_int * (5 * 320))()
        nc = lib.lh_igemm_candidates(C.byref(d), 1, buf, 320)
        cands = {tuple(buf[5 * i:5 * i + 4]) for i in range(nc)}
        ours = {T.FORMS[f] for f in T.CASES[case][14]}
        assert {c for c in cands if c[2] in (1, 100)} == {c for c in ours if c[2] in (1, 100)}, (case, cands)
        assert ours <= cands, (case, ours - cands)
        seen |= {c for c in ours if c[2] == 1}
    assert seen == {(bm, 16 * pt, 1, kc) for bm, kc, pt in E.PW_CFGS} and len(seen) == 14


@pytest.mark.parametrize("flavour", ["random", "exact", "exact_small"])
@pytest.mark.parametrize("mode", T.MODES + ["gate2"])
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("case", PW_SHORT)
def test_pointwise_epilogue_mode_on_every_configuration(case, precision, mode, flavour):
    T._check(case, precision, mode, flavour)


@pytest.mark.parametrize("flavour", ["random", "exact", "exact_small"])
@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("case", D3_SHORT)
def test_direct3x3_epilogue_mode(case, precision, mode, flavour):
    T._check(case, precision, mode, flavour)


def _trips(case, precision, modes):
    """The tile counts of a long case, from the rows the library reports for its statistics / gate instantiations (one row per workgroup of
    a channel block): every unit -- a wave of the pointwise kernel, a workgroup of the direct one -- takes at least two tiles, some three."""
    from lighthand_amd import _lib
    lib = _lib.load()
    n, ho, wo, cout = T.CASES[case][0], T.CASES[case][4], T.CASES[case][5], T.CASES[case][6]
    form = T.CASES[case][14][0]
    bm, bp, depth, _ = T.FORMS[form]
    d = T._desc(case, form)
    if depth == 1:
        ntile, per_row, cap = (n * ho * wo + bp - 1) // bp, 4, E.pw_long_grid_cap(bm, cout)
    else:
        ntile, per_row, cap = n * ((ho + 15) // 16) * ((wo + 15) // 16), 1, 512 // ((cout + 63) // 64) // 8 * 8
    assert (n * ho * wo) % 16 != 0 and ntile >= 2 * per_row * cap + 1, (case, ntile, cap)      # whatever the occupancy (plain launches report no rows)
    rows = {"stats": lib.lh_igemm_stats_rows(C.byref(d), T._DT[precision]), "gate": lib.lh_igemm_gated_rows(C.byref(d), T._DT[precision], 1)}
    if "gate2" in modes:
        rows["gate2"] = lib.lh_igemm_gated_rows(C.byref(d), T._DT[precision], 2)
    for what, r in rows.items():
        units = per_row * r
        assert 0 < r <= cap and ntile >= 2 * units + 1, (case, what, r, ntile)
        print(f"{case} {precision} {form}: {n * ho * wo} pixels, {ntile} tiles; {what}: {r} slab rows, {units} "
              f"{'waves' if depth == 1 else 'workgroups'} per channel block, {ntile // units}..{-(-ntile // units)} tiles each")


@pytest.mark.parametrize("case,precision", LONG_PW)
def test_pointwise_tile_loop(case, precision):
    modes = LONG_MODES + ["gate2"]
    _trips(case, precision, modes)
    for mode in modes:
        T._check(case, precision, mode, "exact_small")


@pytest.mark.parametrize("case,precision", LONG_D3)
def test_direct3x3_tile_loop(case, precision):
    _trips(case, precision, LONG_MODES)
    for mode in LONG_MODES:
        T._check(case, precision, mode, "exact_small")


def test_two_batchnorm_terms_are_refused_on_the_direct_kernel():
    from lighthand_amd import _lib
    assert T._launch("d64", "bf16", "gate2", "direct 64", status_only=True) == -3           # LH_ERR_UNSUPPORTED
    assert b"two BatchNorm terms are gated by the pointwise kernel only" in _lib.load().lh_last_error()


def test_direct_kernel_is_refused_for_40_input_channels():
    """The direct kernel exists for 32 and 64 input channels per tap: cfg[2] == 100 on a K run of 40 is no legal choice."""
    from lighthand_amd import _lib
    T.FORMS["direct 40"] = (64, 256, 100, 40)
    try:
        assert T._launch("c136", "bf16", "plain", "direct 40", status_only=True) == -1       # LH_ERR_ARG
    finally:
        del T.FORMS["direct 40"]
    assert b"direct 3x3 configuration (64, 256, 100, 40) does not fit" in _lib.load().lh_last_error()
