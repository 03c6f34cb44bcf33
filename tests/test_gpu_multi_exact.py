"""The multi-problem launches of the convolution and of the weight gradient, straight through the C ABI, held BIT FOR BIT against a host
reference: lh_igemm_multi (igemm_ring_multi_kernel) and lh_wgrad_fused_multi (wgrad_ring_multi_kernel, then wgrad_reduce_multi_kernel).

What only these forms have, and a comparison of merged with unmerged launches through the same host code cannot see: the by-value argument
array and lh_multi_pick (csrc/multi.h), the workgroup ranges first[] built from per-problem tile counts, the host-side reorder (longest K
loop / most stages per split first; of the weight gradient only the launch array -- the fold's array keeps caller order), lh_xcd_remap on a
problem-local index and count, groups of four with a lone fifth problem on the plain kernel, the flush logic of lh_wgrad_fused_multi and
the multi fold kernel.

Every comparison is torch.equal: the operands are the integer grids of tests/exact_data.py, on which every partial sum in any order stays
below 2^24 quanta (proved on the CPU by tests/test_exact_host.py), so a stored 16-bit value is ONE round-to-nearest-even of the fp64
result and an fp32 weight gradient equals the fp64 sum.  The tests bite without a mutated kernel: tests/test_exact_host.py asserts that any
two members of a call expect different values in every row they share, so a pointer paired with the wrong problem, a first[] that is a
tile off, or a slab row count taken from another member shows as wrong bits, an unwritten (NaN) row or a written sentinel.

A. lh_igemm_multi: the members are exact cases of tests/test_gpu_epilogue_modes.py with distinct data -- pw40 (1 tap, 286 pixels, 136
channels), phase (4 taps, strided placement into 18 x 14), m35 (35 pixels: one workgroup under a 128-channel tile), c72 and c136 (9 taps)
-- listed so that the library's sort permutes the first four and the fifth runs alone; n = 2 and n = 3 as well.  Every configuration of
LH_RING_CFGS_MID and LH_RING_CFGS_SMALL, bf16 and fp16; modes mixed across the members of a call (exact_data.MULTI_MODES), so that a
pointer taken from the wrong problem lands on a member that uses it differently.

B. lh_wgrad_fused_multi: members W1..W5 of exact_data.WGRAD_MULTI_CASES on every compiled four-wave configuration, with different split
counts, one accumulating member, one that writes the ConvTranspose layout, one with operand slack; calls that flush around a member on
the 256 x 256 tile and at a change of tile class; static plans.  Every workspace and every gradient tensor stands in front of a
sentinel block.

A launch that faults ends the session: nothing more is started on the device."""
import ctypes as C

import pytest
import torch

import exact_data as E
import test_gpu_epilogue_modes as T

pytestmark = pytest.mark.gpu

GUARD = 1024                  # floats (4 KiB) of sentinel around every statistics slab, behind every workspace, around every gradient
PRECISIONS = ["bf16", "fp16"]
_ids = lambda c: "x".join(map(str, c))


def _sync(what):
    """The one synchronisation of a call.  A fault leaves the device in no state to go on with: the session ends here."""
    try:
        torch.cuda.synchronize()
    except Exception as e:          # noqa: BLE001 -- whatever the runtime raises
        pytest.exit(f"{what}: the device faulted ({e}); nothing more is run", returncode=1)


def _guarded(inner, fill=float("nan")):
    """A float32 device buffer of `inner` elements (filled with `fill`) between two GUARD-element sentinel blocks: (whole, inner view)."""
    whole = torch.full((2 * GUARD + inner,), T.SENTINEL, dtype=torch.float32, device="cuda")
    whole[GUARD:GUARD + inner] = fill
    return whole, whole[GUARD:GUARD + inner]


def _guards_intact(whole):
    return bool((whole[:GUARD] == T.SENTINEL).all()) and bool((whole[-GUARD:] == T.SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# A. lh_igemm_multi
def _igemm_problem(case, mode, cfg, precision, flavour):
    """Descriptor, buffers and lh_igemm_call fields of one member.  EVERY member gets an output, a slab and (from the shared data) an
    addend; only what its mode names is handed to the library, the rest must come back unchanged."""
    from lighthand_amd import _lib
    lib = _lib.load()
    _, dv = T._data(case, precision, flavour)
    d = T._desc(case, "64x64", mode)
    for i, v in enumerate(cfg):
        d.cfg[i] = v
    d.relu = 1 if mode in ("relu", "affine_relu") else 0
    n, cout, OH, OW = T.CASES[case][0], T.CASES[case][6], T.CASES[case][7], T.CASES[case][8]
    out = torch.full((2 * T.MARGIN + n * OH * OW * cout,), T.SENTINEL, dtype=T._TD[precision], device="cuda")
    rows = lib.lh_igemm_stats_rows(C.byref(d), T._DT[precision])
    slab_whole, slab = _guarded(rows * 2 * cout)
    q = _lib.IgemmCall()
    q.d, q.in_, q.wpack, q.out = C.pointer(d), dv["x"].data_ptr(), dv["pack"].data_ptr(), out.data_ptr() + T.MARGIN * out.element_size()
    if mode in ("addend", "addend_mask"):
        q.addend = dv["addend"].data_ptr()
    if mode == "addend_mask":
        q.addend_mask = dv["amask"].data_ptr()
    if mode in ("bias", "affine_relu"):
        q.bias = dv["bias"].data_ptr()
    if mode == "affine_relu":
        q.scale, q.shift = dv["scale"].data_ptr(), dv["shift"].data_ptr()
    if mode == "stats":
        q.stats = slab.data_ptr()
    return dict(case=case, mode=mode, d=d, call=q, out=out, slab_whole=slab_whole, rows=rows, cout=cout)


def _igemm_multi(problems, precision):
    from lighthand_amd import _lib
    arr = (_lib.IgemmCall * len(problems))(*[p["call"] for p in problems])
    return _lib.load().lh_igemm_multi(arr, len(problems), T._DT[precision], None)


def _run_igemm_call(name, flavour, call, cfg, precision):
    from lighthand_amd import _lib
    td = T._TD[precision]
    problems = [_igemm_problem(case, mode, cfg, precision, flavour) for case, mode in call]
    rc = _igemm_multi(problems, precision)
    _sync(f"lh_igemm_multi {name} {cfg} {precision}")
    _lib.check(rc, f"lh_igemm_multi {name} {cfg} {precision}")
    bp = cfg[1]
    for p in problems:
        case, mode, cout = p["case"], p["mode"], p["cout"]
        tag = (name, cfg, precision, case, mode)
        h, dv = T._data(case, precision, flavour)
        want, on = T._host(case, precision, mode, flavour)
        assert on is None and torch.equal(want, E.epilogue_expected(case, precision, mode, flavour)), tag      # the CPU test's twin of _host
        pos = h["pos"]
        M, P = pos.numel(), T.CASES[case][0] * T.CASES[case][7] * T.CASES[case][8]
        buf = p["out"].cpu()
        assert bool((buf[:T.MARGIN].float() == T.SENTINEL).all()) and bool((buf[-T.MARGIN:].float() == T.SENTINEL).all()), (tag, "a margin of the output was written")
        out = buf[T.MARGIN:-T.MARGIN].view(P, cout)
        untouched = torch.ones(P, dtype=torch.bool)
        untouched[pos] = False
        assert bool((out[untouched].float() == T.SENTINEL).all()), (tag, "a pixel outside the launch was written")
        same = out[pos].view(torch.int16) == want.to(td).view(torch.int16)
        assert bool(same.all()), (tag, f"{int((~same).sum())} of {same.numel()} stored values differ from the host's bits, first at "
                                       f"{tuple(int(v) for v in (~same).nonzero()[0])}")
        whole = p["slab_whole"].cpu()
        assert _guards_intact(whole), (tag, "the surroundings of the statistics slab were written")
        slab = whole[GUARD:-GUARD].view(p["rows"], 2, cout)
        assert p["rows"] == (M + bp - 1) // bp, (tag, p["rows"])
        if mode != "stats":
            assert bool(torch.isnan(slab).all()), (tag, "the slab of a member without statistics was written")
        else:
            assert not bool(torch.isnan(slab).any()), (tag, "a statistics row was not written")
            sd = out[pos].double()
            got = slab.double().sum(0)
            for which, term in ((0, sd), (1, sd * sd)):
                holds, worst = E.check_exact_rows(term)
                if which == 0 or flavour == "exact_small":
                    assert holds, (tag, which, worst)
                if holds:
                    assert torch.equal(got[which], term.sum(0)), (tag, which, "a statistics row differs from the sums of the stored values")
                else:            # sums of squares of values that needed rounding: the rule of tests/test_gpu_epilogue_modes.py
                    assert torch.allclose(got[which], term.sum(0), rtol=2e-3, atol=2e-3 * float(term.abs().sum(0).max())), (tag, which)
        # the shared operands: an addend (handed over or not) and the epilogue vectors are read-only
        assert torch.equal(dv["addend"].cpu().float(), h["addend"]), (tag, "the addend was written")
        for k in ("bias", "scale", "shift"):
            assert torch.equal(dv[k].cpu(), h[k]), (tag, k)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("cfg", E.MULTI_RING_CFGS, ids=_ids)
def test_igemm_multi_stores_the_host_s_bits(cfg, precision):
    """Five calls per configuration and precision (exact_data.multi_igemm_calls): all five members in two rotations of the mode list, all
    five with statistics on "exact_small", n = 2 and n = 3 in the third rotation.  Per member: the stored bits, both margins and every
    pixel outside the launch, the slab's row count and that every row was written, its column sums, and that what the member's mode does
    not name came back unchanged."""
    for name, flavour, call in E.multi_igemm_calls():
        _run_igemm_call(name, flavour, call, cfg, precision)


def _refused(members, cfgs, precision="bf16"):
    """lh_igemm_multi on members that name the given configurations: (status, error text).  For calls the library must refuse before it
    launches anything."""
    from lighthand_amd import _lib
    problems = [_igemm_problem(case, "plain", cfg, precision, "exact") for case, cfg in zip(members, cfgs)]
    rc = _igemm_multi(problems, precision)
    _sync(f"lh_igemm_multi {members} {cfgs}")
    for p in problems:
        assert bool((p["out"].float() == T.SENTINEL).all()), "a refused call wrote an output"
    return rc, _lib.load().lh_last_error()


def test_igemm_multi_refuses_members_of_different_configurations():
    rc, err = _refused(["c136", "pw40"], [(64, 64, 2, 64), (64, 64, 4, 64)])
    assert rc == -1 and b"one tiled configuration per call" in err, (rc, err)          # LH_ERR_ARG


@pytest.mark.parametrize("cfg", [(128, 128, 22, 128), (64, 64, 24, 128), (128, 256, 3, 64), (256, 256, 2, 128)], ids=_ids)
def test_igemm_multi_has_no_kernel_for_dense_wave_forms_and_256_wide_tiles(cfg):
    """Ring depth + 20, a 256-pixel tile, a 256-channel tile, each named by two members that it fits: LH_ERR_UNSUPPORTED."""
    rc, err = _refused(["c136", "pw40"], [cfg, cfg])
    assert rc == -3 and b"no multi-problem kernel" in err, (rc, err)


def test_igemm_multi_refuses_a_direct_3x3_member_beside_a_tiled_one():
    rc, err = _refused(["d64", "c136"], [(64, 256, 100, 64), (64, 64, 2, 64)])
    assert rc == -3 and b"do not share a launch" in err, (rc, err)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_engine_s_partition_is_the_library_s(precision):
    """BatchGroups._merge_groups merges tiled members with 2 <= ring depth < 10 on a tile of _MULTI_TILES.  Every candidate the library
    offers a member that the rule accepts is a configuration of exact_data.MULTI_RING_CFGS -- each of which the test above runs --, and
    every candidate the rule rejects is refused when two members name it."""
    from lighthand_amd import _lib
    from lighthand_amd.batch_groups import BatchGroups
    lib = _lib.load()
    rejected = set()
    for case in E.MULTI_MEMBERS:
        buf = (C.c_int * (5 * 320))()
        nc = lib.lh_igemm_candidates(C.byref(T._desc(case, "64x64")), T._DT[precision], buf, 320)
        for c in (tuple(buf[5 * i:5 * i + 4]) for i in range(nc)):
            if 2 <= c[2] < 10 and (c[0], c[1]) in BatchGroups._MULTI_TILES:
                assert c in E.MULTI_RING_CFGS, (case, c)
            else:
                rejected.add(c)
    assert any(20 <= c[2] < 30 for c in rejected) and any(c[2] == 1 for c in rejected) and any(max(c[:2]) == 256 for c in rejected)
    for c in sorted(rejected):
        rc, err = _refused(["c136", "pw40"], [c, c], precision)
        assert rc != 0, (c, "a configuration the engine never merges was accepted")


# ---------------------------------------------------------------------------------------------------------------------------------
# B. lh_wgrad_fused_multi
_WDEV = {}


def _wgrad_operands(member, precision):
    """x as NHWC [n][h][w][cin + slack] and dy as [pixels][cout + slack] on the device, in the run precision: made once, never changed."""
    key = (member, precision)
    if key not in _WDEV:
        m = E.wgrad_member(member, precision)
        td = T._TD[precision]
        cin, cout = E.WGRAD_MULTI_CASES[member][:2]
        x = m["x"].permute(0, 2, 3, 1).contiguous().to(td)
        dy = m["dy"].permute(0, 2, 3, 1).contiguous().view(-1, cout).to(td)         # (one image: a reshape of the permuted view stays a view)
        assert torch.equal(x.float(), m["x"].permute(0, 2, 3, 1)) and torch.equal(dy.float(), m["dy"].permute(0, 2, 3, 1).reshape(-1, cout))
        slack = E.wgrad_slack(member)
        if slack:
            x = torch.cat([x, torch.full(x.shape[:3] + (slack,), E.WGRAD_SLACK_FILL, dtype=td)], 3)
            dy = torch.cat([dy, torch.full((dy.shape[0], slack), E.WGRAD_SLACK_FILL, dtype=td)], 1)
        _WDEV[key] = (x.contiguous().cuda(), dy.contiguous().cuda())
    return _WDEV[key]


def _wgrad_problem(member, precision, cfg, splits=None, dtype=None, workspace=True):
    """Descriptor, buffers and lh_wgrad_call fields of one member under plan cfg = (bo, bi, kps, depth) (None: the static plan)."""
    from lighthand_amd import _lib
    lib = _lib.load()
    cin, cout, k = E.WGRAD_MULTI_CASES[member][:3]
    code = T._DT[precision] if dtype is None else dtype
    d = E.wgrad_desc(_lib.IgemmDesc(), member, cfg, splits)
    x, dy = _wgrad_operands(member, precision)
    want = E.wgrad_expected(member, precision)
    pre = E.wgrad_member(member, precision)["pre"]
    grad_whole, grad = _guarded(want.numel())
    if pre is not None:
        grad.copy_(pre.reshape(-1))
    ws_bytes = lib.lh_wgrad_workspace_bytes(C.byref(d), cout, cin, code)
    ws_whole, ws = _guarded(max(ws_bytes // 4, 4))          # a slab element no split writes stays NaN and reaches the fold
    taps = (C.c_int * (2 * k * k))(*[v for r in range(k) for s in range(k) for v in (r, s)])
    q = _lib.WgradCall()
    q.d, q.rows, q.x, q.dy, q.dy_pix_stride, q.n_out, q.n_in = C.pointer(d), 0, x.data_ptr(), dy.data_ptr(), dy.shape[1], cout, cin
    q.workspace, q.grad = (ws.data_ptr() if workspace else None), grad.data_ptr()
    q.so, q.si, q.sr, q.ss = (k * k, cout * k * k, k, 1) if member == E.WGRAD_MULTI_TRANSPOSED else (cin * k * k, k * k, k, 1)
    q.taps_rs, q.accumulate = C.cast(taps, C.POINTER(C.c_int)), int(pre is not None)
    return dict(member=member, d=d, call=q, taps=taps, grad_whole=grad_whole, ws_whole=ws_whole, ws_bytes=ws_bytes, want=want)


def _wgrad_multi(problems, code):
    from lighthand_amd import _lib
    arr = (_lib.WgradCall * len(problems))(*[p["call"] for p in problems])
    return _lib.load().lh_wgrad_fused_multi(arr, len(problems), code, None)


def _run_wgrad_call(what, plans, precision):
    """plans: [(member, cfg or None, splits or None)] in caller order.  One call, one synchronisation; then every member's gradient bit
    for bit, the sentinels around it and the sentinel behind its workspace."""
    from lighthand_amd import _lib
    problems = [_wgrad_problem(m, precision, cfg, splits) for m, cfg, splits in plans]
    rc = _wgrad_multi(problems, T._DT[precision])
    _sync(f"lh_wgrad_fused_multi {what} {precision}")
    _lib.check(rc, f"lh_wgrad_fused_multi {what} {precision}")
    for p in problems:
        tag = (what, precision, p["member"])
        assert p["ws_bytes"] > 0, tag
        assert _guards_intact(p["ws_whole"].cpu()), (tag, "a slab was written outside the member's workspace")
        whole = p["grad_whole"].cpu()
        assert _guards_intact(whole), (tag, "a margin of the gradient tensor was written")
        got = whole[GUARD:-GUARD].view(p["want"].shape)
        same = got == p["want"]                             # (an element that was never written, or folded from an unwritten slab, is NaN)
        assert bool(same.all()), (tag, f"{int((~same).sum())} of {same.numel()} gradient elements differ from the fp64 sum, first at "
                                       f"{tuple(int(v) for v in (~same).nonzero()[0])}: {float(got[~same][0])} for {float(p['want'][~same][0])}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("cfg", E.WGRAD_MULTI_CFGS, ids=_ids)
def test_wgrad_multi_equals_the_fp64_sum(cfg, precision):
    """Every compiled four-wave configuration on the members that fit it (exact_data.WGRAD_MULTI_ORDER: all five -- a launch of four, then
    one alone -- under the 64 x 64 tile, three or two under the others), W1 in three pixel splits and W4 in two: the library's sort permutes
    the launch array while the fold array keeps caller order."""
    members = E.WGRAD_MULTI_ORDER[cfg[:2]]
    assert len(members) >= 2
    _run_wgrad_call(f"{cfg}", [(m, cfg, None) for m in members], precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_wgrad_multi_flushes_around_a_member_on_the_256_tile(precision):
    """Three batchable members with W5 on the 256 x 256 tile between them: the library launches (W1, W2) together, runs W5 through
    lh_wgrad_fused, and goes on with W3 alone."""
    cfg = (64, 64, 64, 3)
    _run_wgrad_call("around the 256 tile", [("W1", cfg, None), ("W2", cfg, None), ("W5", E.WGRAD_BIG_CFG, 1), ("W3", cfg, None)], precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_wgrad_multi_flushes_at_another_tile_class(precision):
    """The third member names another four-wave tile class: (W1, W2) on 64 x 64, then (W4, W5) on 64 x 128."""
    a, b = (64, 64, 32, 4), (64, 128, 32, 4)
    _run_wgrad_call("two tile classes", [("W1", a, None), ("W2", a, None), ("W4", b, None), ("W5", b, None)], precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_wgrad_multi_with_static_plans(precision):
    """cfg[5..7] = 0: the planner's own tile (128 x 128 for all five), stage, depth and split counts."""
    _run_wgrad_call("static plans", [(m, None, None) for m in E.WGRAD_MULTI_CASES], precision)


def test_wgrad_multi_refuses_a_null_workspace_and_fp32_ring_plans():
    """Status only: nothing is launched, no gradient is touched."""
    from lighthand_amd import _lib
    lib = _lib.load()
    cfg = (64, 64, 32, 2)
    for what, problems, code, status, text in (
            ("null workspace", [_wgrad_problem("W4", "bf16", cfg), _wgrad_problem("W5", "bf16", cfg, workspace=False)], _lib.LH_BF16, -1, b"null pointer (problem 1)"),
            ("fp32 ring plan", [_wgrad_problem(m, "bf16", cfg, dtype=_lib.LH_F32) for m in ("W4", "W5")], _lib.LH_F32, -3, b"is not available for this launch")):
        rc = _wgrad_multi(problems, code)
        _sync(what)
        assert rc == status and text in lib.lh_last_error(), (what, rc, lib.lh_last_error())
        for p in problems:
            g = p["grad_whole"].cpu()
            assert _guards_intact(g) and bool(torch.isnan(g[GUARD:-GUARD]).all()), (what, "a refused call wrote a gradient")
