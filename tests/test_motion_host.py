"""CPU: motion-aware tracking on the host -- topdown.rois_predict_host (ROI velocity prediction and coasting) on a float64 simulation of a
hand that accelerates and of one that is hidden for three frames, its identities clause by clause, topdown.one_euro_gated_host against
topdown.one_euro_host and on a gated joint, and every refusal of ManagedInferStep's ``motion=`` / ``smooth_gate=``.  The kernels are held
to these restatements bit for bit in tests/test_gpu_motion.py."""
import ctypes as C

import numpy as np
import pytest

F = np.float32
DT = 1.0 / 30.0


# ------------------------------------------------------------------------------------------------ 1. the simulation
def _simulate(top_speed, hidden=(), predict=None, frames=60):
    """A 100 px hand under box_padding 1.25 (12.5 px of margin per side) at 30 fps, float64.  Its speed ramps by 1 px/frame each frame up
    to ``top_speed`` px/frame in x and half that in y.  The hand is found when its centre lies within 12.5 px of the ROI's centre on both
    axes and the frame is not in ``hidden``; a found hand's next box is its own bounds, a lost one's repeats the box, and with
    ``predict`` (rois_predict_host's options) the next box then goes through the predictor.  Returns (the lost frames, the centre error
    of every frame)."""
    from lighthand_amd.topdown import rois_predict_host
    p = np.array([500.0, 400.0])
    box = state = None
    lost, err = [], []
    for t in range(frames):
        v = float(min(t, top_speed))
        p = p + np.array([v, v / 2.0])
        hand = np.array([p[0] - 50.0, p[1] - 50.0, p[0] + 50.0, p[1] + 50.0])
        if box is None:
            box = hand.copy()
        e = np.abs(p - np.array([(box[0] + box[2]) / 2.0, (box[1] + box[3]) / 2.0]))
        found = bool((e <= 12.5).all()) and t not in hidden
        err.append(float(e.max()))
        if not found:
            lost.append(t)
        nxt = hand.copy() if found else box.copy()
        if predict is not None:
            out, state = rois_predict_host(nxt[None], [0 if found else 1], [0], None, DT, state, dtype=np.float64, **predict)
            nxt = out[0]
        box = nxt
    return lost, err


def test_the_follower_loses_an_accelerating_hand_and_the_predictor_does_not():
    lost, _ = _simulate(20)
    assert lost[0] == 13 and len(lost) == 47 and lost == list(range(13, 60))
    lost, err = _simulate(20, predict=dict(cutoff=10.0))
    print(f"cutoff 10 Hz: {len(lost)} frames lost, largest centre error {max(err):.4f} px")
    assert lost == [] and max(err) <= 2.0
    # the other cut-offs of the table this rule was designed on, which quotes two decimals: within one unit of the second
    for cutoff, worst in ((2.0, 3.38), (5.0, 1.96), (30.0, 1.16)):
        lost, err = _simulate(20, predict=dict(cutoff=cutoff))
        assert lost == [] and abs(max(err) - worst) < 0.01, (cutoff, max(err))


def test_coasting_carries_the_roi_over_a_three_frame_occlusion():
    hidden = (30, 31, 32)
    assert _simulate(10, hidden)[0] == list(range(30, 60))
    assert _simulate(10, hidden, predict=dict(cutoff=10.0, coast=0))[0] == list(range(30, 60))
    assert _simulate(10, hidden, predict=dict(cutoff=10.0, coast=5))[0] == [30, 31, 32]


# ------------------------------------------------------------------------------------------------ 2. rois_predict_host, clause by clause
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype.itemsize == 4 else np.int64)


def _moving(b=6, frames=5, seed=0):
    """``frames`` boxes per slot of hands that move by a few pixels a frame, fp32."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(200, 800, size=(1, b, 2)) + np.cumsum(rng.uniform(-9, 9, size=(frames, b, 2)), 0)
    h = rng.uniform(30, 80, size=(1, b, 2))
    return np.concatenate([c - h, c + h], 2).astype(F)


def test_without_lead_and_coast_no_box_changes_a_bit():
    from lighthand_amd.topdown import rois_predict_host
    seq, state = _moving(), None
    for t, boxes in enumerate(seq):
        lost = (np.arange(6) == t).astype(np.int32)
        out, state = rois_predict_host(boxes, lost, np.zeros(6, np.int32), None, DT, state, lead=0.0, coast=0)
        assert out.dtype == F and np.array_equal(_bits(out), _bits(boxes))
    assert np.abs(state[1]).max() > 10                                    # the velocity is estimated all the same


def test_a_reset_slot_keeps_its_box_and_loses_its_state():
    from lighthand_amd.topdown import rois_predict_host
    seq = _moving(b=4)
    src = np.zeros(4, np.int32)
    state = None
    for boxes in seq[:3]:
        _, state = rois_predict_host(boxes, np.zeros(4), src, None, DT, state, coast=3)
    assert state[2].tolist() == [1, 1, 1, 1] and (np.abs(state[1]) > 0).all()
    state = (state[0], state[1], state[2], np.array([0, 2, 0, 1], np.int32))
    boxes = seq[3].copy()
    boxes[2] = 0                                                          # emptied by track management
    out, new = rois_predict_host(boxes, [0, 0, 1, 0], [-1, 0, 0, 0], [-1, 5, -1, -1], DT, state, coast=3)
    assert np.array_equal(_bits(out[:3]), _bits(boxes[:3]))               # empty, seeded, emptied: the box stays
    assert new[2].tolist() == [0, 0, 0, 1] and new[3].tolist() == [0, 0, 0, 0] and not new[1][:3].any() and new[1][3].any()
    assert not np.array_equal(out[3], boxes[3])
    out2, new2 = rois_predict_host(boxes, [0, 0, 1, 0], [-1, 0, 0, 0], None, DT, state, coast=3)      # seeded = None: slot 1 is tracked
    assert new2[2].tolist() == [0, 1, 0, 1] and not np.array_equal(out2[1], boxes[1])
    # a box that is not positive on one axis only, or NaN, is a reset as well
    odd = np.array([[10, 10, 10, 50], [10, 10, 50, np.nan]], F)
    out, new = rois_predict_host(odd, [0, 0], [0, 0], None, DT, (np.ones((2, 2), F), np.ones((2, 2), F), [1, 1], [1, 1]))
    assert np.array_equal(_bits(out), _bits(odd)) and new[2].tolist() == [0, 0] and not new[1].any() and new[3].tolist() == [0, 0]


def test_the_clamp_binds_at_exactly_max_shift_times_the_larger_side():
    from lighthand_amd.topdown import rois_predict_host
    first = np.array([[100, 100, 180, 140], [100, 100, 180, 140]], F)      # 80 x 40: the larger side is 80
    jump = first + np.array([[60, -3, 60, -3], [3, -60, 3, -60]], F)
    _, state = rois_predict_host(first, [0, 0], [0, 0], None, DT, None, cutoff=1000.0, lead=4.0, max_shift=0.25)
    out, state = rois_predict_host(jump, [0, 0], [0, 0], None, DT, state, cutoff=1000.0, lead=4.0, max_shift=0.25)
    shift = out - jump
    assert shift[0, 0] == shift[0, 2] == 20.0 and shift[1, 1] == shift[1, 3] == -20.0          # 0.25 * 80, on either axis and sign
    assert 0 > shift[0, 1] == shift[0, 3] > -20.0 and 0 < shift[1, 0] == shift[1, 2] < 20.0     # the other axis is inside the limit
    assert abs(state[1][0, 0]) > 1500                                     # the velocity itself is not clamped
    # coasting is clamped by the same limit
    out, state = rois_predict_host(jump, [1, 1], [0, 0], None, DT, state, cutoff=1000.0, lead=4.0, max_shift=0.25, coast=1)
    assert (out - jump)[0, 0] == 20.0 and (out - jump)[1, 1] == -20.0 and state[3].tolist() == [1, 1]
    out, _ = rois_predict_host(jump, [0, 0], [0, 0], None, DT, state, max_shift=0.0)
    assert np.array_equal(out, jump)


def test_coasting_counts_and_then_forgets():
    from lighthand_amd.topdown import rois_predict_host
    a, b_ = np.array([[100, 100, 200, 200]], F), np.array([[103, 106, 203, 206]], F)
    _, state = rois_predict_host(a, [0], [0], None, DT, None, coast=2)
    box, state = rois_predict_host(b_, [0], [0], None, DT, state, coast=2)
    vel = state[1].copy()
    assert vel[0, 0] > 0 and vel[0, 1] > vel[0, 0]
    for n in (1, 2):
        moved, state = rois_predict_host(box, [1], [0], None, DT, state, coast=2)
        step = (vel * F(DT))[0]
        assert np.array_equal(moved[0], box[0] + np.tile(step, 2)) and state[3].tolist() == [n] and state[2].tolist() == [1]
        assert np.array_equal(state[1], vel)
        box = moved
    assert np.allclose(state[0][0], [153 + 2 * step[0], 156 + 2 * step[1]])                  # the centre has moved along
    same, state = rois_predict_host(box, [1], [0], None, DT, state, coast=2)                  # past coast: forgotten, the box stays
    assert np.array_equal(_bits(same), _bits(box)) and state[2].tolist() == [0] and not state[1].any()
    fresh, state = rois_predict_host(b_, [0], [0], None, DT, state, coast=2)                  # found again: fresh, no shift
    assert np.array_equal(_bits(fresh), _bits(b_)) and state[2].tolist() == [1] and state[3].tolist() == [0] and not state[1].any()


@pytest.mark.parametrize("dt", [0.0, np.nan, np.inf, -DT])
def test_a_bad_dt_starts_fresh(dt):
    from lighthand_amd.topdown import rois_predict_host
    seq = _moving(b=3)
    state = None
    for boxes in seq[:3]:
        _, state = rois_predict_host(boxes, np.zeros(3), np.zeros(3), None, DT, state, coast=4)
    dts = np.array([DT, dt, dt], F)
    with np.errstate(all="ignore"):
        out, new = rois_predict_host(seq[3], [0, 0, 1], np.zeros(3), None, dts, state, coast=4)
    assert not np.array_equal(out[0], seq[3][0]) and np.array_equal(_bits(out[1:]), _bits(seq[3][1:]))
    assert new[2].tolist() == [1, 1, 0] and not new[1][1:].any() and new[3].tolist() == [0, 0, 0]
    assert np.array_equal(new[0][1], [(seq[3][1, 0] + seq[3][1, 2]) * F(0.5), (seq[3][1, 1] + seq[3][1, 3]) * F(0.5)])
    # a velocity that overflows is dropped, the slot stays seen at the new centre
    far = np.array([[1e38, 0, 1.2e38, 10]], F)
    with np.errstate(all="ignore"):
        out, new = rois_predict_host(far, [0], [0], None, F(1e-6), (np.array([[-3e38, 0]], F), np.zeros((1, 2), F), [1], [2]))
    assert np.array_equal(_bits(out), _bits(far)) and new[2].tolist() == [1] and not new[1].any() and new[3].tolist() == [0]
    assert new[0][0, 0] == (far[0, 0] + far[0, 2]) * F(0.5)


def test_the_inputs_are_not_modified_and_fp64_is_close():
    from lighthand_amd.topdown import rois_predict_host
    seq = _moving(b=5, frames=8, seed=4)
    s32 = s64 = None
    for t, boxes in enumerate(seq):
        lost = (np.arange(5) % 3 == t % 3).astype(np.int32) if t > 2 else np.zeros(5, np.int32)
        keep = boxes.copy(), None if s32 is None else [a.copy() for a in s32]
        o32, n32 = rois_predict_host(boxes, lost, np.zeros(5), None, DT, s32, coast=1)
        o64, s64 = rois_predict_host(boxes, lost, np.zeros(5), None, DT, s64, coast=1, dtype=np.float64)
        assert np.array_equal(boxes, keep[0]) and (s32 is None or all(np.array_equal(a, k) for a, k in zip(s32, keep[1])))
        assert o64.dtype == np.float64 and np.abs(o32 - o64).max() < 1e-2 and np.array_equal(n32[2], s64[2]) and np.array_equal(n32[3], s64[3])
        s32 = n32


# ------------------------------------------------------------------------------------------------ 3. one_euro_gated_host
def _noisy(frames, b, j, seed):
    rng = np.random.RandomState(seed)
    base = rng.uniform(100, 900, size=(1, b, j, 2))
    t = np.arange(frames).reshape(frames, 1, 1, 1)
    return (base + 40 * np.sin(t * 0.2 + base * 0.01) + rng.normal(0, 2, size=(frames, b, j, 2))).astype(F)


def test_with_the_gate_open_it_is_the_one_euro_filter_bit_for_bit():
    from lighthand_amd.topdown import GATE_OPEN, one_euro_gated_host, one_euro_host
    frames, b, j = 20, 67, 21
    seq = _noisy(frames, b, j, 5)
    rng = np.random.RandomState(6)
    plain = gated = None
    for t in range(frames):
        src = np.where(rng.uniform(size=b) < 0.1, -1, 0).astype(np.int32)
        lost = (rng.uniform(size=b) < 0.15).astype(np.int32)
        dt = rng.uniform(0.01, 0.05, size=b).astype(F)
        dt[rng.uniform(size=b) < 0.05] = 0.0
        mv = rng.uniform(-1, 1, size=(b, j)).astype(F)
        boxes = rng.uniform(0, 300, size=(b, 4)).astype(F)
        want, plain = one_euro_host(seq[t], dt, plain, src, lost, 1.0, 0.007, 1.0)
        got, gated = one_euro_gated_host(seq[t], mv, dt, gated, src, lost, boxes, 1.0, 0.007, 1.0, gate_min_score=GATE_OPEN, by_size=False)
        assert np.array_equal(_bits(got), _bits(want)), t
        assert np.array_equal(_bits(gated[0]), _bits(plain[0])) and np.array_equal(_bits(gated[1]), _bits(plain[1])), t
        assert np.array_equal(gated[2], np.repeat(plain[2][:, None], j, 1)) and not gated[3].any()
    assert (np.abs(want - seq[-1]) > 0).sum() > b * j                       # the filter did filter


def test_a_joint_gated_out_for_three_frames_holds_and_returns_over_four_dt():
    from lighthand_amd.topdown import one_euro_gated_host, one_euro_host
    seq = _noisy(7, 2, 3, 8)
    score = np.full((7, 2, 3), 0.9, F)
    score[2:5, 0, 1] = 0.05                                               # slot 0's joint 1 is gated out on frames 2, 3, 4
    state, outs = None, []
    for t in range(7):
        out, state = one_euro_gated_host(seq[t], score[t], DT, state, min_cutoff=1.0, beta=0.007, gate_min_score=0.5)
        outs.append(out)
        if t == 1:
            held = state[0][0, 1].copy(), state[1][0, 1].copy()
        if 2 <= t <= 4:
            assert np.array_equal(_bits(out[0, 1]), _bits(held[0])) and np.array_equal(_bits(state[0][0, 1]), _bits(held[0]))
            assert np.array_equal(_bits(state[1][0, 1]), _bits(held[1])) and state[2][0, 1] == 1
            gap = F(0)
            for _ in range(t - 1):
                gap = F(gap + F(DT))
            assert state[3][0, 1] == gap and state[3].sum() == gap        # the other joints carry no gap
    assert not state[3].any() and state[2].all()
    # frame 5: one One-Euro step from the held state over T = gap + dt = 4 dt (summed as the filter sums it)
    span = F(F(F(F(DT) + F(DT)) + F(DT)) + F(DT))
    want, _ = one_euro_host(seq[5][:1, 1:2], span, (held[0].reshape(1, 1, 2), held[1].reshape(1, 1, 2), [1]), min_cutoff=1.0, beta=0.007)
    assert np.array_equal(_bits(outs[5][0, 1]), _bits(want[0, 0]))
    short, _ = one_euro_host(seq[5][:1, 1:2], DT, (held[0].reshape(1, 1, 2), held[1].reshape(1, 1, 2), [1]), min_cutoff=1.0, beta=0.007)
    assert not np.array_equal(short[0, 0], want[0, 0])
    # every other joint is the ungated filter's
    plain, pstate = [], None
    for t in range(7):
        out, pstate = one_euro_host(seq[t], DT, pstate, min_cutoff=1.0, beta=0.007)
        plain.append(out)
    others = np.ones((2, 3), bool)
    others[0, 1] = False
    assert all(np.array_equal(_bits(outs[t][others]), _bits(plain[t][others])) for t in range(7))
    # a joint that has never been seen passes its raw position through while it is gated out; an away slot clears seen_j and gap
    out, st = one_euro_gated_host(seq[0], np.full((2, 3), 0.1, F), DT, None, gate_min_score=0.5)
    assert np.array_equal(_bits(out), _bits(seq[0])) and not st[2].any() and (st[3] == F(DT)).all()
    out, st = one_euro_gated_host(seq[3], score[3], DT, state, src_frame=[0, -1], lost=[1, 0], gate_min_score=0.5)
    assert np.array_equal(_bits(out), _bits(seq[3])) and not st[2].any() and not st[3].any()
    # a NaN maxval is gated out; a dt that is not finite and > 0 adds nothing to the gap and starts a gated-in joint fresh
    mv = np.array([[np.nan, 0.9, 0.1]] * 2, F)
    with np.errstate(all="ignore"):
        out, st = one_euro_gated_host(seq[6], mv, [np.nan, 0.0], state, gate_min_score=0.5)
    assert np.array_equal(_bits(out[:, 0]), _bits(state[0][:, 0])) and np.array_equal(_bits(out[:, 1]), _bits(seq[6][:, 1]))
    assert not st[3].any() and st[2].all() and not st[1][:, 1].any()


def test_by_size_divides_the_speed_by_the_larger_extent_floored_at_one():
    from lighthand_amd.topdown import one_euro_gated_host
    seq = _noisy(3, 4, 5, 9)
    mv = np.ones((4, 5), F)
    boxes = np.array([[0, 0, 200, 50], [0, 0, 50, 200], [0, 0, 0.5, 0.25], [0, 0, 1, 1]], F)       # sizes 200, 200, 1 (floored), 1
    _, state = one_euro_gated_host(seq[0], mv, DT, None, beta=0.5)
    _, state = one_euro_gated_host(seq[1], mv, DT, state, beta=0.5)
    sized, s_sized = one_euro_gated_host(seq[2], mv, DT, state, next_boxes=boxes, beta=0.5, by_size=True)
    plain, s_plain = one_euro_gated_host(seq[2], mv, DT, state, beta=0.5)
    scaled, _ = one_euro_gated_host(seq[2], mv, DT, state, beta=0.5 / 200.0)                  # beta / 200: the same cut-off (200 = 2^3 * 25)
    assert np.array_equal(_bits(sized[2:]), _bits(plain[2:])) and np.array_equal(_bits(s_sized[1]), _bits(s_plain[1]))
    assert not np.array_equal(sized[:2], plain[:2]) and np.abs(sized[:2] - scaled[:2]).max() < 1e-3
    # restated by hand for one coordinate
    x, xh, dxh0 = seq[2][0, 0, 0], state[0][0, 0, 0], state[1][0, 0, 0]
    rd = F(F(6.2831855) * F(1.0)) * F(DT)
    ad = rd / F(rd + F(1))
    dxh = F(ad * F(F(x - xh) / F(DT))) + F(F(F(1) - ad) * dxh0)
    fc = F(F(1.0) + F(F(0.5) * F(np.abs(dxh) / F(200))))
    r = F(F(F(6.2831855) * fc) * F(DT))
    al = r / F(r + F(1))
    assert sized[0, 0, 0] == F(F(al * x) + F(F(F(1) - al) * xh))
    with pytest.raises(Exception):
        one_euro_gated_host(seq[2], mv, DT, state, by_size=True)          # by_size reads next_boxes


def test_gated_fp64_form_and_inputs():
    from lighthand_amd.topdown import one_euro_gated_host
    seq = _noisy(12, 3, 4, 10)
    rng = np.random.RandomState(1)
    s32 = s64 = None
    for t in range(12):
        mv = rng.uniform(0, 1, size=(3, 4, 1)).astype(F)
        boxes = rng.uniform(0, 100, size=(3, 4)).astype(F) + F([0, 0, 100, 100])
        keep = None if s32 is None else [a.copy() for a in s32]
        o32, n32 = one_euro_gated_host(seq[t], mv, DT, s32, next_boxes=boxes, gate_min_score=0.3, by_size=True)
        o64, s64 = one_euro_gated_host(seq[t], mv, DT, s64, next_boxes=boxes, gate_min_score=0.3, by_size=True, dtype=np.float64)
        assert s32 is None or all(np.array_equal(a, k) for a, k in zip(s32, keep))
        assert o64.dtype == np.float64 and np.abs(o32 - o64).max() < 2e-3 and np.array_equal(n32[2], s64[2])
        s32 = n32


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_motion_refusals_before_any_device_work():
    from lighthand_amd.runtime import FrameInput, ManagedInferStep, _check_motion as check
    fi = FrameInput.check(frames=(4, 96, 128))
    assert check(fi, True, None) is None and check(fi, True, False) is None and check(FrameInput.check(), False, None) is None
    assert check(fi, True, True) == dict(cutoff=10.0, lead=1.0, max_shift=0.5, coast=0)
    got = check(fi, True, dict(coast=2, cutoff=5))
    assert got == dict(cutoff=5.0, lead=1.0, max_shift=0.5, coast=2) and isinstance(got["coast"], int) and isinstance(got["cutoff"], float)
    with pytest.raises(ValueError, match="track=True"):
        check(fi, False, True)
    with pytest.raises(ValueError, match="track=True"):
        check(FrameInput.check(), True, True)
    with pytest.raises(ValueError, match="unknown keys.*horizon"):
        check(fi, True, dict(horizon=2))
    with pytest.raises(ValueError, match="must be None, True or a dict"):
        check(fi, True, 10.0)
    for key, bad in (("cutoff", (0, -1.0, float("nan"), float("inf"), "10", True, None)), ("lead", (-0.5, float("nan"), float("inf"), "1", None)),
                     ("max_shift", (-0.5, float("inf"), [0.5], None)), ("coast", (-1, 1.5, True, "2", None, 2 ** 31))):
        for v in bad:
            with pytest.raises(ValueError, match=f"motion: {key}"):
                check(fi, True, {key: v})
    # through the constructor: refused before the model is looked at
    for kwargs in (dict(motion=True), dict(motion=True, frames=(4, 96, 128)), dict(motion=dict(speed=1), frames=(4, 96, 128), track=True),
                   dict(motion=dict(coast=-1), frames=(4, 96, 128), track=True)):
        for manage in (False, True) if kwargs.get("track") else (False,):
            with pytest.raises(ValueError, match="motion"):
                ManagedInferStep(None, 4, 64, 64, manage_tracks=manage, **kwargs)


def test_smooth_gate_refusals_before_any_device_work():
    from lighthand_amd.runtime import ManagedInferStep, _check_smooth_gate as check
    smooth = (1.0, 0.007, 1.0)
    assert check(smooth, None, 0.1) is None and check(None, None, 0.1) is None and check(None, False, 0.1) is None
    assert check(smooth, True, 0.25) == dict(min_score=0.25, by_size=True)
    assert check(smooth, dict(min_score=0.5, by_size=False), 0.1) == dict(min_score=0.5, by_size=False)
    assert check(smooth, dict(min_score=-3.0e38), 0.1)["min_score"] == -3.0e38
    with pytest.raises(ValueError, match="smooth="):
        check(None, True, 0.1)
    with pytest.raises(ValueError, match="unknown keys.*score"):
        check(smooth, dict(score=0.5), 0.1)
    with pytest.raises(ValueError, match="must be None, True or a dict"):
        check(smooth, 0.5, 0.1)
    for v in (float("nan"), float("inf"), "0.5", None, True, 1e39):
        with pytest.raises(ValueError, match="smooth_gate: min_score"):
            check(smooth, dict(min_score=v), 0.1)
    for v in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="smooth_gate: by_size"):
            check(smooth, dict(by_size=v), 0.1)
    with pytest.raises(ValueError, match="smooth_gate: min_score"):
        check(smooth, True, None)                                         # the default is the step's track_min_score
    for kwargs in (dict(smooth_gate=True), dict(smooth_gate=True, frames=(4, 96, 128), track=True),
                   dict(smooth_gate=dict(gate=1), frames=(4, 96, 128), smooth=(1.0, 0.007), manage_tracks=False)):
        with pytest.raises(ValueError, match="smooth_gate"):
            ManagedInferStep(None, 4, 64, 64, **dict(kwargs, manage_tracks=False))


def test_argument_refusals_of_the_entries_before_any_launch():
    from lighthand_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    q = [p + 16 * k for k in range(12)]

    def predict(boxes=q[0], lost=q[1], src=q[2], seeded=None, dt=q[3], b=1, cutoff=10.0, lead=1.0, max_shift=0.5, coast=0, centre=q[4], vel=q[5],
                seen=q[6], coasted=q[7]):
        return lib.lh_rois_predict(boxes, lost, src, seeded, dt, b, cutoff, lead, max_shift, coast, centre, vel, seen, coasted, None)

    for bad in (dict(boxes=None), dict(lost=None), dict(dt=None), dict(vel=None), dict(coasted=None), dict(b=0), dict(cutoff=0.0),
                dict(cutoff=float("nan")), dict(cutoff=float("inf")), dict(lead=-1.0), dict(max_shift=float("nan")), dict(coast=-1), dict(vel=q[4])):
        assert predict(**bad) == -1 and b"lh_rois_predict" in lib.lh_last_error(), bad

    def gated(x=q[0], mv=q[1], boxes=q[2], src=q[3], lost=None, dt=q[4], b=1, j=1, fc=1.0, beta=0.007, dc=1.0, gate=0.5, by_size=0, xhat=q[5],
              dxhat=q[6], seen=q[7], gap=q[8], out=q[9]):
        return lib.lh_one_euro_gated(x, mv, boxes, src, lost, dt, b, j, fc, beta, dc, gate, by_size, xhat, dxhat, seen, gap, out, None)

    for bad in (dict(x=None), dict(mv=None), dict(gap=None), dict(seen=None), dict(boxes=None, by_size=1), dict(b=0), dict(j=0), dict(fc=0.0),
                dict(beta=-1.0), dict(dc=float("nan")), dict(gate=float("nan")), dict(gate=float("-inf")), dict(xhat=q[0]), dict(out=q[5]),
                dict(gap=q[6])):
        assert gated(**bad) == -1 and b"lh_one_euro_gated" in lib.lh_last_error(), bad


def test_track_frames_parser_takes_the_new_flags():
    from lighthand_amd.tools import track_frames as T
    args = T.build_parser().parse_args(["--synthetic", "4"])
    assert (args.motion, args.motion_cutoff, args.motion_lead, args.coast, args.smooth_gate, args.gate_min_score, args.no_size_norm) == \
        (False, 10.0, 1.0, 0, False, None, False)
    args = T.build_parser().parse_args(["--synthetic", "4", "--motion", "--motion_cutoff", "5", "--motion_lead", "0.5", "--coast", "3", "--one_euro",
                                        "1.0", "0.007", "--smooth_gate", "--gate_min_score", "0.3", "--no_size_norm"])
    assert (args.motion, args.motion_cutoff, args.motion_lead, args.coast, args.smooth_gate, args.gate_min_score, args.no_size_norm) == \
        (True, 5.0, 0.5, 3, True, 0.3, True)


# ------------------------------------------------------------------------------------------------ 5. the GPU test's data
def test_the_seeded_sequence_reaches_every_branch():
    """tests/test_gpu_motion.py holds lh_rois_predict to the restatement on this sequence: every clause must occur, with and without a
    seeded list, and the gated filter's sequence must gate joints out, bring them back and meet away slots and bad dt."""
    import motion_data as D
    from lighthand_amd.topdown import one_euro_gated_host
    seq = D.predict_sequence()
    for use_seeded in (True, False):
        names = np.concatenate([n for _, _, n in D.run_predict_host(seq, D.PREDICT, use_seeded)])
        counts = {k: int((names == k).sum()) for k in D.BRANCHES}
        print(f"seeded {'given' if use_seeded else 'None'}: {counts}")
        assert sum(counts.values()) == D.B * D.FRAMES
        assert all(counts[k] >= 3 for k in D.BRANCHES if use_seeded or k != "seeded"), counts
        assert use_seeded or counts["seeded"] == 0
    for j in (21, 40):
        state, back, held = None, 0, 0
        for f in D.gated_sequence(j):
            seen_before = np.zeros((D.B, j), bool) if state is None else state[2] != 0
            gap_before = np.zeros((D.B, j), F) if state is None else state[3]
            gin = f["maxvals"] >= F(0.5)
            live = ((f["src_frame"] >= 0) & (f["lost"] == 0))[:, None]
            back += int((live & gin & seen_before & (gap_before > 0)).sum())
            held += int((live & ~gin & seen_before).sum())
            _, state = one_euro_gated_host(f["x"], f["maxvals"], f["dt"], state, f["src_frame"], f["lost"], f["next_boxes"], gate_min_score=0.5,
                                           by_size=True)
        assert back > 100 and held > 100, (j, back, held)
