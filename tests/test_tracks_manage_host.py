"""CPU: track management of the tracked top-down step -- topdown.manage_tracks_host on hand-built frames, one case per clause of the
rule, the refusals of ManagedInferStep(manage_tracks=) and of lh_tracks_manage before any device work, and the guard that the seeded scene of
tests/tracks_manage_data.py, which tests/test_gpu_tracks_manage.py runs on the device, produces every outcome."""
import ctypes as C

import numpy as np
import pytest

import tracks_manage_data as D

F = np.float32
NAN = float("nan")
OLD = [7.0, 8.0, 9.0, 10.0]                                          # the box a slot holds before the call


def run(slots, dets=(), n_frames=2, lost_count=None, rot=True, **options):
    """``slots``: (box or None, confidence, frame, lost[, src_frame]) -- four joints on the box's corners with that maxval each, so kb is the
    box and the score 4 * confidence (min_side 0); a box of None is an empty slot.  ``dets``: (box, frame, score).  Returns
    manage_tracks_host's tuple as lists, next_boxes / next_rot row by row."""
    from lighthand_amd.topdown import manage_tracks_host
    b = len(slots)
    preds, mv = np.zeros((b, 4, 2), F), np.zeros((b, 4), F)
    src, fidx, lost = np.zeros(b, np.int32), np.zeros(b, np.int32), np.zeros(b, np.int32)
    for i, (box, conf, frame, is_lost, *rest) in enumerate(slots):
        if box is not None:
            x0, y0, x1, y1 = box
            preds[i], mv[i] = [(x0, y0), (x1, y0), (x0, y1), (x1, y1)], conf
        fidx[i], lost[i] = frame, is_lost
        src[i] = rest[0] if rest else (frame if box is not None and 0 <= frame < n_frames else -1)
    dets = list(dets) or [((0, 0, 0, 0), -1, 0.0)]
    out = manage_tracks_host(preds, mv, src, fidx, n_frames, np.tile(F(OLD), (b, 1)), np.tile(F([0.6, 0.8]), (b, 1)) if rot else None, lost,
                             np.zeros(b, np.int32) if lost_count is None else lost_count, [d[0] for d in dets], [d[1] for d in dets],
                             [d[2] for d in dets], dup_of=np.full(b, D.SENTINEL), seeded=np.full(b, D.SENTINEL),
                             **dict(dict(min_score=0.1, min_side=0.0), **options))
    return [None if a is None else a.tolist() for a in out]


HAND = (100.0, 100.0, 200.0, 200.0)
NEAR = (110.0, 105.0, 210.0, 205.0)                                  # 90 * 95 of 100 * 100: over 0.5
FAR = (400.0, 300.0, 480.0, 380.0)
ZERO = [0.0] * 4


def test_of_two_slots_on_one_hand_the_higher_score_survives_and_a_tie_goes_to_the_lower_index():
    nbox, nrot, lost, count, dup_of, seeded, state = run([(HAND, 0.5, 0, 0), (NEAR, 0.75, 0, 0), (FAR, 0.2, 0, 0)], lost_count=[3, 3, 3])
    assert (lost, dup_of, count) == ([1, 0, 0], [1, -1, -1], [0, 0, 0])
    assert nbox == [ZERO, OLD, OLD] and nrot == [[F(0.6), F(0.8)]] * 3 and seeded == [-1] * 3 and state == [-1]
    nbox, _, lost, _, dup_of, _, _ = run([(FAR, 0.9, 0, 0), (HAND, 0.5, 0, 0), (NEAR, 0.5, 0, 0)])
    assert (lost, dup_of) == ([0, 0, 1], [-1, -1, 1]) and nbox == [OLD, OLD, ZERO]
    # the same two boxes on two frames are two hands; and at dup_overlap = 0.9 they are two hands on one frame
    assert run([(HAND, 0.5, 0, 0), (NEAR, 0.75, 1, 0)])[2:5] == [[0, 0], [0, 0], [-1, -1]]
    assert run([(HAND, 0.5, 0, 0), (NEAR, 0.75, 0, 0)], dup_overlap=0.9)[2] == [0, 0]


def test_overlap_is_intersection_over_the_smaller_area_with_a_strict_threshold():
    from lighthand_amd.topdown import _over_host
    big, palm = F([0, 0, 100, 100]), F([40, 40, 60, 60])
    assert _over_host(big, palm, F(0.99)) and _over_host(palm, big, F(0.99)) and not _over_host(big, palm, F(1.0))
    half = F([50, 0, 150, 100])                                      # exactly half of either: not over 0.5
    assert not _over_host(big, half, F(0.5)) and _over_host(big, half, F(0.49))
    assert not _over_host(big, F([100, 0, 200, 100]), F(0.0))        # touching boxes do not overlap, at any threshold
    assert not _over_host(big, F([NAN, 0, 50, 50]), F(0.0))


def test_greedy_chain_keeps_both_ends():
    a, bb, c = (100.0, 100.0, 200.0, 200.0), (140.0, 100.0, 240.0, 200.0), (180.0, 100.0, 280.0, 200.0)      # a~b, b~c (0.6), a !~ c (0.2)
    _, _, lost, _, dup_of, _, _ = run([(a, 0.9, 0, 0), (bb, 0.8, 0, 0), (c, 0.7, 0, 0)])
    assert (lost, dup_of) == ([0, 1, 0], [-1, 0, -1])
    # with b the best, both ends go, each to b
    assert run([(a, 0.7, 0, 0), (bb, 0.9, 0, 0), (c, 0.8, 0, 0)])[4] == [1, -1, 1]


def test_a_detection_covered_by_a_track_is_tracked():
    palm = (130.0, 130.0, 170.0, 170.0)
    nbox, _, lost, _, _, seeded, state = run([(HAND, 0.5, 0, 0), (None, 0, 0, 1)], [(palm, 0, 0.9), (palm, 1, 0.9)])
    assert state == [-2, -4] and seeded == [-1, -1] and nbox == [OLD, OLD] and lost == [0, 1]      # frame 1 has no slot at all: no room
    # a lost slot's keypoints cover nothing: the detection takes the first free slot, which is that one
    assert run([(HAND, 0.5, 0, 1)], [(palm, 0, 0.9)])[5:] == [[0], [0]]


def test_two_detections_on_one_fresh_hand_seed_once():
    d0, d1 = (300.0, 100.0, 380.0, 180.0), (305.0, 102.0, 385.0, 182.0)
    nbox, nrot, lost, count, dup_of, seeded, state = run([(HAND, 0.5, 0, 0), (None, 0, 0, 1), (None, 0, 0, 1)], [(d0, 0, 0.6), (d1, 0, 0.8)],
                                                         lost_count=[0, 4, 4])
    assert state == [-3, 1] and seeded == [-1, 1, -1] and nbox == [OLD, list(d1), OLD]
    assert nrot == [[F(0.6), F(0.8)], [1.0, 0.0], [F(0.6), F(0.8)]] and lost == [0, 1, 1] and count == [0, 0, 0] and dup_of == [-1] * 3
    # equal scores: the lower entry is the one that seeds; without next_rot (an upright step) the boxes alone are written
    out = run([(None, 0, 0, 1)], [(d0, 0, 0.7), (d1, 0, 0.7)], rot=False)
    assert out[6] == [0, -3] and out[0] == [list(d0)] and out[1] is None


def test_more_fresh_detections_than_free_slots():
    dets = [((300.0 + 100 * q, 100.0, 380.0 + 100 * q, 180.0), 0, s) for q, s in enumerate([0.5, 0.9, 0.7])]
    nbox, _, lost, _, dup_of, seeded, state = run([(None, 0, 0, 1), (HAND, 0.5, 0, 0), (NEAR, 0.4, 0, 0)], dets)
    # the free slots are 0 (empty) and 2 (suppressed), in that order; the detections come by score
    assert dup_of == [-1, -1, 1] and state == [-4, 0, 2] and seeded == [1, -1, 2] and lost == [1, 0, 1]
    assert nbox == [list(dets[1][0]), OLD, list(dets[2][0])]


def test_every_invalid_kind_is_marked():
    ok = (300.0, 100.0, 380.0, 180.0)
    dets = [((300.0, 100.0, 300.0, 180.0), 0, 0.9), ((300.0, 180.0, 380.0, 100.0), 0, 0.9), ((NAN, 100.0, 380.0, 180.0), 0, 0.9),
            ((300.0, 100.0, float("inf"), 180.0), 0, 0.9), (ok, 0, NAN), (ok, 0, float("inf")), (ok, 0, 0.29), (ok, -1, 0.9), (ok, 2, 0.9),
            (ok, 0, 0.3)]
    out = run([(None, 0, 0, 1)] * 3, dets, det_min_score=0.3)
    assert out[6] == [-1] * 9 + [0] and out[5] == [9, -1, -1]


def test_a_lost_slot_expires_after_exactly_max_lost_frames():
    from lighthand_amd.topdown import manage_tracks_host
    preds, mv = np.zeros((3, 4, 2), F), np.zeros((3, 4), F)
    src, fidx, lost = np.int32([0, -1, 0]), np.int32([0, 0, 0]), np.int32([1, 1, 0])
    preds[2], mv[2] = [(0, 0), (50, 0), (0, 50), (50, 50)], 0.9
    boxes, count = np.tile(F(OLD), (3, 1)), np.int32([0, 0, 0])
    history = []
    for _ in range(4):
        boxes, _, _, count, _, _, _ = manage_tracks_host(preds, mv, src, fidx, 1, boxes, None, lost, count, np.zeros((1, 4)), [-1], [0.0],
                                                         min_side=0.0, max_lost=3)
        history.append((count.tolist(), boxes[0].tolist()))
    # slot 0 counts 1, 2, and the third lost frame empties it; the empty slot and the kept one stay at 0
    assert history[:3] == [([1, 0, 0], OLD), ([2, 0, 0], OLD), ([0, 0, 0], ZERO)]
    assert history[3] == ([1, 0, 0], ZERO)                           # (the caller's advance() would have made the slot empty by now)
    # max_lost = 0: nothing expires, and the count saturates
    out = manage_tracks_host(preds, mv, src, fidx, 1, boxes, None, lost, np.int32([2 ** 30 - 1, 5, 5]), np.zeros((1, 4)), [-1], [0.0], max_lost=0)
    assert out[3].tolist() == [2 ** 30, 0, 0]
    out = manage_tracks_host(preds, mv, src, fidx, 1, boxes, None, lost, out[3], np.zeros((1, 4)), [-1], [0.0], max_lost=0)
    assert out[3].tolist() == [2 ** 30, 0, 0]


def test_a_seed_wins_over_expiry_in_the_same_frame():
    d = (300.0, 100.0, 380.0, 180.0)
    nbox, _, lost, count, _, seeded, state = run([(HAND, 0.5, 0, 1), (HAND, 0.5, 0, 1)], [(d, 0, 0.9)], lost_count=[2, 2], max_lost=3)
    assert state == [0] and seeded == [0, -1] and nbox == [list(d), ZERO] and count == [0, 0] and lost == [1, 1]


def test_slots_of_no_frame_are_never_touched():
    d = (300.0, 100.0, 380.0, 180.0)
    slots = [(HAND, 0.9, -1, 0, 0), (NEAR, 0.5, 2, 0, 1), (HAND, 0.5, 7, 1, 0), (NEAR, 0.4, 1, 0)]
    nbox, nrot, lost, count, dup_of, seeded, state = run(slots, [(d, 0, 0.9), (d, 2, 0.9)], lost_count=[5, 6, 7, 8], max_lost=1)
    s = D.SENTINEL
    assert nbox == [OLD] * 4 and lost == [0, 0, 1, 0] and count == [5, 6, 7, 0] and dup_of == [s, s, s, -1] and seeded == [s, s, s, -1]
    assert state == [-4, -1]


def test_the_no_op_case_changes_no_bit():
    s = D.scene()
    live = s["lost"] == 0
    s["lost"][:] = 1                                                 # no live slot: no duplicates
    s["lost"][np.nonzero(live)[0][:1]] = 0
    s["det_frame"][:] = -1
    nbox, nrot, lost, count, _, seeded, state = D.run_host(s, max_lost=0)
    assert nbox.tobytes() == s["next_boxes"].tobytes() and nrot.tobytes() == s["next_rot"].tobytes() and lost.tobytes() == s["lost"].tobytes()
    assert (state == -1).all() and (seeded[(s["frame_index"] >= 0) & (s["frame_index"] < D.N_FRAMES)] == -1).all()


def test_the_inputs_are_not_modified():
    s = D.scene()
    before = {k: v.copy() for k, v in s.items()}
    D.run_host(s)
    assert all(before[k].tobytes() == s[k].tobytes() for k in s)


# ------------------------------------------------------------------------------------------------ refusals
def test_option_refusals_before_any_device_work():
    from lighthand_amd.runtime import FrameInput, _check_manage_tracks as check
    fi, none = FrameInput.check((2, 96, 128)), FrameInput.check(None)
    assert check(fi, True, False, 8) is None and check(none, False, None, 8) is None
    assert check(fi, True, True, 8) == dict(max_detections=8, dup_overlap=0.5, match_overlap=0.5, det_min_score=0.0, max_lost=0)
    assert check(fi, True, dict(max_detections=1024, max_lost=30, dup_overlap=0), 1024)["max_detections"] == 1024
    with pytest.raises(ValueError, match="track=True"):
        check(fi, False, True, 8)
    with pytest.raises(ValueError, match="track=True"):
        check(none, False, dict(max_lost=3), 8)
    with pytest.raises(ValueError, match="unknown keys.*max_age"):
        check(fi, True, dict(max_age=3), 8)
    for key in ("dup_overlap", "match_overlap", "det_min_score", "max_lost"):
        for bad in (-1, NAN, float("inf"), "0.5", None, True):
            with pytest.raises(ValueError, match=key):
                check(fi, True, {key: bad}, 8)
    with pytest.raises(ValueError, match="max_lost"):
        check(fi, True, dict(max_lost=2.5), 8)
    for bad in (0, 1025, -3, 2.0, True):
        with pytest.raises(ValueError, match="max_detections"):
            check(fi, True, dict(max_detections=bad), 8)
    with pytest.raises(ValueError, match="1024 slots"):
        check(fi, True, True, 1025)
    with pytest.raises(ValueError, match="must be False, True or a dict"):
        check(fi, True, 3, 8)


def test_argument_refusals_of_the_entry_before_any_launch():
    from lighthand_amd import _lib
    lib = _lib.load()
    buf = (C.c_int * 16)()
    p = C.addressof(buf)                                             # a pointer that is not null; a refused call reads nothing

    def call(b=4, j=21, n_frames=2, k=4, thresholds=(0.1, 16.0, 0.5, 0.5, 0.0), max_lost=0, nulls=()):
        ptr = [None if q in nulls else p for q in range(14)]
        rc = lib.lh_tracks_manage(ptr[0], ptr[1], ptr[2], ptr[3], b, j, n_frames, ptr[4], ptr[5], ptr[6], k, *thresholds, max_lost, ptr[7], ptr[8],
                                  ptr[9], ptr[10], ptr[11], ptr[12], ptr[13], None)
        return rc, lib.lh_last_error().decode()

    for kw, word in ((dict(b=0), "slots"), (dict(b=1025), "slots"), (dict(k=0), "detections"), (dict(k=1025), "detections"), (dict(j=0), "j "),
                     (dict(n_frames=0), "n_frames"), (dict(max_lost=-1), "max_lost")):
        rc, text = call(**kw)
        assert rc == -1 and "lh_tracks_manage" in text and word in text, (kw, text)
    for q in (0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13):             # every pointer but next_rot (8)
        rc, text = call(nulls=(q,))
        assert rc == -1 and "null" in text, q
    for q in range(5):
        for bad in (NAN, float("inf")) + ((-1.0,) if q else ()):      # track_min_score may be negative, as InferStep's
            t = [0.1, 16.0, 0.5, 0.5, 0.0]
            t[q] = bad
            rc, text = call(thresholds=t)
            assert rc == -1 and "thresholds" in text, (q, bad)


# ------------------------------------------------------------------------------------------------ the seeded scene
def test_the_seeded_scene_has_what_it_promises_and_produces_every_outcome():
    s = D.scene()
    fidx = s["frame_index"]
    member = (fidx >= 0) & (fidx < D.N_FRAMES)
    assert s["preds"].shape == (130, 21, 2) and s["det_boxes"].shape == (75, 4) and D.N_FRAMES == 5
    assert np.bincount(fidx[member], minlength=5).tolist() == [70, 30, 12, 0, 10] and (~member).sum() == 8
    assert int((s["det_frame"] == 0).sum()) == 66
    assert 0.10 <= (s["src_frame"] < 0).mean() <= 0.20
    assert np.ptp(np.nonzero(fidx == 0)[0]) > 100                    # a frame's slots lie all over the batch
    result = D.run_host(s)
    got = D.outcomes(s, result)
    print(got)
    assert all(got[k] >= 3 for k in ("kept", "suppressed", "expired", "expired_unseeded", "seeded", "det-1", "det-2", "det-3", "det-4")), got
    # the crowded frame: fewer free slots than fresh detections
    two_free = int(((fidx == 2) & (result[2] != 0)).sum())
    fresh = (s["det_frame"] == 2) & (result[6] != -2) & (result[6] != -1) & (result[6] != -3)
    assert 0 < two_free < int(fresh.sum()) and int((result[6][fresh] == -4).sum()) == int(fresh.sum()) - two_free
    # an exact tie of two live slots' scores is in it, and the slots of no frame kept everything
    assert (result[4][~member] == D.SENTINEL).all() and (result[5][~member] == D.SENTINEL).all()
    assert result[0][~member].tobytes() == s["next_boxes"][~member].tobytes() and (result[3][~member] == s["lost_count"][~member]).all()
