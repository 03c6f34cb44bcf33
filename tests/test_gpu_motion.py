"""GPU: motion-aware tracking -- lh_rois_predict and lh_one_euro_gated bit for bit against topdown.rois_predict_host /
one_euro_gated_host on the seeded sequences of tests/motion_data.py (tests/test_motion_host.py guards that they reach every branch),
lh_one_euro_gated with the gate open against lh_one_euro itself, and ManagedInferStep / ManagedInferPipeline(motion=, smooth_gate=) on
the steps of tests/test_gpu_tracks_manage.py: ResNet-18, 64 x 64 crops, 4 frames of 96 x 128 (frame 2 is black), 5 slots."""
import numpy as np
import pytest
import torch

import motion_data as D
from test_gpu_tracks_manage import APART, B, BOXES, SHARED, SIZE, _dev, _options, _Recorder, _same, _snap, _step_frames
from test_gpu_topdown import _model

pytestmark = pytest.mark.gpu

F = np.float32


def _bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.nonzero((got.view(np.int32) != want.view(np.int32)).reshape(got.shape[0], -1).any(1))[0]
    assert bad.size == 0, f"{what}: rows {bad[:8].tolist()} differ: got {got[bad[:3]].tolist()}, want {want[bad[:3]].tolist()}"


# ------------------------------------------------------------------------------------------------ 1. lh_rois_predict
def _run_predict(seq, use_seeded, state=None):
    """The chained launches on ``seq`` from ``state`` (None: zeros) -> per frame (boxes, centre, vel, seen, coasted) as numpy."""
    from lighthand_amd.topdown import rois_predict
    b = seq[0]["next_boxes"].shape[0]
    if state is None:
        state = (np.zeros((b, 2), F), np.zeros((b, 2), F), np.zeros(b, np.int32), np.zeros(b, np.int32))
    state = tuple(_dev(a, a.dtype) for a in state)
    out = []
    for f in seq:
        boxes = _dev(f["next_boxes"], F)
        got = rois_predict(boxes, _dev(f["lost"], np.int32), _dev(f["src_frame"], np.int32), _dev(f["seeded"], np.int32) if use_seeded else None,
                           _dev(f["dt"], F), state, **D.PREDICT)
        assert got is boxes
        out.append(tuple(t.cpu().numpy() for t in (boxes,) + state))
    return out


@pytest.mark.parametrize("use_seeded", [True, False], ids=["seeded", "seeded-null"])
def test_rois_predict_is_bit_equal_to_the_host_restatement(use_seeded):
    seq = D.predict_sequence()
    want = D.run_predict_host(seq, D.PREDICT, use_seeded)
    got = _run_predict(seq, use_seeded)
    for t, (g, (boxes, state, _)) in enumerate(zip(got, want)):
        for name, a, w in zip(("next_boxes", "centre", "vel", "seen", "coasted"), g, (boxes,) + tuple(state)):
            _bits_equal(a, w, f"frame {t} {name}")
    moved = sum(int((g[0] != f["next_boxes"]).any(1).sum()) for g, f in zip(got, seq))
    assert moved > 200                                                    # it did shift boxes
    # two runs from the same state are bit-equal: the second half of the sequence from the state after the first
    mid = tuple(got[5][1:])
    for again in (_run_predict(seq[6:], use_seeded, mid), _run_predict(seq[6:], use_seeded, mid)):
        for t, (g, w) in enumerate(zip(again, got[6:])):
            for a, b_ in zip(g, w):
                _bits_equal(a, b_, f"rerun frame {6 + t}")


def test_rois_predict_single_slot_and_refusals():
    from lighthand_amd._lib import LightHandError
    from lighthand_amd.topdown import rois_predict, rois_predict_host
    a, b_ = np.array([[100, 100, 200, 200]], F), np.array([[103, 106, 203, 206]], F)
    state = tuple(torch.zeros(s, dtype=d, device="cuda") for s, d in (((1, 2), torch.float32), ((1, 2), torch.float32), ((1,), torch.int32), ((1,), torch.int32)))
    zero, dt, host = _dev([0], np.int32), _dev([1 / 30], F), None
    for box in (a, b_):
        dev = _dev(box, F)
        rois_predict(dev, zero, zero, None, dt, state)
        want, host = rois_predict_host(box, [0], [0], None, F(1 / 30), host)
        _bits_equal(dev.cpu().numpy(), want, "b = 1")
    _bits_equal(state[1].cpu().numpy(), host[1], "b = 1 vel")
    assert state[1].abs().min() > 0
    with pytest.raises(LightHandError, match="rois_predict"):
        rois_predict(_dev(a, F), zero, zero, None, dt.double(), state)
    with pytest.raises(LightHandError, match="lh_rois_predict"):
        rois_predict(_dev(a, F), zero, zero, None, dt, state, cutoff=0.0)


# ------------------------------------------------------------------------------------------------ 2. lh_one_euro_gated
@pytest.mark.parametrize("j", [21, 40], ids=["j21", "j40-strided"])
def test_one_euro_gated_is_bit_equal_to_the_host_restatement(j):
    from lighthand_amd.topdown import one_euro_gated, one_euro_gated_host
    seq = D.gated_sequence(j)
    for by_size, use_lost in ((True, True), (False, False)):
        kw = dict(min_cutoff=1.0, beta=0.05 if by_size else 0.007, d_cutoff=1.0, gate_min_score=0.5, by_size=by_size)
        state = (torch.zeros(D.B, j, 2, device="cuda"), torch.zeros(D.B, j, 2, device="cuda"), torch.zeros(D.B, j, dtype=torch.int32, device="cuda"),
                 torch.zeros(D.B, j, device="cuda"))
        host, filtered = None, 0
        for t, f in enumerate(seq):
            want, host = one_euro_gated_host(f["x"], f["maxvals"], f["dt"], host, f["src_frame"], f["lost"] if use_lost else None, f["next_boxes"], **kw)
            got = one_euro_gated(_dev(f["x"], F), _dev(f["maxvals"], F), _dev(f["dt"], F), state, _dev(f["src_frame"], np.int32),
                                 _dev(f["lost"], np.int32) if use_lost else None, _dev(f["next_boxes"], F) if by_size else None, **kw)
            _bits_equal(got.cpu().numpy(), want, f"frame {t} out (by_size {by_size})")
            for name, a, w in zip(("xhat", "dxhat", "seen_j", "gap"), state, host):
                _bits_equal(a.cpu().numpy(), w, f"frame {t} {name} (by_size {by_size})")
            filtered += int((want != f["x"]).any(2).sum())
        assert filtered > D.B * j * 3


@pytest.mark.parametrize("j", [21, 40], ids=["j21", "j40-strided"])
def test_with_the_gate_open_it_is_lh_one_euro_launched_beside_it(j):
    from lighthand_amd.topdown import GATE_OPEN, one_euro, one_euro_gated
    seq = D.gated_sequence(j)
    plain = (torch.zeros(D.B, j, 2, device="cuda"), torch.zeros(D.B, j, 2, device="cuda"), torch.zeros(D.B, dtype=torch.int32, device="cuda"))
    gated = (torch.zeros(D.B, j, 2, device="cuda"), torch.zeros(D.B, j, 2, device="cuda"), torch.zeros(D.B, j, dtype=torch.int32, device="cuda"),
             torch.zeros(D.B, j, device="cuda"))
    for t, f in enumerate(seq):
        x, dt, src, lost = _dev(f["x"], F), _dev(f["dt"], F), _dev(f["src_frame"], np.int32), _dev(f["lost"], np.int32)
        use_lost = lost if t % 3 else None
        want = one_euro(x, dt, plain, src, use_lost, 1.0, 0.007, 1.0)
        got = one_euro_gated(x, _dev(f["maxvals"], F), dt, gated, src, use_lost, None, 1.0, 0.007, 1.0, gate_min_score=GATE_OPEN, by_size=False)
        _bits_equal(got.cpu().numpy(), want.cpu().numpy(), f"frame {t} out")
        _bits_equal(gated[0].cpu().numpy(), plain[0].cpu().numpy(), f"frame {t} xhat")
        _bits_equal(gated[1].cpu().numpy(), plain[1].cpu().numpy(), f"frame {t} dxhat")
        assert torch.equal(gated[2], plain[2][:, None].expand(D.B, j)) and not gated[3].any()
    assert (got != x).any()


# ------------------------------------------------------------------------------------------------ 3. the captured step
MOTION = ("preds", "maxvals", "next_boxes", "next_rot", "lost", "boxes", "rot", "velocity", "coasted", "_centre", "_motion_seen")
BLACK = [2, 3, 1, 1, 2]                                            # APART with slot 0 on the black frame: a hand that was found goes lost


def _first():
    return dict(frames=_step_frames(), boxes=_dev(BOXES, F), frame_index=_dev(APART, np.int32))


def _pre_shift(step, oriented):
    """What the step's own next-ROI launch gives on its current outputs: the boxes lh_rois_predict was handed, and ``lost``."""
    from lighthand_amd.topdown import boxes_from_keypoints, rois_from_keypoints
    src = step.plan.src_frame
    if oriented:
        nxt, _, lost = rois_from_keypoints(step.preds, step.maxvals, step.boxes, step.rot, src, step.track_axis, step.track_min_score,
                                           step.track_min_joints, step.track_min_side, step.track_min_axis)
    else:
        nxt, lost = boxes_from_keypoints(step.preds, step.maxvals, step.boxes, src, step.track_min_score, step.track_min_joints, step.track_min_side)
    torch.cuda.synchronize()
    return nxt.cpu().numpy(), lost.cpu().numpy(), src.cpu().numpy()


def _six_replays(step, oriented, check_host=False):
    """Six replays with advance() between them; slot 0 looks at the black frame on replays 3 and 4.  Returns the snapshots."""
    from lighthand_amd.topdown import rois_predict_host
    step.reset_motion()
    if oriented:
        step.rot.copy_(torch.tensor([1.0, 0.0]).expand(B, 2))          # (a step that ran before has advanced its directions)
    host, snaps = None, []
    for t in range(6):
        feed = _first() if t == 0 else dict(frame_index=_dev(BLACK, np.int32)) if t == 3 else dict(frame_index=_dev(APART, np.int32)) if t == 5 else {}
        step(dt=1 / 30 if t != 4 else torch.tensor([1 / 30, 1 / 60, 1 / 30, 1 / 30, 1 / 30]).cuda(), **feed)
        snaps.append(_snap(step, MOTION))
        if check_host:
            nxt, lost, src = _pre_shift(step, oriented)
            assert np.array_equal(lost, snaps[-1]["lost"])
            want, host = rois_predict_host(nxt, lost, src, None, step.dt.cpu().numpy(), host, **step.motion)
            _bits_equal(snaps[-1]["next_boxes"], want, f"replay {t} next_boxes")
            for name, w in zip(("_centre", "velocity", "_motion_seen", "coasted"), host):
                _bits_equal(snaps[-1][name], w, f"replay {t} {name}")
            if oriented:
                assert np.array_equal(snaps[-1]["next_rot"].view(np.int32), _pre_rot(step).view(np.int32))
        step.advance()
    return snaps


def _pre_rot(step):
    from lighthand_amd.topdown import rois_from_keypoints
    _, nrot, _ = rois_from_keypoints(step.preds, step.maxvals, step.boxes, step.rot, step.plan.src_frame, step.track_axis, step.track_min_score,
                                     step.track_min_joints, step.track_min_side, step.track_min_axis)
    return nrot.cpu().numpy()


@pytest.mark.parametrize("oriented", [False, True], ids=["upright", "oriented"])
def test_step_predicts_coasts_and_matches_the_host_rule(oriented, monkeypatch):
    from lighthand_amd._lib import LightHandError
    from lighthand_amd.runtime import InferStep, ManagedInferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    options = _options(model, oriented)
    step = ManagedInferStep(model, B, SIZE, SIZE, manage_tracks=False, motion=dict(coast=2), **options)
    assert step.motion == dict(cutoff=10.0, lead=1.0, max_shift=0.5, coast=2) and step.smooth is None and step.dt.shape == (B,)
    assert step.velocity.shape == (B, 2) and step.coasted.dtype == torch.int32
    snaps = _six_replays(step, oriented, check_host=True)
    # the scenario is what it says (the weights are seeded random ones, so which crops of noise are found after the first frame is theirs to
    # say; the black frame's never are): slot 0 is found, then lost on the black frame; slots coasted, velocities were estimated, boxes moved
    print("lost per replay:", [s["lost"].tolist() for s in snaps], "coasted:", [s["coasted"].tolist() for s in snaps])
    assert snaps[0]["lost"].tolist() == [0, 0, 0, 1, 1] and snaps[3]["lost"][0] == 1 and snaps[4]["lost"][0] == 1
    assert snaps[0]["_motion_seen"].tolist() == [1, 1, 1, 0, 0] and not snaps[0]["velocity"].any()       # slot 3 is empty, slot 4 never found
    assert sum(int(s["coasted"].sum()) for s in snaps) > 0 and sum(int(s["velocity"].any(1).sum()) for s in snaps) > 0
    assert sum(int((s["next_boxes"] != s["boxes"]).any(1).sum()) for s in snaps) > 0
    assert all(np.array_equal(s["next_boxes"][3:], s["boxes"][3:]) for s in snaps)
    # the captured step equals the eager one (which has no warm-up run), and a second run of the captured one itself
    eager = ManagedInferStep(model, B, SIZE, SIZE, manage_tracks=False, motion=dict(coast=2), use_graph=False, **options)
    for other in (eager, step):
        for a, b_ in zip(snaps, _six_replays(other, oriented)):
            _same(a, b_)
    # reset_motion: the named slots, or all
    step._motion_seen.fill_(1)
    step.coasted.fill_(2)
    step.velocity.add_(3.0)
    before = _snap(step, ("velocity", "coasted", "_centre", "_motion_seen"))
    assert before["_centre"][:3].any(1).all()
    step.reset_motion([1, 3])
    after = _snap(step, ("velocity", "coasted", "_centre", "_motion_seen"))
    assert after["_motion_seen"].tolist() == [1, 0, 1, 0, 1] and after["coasted"].tolist() == [2, 0, 2, 0, 2]
    assert not after["velocity"][[1, 3]].any() and not after["_centre"][[1, 3]].any()
    for n in before:
        assert np.array_equal(before[n][[0, 2, 4]], after[n][[0, 2, 4]]), n
    step.reset_motion()
    assert not any(v.any() for v in _snap(step, ("velocity", "coasted", "_centre", "_motion_seen")).values())
    # calls the step cannot serve
    plain = InferStep(model, B, SIZE, SIZE, **options)
    with pytest.raises(LightHandError, match="motion"):
        plain.reset_motion()
    with pytest.raises(ValueError, match="dt is the input of InferStep"):
        plain(dt=1 / 30, **_first())
    with pytest.raises(TypeError, match="motion"):
        InferStep(model, B, SIZE, SIZE, motion=True, **options)


@pytest.mark.parametrize("oriented", [False, True], ids=["upright", "oriented"])
def test_without_the_keywords_the_step_and_its_launches_are_unchanged(oriented, monkeypatch):
    from lighthand_amd.runtime import ManagedInferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    options = dict(_options(model, oriented), smooth=(1.0, 0.007), use_graph=False)
    runs = []
    for extra in ({}, dict(motion=None, smooth_gate=None), dict(motion=True), dict(smooth_gate=True), dict(motion=True, smooth_gate=True)):
        step = ManagedInferStep(model, B, SIZE, SIZE, **options, **extra)
        names, snaps = [], []
        step.lib = _Recorder(step.lib, names)
        for t in range(3):
            if t:
                step.advance()
            step(**(_first() if t == 0 else {}))
            snaps.append(_snap(step, ("preds", "maxvals", "next_boxes", "next_rot", "lost", "lost_count", "smooth_preds", "boxes")))
        runs.append((names[:len(names) // 3], snaps, step))
    (plain, snaps0, step0), (none, snaps1, step1), (motion, _, _), (gate, _, _), (both, _, _) = runs
    assert none == plain and plain[-2:] == ["lh_tracks_manage", "lh_one_euro"]
    assert step1.motion is None and step1.smooth_gate is None and step1.velocity is None and step1.coasted is None
    for a, b_ in zip(snaps0, snaps1):
        _same(a, b_)
    assert motion == plain[:-1] + ["lh_rois_predict", "lh_one_euro"]
    assert gate == plain[:-1] + ["lh_one_euro_gated"] and "lh_one_euro" not in gate
    assert both == plain[:-1] + ["lh_rois_predict", "lh_one_euro_gated"]


def test_the_warm_up_run_is_not_a_frame(monkeypatch):
    """The first call of a captured step enqueues once eagerly before it captures; with the replay behind it left out, the motion state
    and the gated filter's must be as untouched as a new step's."""
    from lighthand_amd.runtime import ManagedInferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    options = dict(_options(model, False), smooth=(1.0, 0.007))
    step = ManagedInferStep(model, B, SIZE, SIZE, motion=dict(coast=2), smooth_gate=True, **options)
    assert step.smooth_gate == dict(min_score=step.track_min_score, by_size=True)
    with monkeypatch.context() as m:
        m.setattr(torch.cuda.CUDAGraph, "replay", lambda self: None)
        step(**_first())
    torch.cuda.synchronize()
    assert step.graph is not None and step.lost.cpu().tolist() == [0, 0, 0, 1, 1]                    # the warm-up did run
    for name in ("velocity", "coasted", "_centre", "_motion_seen", "_seen_j", "_gap", "_seen", "lost_count"):
        assert not getattr(step, name).any(), name
    step()                                                            # the first replay is the first frame
    torch.cuda.synchronize()
    assert step._motion_seen.cpu().tolist() == [1, 1, 1, 0, 0] and not step.velocity.any()
    assert np.array_equal(step.smooth_preds.cpu().numpy().view(np.int32), step.preds.cpu().numpy().view(np.int32))
    gin = (step.maxvals.reshape(B, -1) >= step.track_min_score).cpu().numpy()
    assert np.array_equal(step._seen_j.cpu().numpy()[:3] != 0, gin[:3]) and not step._seen_j[3:].any() and gin[:3].any() and not gin[:3].all()


def test_smooth_gate_in_the_step_is_the_eager_launch_on_its_own_state(monkeypatch):
    from lighthand_amd.runtime import ManagedInferStep
    from lighthand_amd.topdown import one_euro_gated
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    options = dict(_options(model, True), smooth=(1.0, 0.5))
    step = ManagedInferStep(model, B, SIZE, SIZE, manage_tracks=False, smooth_gate=dict(by_size=True), **options)
    state = tuple(torch.zeros_like(t) for t in (step._xhat, step._dxhat, step._seen_j, step._gap))
    differs = 0
    for t in range(6):                                                # slot 1 alternates between two frames that both layouts find it on
        step(dt=1 / 30, **(_first() if t == 0 else dict(frame_index=_dev(SHARED if t % 2 else APART, np.int32))))
        want = one_euro_gated(step.preds, step.maxvals, step.dt, state, step.plan.src_frame, step.lost, step.next_boxes, 1.0, 0.5, 1.0,
                              gate_min_score=step.track_min_score, by_size=True)
        torch.cuda.synchronize()
        assert torch.equal(step.smooth_preds.view(torch.int32), want.view(torch.int32)), t
        for a, b_ in zip(state, (step._xhat, step._dxhat, step._seen_j, step._gap)):
            assert torch.equal(a.view(torch.int32), b_.view(torch.int32)), t
        differs += int((step.smooth_preds != step.preds).any(2).sum())
    assert differs > 0 and step._gap.any() and step.lost.cpu().tolist() == [0, 0, 0, 1, 1]
    step.reset_filter([0])
    assert not step._seen_j[0].any() and not step._gap[0].any() and step._seen_j[1].any() and step._seen.cpu().tolist()[0] == 0
    step.reset_filter()
    assert not step._seen_j.any() and not step._gap.any()


def test_a_seeded_slot_starts_its_motion_state_fresh(monkeypatch):
    from lighthand_amd.runtime import ManagedInferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    options = _options(model, False)
    det = [30.0, 20.5, 100.0, 80.25]                                     # a detection on the black frame
    runs = {}
    for seeds in (True, False):
        step = ManagedInferStep(model, B, SIZE, SIZE, manage_tracks=dict(max_detections=2), motion=dict(coast=5), **options)
        for t in range(4):
            feed = _first() if t == 0 else dict(frame_index=_dev(BLACK, np.int32)) if t == 2 else {}
            dets = (_dev([det], F), _dev([2], np.int32), _dev([0.9], F)) if seeds and t == 3 else None
            step(detections=dets, **feed)
            if t < 3:
                step.advance()
        runs[seeds] = _snap(step, MOTION + ("seeded",))
    seeded, coasting = runs[True], runs[False]
    # without the detection slot 0, found on the first frame and lost on the black one, coasts at least for the second time
    assert coasting["lost"][0] == 1 and coasting["coasted"][0] >= 2 and coasting["_motion_seen"][0] == 1
    assert np.array_equal(coasting["next_boxes"][0], coasting["boxes"][0]) == (not coasting["velocity"][0].any())
    # with it the detection takes slot 0, the lowest slot of frame 2 that is not kept: its box is the detection's, unshifted, its state new
    assert seeded["seeded"].tolist() == [0, -1, -1, -1, -1] and seeded["next_boxes"][0].tobytes() == np.asarray(det, F).tobytes()
    assert seeded["_motion_seen"][0] == 0 and seeded["coasted"][0] == 0 and not seeded["velocity"][0].any()
    for n in ("velocity", "coasted", "_motion_seen", "next_boxes"):
        assert np.array_equal(seeded[n][1:], coasting[n][1:]), n


# ------------------------------------------------------------------------------------------------ 4. the pipeline, the tool
def test_pipeline_slots_own_their_motion_state(monkeypatch):
    from lighthand_amd.runtime import ManagedInferPipeline, ManagedInferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    options = dict(_options(model, False), smooth=(1.0, 0.007))
    moved = (np.asarray(BOXES, F) + F([6, -4, 6, -4]) * (np.asarray(BOXES, F).any(1, keepdims=True))).astype(F)
    pipe = ManagedInferPipeline(model, B, SIZE, SIZE, depth=2, manage_tracks=False, motion=True, smooth_gate=True, **options)
    t0 = pipe.submit(**_first())                        # pipeline slot 0
    t1 = pipe.submit(**_first())                        # pipeline slot 1
    t2 = pipe.submit(boxes=_dev(moved, F))              # pipeline slot 0 again: its second frame, somewhere else
    pipe.result(t1)
    pipe.result(t2)
    torch.cuda.synchronize()
    assert t0 == 0 and pipe.steps[0].velocity is not pipe.steps[1].velocity
    one = _snap(pipe.steps[1], ("velocity", "coasted", "_motion_seen", "_gap"))
    assert one["_motion_seen"].tolist() == [1, 1, 1, 0, 0] and not one["velocity"].any()
    two = _snap(pipe.steps[0], ("velocity", "next_boxes", "smooth_preds", "_centre", "_seen_j", "_gap"))
    assert two["velocity"][:3].any() and not two["velocity"][3:].any()      # (a slot the weights lose on the moved crop forgets its own)
    single = ManagedInferStep(model, B, SIZE, SIZE, manage_tracks=False, motion=True, smooth_gate=True, **options)
    single(**_first())
    single(boxes=_dev(moved, F))
    _same(two, _snap(single, tuple(two)))


def test_track_frames_cli_with_motion_and_the_gate(capsys):
    import json

    from lighthand_amd.tools import track_frames as T
    result = T.main(["--synthetic", "8", "--frame_size", "96x128", "--hands", "3", "--depth", "18", "--size", "64", "--oriented", "--one_euro", "1.0",
                     "0.007", "--motion", "--coast", "2", "--smooth_gate"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == result
    assert result["motion"] == dict(cutoff=10.0, lead=1.0, coast=2) and result["frames"] == 8 and result["mean_speed_px_s"] >= 0
    assert 0 <= result["slots_coasted"] <= result["slots_lost"] <= 24
    assert result["smooth_gate"] == dict(min_score=result["track_min_score"], by_size=True)
