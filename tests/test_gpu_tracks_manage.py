"""GPU: track management of the tracked top-down step -- lh_tracks_manage bit for bit against topdown.manage_tracks_host on the seeded
scene of tests/tracks_manage_data.py (tests/test_tracks_manage_host.py guards that the scene produces every outcome), its edge shapes,
and ManagedInferStep / ManagedInferPipeline on top of it: ResNet-18, 64 x 64 crops, 4 frames of 96 x 128 (frame 2 is black) and 5
slots, as tests/test_gpu_roi.py builds its steps."""
import numpy as np
import pytest
import torch

import tracks_manage_data as D
from test_gpu_topdown import _frames, _model

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("next_boxes", "next_rot", "lost", "lost_count", "dup_of", "seeded", "det_state")


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a, dtype)).cuda()


def _launch(s, n_frames, next_rot=True, **options):
    """topdown.manage_tracks on the arrays of ``s``, dup_of / seeded / det_state starting at the sentinel -> the seven outputs as numpy."""
    from lighthand_amd.topdown import manage_tracks
    b, k = s["preds"].shape[0], s["det_boxes"].shape[0]
    f32 = {n: _dev(s[n], np.float32) for n in ("preds", "maxvals", "next_boxes", "det_boxes", "det_score")}
    i32 = {n: _dev(s[n], np.int32) for n in ("src_frame", "frame_index", "lost", "lost_count", "det_frame")}
    rot = _dev(s["next_rot"], np.float32) if next_rot else None
    sent = [torch.full((n,), D.SENTINEL, dtype=torch.int32, device="cuda") for n in (b, b, k)]
    out = manage_tracks(f32["preds"], f32["maxvals"], i32["src_frame"], i32["frame_index"], n_frames, f32["next_boxes"], rot, i32["lost"],
                        i32["lost_count"], f32["det_boxes"], i32["det_frame"], f32["det_score"], *sent, **options)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def _assert_bit_equal(got, want):
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            assert g is None, name
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, name
        bad = np.nonzero((g.view(np.int32) != w.view(np.int32)).reshape(g.shape[0], -1).any(1))[0]
        assert bad.size == 0, f"{name}: rows {bad[:8].tolist()} differ: got {g[bad[:3]].tolist()}, want {w[bad[:3]].tolist()}"


# ------------------------------------------------------------------------------------------------ 1. the kernel
def test_kernel_is_bit_equal_to_the_host_restatement_on_the_seeded_scene():
    s = D.scene()
    want = list(D.run_host(s))
    # det_state has no sentinel in the host's result: every entry is written (-1 for the invalid ones)
    got = _launch(s, D.N_FRAMES, **D.OPTIONS)
    _assert_bit_equal(got, want)
    member = (s["frame_index"] >= 0) & (s["frame_index"] < D.N_FRAMES)
    assert (got[4][~member] == D.SENTINEL).all() and (got[5][~member] == D.SENTINEL).all() and (got[6] != D.SENTINEL).all()
    assert got[0][~member].tobytes() == s["next_boxes"][~member].tobytes() and got[1][~member].tobytes() == s["next_rot"][~member].tobytes()
    untouched = member & (got[4] < 0) & (got[5] < 0) & ~((got[0] == 0).all(1))          # neither suppressed, seeded nor expired
    assert untouched.sum() > 30 and got[0][untouched].tobytes() == s["next_boxes"][untouched].tobytes()
    again = _launch(s, D.N_FRAMES, **D.OPTIONS)
    _assert_bit_equal(again, got)
    # other thresholds take other decisions, and the same ones as the host
    other = dict(dup_overlap=0.2, match_overlap=0.8, det_min_score=0.0, max_lost=0)
    got2 = _launch(s, D.N_FRAMES, **dict(D.OPTIONS, **other))
    _assert_bit_equal(got2, list(D.run_host(s, **other)))
    assert not np.array_equal(got2[6], got[6]) and not np.array_equal(got2[4], got[4])


def test_kernel_edge_shapes():
    from lighthand_amd.topdown import manage_tracks_host
    s = D.scene()
    # next_rot null: an upright step
    got = _launch(s, D.N_FRAMES, next_rot=False, **D.OPTIONS)
    _assert_bit_equal(got, list(D.run_host(s, next_rot=False)))
    # b = 1, k = 1: a lost slot takes the one detection; then a live one that the detection covers
    for lost, state in ((1, 0), (0, -2)):
        one = dict(preds=np.tile(F([[100, 100], [180, 190]]), (1, 11, 1))[:, :21], maxvals=np.full((1, 21), 0.5, F), src_frame=[0], frame_index=[0],
                   lost=[lost], lost_count=[4], next_boxes=[[1, 2, 3, 4]], next_rot=[[0.6, 0.8]], det_boxes=[[120, 120, 160, 170]], det_frame=[0],
                   det_score=[0.5])
        one = {k: np.asarray(v, np.int32 if k in ("src_frame", "frame_index", "lost", "lost_count", "det_frame") else F) for k, v in one.items()}
        got = _launch(one, 1)
        want = manage_tracks_host(one["preds"], one["maxvals"], one["src_frame"], one["frame_index"], 1, one["next_boxes"], one["next_rot"],
                                  one["lost"], one["lost_count"], one["det_boxes"], one["det_frame"], one["det_score"],
                                  dup_of=[D.SENTINEL], seeded=[D.SENTINEL])
        _assert_bit_equal(got, list(want))
        assert got[6].tolist() == [state] and got[5].tolist() == [0 if state == 0 else -1]
    # j = 1: a one-joint box is min_side wide
    rng = np.random.RandomState(3)
    few = dict(preds=rng.uniform(0, 60, size=(9, 1, 2)).astype(F), maxvals=rng.uniform(0.05, 1, size=(9, 1)).astype(F), src_frame=np.zeros(9, np.int32),
               frame_index=np.zeros(9, np.int32), lost=(np.arange(9) % 4 == 3).astype(np.int32), lost_count=np.arange(9, dtype=np.int32),
               next_boxes=rng.uniform(1, 9, size=(9, 4)).astype(F), next_rot=rng.uniform(-1, 1, size=(9, 2)).astype(F),
               det_boxes=np.concatenate([rng.uniform(0, 40, size=(6, 2)), rng.uniform(45, 80, size=(6, 2))], 1).astype(F),
               det_frame=np.zeros(6, np.int32), det_score=rng.uniform(0, 1, 6).astype(F))
    got = _launch(few, 1, max_lost=5)
    want = manage_tracks_host(few["preds"], few["maxvals"], few["src_frame"], few["frame_index"], 1, few["next_boxes"], few["next_rot"], few["lost"],
                              few["lost_count"], few["det_boxes"], few["det_frame"], few["det_score"], max_lost=5,
                              dup_of=np.full(9, D.SENTINEL), seeded=np.full(9, D.SENTINEL))
    _assert_bit_equal(got, list(want))
    assert (got[4] >= 0).any()


def _crowd(b, k, n_frames, seed):
    """b slots and k detections on hands spread over n_frames large frames, three quarters of the slots live, no slot of no frame."""
    rng = np.random.RandomState(seed)
    centre = rng.uniform(100, 3900, size=(b, 1, 2))
    det_c, det_h = rng.uniform(100, 3900, size=(k, 2)), rng.uniform(20, 60, size=(k, 1))
    return dict(preds=(centre + rng.uniform(-50, 50, size=(b, D.J, 2))).astype(F), maxvals=rng.uniform(0.05, 1, size=(b, D.J)).astype(F),
                src_frame=np.arange(b, dtype=np.int32) % n_frames, frame_index=np.arange(b, dtype=np.int32) % n_frames,
                lost=(np.arange(b) % 4 == 3).astype(np.int32), lost_count=rng.randint(0, 4, size=b).astype(np.int32),
                next_boxes=rng.uniform(1, 9, size=(b, 4)).astype(F), next_rot=rng.uniform(-1, 1, size=(b, 2)).astype(F),
                det_boxes=np.concatenate([det_c - det_h, det_c + det_h], 1).astype(F), det_frame=rng.randint(0, n_frames, size=k).astype(np.int32),
                det_score=rng.uniform(0, 1, size=k).astype(F))


def test_kernel_at_the_largest_shapes_the_entry_admits():
    """1024 slots and 1024 detections: the launch's LDS block, sized by b and k, is at its largest (59 KB), on one frame (every walk at
    its longest) and on three."""
    from lighthand_amd.topdown import manage_tracks_host
    for n_frames in (1, 3):
        s = _crowd(1024, 1024, n_frames, 11 + n_frames)
        got = _launch(s, n_frames, max_lost=3)
        want = manage_tracks_host(s["preds"], s["maxvals"], s["src_frame"], s["frame_index"], n_frames, s["next_boxes"], s["next_rot"], s["lost"],
                                  s["lost_count"], s["det_boxes"], s["det_frame"], s["det_score"], max_lost=3,
                                  dup_of=np.full(1024, D.SENTINEL), seeded=np.full(1024, D.SENTINEL))
        _assert_bit_equal(got, list(want))
        counts = [int((got[4] >= 0).sum()), int((got[5] >= 0).sum())] + [int((got[6] == v).sum()) for v in (-2, -3)]
        print(f"{n_frames} frames: suppressed, seeded, tracked, repeated = {counts}")
        assert min(counts) >= 3


# ------------------------------------------------------------------------------------------------ 2. the captured step
B, SIZE, NF, FH, FW = 5, 64, 4, 96, 128
HAND, OTHER, DARK = [20.0, 10.0, 90.0, 80.0], [5.0, 20.0, 45.0, 70.0], [30.0, 20.0, 100.0, 80.0]
DET = [84.0, 20.5, 124.0, 70.25]                                    # a detection on frame 1, clear of OTHER's crop
BOXES = [HAND, HAND, OTHER, [0.0, 0.0, 0.0, 0.0], DARK]             # slot 3 starts empty, slot 4 looks at the black frame
APART = [0, 3, 1, 1, 2]                                             # every live slot on a frame of its own: no duplicates
SHARED = [0, 0, 1, 1, 2]                                            # slots 0 and 1 crop the same pixels: an exact tie
OUTPUTS = ("preds", "maxvals", "next_boxes", "next_rot", "lost")
MANAGED = OUTPUTS + ("lost_count", "dup_of", "seeded", "det_state", "boxes", "rot", "smooth_preds")


def _step_frames():
    frames = _frames(NF, FH, FW, 31)
    frames[2] = 0
    return torch.from_numpy(frames).cuda()


def _options(model, oriented):
    """The tracking options of every step here.  The weights are seeded random ones, so a crop's confidences mean nothing and the black
    crop's lie among those of the crops of noise; the probe step's maxvals are searched for the threshold s at which the three crops of
    noise (under both slot layouts) have the most joints at or above s in excess of the black crop's: track_min_score = s (moved half-way
    to the next lower maxval) and track_min_joints = the lowest such count of a crop of noise make the black slot lost and the others live."""
    from lighthand_amd.runtime import InferStep
    probe = InferStep(model, B, SIZE, SIZE, frames=(NF, FH, FW), oriented=oriented)
    noise = []
    for index in (SHARED, APART):
        probe(frames=_step_frames(), boxes=_dev(BOXES, np.float32), frame_index=_dev(index, np.int32))
        torch.cuda.synchronize()
        assert probe.valid.cpu().tolist() == [True, True, True, False, True]
        mv = probe.maxvals.cpu().numpy().reshape(B, -1)
        noise += [mv[0], mv[1], mv[2]]
    black, noise = mv[4], np.stack(noise)
    values = np.unique(np.concatenate([black, noise.reshape(-1)]))
    best = max(((noise >= s).sum(1).min() - (black >= s).sum(), n) for n, s in enumerate(values) if n)
    print(f"threshold {float(values[best[1]]):.6f}: {int((black >= values[best[1]]).sum())} joints of the black crop at or above it, "
          f"{(noise >= values[best[1]]).sum(1).tolist()} of the crops of noise")
    assert best[0] >= 1, "no threshold makes the black crop lost and the crops of noise live"
    s = values[best[1]]
    return dict(frames=(NF, FH, FW), oriented=oriented, track=True, track_min_joints=int((noise >= s).sum(1).min()), track_min_side=12.0,
                track_min_score=float((s + values[best[1] - 1]) * 0.5))


def _snap(step, names):
    torch.cuda.synchronize()
    return {n: getattr(step, n).cpu().numpy().copy() for n in names if getattr(step, n) is not None}


def _same(a, b, names=None):
    for n in names or a:
        assert np.array_equal(a[n].view(np.int32), b[n].view(np.int32)), n


@pytest.mark.parametrize("oriented", [False, True], ids=["upright", "oriented"])
def test_with_nothing_to_manage_the_step_is_the_plain_step(oriented, monkeypatch):
    from lighthand_amd.runtime import InferStep, ManagedInferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    options = _options(model, oriented)
    first = dict(frames=_step_frames(), boxes=_dev(BOXES, np.float32), frame_index=_dev(APART, np.int32))
    runs = []
    for extra in (None, dict(manage_tracks=True)):
        step = ManagedInferStep(model, B, SIZE, SIZE, **options, **extra) if extra else InferStep(model, B, SIZE, SIZE, **options)
        snaps = []
        for t in range(3):
            if t:
                step.advance()
            step(**(first if t == 0 else {}))
            snaps.append(_snap(step, OUTPUTS))
        runs.append(snaps)
        if extra:
            lost = np.stack([x["lost"] for x in snaps])
            runs_lost = [int(lost[:, i][::-1].cumprod().sum()) for i in range(B)]      # the replays in a row a slot has been lost
            runs_lost[3] = 0                                                          # ... an empty slot does not count
            assert runs_lost[4] == 3 and step.lost_count.cpu().tolist() == runs_lost   # max_lost = 0 counts and never expires
            assert step.dup_of.cpu().tolist() == [-1] * B and step.seeded.cpu().tolist() == [-1] * B and step.det_state.cpu().tolist() == [-1] * B
    assert runs[0][0]["lost"].tolist() == [0, 0, 0, 1, 1] and ("next_rot" in runs[0][0]) == oriented
    assert not np.array_equal(runs[0][0]["preds"], runs[0][1]["preds"])               # the slots moved: three different frames
    for plain, managed in zip(*runs):
        _same(plain, managed)


def _scenario(step, first):
    """Three frames with advance() between them, a detection list on the first call only (its second entry names no frame).  Returns
    the snapshots after each replay and, for the first two, after the advance() behind it, and ``valid`` after every replay."""
    step.reset_tracks()
    step.reset_filter()
    out, valid = [], []
    for t in range(3):
        if t == 0:
            step(detections=(_dev([DET, DET], np.float32), [1, 7], torch.tensor([0.9, 0.9])), **first)
        else:
            step()
        out.append(_snap(step, MANAGED))
        valid.append(step.valid.cpu().tolist())
        if t < 2:
            step.advance()
            out.append(_snap(step, ("boxes", "rot")))
    return out, valid


@pytest.mark.parametrize("oriented", [False, True], ids=["upright", "oriented"])
def test_step_suppresses_a_duplicate_seeds_a_detection_and_expires_a_lost_slot(oriented, monkeypatch):
    from lighthand_amd._lib import LightHandError
    from lighthand_amd.runtime import InferStep, ManagedInferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    options = dict(_options(model, oriented), smooth=(1.0, 0.007))
    first = dict(frames=_step_frames(), boxes=_dev(BOXES, np.float32), frame_index=_dev(SHARED, np.int32))
    manage = dict(max_lost=2, max_detections=4)
    step = ManagedInferStep(model, B, SIZE, SIZE, manage_tracks=manage, **options)
    assert step.manage_tracks == dict(max_detections=4, dup_overlap=0.5, match_overlap=0.5, det_min_score=0.0, max_lost=2)
    assert step.det_boxes.shape == (4, 4) and step.det_frame.cpu().tolist() == [-1] * 4 and step.lost_count.cpu().tolist() == [0] * B
    (one, moved1, two, moved2, three), valid = _scenario(step, first)
    zero, det = [0.0] * 4, np.asarray(DET, np.float32)

    # frame 1: slots 0 and 1 tie, the higher index goes; the detection takes the empty slot 3; the black slot has been lost once
    assert one["lost"].tolist() == [0, 1, 0, 1, 1] and one["dup_of"].tolist() == [-1, 0, -1, -1, -1]
    assert np.array_equal(one["preds"][0].view(np.int32), one["preds"][1].view(np.int32)) and one["next_boxes"][1].tolist() == zero
    assert one["seeded"].tolist() == [-1, -1, -1, 0, -1] and one["det_state"].tolist() == [3, -1, -1, -1]
    assert one["next_boxes"][3].tobytes() == det.tobytes() and one["next_boxes"][4].tolist() == DARK
    assert one["lost_count"].tolist() == [0, 0, 0, 0, 1]              # the warm-up run before the capture did not count
    assert np.array_equal(one["smooth_preds"][1].view(np.int32), one["preds"][1].view(np.int32))      # the filter saw the final lost
    assert moved1["boxes"][1].tolist() == zero and moved1["boxes"][3].tobytes() == det.tobytes()
    if oriented:
        assert one["next_rot"][3].tolist() == [1.0, 0.0] and moved1["rot"][3].tolist() == [1.0, 0.0]
    # frame 2: the suppressed slot is empty and the seeded one is not; nothing is seeded by the stale list; the black slot expires
    assert two["boxes"][3].tobytes() == det.tobytes()
    assert two["seeded"].tolist() == [-1] * B and two["det_state"].tolist() == [-1] * 4 and two["dup_of"].tolist() == [-1] * B
    assert step.det_frame.cpu().tolist() == [-1] * 4
    assert two["lost"][1] == 1 and two["next_boxes"][1].tolist() == zero
    assert two["next_boxes"][4].tolist() == zero and two["lost_count"][4] == 0 and two["lost"][4] == 1
    assert moved2["boxes"][4].tolist() == zero
    assert valid == [[True, True, True, False, True], [True, False, True, True, True], [True, False, True, True, False]]

    # the winner goes on as in the plain step, frame after frame
    plain = InferStep(model, B, SIZE, SIZE, **options)
    count = np.zeros(B, np.int64)
    for t, managed in enumerate((one, two, three)):
        if t:
            plain.advance()
        plain(**(first if t == 0 else {}))
        p = _snap(plain, OUTPUTS + ("smooth_preds",))
        for i in (0, 2):
            # (a slot the seeded weights lose twice in a row expires like any other: its next box is then the zero box, nothing else differs)
            expired = managed["lost"][i] == 1 and count[i] + 1 >= manage["max_lost"]
            for n in p:
                want = np.zeros(4, np.float32) if expired and n == "next_boxes" else p[n][i]
                assert np.array_equal(want.view(np.int32), managed[n][i].view(np.int32)), (t, i, n)
        count = managed["lost_count"]
    # the captured step equals the eager one (which has no warm-up run) on every output, and a second run of the captured one itself
    eager = ManagedInferStep(model, B, SIZE, SIZE, manage_tracks=manage, use_graph=False, **options)
    for other in (eager, step):
        snaps, valid2 = _scenario(other, first)
        assert valid2 == valid
        for a, b_ in zip((one, moved1, two, moved2, three), snaps):
            _same(a, b_)
    # refusals of the calls the step cannot serve
    off = ManagedInferStep(model, B, SIZE, SIZE, manage_tracks=False, **options)          # InferStep as it is: nothing of the option exists
    assert off.manage_tracks is None and off.det_boxes is None and off.lost_count is None
    with pytest.raises(ValueError, match="manage_tracks"):
        off(detections=(_dev([DET], np.float32), [1], [0.9]))
    with pytest.raises(TypeError, match="detections"):
        plain(detections=(_dev([DET], np.float32), [1], [0.9]))
    with pytest.raises(LightHandError, match="manage_tracks"):
        plain.reset_tracks()
    with pytest.raises(ValueError, match="max_detections"):
        step(detections=(np.zeros((5, 4), F), [0] * 5, [0.5] * 5))
    with pytest.raises(ValueError, match="track=True"):
        ManagedInferStep(model, B, SIZE, SIZE, frames=(NF, FH, FW))
    # reset_tracks: all, or the named slots
    step.lost_count.copy_(torch.tensor([5, 6, 7, 8, 9], dtype=torch.int32))
    step.reset_tracks([1, 3])
    assert step.lost_count.cpu().tolist() == [5, 0, 7, 0, 9]
    step.reset_tracks()
    assert step.lost_count.cpu().tolist() == [0] * B


# ------------------------------------------------------------------------------------------------ 3. InferPipeline
def test_pipeline_slots_own_their_detections_and_counts(monkeypatch):
    from lighthand_amd.runtime import ManagedInferPipeline
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    options = _options(model, False)
    pipe = ManagedInferPipeline(model, B, SIZE, SIZE, depth=2, manage_tracks=dict(max_lost=5, max_detections=3), **options)
    first = dict(frames=_step_frames(), boxes=_dev(BOXES, np.float32), frame_index=_dev(SHARED, np.int32))
    dets = (_dev([DET], np.float32), _dev([1], np.int32), _dev([0.9], np.float32))
    t0 = pipe.submit(detections=dets, **first)          # pipeline slot 0, with the detection
    t1 = pipe.submit(**first)                           # pipeline slot 1, without
    t2 = pipe.submit()                                  # pipeline slot 0 again: its second replay, the list is stale
    pipe.result(t1)
    pipe.result(t2)
    torch.cuda.synchronize()
    assert t0 == 0 and pipe.steps[1].seeded.cpu().tolist() == [-1] * B and pipe.steps[1].det_state.cpu().tolist() == [-1] * 3
    assert pipe.steps[1].dup_of.cpu().tolist() == [-1, 0, -1, -1, -1]
    assert pipe.steps[0].seeded.cpu().tolist() == [-1] * B and pipe.steps[0].det_frame.cpu().tolist() == [-1] * 3
    assert pipe.steps[0].lost_count.cpu().tolist() == [0, 0, 0, 0, 2] and pipe.steps[1].lost_count.cpu().tolist() == [0, 0, 0, 0, 1]
    t3 = pipe.submit(detections=dets)                   # pipeline slot 1: the detection reaches the slot that runs the ticket
    pipe.result(t3)
    torch.cuda.synchronize()
    assert pipe.steps[1].seeded.cpu().tolist() == [-1, -1, -1, 0, -1] and pipe.steps[1].det_state.cpu().tolist() == [3, -1, -1]
    assert pipe.steps[1].next_boxes[3].cpu().numpy().tobytes() == np.asarray(DET, np.float32).tobytes()
    assert pipe.steps[0].seeded.cpu().tolist() == [-1] * B


# ------------------------------------------------------------------------------------------------ 4. launch order
class _Recorder:
    """The library of a step with every entry's name noted as it is called (tests/test_gpu_step_launch_lists.py reads ``fn.__name__``
    of the plan's list; the tracking launches are the step's own calls, so they are read here)."""

    def __init__(self, lib, names):
        self._lib, self._names = lib, names

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self._names.append(fn.__name__)
            return fn(*args)
        return call


@pytest.mark.parametrize("oriented", [False, True], ids=["upright", "oriented"])
def test_the_launch_sits_between_the_next_roi_and_the_filter(oriented, monkeypatch):
    from lighthand_amd.runtime import InferStep, ManagedInferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    lists = []
    for cls in (InferStep, ManagedInferStep):
        step = cls(model, B, SIZE, SIZE, frames=(NF, FH, FW), oriented=oriented, track=True, smooth=(1.0, 0.007), use_graph=False)
        plan_list = [c.fn.__name__ for c in step.plan.fwd if hasattr(c, "fn")]
        names = []
        step.lib = _Recorder(step.lib, names)
        step(frames=_step_frames(), boxes=_dev(BOXES, np.float32), frame_index=_dev(APART, np.int32))
        torch.cuda.synchronize()
        lists.append((plan_list, names))
    (plan_plain, plain), (plan_managed, managed) = lists
    to_next = "lh_keypoints_to_rois" if oriented else "lh_keypoints_to_boxes"
    assert plan_managed == plan_plain and "lh_tracks_manage" not in plan_plain
    assert plain[-3:] == ["lh_affine_points", to_next, "lh_one_euro"] and "lh_tracks_manage" not in plain
    assert managed[-4:] == ["lh_affine_points", to_next, "lh_tracks_manage", "lh_one_euro"] and managed.count("lh_tracks_manage") == 1
    assert [n for n in managed if n != "lh_tracks_manage"] == plain


# ------------------------------------------------------------------------------------------------ 5. the tool
def test_track_frames_cli_with_detections(capsys):
    import json

    from lighthand_amd.tools import track_frames as T
    result = T.main(["--synthetic", "10", "--frame_size", "96x128", "--hands", "3", "--depth", "18", "--size", "64", "--oriented", "--one_euro", "1.0",
                     "0.007", "--detect_every", "3", "--max_lost", "2"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == result
    # frames 0, 3, 6, 9 with 3 hands each, less hand 0 on the frames it is away (4 and 5: none of those), plus its re-entry on frame 6
    assert result["detect_every"] == 3 and result["max_lost"] == 2 and result["detections"] == 12 and result["frames"] == 10
    assert all(0 <= result[k] <= 30 for k in ("slots_seeded", "slots_suppressed", "slots_expired", "slots_lost"))
    assert result["slots_seeded"] <= result["detections"]
