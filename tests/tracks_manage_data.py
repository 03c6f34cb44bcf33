"""The seeded scene that tests/test_tracks_manage_host.py and tests/test_gpu_tracks_manage.py share: 130 slots and 75 detections on 5
frames of 640 x 480, 21 joints.  Frame 0 owns 70 slots and 66 detections (more than the 64 lanes of lh_tracks_manage's one wave, so every
strided loop wraps), frame 3 owns no slot, 8 slots have a frame_index out of range, about 15 % of the slots are empty, the hands are
clustered (slots share hands, detections repeat hands) and frame 2 has fewer free slots than fresh detections."""
import numpy as np

F = np.float32
B, K, N_FRAMES, J = 130, 75, 5, 21
SEED = 31
SENTINEL = -77                      # what dup_of / seeded / det_state hold before a launch
OPTIONS = dict(min_score=0.1, min_side=16.0, dup_overlap=0.5, match_overlap=0.5, det_min_score=0.2, max_lost=3)
SLOTS_OF = {0: 70, 1: 30, 2: 12, 4: 10}            # frame -> slots; the other 8 belong to no frame


def _hand(rng, centre, size):
    """21 joints spread over a size x size square about centre, maxvals mostly confident."""
    pts = centre + rng.uniform(-0.5, 0.5, size=(J, 2)) * size
    return pts.astype(F), rng.choice([0.05, 0.3, 0.5, 0.7, 0.9, 0.95], size=J).astype(F)


def scene(seed=SEED):
    """dict of numpy arrays: preds [B][J][2], maxvals [B][J], src_frame, frame_index, lost, lost_count [B], next_boxes [B][4], next_rot
    [B][2], det_boxes [K][4], det_frame, det_score [K].  The slots of a frame are dealt over all slot numbers (a frame's slots are not
    contiguous)."""
    rng = np.random.RandomState(seed)
    frame_index = np.concatenate([np.full(n, f) for f, n in SLOTS_OF.items()] + [np.array([-1, -1, -3, 5, 5, 6, 99, -2 ** 31])]).astype(np.int32)
    assert frame_index.shape == (B,)
    frame_index = frame_index[rng.permutation(B)]
    preds, maxvals = np.zeros((B, J, 2), F), np.zeros((B, J), F)
    src, lost, count = np.full(B, -1, np.int32), np.ones(B, np.int32), rng.choice([0, 1, 2, 5, 2 ** 30], size=B).astype(np.int32)
    next_boxes = np.concatenate([rng.uniform(0, 300, size=(B, 2)), rng.uniform(320, 640, size=(B, 2))], 1).astype(F)
    ang = rng.uniform(-np.pi, np.pi, B)
    next_rot = np.stack([np.cos(ang), np.sin(ang)], 1).astype(F)
    hands = {f: np.stack([rng.uniform(60, 580, 25), rng.uniform(60, 420, 25)], 1) for f in range(N_FRAMES)}
    sizes = {f: rng.uniform(50, 110, 25) for f in range(N_FRAMES)}
    in_range = (frame_index >= 0) & (frame_index < N_FRAMES)
    for i in range(B):
        f = int(frame_index[i])
        if not in_range[i]:
            # a slot of no frame: whatever it holds stays; half of them look live
            preds[i], maxvals[i] = _hand(rng, np.array([320.0, 240.0]), 80.0)
            lost[i] = i % 2
            continue
        if f == 2:
            continue
        kind = rng.choice(["live", "lost", "empty"], p=[0.6, 0.25, 0.15])
        h = rng.randint(0, 14)                                              # slots follow the first 14 hands: they share them
        preds[i], maxvals[i] = _hand(rng, hands[f][h] + rng.uniform(-6, 6, 2), sizes[f][h] * rng.uniform(0.8, 1.1))
        if kind != "empty":
            src[i] = f
        if kind == "live":
            lost[i] = 0
        elif kind == "lost":
            maxvals[i] *= F(0.1)                                            # a few confident joints at most
    # frame 2: 12 live slots on a grid of 10 hands far apart (2 are duplicates: 2 free slots), and 5 fresh detections
    two = np.nonzero(frame_index == 2)[0]
    grid = np.array([[80 + 120 * (q % 5), 100 + 200 * (q // 5)] for q in range(10)], float)
    for n, i in enumerate(two):
        preds[i], maxvals[i] = _hand(rng, grid[n % 10], 70.0)
        src[i], lost[i] = 2, 0
    # two slots of frame 0 with the same keypoints: an exact tie of the scores
    zero = np.nonzero((frame_index == 0) & (lost == 0))[0]
    preds[zero[-1]], maxvals[zero[-1]] = preds[zero[0]], maxvals[zero[0]]

    det_boxes, det_frame, det_score = np.zeros((K, 4), F), np.full(K, -1, np.int32), rng.uniform(0.25, 1.0, K).astype(F)
    for d in range(66):                                                    # frame 0: any of the 25 hands, tracked or not, again and again
        h = rng.randint(0, 25)
        c, s = hands[0][h] + rng.uniform(-5, 5, 2), sizes[0][h] * rng.uniform(0.5, 1.0)          # a palm box is smaller than the hand's
        det_boxes[d], det_frame[d] = (c[0] - s / 2, c[1] - s / 2, c[0] + s / 2, c[1] + s / 2), 0
    det_score[[3, 40]] = det_score[[7, 41]]                                # ties
    det_boxes[10, 2] = det_boxes[10, 0]                                    # zero width
    det_boxes[20, 1] = np.nan
    det_score[30] = np.nan
    det_score[50] = 0.1                                                    # under det_min_score
    det_boxes[60, 3] = np.inf
    for n, d in enumerate(range(66, 71)):                                  # frame 2: 5 fresh hands below its grid
        det_boxes[d], det_frame[d] = (40 + 120 * n, 380, 110 + 120 * n, 450), 2
    for d in (71, 72):                                                     # frame 1
        h = 20 + d - 71
        c = hands[1][h]
        det_boxes[d], det_frame[d] = (c[0] - 30, c[1] - 30, c[0] + 30, c[1] + 30), 1
    det_boxes[73], det_frame[73] = (10, 10, 50, 50), N_FRAMES              # entries of no frame
    det_boxes[74], det_frame[74] = (10, 10, 50, 50), -1
    shuffle = rng.permutation(K)                                           # the list is in no order
    return dict(preds=preds, maxvals=maxvals, src_frame=src, frame_index=frame_index, lost=lost, lost_count=count, next_boxes=next_boxes,
                next_rot=next_rot, det_boxes=det_boxes[shuffle], det_frame=det_frame[shuffle], det_score=det_score[shuffle])


def run_host(s, next_rot=True, **options):
    """manage_tracks_host on the scene with OPTIONS (and ``options`` over them), dup_of / seeded starting at SENTINEL."""
    from lighthand_amd.topdown import manage_tracks_host
    sent = np.full(s["preds"].shape[0], SENTINEL, np.int32)
    return manage_tracks_host(s["preds"], s["maxvals"], s["src_frame"], s["frame_index"], N_FRAMES, s["next_boxes"],
                              s["next_rot"] if next_rot else None, s["lost"], s["lost_count"], s["det_boxes"], s["det_frame"], s["det_score"],
                              dup_of=sent, seeded=sent, **dict(OPTIONS, **options))


def outcomes(s, result, max_lost=OPTIONS["max_lost"]):
    """How often each outcome of the rule occurs in ``result`` = manage_tracks_host's tuple on the scene ``s``."""
    nbox, _, lost, count, dup_of, seeded, det_state = result
    member = (s["frame_index"] >= 0) & (s["frame_index"] < N_FRAMES)
    kept = member & (lost == 0)
    suppressed = member & (dup_of >= 0)
    was = np.minimum(s["lost_count"].astype(np.int64) + 1, 2 ** 30)
    expired = member & ~kept & ~suppressed & (s["src_frame"] >= 0) & (was >= max_lost) & (max_lost > 0)
    return dict(kept=int(kept.sum()), suppressed=int(suppressed.sum()), expired=int(expired.sum()), seeded=int((member & (seeded >= 0)).sum()),
                expired_unseeded=int((expired & (seeded < 0)).sum()), **{f"det{v}": int((det_state == v).sum()) for v in (-1, -2, -3, -4)})
