"""The seeded sequences of the motion tests (tests/test_motion_host.py checks that they reach every branch, tests/test_gpu_motion.py holds
the kernels to the host restatements on them): 67 slots -- two workgroups of lh_rois_predict with a ragged tail -- over 12 chained frames."""
import numpy as np

F = np.float32
B, FRAMES, SEED = 67, 12, 20
PREDICT = dict(cutoff=10.0, lead=1.0, max_shift=0.04, coast=2)
BRANCHES = ("empty", "seeded", "emptied", "coasting", "forgotten", "fresh", "clamped", "free", "bad_dt")


def predict_sequence(b=B, frames=FRAMES, seed=SEED):
    """Per frame a dict of lh_rois_predict's inputs: next_boxes fp32 [b][4] of hands that move up to 9 px a frame (the clamp of PREDICT
    binds for the fast ones), lost / src_frame / seeded int32 [b] and dt fp32 [b] with a few bad values."""
    rng = np.random.RandomState(seed)
    centre = rng.uniform(200, 1700, size=(b, 2))
    speed = rng.uniform(-9, 9, size=(b, 2))
    half = rng.uniform(30, 90, size=(b, 2))
    out = []
    for _ in range(frames):
        centre = centre + speed + rng.normal(0, 0.5, size=(b, 2))
        boxes = np.concatenate([centre - half, centre + half], 1).astype(F)
        boxes[rng.uniform(size=b) < 0.05] = 0                             # emptied by track management
        dt = np.full(b, 1.0 / 30.0, F)
        bad = rng.uniform(size=b) < 0.06
        dt[bad] = rng.choice(np.array([0.0, np.nan, np.inf, -0.033], F), size=int(bad.sum()))
        out.append(dict(next_boxes=boxes, lost=(rng.uniform(size=b) < 0.3).astype(np.int32),
                        src_frame=np.where(rng.uniform(size=b) < 0.07, -1, rng.randint(0, 4, size=b)).astype(np.int32),
                        seeded=np.where(rng.uniform(size=b) < 0.06, rng.randint(0, 8, size=b), -1).astype(np.int32), dt=dt))
    return out


def predict_branch(f, state, options, use_seeded=True):
    """Which clause of the rule every slot of frame ``f`` takes from ``state`` (None: nothing seen): an array of BRANCHES names.
    "clamped" / "free": found with a velocity, the limit binding on an axis or on none; "bad_dt": found or lost with a dt that is not
    finite and > 0, after a frame that was seen."""
    b = f["next_boxes"].shape[0]
    seen = np.zeros(b, bool) if state is None else np.asarray(state[2]) != 0
    coasted = np.zeros(b, np.int32) if state is None else np.asarray(state[3])
    box = f["next_boxes"]
    with np.errstate(all="ignore"):
        okdt = (f["dt"] > 0) & np.isfinite(f["dt"])
    name = np.full(b, "", dtype=object)
    pos = (box[:, 2] - box[:, 0] > 0) & (box[:, 3] - box[:, 1] > 0)
    for i in range(b):
        if f["src_frame"][i] < 0:
            name[i] = "empty"
        elif use_seeded and f["seeded"][i] >= 0:
            name[i] = "seeded"
        elif not pos[i]:
            name[i] = "emptied"
        elif seen[i] and not okdt[i]:
            name[i] = "bad_dt"
        elif f["lost"][i]:
            name[i] = "coasting" if seen[i] and coasted[i] < options["coast"] else "forgotten"
        elif not seen[i]:
            name[i] = "fresh"
        else:
            name[i] = "found"                                             # split into clamped / free by the caller, from the result
    return name


def run_predict_host(seq, options, use_seeded=True, dtype=np.float32):
    """The chained restatement -> per frame (boxes, state, branch names)."""
    from lighthand_amd.topdown import rois_predict_host
    state, out = None, []
    for f in seq:
        name = predict_branch(f, state, options, use_seeded)
        boxes, state = rois_predict_host(f["next_boxes"], f["lost"], f["src_frame"], f["seeded"] if use_seeded else None, f["dt"], state,
                                         dtype=dtype, **options)
        with np.errstate(all="ignore"):
            want = np.abs((dtype(options["lead"]) * state[1]) * f["dt"][:, None].astype(dtype))       # the shift the new velocity asks for
        lim = dtype(options["max_shift"]) * np.fmax(f["next_boxes"][:, 2] - f["next_boxes"][:, 0], f["next_boxes"][:, 3] - f["next_boxes"][:, 1])
        found = name == "found"
        name[found] = np.where((want[found] > lim[found, None].astype(dtype)).any(1), "clamped", "free")
        out.append((boxes, state, name))
    return out


def gated_sequence(j, b=B, frames=FRAMES, seed=SEED + 1):
    """Per frame a dict of lh_one_euro_gated's inputs: x fp32 [b][j][2] (a noisy moving constellation), maxvals fp32 [b][j] around the
    gate of 0.5, next_boxes fp32 [b][4] (a few smaller than a pixel), src_frame / lost int32 [b], dt fp32 [b] with a few bad values."""
    rng = np.random.RandomState(seed + j)
    base = rng.uniform(100, 1800, size=(b, j, 2))
    drift = rng.uniform(-6, 6, size=(b, 1, 2))
    out = []
    for t in range(frames):
        x = (base + t * drift + rng.normal(0, 2, size=(b, j, 2))).astype(F)
        lo = rng.uniform(0, 900, size=(b, 2))
        side = np.where(rng.uniform(size=(b, 1)) < 0.1, rng.uniform(0.1, 1.5, size=(b, 2)), rng.uniform(40, 300, size=(b, 2)))
        dt = rng.uniform(0.01, 0.05, size=b).astype(F)
        bad = rng.uniform(size=b) < 0.06
        dt[bad] = rng.choice(np.array([0.0, np.nan, np.inf, -0.033], F), size=int(bad.sum()))
        out.append(dict(x=x, maxvals=rng.uniform(0.2, 1.0, size=(b, j)).astype(F), next_boxes=np.concatenate([lo, lo + side], 1).astype(F),
                        src_frame=np.where(rng.uniform(size=b) < 0.06, -1, 0).astype(np.int32), lost=(rng.uniform(size=b) < 0.12).astype(np.int32),
                        dt=dt))
    return out
