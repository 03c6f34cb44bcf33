"""Seeded scenes for the skeleton overlay (lh_draw_hands / topdown.draw_hands_host), shared by tests/test_overlay_host.py (CPU: closed
forms of the restatement and the guard that the scenes reach every clause of the rule) and tests/test_gpu_overlay.py (the kernel bit
for bit against the restatement).  A scene is a dict of numpy arrays and options; ``frames_of`` encodes its RGB frames in a format."""
import numpy as np

F = np.float32
CROP = (64, 64)
FORMATS = ("rgb", "nv12", "nv21", "yuv420p", "p010")
TREE5 = dict(parents=np.array([-1, 0, 1, 0, 3], np.int32), groups=np.array([0, 1, 1, 2, 2], np.int32),
             palette_rgb=((250, 250, 250), (255, 60, 0), (0, 90, 255), (0, 255, 0), (255, 0, 0)))


def _hand(rng, centre, size, j):
    """j joints scattered about ``centre`` within ``size`` pixels, joint 0 near the middle."""
    p = centre + rng.uniform(-0.5, 0.5, size=(j, 2)) * size
    p[0] = centre + rng.uniform(-0.1, 0.1, size=2) * size
    return p


def _matrix(rng, centre, size, angle, mirror):
    """The crop matrix of a CROP-sized ROI of ``size`` frame pixels about ``centre``, turned by ``angle`` and mirrored or not."""
    a = size / CROP[1]
    c, s, g = a * np.cos(angle), a * np.sin(angle), -1.0 if mirror else 1.0
    m0, m1, m3, m4 = g * c, -s, g * s, c
    hx, hy = (CROP[1] - 1) * 0.5, (CROP[0] - 1) * 0.5
    return [m0, m1, centre[0] - (m0 * hx + m1 * hy), m3, m4, centre[1] - (m3 * hx + m4 * hy)]


def scene(which):
    """"small": 3 frames of 64 x 80, 12 slots, j = 21.  "large": 4 frames of 96 x 128 (the 4:2:0 layouts pitched, with a pitch wider
    than the width), 16 slots, j = 21, by_size > 0 and opacity < 1.  "tree5": 2 frames of 64 x 80, 8 slots of a custom 5-joint tree.
    Every scene holds: two slots overlapping on one frame, a slot half outside and one wholly outside the frame, a lost slot, an empty
    slot, joints under the gate, a zero-length bone, a NaN keypoint, an oriented and mirrored matrix."""
    n, hs, ws, b, j = dict(small=(3, 64, 80, 12, 21), large=(4, 96, 128, 16, 21), tree5=(2, 64, 80, 8, 5))[which]
    rng = np.random.RandomState(dict(small=5, large=6, tree5=7)[which])
    src = (np.arange(b) % n).astype(np.int32)
    centres = np.stack([rng.uniform(0.25, 0.75, b) * ws, rng.uniform(0.25, 0.75, b) * hs], 1)
    sizes = rng.uniform(18, 40, b)
    src[1] = src[0]
    centres[1], sizes[1] = centres[0] + np.array([7.0, -5.0]), sizes[0]     # slot 1 is on slot 0's frame, on top of it
    centres[2] = np.array([ws - 2.0, hs * 0.5])                             # half outside
    centres[3] = np.array([-90.0, -70.0])                                   # wholly outside
    preds = np.stack([_hand(rng, centres[i], sizes[i], j) for i in range(b)]).astype(F)
    maxvals = rng.uniform(0.3, 1.0, size=(b, j)).astype(F)
    maxvals[:, 2::5] = rng.uniform(0.0, 0.09, size=maxvals[:, 2::5].shape)  # joints under the gate (min_score 0.1)
    lost = np.zeros(b, np.int32)
    lost[4] = 1
    src[5] = -1                                                             # an empty slot
    src[6] = n + 3                                                          # a frame that does not exist
    preds[0, 4] = preds[0, 3]                                               # a zero-length bone (3 -> 4 in both trees)
    maxvals[0, 3] = maxvals[0, 4] = 0.9
    preds[7 % b, 1, 0] = np.nan                                             # a NaN keypoint: its joint and its two bones are skipped
    maxvals[7 % b, 1] = 0.9
    preds[0, 0] = (11.0, 13.0)                                              # a joint on an integer pixel
    mat = np.array([_matrix(rng, centres[i], sizes[i] * 1.3, rng.uniform(-np.pi, np.pi), i % 2 == 1) for i in range(b)], F)
    mat[0] = _matrix(rng, centres[0], sizes[0] * 1.3, 0.0, False)           # one upright outline
    half = (sizes * 0.65)[:, None]
    boxes = np.concatenate([centres - half, centres + half], 1).astype(F)
    s = dict(name=which, n=n, hs=hs, ws=ws, b=b, j=j, preds=preds, maxvals=maxvals, src_frame=src, lost=lost, mat=mat, boxes=boxes,
             frames_rgb=rng.randint(0, 256, size=(n, hs, ws, 3)).astype(np.uint8), pitched=which == "large",
             options=dict(min_score=0.1, line_radius=1.0, joint_radius=2.5, by_size=0.0, opacity=1.0, draw_roi=True))
    if which == "large":
        s["options"].update(by_size=0.03, opacity=0.75, line_radius=0.5)
    if which == "tree5":
        s["tree"] = TREE5
    return s


def layout_of(s, fmt):
    from lighthand_amd import topdown
    if fmt == "rgb":
        return None
    if not s["pitched"]:
        return topdown.yuv420_layout(fmt, s["hs"], s["ws"])
    sb = 2 if fmt == "p010" else 1
    pitch = (s["ws"] + 24) * sb                                             # wider than the width
    return topdown.yuv420_layout(fmt, s["hs"], s["ws"], pitch, s["hs"] + 6, pitch // 2 + 8 if fmt == "yuv420p" else pitch + 16 * sb)


def frames_of(s, fmt):
    """The scene's frames as ``fmt`` -> (uint8 [n][...], layout).  The padding bytes and p010's low six bits are filled with seeded
    noise, so a test sees whether they are kept."""
    from lighthand_amd import topdown
    if fmt == "rgb":
        return s["frames_rgb"].copy(), None
    L = layout_of(s, fmt)
    enc = np.asarray(topdown.rgb_to_yuv420_host(s["frames_rgb"], fmt, layout=L)).reshape(s["n"], -1).copy()
    rng = np.random.RandomState(17)
    noise = rng.randint(0, 256, size=enc.shape).astype(np.uint8)
    sample = np.zeros(enc.shape[1], bool)
    y, x = np.meshgrid(np.arange(s["hs"]), np.arange(s["ws"]), indexing="ij")
    cy, cx = np.meshgrid(np.arange(s["hs"] // 2), np.arange(s["ws"] // 2), indexing="ij")
    for byte in range(L.sample_bytes):
        for off in (y * L.pitch + x * L.sample_bytes, L.cb_offset + cy * L.c_pitch + cx * L.c_step, L.cr_offset + cy * L.c_pitch + cx * L.c_step):
            sample[off + byte] = True
    enc[:, ~sample] = noise[:, ~sample]
    if L.sample_bytes == 2:                                                 # the low six bits of every 16-bit sample (little-endian: the even byte)
        low = sample.copy()
        for off in (y * L.pitch + x * 2, L.cb_offset + cy * L.c_pitch + cx * L.c_step, L.cr_offset + cy * L.c_pitch + cx * L.c_step):
            low[off + 1] = False
        enc[:, low] |= noise[:, low] & 63
    return enc, L


def host_kwargs(s, fmt, layout):
    """The keyword arguments of topdown.draw_hands_host / draw_hands for scene ``s`` in ``fmt`` (without the frames and the per-slot
    arrays)."""
    from lighthand_amd import topdown
    kw = dict(crop_size=CROP, frame_format=fmt, frame_size=(s["hs"], s["ws"]), layout=layout, **s["options"])
    if "tree" in s:
        t = s["tree"]
        kw.update(parents=t["parents"], groups=t["groups"], palette=topdown.overlay_palette(t["palette_rgb"], fmt))
    return kw


def run_host(s, fmt, frames=None, layout=None, dtype=np.float32, **over):
    from lighthand_amd import topdown
    if frames is None:
        frames, layout = frames_of(s, fmt)
    kw = host_kwargs(s, fmt, layout)
    kw.update(over)
    return topdown.draw_hands_host(frames, s["preds"], s["maxvals"], s["src_frame"], lost=s["lost"], crop_mat=s["mat"], boxes=s["boxes"], dtype=dtype,
                                   **kw)
