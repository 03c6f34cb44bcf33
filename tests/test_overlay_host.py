"""CPU: the skeleton overlay's rule in numpy (topdown.draw_hands_host) against closed forms that no kernel enters, the palette
conversion, every refusal, and the guard that the seeded scenes of tests/overlay_data.py reach every clause of the rule (the GPU tests
hold lh_draw_hands to the restatement on those scenes)."""
import numpy as np
import pytest

import overlay_data as D
from lighthand_amd import topdown

F = np.float32
WHITE = np.full((8, 3), 255.0, F)


def _one(frames, points, maxvals=None, **kw):
    """One slot on frame 0 with the default tree, all-white palette unless given."""
    p = np.full((1, 21, 2), np.nan, F)
    mv = np.zeros((1, 21), F)
    for i, (xy, v) in enumerate(zip(points, maxvals or [1.0] * len(points))):
        p[0, i], mv[0, i] = xy, v
    kw.setdefault("palette", WHITE)
    return topdown.draw_hands_host(frames, p, mv, [0], **kw)


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("r", [0.75, 2.5, 3.25])
def test_a_joint_is_an_antialiased_disc_about_its_pixel(r):
    out = _one(np.zeros((1, 64, 80, 3), np.uint8), [(40, 30)], joint_radius=r)[0]
    assert (out[..., 0] == out[..., 1]).all() and (out[..., 0] == out[..., 2]).all()
    y, x = np.mgrid[0:64, 0:80]
    d = np.sqrt((x - 40.0) ** 2 + (y - 30.0) ** 2)
    g = out[..., 0].astype(np.int64)
    assert (g[d <= r - 0.5] == 255).all() and (g[d >= r + 0.5] == 0).all()
    mid = (d > r - 0.5) & (d < r + 0.5)
    want = np.floor(F(255) * (F(r + 0.5) - np.sqrt(((x - 40) ** 2 + (y - 30) ** 2).astype(F))) + F(0.5))
    assert mid.sum() >= 4 and np.array_equal(g[mid], want[mid].astype(np.int64))
    assert (g * x).sum() / g.sum() == 40.0 and (g * y).sum() / g.sum() == 30.0           # the centroid is on the keypoint


def test_a_horizontal_bone_has_the_expected_row_profile():
    # wrist (10, 20) -> joint 1 (50, 20), line radius 1.5; the joints' own discs are no wider (radius 1.5 as well)
    out = _one(np.zeros((1, 40, 64, 3), np.uint8), [(10, 20), (50, 20)], line_radius=1.5, joint_radius=1.5)[0][..., 0]
    # |dy| = 0, 1: fully covered (1.5 + 0.5 - 1 = 1); |dy| = 2: coverage 0; between the end points every column is the same
    assert out[18, 30] == 0 and out[19, 30] == 255 and out[20, 30] == 255 and out[21, 30] == 255 and out[22, 30] == 0
    assert (out[:, 10:51] == out[:, 30:31]).all()
    # beyond an end point the cap is the disc: at (52, 20) d = 2 -> 0, at (51, 20) d = 1 -> 255
    assert out[20, 51] == 255 and out[20, 52] == 0 and out[20, 9] == 255 and out[20, 8] == 0
    # a fractional radius: 255 * (1.25 + 0.5 - 1) at |dy| = 1
    out = _one(np.zeros((1, 40, 64, 3), np.uint8), [(10, 20), (50, 20)], line_radius=1.25, joint_radius=0.0)[0][..., 0]
    assert out[19, 30] == int(np.floor(255 * 0.75 + 0.5)) and out[20, 30] == 255 and out[18, 30] == 0


def test_opacity_blends_towards_the_colour():
    grey = np.full((1, 32, 32, 3), 100, np.uint8)
    pal = np.tile(F([[200, 50, 100]]), (8, 1))
    out = _one(grey, [(16, 16)], joint_radius=4.0, opacity=0.5, palette=pal)[0]
    assert out[16, 16].tolist() == [150, 75, 100] and out[16, 18].tolist() == [150, 75, 100]        # 100 + 0.5 * (colour - 100)
    assert out[2, 2].tolist() == [100, 100, 100]
    # three primitives over one pixel composite in order: the (zero-length) bone 0 -> 1, then the two joints on top of it
    out = _one(grey, [(16, 16), (16, 16)], line_radius=4.0, joint_radius=4.0, opacity=0.5, palette=pal)[0]
    assert out[16, 16].tolist() == [188, 56, 100]                   # 100 -> 150 -> 175 -> 187.5; 100 -> 75 -> 62.5 -> 56.25
    out = _one(grey, [(16, 16)], opacity=0.0, palette=pal)[0]
    assert np.array_equal(out, grey[0])


@pytest.mark.parametrize("fmt", ["nv12", "yuv420p", "p010"])
def test_chroma_coverage_is_the_mean_of_the_luma_block(fmt):
    hs, ws = 32, 48
    L = topdown.yuv420_layout(fmt, hs, ws)
    scale = 4 if fmt == "p010" else 1
    frames = topdown.rgb_to_yuv420_host(np.zeros((1, hs, ws, 3), np.uint8), fmt, range="full").reshape(1, -1)
    pal = np.tile(F([[200, 60, 240]]) * scale, (8, 1))
    # a joint of radius 0.5 on (10, 10): coverage 1 on the pixel, 0 on its 2 x 2 block's other three -> chroma coverage 1/4
    out = _one(frames, [(10, 10)], joint_radius=0.5, palette=pal, frame_format=fmt, frame_size=(hs, ws))[0]

    def tex(off):
        return int(out[off]) if L.sample_bytes == 1 else (int(out[off]) | int(out[off + 1]) << 8) >> 6
    assert tex(10 * L.pitch + 10 * L.sample_bytes) == 200 * scale and tex(10 * L.pitch + 11 * L.sample_bytes) == 0
    cb0, cr0 = 128 * scale, 128 * scale
    at = 5 * L.c_pitch + 5 * L.c_step
    assert tex(L.cb_offset + at) == int(np.floor(cb0 + 0.25 * (60 * scale - cb0) + 0.5))
    assert tex(L.cr_offset + at) == int(np.floor(cr0 + 0.25 * (240 * scale - cr0) + 0.5))
    assert tex(L.cb_offset + at + L.c_step) == cb0                  # the next chroma texel is untouched
    # radius 3 covers the whole aligned block at (10..11, 10..11): chroma takes the colour itself
    out = _one(frames, [(10.5, 10.5)], joint_radius=3.0, palette=pal, frame_format=fmt, frame_size=(hs, ws))[0]
    assert tex(L.cb_offset + at) == 60 * scale and tex(L.cr_offset + at) == 240 * scale


def test_p010_keeps_the_low_bits_of_untouched_texels():
    s = D.scene("small")
    frames, L = D.frames_of(s, "p010")
    out = D.run_host(s, "p010", frames, L)
    u_in, u_out = frames.reshape(s["n"], -1, 2), out.reshape(s["n"], -1, 2)
    changed = (u_in != u_out).any(2)
    assert changed.sum() > 500 and (u_in[~changed] == u_out[~changed]).all() and (u_in[..., 0] & 63).any()
    assert ((u_out[changed][:, 0] & 63) == 0).all()                 # what was drawn is a multiple of 64


def test_slots_composite_in_index_order():
    s = D.scene("small")
    kw = dict(D.host_kwargs(s, "rgb", None), opacity=0.6)
    args = lambda idx: dict(lost=s["lost"][idx], crop_mat=s["mat"][idx], boxes=s["boxes"][idx])
    both = topdown.draw_hands_host(s["frames_rgb"], s["preds"][:2], s["maxvals"][:2], s["src_frame"][:2], **args(slice(0, 2)), **kw)
    first = topdown.draw_hands_host(s["frames_rgb"], s["preds"][:1], s["maxvals"][:1], s["src_frame"][:1], **args(slice(0, 1)), **kw)
    then = topdown.draw_hands_host(first, s["preds"][1:2], s["maxvals"][1:2], s["src_frame"][1:2], **args(slice(1, 2)), **kw)
    # one launch composites in floats and rounds once, two launches round in between: within one code value of each other, and the
    # same bytes where slot 1 draws nothing
    diff = np.abs(both.astype(int) - then.astype(int))
    assert diff.max() <= 1 and np.array_equal(both[(then == first).all(3)], first[(then == first).all(3)])
    rev = [1, 0]
    other = topdown.draw_hands_host(s["frames_rgb"], s["preds"][rev], s["maxvals"][rev], s["src_frame"][rev], **args(rev), **kw)
    assert np.abs(both.astype(int) - other.astype(int)).max() > 20          # the reverse order is another picture


def test_fp64_agrees_to_a_code_value():
    s = D.scene("large")
    a, b = D.run_host(s, "rgb").astype(int), D.run_host(s, "rgb", dtype=np.float64).astype(int)
    assert np.abs(a - b).max() <= 1 and (a != b).mean() < 1e-3


# ------------------------------------------------------------------------------------------------ the scenes reach every clause
@pytest.mark.parametrize("which", ["small", "large", "tree5"])
def test_the_scenes_reach_every_clause(which):
    s = D.scene(which)
    n, hs, ws, b = s["n"], s["hs"], s["ws"], s["b"]
    src, lost, mv, p = s["src_frame"], s["lost"], s["maxvals"], s["preds"]
    live = (src >= 0) & (src < n)
    assert src[0] == src[1] and live[0] and live[1] and lost[0] == 0 and lost[1] == 0
    base = s["frames_rgb"]

    def drawn(idx, **over):
        keep = np.where(np.isin(np.arange(b), idx), src, -1)
        out = D.run_host(dict(s, src_frame=keep), "rgb", **over)
        return (out != base).any(3)
    d0, d1 = drawn([0]), drawn([1])
    assert (d0 & d1).sum() > 20                                     # two slots overlapping on one frame
    d2 = drawn([2])
    assert d2.sum() > 20 and d2[:, :, -1].any() and (p[2, :, 0] > ws).any()          # half outside: drawn up to the edge, joints beyond it
    assert drawn([3]).sum() == 0 and live[3]                        # wholly outside
    assert lost[4] == 1 and live[4] and np.array_equal(drawn([4]), drawn([4], min_score=2.0)) and drawn([4]).sum() > 0       # outline alone
    assert src[5] < 0 and src[6] >= n and drawn([5, 6]).sum() == 0  # an empty slot, a frame that does not exist
    assert (mv[live] < 0.1).any() and (mv[live] >= 0.1).any()       # joints under the gate
    assert np.array_equal(p[0, 3], p[0, 4]) and mv[0, 3] >= 0.1 and mv[0, 4] >= 0.1   # a zero-length bone
    assert np.isnan(p[7 % b]).sum() == 1 and live[7 % b] and drawn([7 % b]).sum() > 0  # a NaN keypoint
    m = s["mat"]
    det = m[:, 0] * m[:, 4] - m[:, 1] * m[:, 3]
    assert (det[live] < 0).any() and (np.abs(m[live, 1]) > 0.05).any()                # oriented, mirrored ROIs
    assert (drawn([0]) != drawn([0], draw_roi=False)).any()
    if which == "large":
        assert s["options"]["by_size"] > 0 and s["options"]["opacity"] < 1 and s["pitched"]
        assert (drawn([0]) != drawn([0], by_size=0.0)).any()
        L = D.layout_of(s, "nv12")
        assert L.pitch > ws and D.layout_of(s, "p010").pitch > 2 * ws and D.layout_of(s, "yuv420p").c_pitch > ws // 2
    # an unbound surface: its slots draw nothing, the others are drawn as ever
    frames = list(base)
    frames[0] = None
    out = D.run_host(s, "rgb", frames=frames)
    full = D.run_host(s, "rgb")
    assert out[0] is None and all(np.array_equal(out[f].reshape(hs, ws, 3), full[f]) for f in range(1, n))


# ------------------------------------------------------------------------------------------------ palette, defaults, refusals
def test_palette_conversion_round_trips_grey():
    for yuv in (("bt709", "limited"), ("bt601", "full")):
        for fmt in D.FORMATS[1:]:
            scale = 4.0 if fmt == "p010" else 1.0
            pal = topdown.overlay_palette([(v, v, v) for v in (0, 64, 255)], fmt, yuv)
            assert pal.dtype == np.float32 and pal.shape == (3, 3)
            lo, hi = (16.0, 235.0) if yuv[1] == "limited" else (0.0, 255.75 if fmt == "p010" else 255.0)      # 1023 is 255.75 on the 8-bit scale
            assert np.allclose(pal[:, 1:], 128 * scale, atol=1e-3) and np.allclose(pal[:, 0], scale * (lo + np.array([0, 64, 255]) * (hi - lo) / 255), atol=1e-3)
            k = topdown.yuv_matrix(*yuv, bits=10 if fmt == "p010" else 8).astype(np.float64)
            back = (pal / scale - k[9:]) @ k[:9].reshape(3, 3).T
            assert np.allclose(back, [[0] * 3, [64] * 3, [255] * 3], atol=2e-3 * 255)
    assert np.array_equal(topdown.overlay_palette([(1, 2, 3)], "rgb"), F([[1, 2, 3]]))
    frames = topdown.rgb_to_yuv420_host(np.full((1, 4, 4, 3), 200, np.uint8), "nv12")
    assert abs(float(topdown.overlay_palette([(200, 200, 200)], "nv12")[0, 0]) - int(np.asarray(frames).reshape(-1)[0])) <= 0.5


def test_defaults():
    assert len(topdown.HAND_PARENTS) == 21 and len(topdown.HAND_GROUPS) == 21
    assert list(topdown.HAND_PARENTS) == [-1, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15, 0, 17, 18, 19]
    assert all(topdown.HAND_GROUPS[i] == topdown.HAND_GROUPS[p] or p == 0 for i, p in enumerate(topdown.HAND_PARENTS) if p >= 0)
    assert topdown.OVERLAY_DEFAULTS["line_radius"] == 1.0 and topdown.OVERLAY_DEFAULTS["joint_radius"] == 2.5
    assert topdown.OVERLAY_DEFAULTS["by_size"] == 0.0 and topdown.OVERLAY_DEFAULTS["opacity"] == 1.0 and topdown.OVERLAY_DEFAULTS["draw_roi"] is True
    assert topdown.OVERLAY_DEFAULTS["source"] == "raw" and topdown.OVERLAY_DEFAULTS["target"] == "inplace"


def test_refusals():
    from lighthand_amd.overlay import resolve_overlay
    fr = np.zeros((1, 16, 16, 3), np.uint8)
    p, mv = np.zeros((1, 21, 2), F), np.ones((1, 21), F)
    for bad in (dict(opacity=1.5), dict(opacity=-0.1), dict(line_radius=-1.0), dict(joint_radius=float("nan")), dict(by_size=-0.5),
                dict(min_score=float("inf")), dict(by_size=0.1), dict(parents=[0] * 20), dict(groups=[0] * 22), dict(parents=[21] * 21),
                dict(groups=[6] * 21), dict(palette=np.zeros((2, 3), F)), dict(palette=np.full((8, 3), np.nan, F)),
                dict(crop_mat=np.zeros((1, 6), F)), dict(frame_format="bgr"), dict(frame_format="nv12"),
                dict(frame_format="nv12", frame_size=(15, 16))):
        with pytest.raises(ValueError):
            topdown.draw_hands_host(fr, p, mv, [0], **bad)
    with pytest.raises(ValueError):
        topdown.draw_hands_host(fr, np.zeros((1, 5, 2), F), np.ones((1, 5), F), [0])       # no default tree for 5 joints
    with pytest.raises(ValueError):
        topdown.overlay_palette([(1, 2)], "rgb")
    with pytest.raises(ValueError):
        topdown.overlay_palette([(1, 2, 3)], "bgr")
    # the step's keyword
    ok = resolve_overlay(True, 21, 0.25, "rgb", ("bt709", "limited"), None)
    assert ok["min_score"] == 0.25 and ok["parents"].dtype == np.int32 and ok["palette"].shape == (8, 3) and ok["target"] == "inplace"
    assert resolve_overlay(None, 21, 0.1, "rgb", ("bt709", "limited"), None) is None
    assert resolve_overlay(dict(min_score=0.5, source="smooth"), 21, 0.1, "nv12", ("bt709", "limited"), (1.0, 0.1, 1.0))["min_score"] == 0.5
    for bad in (dict(colour=1), dict(source="smooth"), dict(source="filtered"), dict(target="copy"), dict(opacity=2), dict(parents=[0] * 3),
                dict(groups=[9] * 21), "yes", 1):
        with pytest.raises(ValueError):
            resolve_overlay(bad, 21, 0.1, "rgb", ("bt709", "limited"), None)
    with pytest.raises(ValueError):
        resolve_overlay(True, 17, 0.1, "rgb", ("bt709", "limited"), None)
