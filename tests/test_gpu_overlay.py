"""GPU: the skeleton overlay -- lh_draw_hands bit for bit against topdown.draw_hands_host on every byte of every frame (untouched texels
and padding included) on the seeded scenes of tests/overlay_data.py (tests/test_overlay_host.py guards that they reach every clause
and holds the restatement to closed forms), for every frame format, from a buffer and through a surface table; and
ManagedInferStep / ManagedInferPipeline(overlay=...) on the fixtures of tests/test_gpu_tracks_manage.py: ResNet-18, 64 x 64 crops, 4
frames of 96 x 128 and 5 slots."""
import ctypes as C

import numpy as np
import pytest
import torch

import overlay_data as D
from test_gpu_topdown import _model
from test_gpu_tracks_manage import APART, B, BOXES, FH, FW, NF, SHARED, SIZE, _dev, _options, _Recorder, _same, _snap, _step_frames

pytestmark = pytest.mark.gpu

F = np.float32
SNAP = ("preds", "maxvals", "next_boxes", "lost", "smooth_preds", "boxes")


def _device_args(s):
    return dict(preds=_dev(s["preds"], F), maxvals=_dev(s["maxvals"], F), src_frame=_dev(s["src_frame"], np.int32), lost=_dev(s["lost"], np.int32),
                crop_mat=_dev(s["mat"], F), boxes=_dev(s["boxes"], F))


def _draw(s, fmt, frames, layout, table, **over):
    """topdown.draw_hands on the scene: from one buffer, or through a surface table whose frame 0 is unbound with ``table`` -> the
    frames as numpy (a list with None for the unbound one)."""
    from lighthand_amd import topdown
    a = _device_args(s)
    kw = D.host_kwargs(s, fmt, layout)
    kw.update(over)
    if table:
        dev = [None] + [torch.from_numpy(f.copy()).cuda().reshape(-1) for f in frames[1:]]
        topdown.draw_hands(dev, a.pop("preds"), a.pop("maxvals"), a.pop("src_frame"), **a, **kw)
        torch.cuda.synchronize()
        return [None if t is None else t.cpu().numpy() for t in dev]
    dev = torch.from_numpy(frames.copy()).cuda()
    topdown.draw_hands(dev, a.pop("preds"), a.pop("maxvals"), a.pop("src_frame"), **a, **kw)
    torch.cuda.synchronize()
    return dev.cpu().numpy()


def _assert_same_bytes(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, what
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[:8].tolist()}: got {got[bad[:8]].tolist()}, want {want[bad[:8]].tolist()}"


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("fmt", D.FORMATS)
@pytest.mark.parametrize("which", ["small", "large", "tree5"])
def test_kernel_is_bit_equal_to_the_host_restatement(which, fmt):
    s = D.scene(which)
    frames, L = D.frames_of(s, fmt)
    want = D.run_host(s, fmt, frames, L)
    changed = int((np.asarray(want) != frames).sum())
    print(f"{which} {fmt}: {changed} of {frames.size} bytes drawn")
    assert changed > 300
    got = _draw(s, fmt, frames, L, table=False)
    _assert_same_bytes(got, want, f"{which} {fmt} buffer")
    _assert_same_bytes(_draw(s, fmt, frames, L, table=False), got, f"{which} {fmt} second launch")       # a replay is bit-reproducible
    # through a surface table, frame 0 unbound: its slots are skipped, the other frames are the buffer's
    want_t = D.run_host(s, fmt, [None] + list(frames[1:]), L)
    got_t = _draw(s, fmt, frames, L, table=True)
    assert got_t[0] is None and want_t[0] is None
    for f in range(1, s["n"]):
        _assert_same_bytes(got_t[f], want_t[f], f"{which} {fmt} table frame {f}")
        _assert_same_bytes(got_t[f], np.asarray(want[f]), f"{which} {fmt} table frame {f} against the buffer's")


def test_kernel_options_and_null_pointers():
    """No lost array, no matrix, no boxes; draw_roi off; opacity 0 writes nothing; many slots on one frame (more than a wave of them)."""
    from lighthand_amd import topdown
    s = D.scene("small")
    frames = s["frames_rgb"]
    a = _device_args(s)
    dev = torch.from_numpy(frames.copy()).cuda()
    topdown.draw_hands(dev, a["preds"], a["maxvals"], a["src_frame"])
    want = topdown.draw_hands_host(frames, s["preds"], s["maxvals"], s["src_frame"])
    _assert_same_bytes(dev.cpu().numpy(), want, "no optional input")
    for over in (dict(draw_roi=False), dict(opacity=0.0), dict(min_score=0.95, joint_radius=0.0, line_radius=0.0), dict(by_size=0.2)):
        want = D.run_host(s, "rgb", frames, None, **over)
        _assert_same_bytes(_draw(s, "rgb", frames, None, table=False, **over), want, str(over))
        if over.get("opacity") == 0.0:
            assert np.array_equal(want, frames)
    rng = np.random.RandomState(3)
    b = 150
    crowd = dict(s, b=b, preds=(rng.uniform(8, 72, size=(b, 1, 2)) + rng.uniform(-9, 9, size=(b, 21, 2))).astype(F),
                 maxvals=rng.uniform(0, 1, size=(b, 21)).astype(F), src_frame=(rng.randint(0, 3, size=b) * (np.arange(b) % 7 != 0)).astype(np.int32),
                 lost=(np.arange(b) % 5 == 0).astype(np.int32), mat=np.tile(s["mat"], (13, 1))[:b], boxes=np.tile(s["boxes"], (13, 1))[:b])
    for fmt in ("rgb", "nv12"):
        fr, L = D.frames_of(crowd, fmt)
        _assert_same_bytes(_draw(crowd, fmt, fr, L, table=False, opacity=0.5), D.run_host(crowd, fmt, fr, L, opacity=0.5), f"crowd {fmt}")


def test_argument_refusals_set_the_error_text():
    from lighthand_amd import _lib, topdown
    lib = _lib.load()
    s = D.scene("small")
    a = _device_args(s)
    frames = torch.from_numpy(s["frames_rgb"].copy()).cuda()
    par, grp, pal = (torch.from_numpy(t).cuda() for t in topdown.overlay_tables(21))
    desc = topdown.frames_layout_struct(topdown.frame_layout_of("rgb", s["hs"], s["ws"]), ("bt709", "limited"), "left")
    good = dict(frames=frames.data_ptr(), frame_stride=frames.stride(0), table=None, layout=C.byref(desc), n_frames=s["n"], hs=s["hs"], ws=s["ws"],
                preds=a["preds"].data_ptr(), maxvals=a["maxvals"].data_ptr(), src_frame=a["src_frame"].data_ptr(), lost=a["lost"].data_ptr(),
                mat=a["crop_mat"].data_ptr(), boxes=a["boxes"].data_ptr(), b=s["b"], j=21, crop_h=64, crop_w=64, parents=par.data_ptr(),
                group=grp.data_ptr(), palette=pal.data_ptr(), n_groups=6, min_score=0.1, line_radius=1.0, joint_radius=2.5, by_size=0.0, opacity=1.0,
                draw_roi=1, stream=None)
    table = torch.zeros(s["n"], dtype=torch.int64, device="cuda")
    nv12 = topdown.frames_layout_struct(topdown.yuv420_layout("nv12", s["hs"], s["ws"])._replace(pitch=s["ws"] - 2), ("bt709", "limited"), "left")
    for over, word in ((dict(preds=None), b"null"), (dict(palette=None), b"null"), (dict(frames=None), b"no frame source"),
                       (dict(table=table.data_ptr()), b"two frame sources"), (dict(b=0), b"slots"), (dict(b=1025), b"slots"), (dict(j=0), b"> 0"),
                       (dict(n_groups=0), b"> 0"), (dict(crop_w=0), b"> 0"), (dict(line_radius=-1.0), b"finite and >= 0"),
                       (dict(joint_radius=float("inf")), b"finite and >= 0"), (dict(by_size=float("nan")), b"finite and >= 0"),
                       (dict(min_score=float("nan")), b"min_score"), (dict(opacity=1.5), b"opacity"), (dict(opacity=float("nan")), b"opacity"),
                       (dict(by_size=0.5, boxes=None), b"boxes"), (dict(frame_stride=100), b"frame_stride"), (dict(layout=C.byref(nv12)), b"pitch"),
                       (dict(preds=frames.data_ptr()), b"distinct"), (dict(palette=a["preds"].data_ptr()), b"distinct")):
        rc = lib.lh_draw_hands(*dict(good, **over).values())
        assert rc == -1 and word in lib.lh_last_error(), (over, lib.lh_last_error())
    assert lib.lh_draw_hands(*good.values()) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(frames.cpu().numpy(), s["frames_rgb"])
    with pytest.raises(ValueError):
        topdown.draw_hands(frames, a["preds"], a["maxvals"], a["src_frame"], opacity=2.0)
    with pytest.raises(_lib.LightHandError):
        topdown.draw_hands(frames, a["preds"].cpu(), a["maxvals"], a["src_frame"])


# ------------------------------------------------------------------------------------------------ 2. the captured step
def _first(index=APART):
    return dict(frames=_step_frames(), boxes=_dev(BOXES, F), frame_index=_dev(index, np.int32))


def _host_of(step, before, source="preds", **over):
    """draw_hands_host of ``before`` and the step's own outputs, under the step's resolved options."""
    from lighthand_amd import topdown
    o = dict(step.overlay)
    o.pop("source"), o.pop("target")
    o.update(frame_size=(FH, FW))
    o.update(over)
    torch.cuda.synchronize()
    return topdown.draw_hands_host(before, getattr(step, source).cpu().numpy(), step.maxvals.cpu().numpy(), step.plan.src_frame.cpu().numpy(),
                                   lost=None if step.lost is None else step.lost.cpu().numpy(), crop_mat=step.plan.crop_mat.cpu().numpy(),
                                   crop_size=(SIZE, SIZE), boxes=step.boxes.cpu().numpy(), **o)


def test_overlay_is_the_last_launch_and_draws_what_the_host_draws(monkeypatch):
    from lighthand_amd.runtime import ManagedInferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    options = dict(_options(model, True), smooth=(1.0, 0.007))
    clean = _step_frames().cpu().numpy()
    runs = {}
    for key, extra in (("plain", {}), ("none", dict(overlay=None)), ("on", dict(overlay=True)), ("eager", dict(overlay=True, use_graph=False)),
                       ("smooth", dict(overlay=dict(source="smooth", opacity=0.5, by_size=0.02, line_radius=0.5)))):
        step = ManagedInferStep(model, B, SIZE, SIZE, **options, **extra)
        names = []
        step.lib = _Recorder(step.lib, names)
        step(**_first())                                            # warm-up + capture + replay (eager: one run)
        one, frames_one, n_first = _snap(step, SNAP), step.frames.cpu().numpy().copy(), len(names)
        if step.overlay:                                            # the first call drew once, on clean frames
            src = "smooth_preds" if key == "smooth" else "preds"
            _assert_same_bytes(frames_one, _host_of(step, clean, src), f"{key}: first call")
            assert not np.array_equal(frames_one, clean)
        else:
            assert np.array_equal(frames_one, clean)
        step.advance()
        step(frames=_step_frames())                                 # the caller brings new frames: the crop sees clean pixels
        two, frames_two = _snap(step, SNAP), step.frames.cpu().numpy().copy()
        if step.overlay:
            _assert_same_bytes(frames_two, _host_of(step, clean, "smooth_preds" if key == "smooth" else "preds"), f"{key}: second call")
        runs[key] = (names[:n_first], one, two, step)
    plain, none, on = runs["plain"][0], runs["none"][0], runs["on"][0]
    assert none == plain and runs["none"][3].overlay is None and runs["none"][3].overlay_table is None
    half = len(plain) // 2
    assert plain[:half] == plain[half:] and plain[-1] == "lh_one_euro"
    # the warm-up run draws nothing (the list of the plain step), the captured one ends with the overlay
    assert on == plain[:half] + plain[half:] + ["lh_draw_hands"] and on.count("lh_draw_hands") == 1
    assert runs["eager"][0] == plain[:half] + ["lh_draw_hands"]
    assert runs["on"][3].overlay["min_score"] == options["track_min_score"] and runs["on"][3].overlay["target"] == "inplace"
    for key in ("none", "on", "eager", "smooth"):                   # the overlay changes no output, captured equals eager
        _same(runs["plain"][1], runs[key][1])
        _same(runs["plain"][2], runs[key][2])


def test_overlay_on_a_second_table_leaves_the_source_untouched(monkeypatch):
    from lighthand_amd.runtime import ManagedInferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    options = _options(model, False)
    clean = _step_frames().cpu().numpy()
    step = ManagedInferStep(model, B, SIZE, SIZE, overlay=dict(target="surfaces"), **options)
    assert step.overlay_table.cpu().tolist() == [0] * NF
    step(**_first())                                                # no destination is bound: nothing is drawn, nothing faults
    torch.cuda.synchronize()
    assert np.array_equal(step.frames.cpu().numpy(), clean)
    dst = [t.clone().reshape(-1) for t in _step_frames()]
    step.bind_overlay_surfaces(dst[:1] + dst[2:], start=0)          # frames 0, 1, 2 <- dst 0, 2, 3; frame 3 stays unbound
    step.bind_overlay_surfaces([dst[1]], start=1)
    step.bind_overlay_surfaces([dst[2]], start=2)
    step(frames=_step_frames())
    torch.cuda.synchronize()
    assert np.array_equal(step.frames.cpu().numpy(), clean)         # the source bytes are untouched
    want = _host_of(step, [clean[0], clean[1], clean[2], None])
    for f in range(3):
        _assert_same_bytes(dst[f].cpu().numpy(), want[f], f"destination {f}")
    assert not np.array_equal(dst[0].cpu().numpy().reshape(clean[0].shape), clean[0])
    _assert_same_bytes(dst[3].cpu().numpy(), clean[3], "the unbound frame's tensor")
    step.unbind_overlay_surfaces()
    assert step.overlay_table.cpu().tolist() == [0] * NF
    with pytest.raises(ValueError):
        step.bind_overlay_surfaces([dst[0][:100]])
    with pytest.raises(ValueError):
        step.bind_overlay_surfaces(dst, start=1)
    plain = ManagedInferStep(model, B, SIZE, SIZE, overlay=True, **options)
    with pytest.raises(ValueError):
        plain.bind_overlay_surfaces(dst)


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
def test_overlay_on_bound_surfaces_in_place(fmt, monkeypatch):
    from lighthand_amd import topdown
    from lighthand_amd.runtime import ManagedInferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    options = dict(_options(model, True), frame_format=fmt, surfaces=True)
    rgb = _step_frames().cpu().numpy()
    enc = np.asarray(topdown.rgb_to_yuv420_host(rgb, fmt)).reshape(NF, -1)
    step = ManagedInferStep(model, B, SIZE, SIZE, overlay=True, **options)
    surfaces = [torch.from_numpy(f.copy()).cuda() for f in enc]
    step(surfaces=surfaces[:3], boxes=_dev(BOXES, F), frame_index=_dev(APART, np.int32))       # frame 3 is unbound: its slot is skipped
    torch.cuda.synchronize()
    want = _host_of(step, [enc[0], enc[1], enc[2], None], frame_format=fmt, frame_size=(FH, FW))
    for f in range(3):
        _assert_same_bytes(surfaces[f].cpu().numpy(), want[f], f"{fmt} surface {f}")
    assert not np.array_equal(surfaces[0].cpu().numpy(), enc[0])
    _assert_same_bytes(surfaces[3].cpu().numpy(), enc[3], "the unbound surface")


def test_pipeline_slots_draw_on_their_own_frames_and_refusals(monkeypatch):
    from lighthand_amd.runtime import InferStep, ManagedInferPipeline, ManagedInferStep
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    model = _model()
    options = _options(model, False)
    clean = _step_frames().cpu().numpy()
    pipe = ManagedInferPipeline(model, B, SIZE, SIZE, depth=2, overlay=dict(draw_roi=False), **options)
    other = clean[::-1].copy()
    t0 = pipe.submit(**_first(SHARED))
    t1 = pipe.submit(frames=torch.from_numpy(other).cuda(), boxes=_dev(BOXES, F), frame_index=_dev(APART, np.int32))
    pipe.result(t0), pipe.result(t1)
    torch.cuda.synchronize()
    for step, before in zip(pipe.steps, (clean, other)):
        assert step.overlay["draw_roi"] is False
        got = step.frames.cpu().numpy()
        _assert_same_bytes(got, _host_of(step, before), "pipeline slot")
        assert not np.array_equal(got, before)
    # refusals at construction
    no_frames = {k: v for k, v in options.items() if k not in ("frames", "oriented", "track", "track_min_joints", "track_min_side", "track_min_score")}
    with pytest.raises(ValueError, match="frames"):
        ManagedInferStep(model, B, SIZE, SIZE, manage_tracks=False, overlay=True, **no_frames)
    for bad in (dict(colour="red"), dict(parents=[0] * 20), dict(groups=[0] * 3), dict(source="smooth"), dict(target="host"), dict(opacity=-1)):
        with pytest.raises(ValueError):
            ManagedInferStep(model, B, SIZE, SIZE, overlay=bad, **options)
    with pytest.raises(TypeError):
        InferStep(model, B, SIZE, SIZE, overlay=True, **options)    # the keyword lives on the subclass


@pytest.mark.parametrize("fmt", ["rgb", "nv12"])
def test_cli_writes_the_steps_frames(fmt, tmp_path, monkeypatch, capsys):
    from lighthand_amd.tools import track_frames
    monkeypatch.setenv("LH_AUTOTUNE", "0")
    seen, write = [], track_frames.write_overlay_frame

    def spy(directory, t, frame, *rest):
        seen.append((t, frame.cpu().numpy().reshape(-1).copy()))
        return write(directory, t, frame, *rest)
    monkeypatch.setattr(track_frames, "write_overlay_frame", spy)
    argv = ["--synthetic", "3", "--frame_size", "96x128", "--hands", "2", "--depth", "18", "--size", "64", "--overlay_out", str(tmp_path),
            "--overlay_every", "2", "--frame_format", fmt] + (["--surfaces"] if fmt == "nv12" else [])
    result = track_frames.main(argv)
    capsys.readouterr()
    assert [t for t, _ in seen] == [0, 2] and len(result["overlay_files"]) == 2
    frames, _ = track_frames.synthetic_sequence(3, 96, 128, 2, 0)
    for (t, data), name in zip(seen, result["overlay_files"]):
        raw = open(name, "rb").read()
        if fmt == "rgb":
            head = b"P6\n128 96\n255\n"
            assert raw[:len(head)] == head and raw[len(head):] == data.tobytes() and len(data) == 96 * 128 * 3
            assert (data.reshape(96, 128, 3) != frames[t]).any()     # something was drawn
        else:
            assert raw == data.tobytes() and len(raw) == 96 * 128 * 3 // 2
            assert open(name + ".txt").read().split()[:3] == ["format=nv12", "width=128", "height=96"]
