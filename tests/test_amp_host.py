"""CPU: dynamic loss scaling's host side -- DynamicLossScale's arguments and state dict against torch.amp.GradScaler, the new
C-ABI symbols, the train CLI's --loss_scale flag."""
import pytest
import torch


def _gradscaler(**kw):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")              # "CUDA is not available.  Disabling." on a CPU box: validation still runs
        return torch.amp.GradScaler("cpu", **kw)


def test_defaults_and_argument_checks_match_gradscaler():
    from lighthand_amd.amp import DynamicLossScale
    s = DynamicLossScale(device="cpu")
    g = _gradscaler()
    assert (s.scale, s.growth_factor, s.backoff_factor, s.growth_interval) == \
        (g._init_scale, g._growth_factor, g._backoff_factor, g._growth_interval) == (2.0 ** 16, 2.0, 0.5, 2000)
    assert s.skipped_steps == 0 and int(s.found_inf) == 0
    for bad in (dict(growth_factor=1.0), dict(growth_factor=0.5), dict(backoff_factor=1.0), dict(backoff_factor=2.0)):
        with pytest.raises(AssertionError) as want:
            _gradscaler(**bad)
        with pytest.raises(AssertionError) as got:
            DynamicLossScale(device="cpu", **bad)
        assert str(got.value) == str(want.value)
    for ok in (dict(growth_factor=1.5, backoff_factor=0.0), dict(growth_interval=0), dict(init_scale=1.0)):
        _gradscaler(**ok)
        DynamicLossScale(device="cpu", **ok)


def test_state_dict_round_trips_with_gradscaler():
    from lighthand_amd.amp import DynamicLossScale
    g = _gradscaler(init_scale=512.0, growth_factor=4.0, backoff_factor=0.25, growth_interval=7)
    g._lazy_init_scale_growth_tracker(torch.device("cpu"))
    g._growth_tracker.fill_(3)
    want = g.state_dict()
    s = DynamicLossScale(device="cpu")
    s.load_state_dict(want)
    got = s.state_dict()
    assert got == want and sorted(got) == ["_growth_tracker", "backoff_factor", "growth_factor", "growth_interval", "scale"]
    assert s.scale_tensor.dtype == torch.float32 and int(s._growth_tracker) == 3
    assert s._hyper.tolist() == [4.0, 0.25, 7.0]
    # and back: GradScaler takes ours
    s._scale.fill_(2.0 ** 20)
    s._growth_tracker.fill_(11)
    g2 = _gradscaler()
    g2.load_state_dict(s.state_dict())
    assert g2.state_dict() == {"scale": 2.0 ** 20, "growth_factor": 4.0, "backoff_factor": 0.25, "growth_interval": 7,
                               "_growth_tracker": 11}
    with pytest.raises(RuntimeError):
        s.load_state_dict({})


def test_loading_writes_the_device_tensors_in_place():
    """A captured graph holds the addresses of the scaler's tensors: load_state_dict must not replace them."""
    from lighthand_amd.amp import DynamicLossScale
    s = DynamicLossScale(device="cpu")
    ptrs = [t.data_ptr() for t in (s._scale, s._growth_tracker, s._hyper)]
    s.load_state_dict({"scale": 8.0, "growth_factor": 3.0, "backoff_factor": 0.125, "growth_interval": 5, "_growth_tracker": 2})
    assert [t.data_ptr() for t in (s._scale, s._growth_tracker, s._hyper)] == ptrs
    assert s.scale == 8.0 and s._hyper.tolist() == [3.0, 0.125, 5.0]


def test_new_symbols_are_exported_with_prototypes():
    from lighthand_amd import _lib
    lib = _lib.load()
    for name in ("lh_amp_check_blocks", "lh_amp_check", "lh_amp_update", "lh_adam_apply_guarded"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    n = lib.lh_amp_check_blocks()
    assert 256 <= n <= 4096 and n % 256 == 0           # a fixed grid, a small multiple of the MI355X's 256 CUs
    # argument validation runs on the host
    assert lib.lh_amp_check(None, 16, None, None) != 0 and b"lh_amp_check" in lib.lh_last_error()
    assert lib.lh_amp_check(4, 16, 64, None) != 0 and b"16-byte" in lib.lh_last_error()
    assert lib.lh_adam_apply_guarded(16, 16, 16, 16, 8, 16, None, 16, None) != 0 and b"lh_adam_apply_guarded" in lib.lh_last_error()
    assert lib.lh_amp_update(16, 16, 16, 16, 16, 16, 16, 1.0, 16, 16, None, None) != 0 and b"null" in lib.lh_last_error()


def test_adam_step_with_amp_needs_the_arena():
    from lighthand_amd import _lib
    from lighthand_amd.amp import DynamicLossScale
    from lighthand_amd.optim import Adam
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(_lib.LightHandError):
        Adam([p]).step(amp=DynamicLossScale(device="cpu"))


def test_train_parser_takes_loss_scale():
    import argparse
    from lighthand_amd.tools import train as T
    assert T.parse_args([]).loss_scale == "auto"
    assert T.parse_args(["--loss_scale", "dynamic"]).loss_scale == "dynamic"
    assert T.parse_args(["--loss_scale", "auto"]).loss_scale == "auto"
    assert T.parse_args(["--loss_scale", "512"]).loss_scale == 512.0
    with pytest.raises(SystemExit):
        T.parse_args(["--loss_scale", "large"])
    assert isinstance(T._loss_scale_arg("2e3"), float)
    with pytest.raises(argparse.ArgumentTypeError):
        T._loss_scale_arg("x")


def test_checkpoint_keys_unchanged_without_a_scaler(tmp_path):
    """--loss_scale auto / static keeps the reference's checkpoint keys; dynamic adds scaler_state_dict, which a resume loads."""
    import types
    from lighthand_amd.amp import DynamicLossScale
    from lighthand_amd.tools import train as T
    model = torch.nn.Linear(2, 2)
    opt = torch.optim.Adam(model.parameters())
    args = types.SimpleNamespace(output_dir=str(tmp_path / "run"), reset=False)
    path = tmp_path / "run" / "checkpoint-good" / "state_dict.bin"
    T.save_checkpoint(model, args, 0, opt, 1.0, 0)
    assert sorted(torch.load(path, map_location="cpu")) == ["best_loss", "count", "epoch", "model_state_dict", "optimizer_state_dict"]
    assert not T.load_scaler_state(DynamicLossScale(device="cpu"), args)
    s = DynamicLossScale(init_scale=256.0, device="cpu")
    s._growth_tracker.fill_(9)
    T.save_checkpoint(model, args, 1, opt, 0.5, 0, scaler=s)
    assert torch.load(path, map_location="cpu")["scaler_state_dict"] == s.state_dict()
    r = DynamicLossScale(device="cpu")
    assert T.load_scaler_state(r, args) and r.state_dict() == s.state_dict()
    args.reset = True
    assert not T.load_scaler_state(DynamicLossScale(device="cpu"), args)
