"""CPU: the host side of the visibility-weighted heat-map loss and hard-keypoint mining -- the new C-ABI symbols and their
argument checks, the train CLI's flags, the visibility column of the synthetic samples and of the loader wrapper."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_new_symbols_are_declared_and_bound_with_the_header_arity():
    from lighthand_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "lighthand_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"\b(lh_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S))
    for name, arity in (("lh_gaussian_target_w", 12), ("lh_joints_mse", 13), ("lh_joints_mse_workspace_bytes", 2)):
        assert name in protos, f"{name} is not declared in the header"
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert len(protos[name].split(",")) == len(_lib.SIGNATURES[name][1]) == arity, name


def test_workspace_size_and_argument_validation_run_on_the_host():
    from lighthand_amd import _lib
    lib = _lib.load()
    # fp64 plane sums + fp32 coefficients + int32 selection flags per joint plane
    assert lib.lh_joints_mse_workspace_bytes(64, 21) == 64 * 21 * 16
    assert lib.lh_joints_mse_workspace_bytes(0, 21) == 0
    ok = (64, 128, None, 2, 21, 256, 0, 192, None, 256, None, 320, None)

    def call(**kw):
        names = ("pred", "target", "weight", "b", "j", "hw", "topk", "loss", "joint_loss", "grad", "grad_scale", "workspace", "stream")
        a = dict(zip(names, ok))
        a.update(kw)
        return lib.lh_joints_mse(*[a[n] for n in names])

    assert call(pred=None) == -1 and b"lh_joints_mse" in lib.lh_last_error()
    assert call(loss=None) == -1 and call(workspace=None) == -1
    assert call(hw=254) == -1 and b"multiple of 4" in lib.lh_last_error()
    assert call(pred=68) == -1 and b"16-byte" in lib.lh_last_error()
    assert call(grad=260) == -1 and b"16-byte" in lib.lh_last_error()
    assert call(topk=22) == -1 and b"topk" in lib.lh_last_error()
    assert call(topk=-1) == -1
    # the weighted render: weight is a required output, the visibility is optional
    assert lib.lh_gaussian_target_w(64, 2, None, 0, 64, 6, 64, None, 2, 21, 64, None) == -1
    assert b"lh_gaussian_target_w" in lib.lh_last_error()
    assert lib.lh_gaussian_target_w(64, 1, None, 0, 64, 6, 64, 64, 2, 21, 64, None) == -1          # jstride < 2


def test_train_parser_takes_the_two_flags():
    from lighthand_amd.tools import train as T
    a = T.parse_args([])
    assert a.use_target_weight is False and a.ohkm_topk == 0
    a = T.parse_args(["--use_target_weight", "--ohkm_topk", "8"])
    assert a.use_target_weight is True and a.ohkm_topk == 8
    with pytest.raises(SystemExit):
        T.parse_args(["--ohkm_topk", "many"])


def test_synthetic_hands_optional_visibility_column():
    from lighthand_amd.tools.train import SyntheticHands
    plain = SyntheticHands(16, 32, 7)
    img, j = plain[3]
    assert tuple(j.shape) == (21, 2) and tuple(img.shape) == (3, 32, 32)
    ds = SyntheticHands(16, 32, 7, invisible=0.25)
    img3, j3 = ds[3]
    assert tuple(j3.shape) == (21, 3) and j3.dtype == torch.float32
    assert torch.equal(img3, img) and torch.equal(j3[:, :2], j)            # the option does not move the other draws
    col = torch.stack([ds[i][1][:, 2] for i in range(len(ds))])
    assert set(col.unique().tolist()) == {0.0, 1.0}
    assert 0.1 < float((col == 0).float().mean()) < 0.4
    assert float(SyntheticHands(4, 32, 7, invisible=0.0)[0][1][:, 2].min()) == 1.0


def test_loader_wrapper_keeps_the_visibility_column():
    from lighthand_amd.tools.train import SyntheticHands, _WithAugFlag
    w3 = _WithAugFlag(SyntheticHands(8, 32, 1, invisible=0.5), 0.5)
    img, j, aug = w3[0]
    assert tuple(j.shape) == (21, 3) and aug is True and w3[7][2] is False
    assert torch.equal(j, w3.base[0][1])
    w2 = _WithAugFlag(SyntheticHands(8, 32, 1), 0.5)
    assert tuple(w2[0][1].shape) == (21, 2)

    class Wide(torch.utils.data.Dataset):                                  # columns past the third are dropped, as before
        def __len__(self):
            return 2

        def __getitem__(self, i):
            return np.zeros((3, 32, 32), np.float32), np.ones((21, 5), np.float32)
    assert tuple(_WithAugFlag(Wide(), 0.0)[1][1].shape) == (21, 3)


def test_loss_module_and_step_options_exist():
    import inspect
    from lighthand_amd import heatmap
    from lighthand_amd.runtime import TrainStep
    assert heatmap.WeightedJointsMSELoss().topk == 0 and heatmap.WeightedJointsMSELoss(topk=8).topk == 8
    with pytest.raises(ValueError):
        heatmap.WeightedJointsMSELoss(topk=-1)
    assert inspect.signature(heatmap.render_targets).parameters["return_weight"].default is False
    assert inspect.signature(heatmap.generate_target).parameters["return_weight"].default is False
    p = inspect.signature(TrainStep.__init__).parameters
    assert p["use_target_weight"].default is False and p["ohkm_topk"].default == 0
