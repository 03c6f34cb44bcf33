"""GPU: the forward launch lists that TrainStep / InferStep build, entry for entry, against tests/golden/step_launch_lists.json -- recorded
with this module's table from the commit before runtime.py was split by role, where every step chose by hand which keyword arguments of
Plan.use_frame_input to leave out.  Constructing a step runs no network and no step is called: the lists alone are compared.  R18 at
batch 2 on 64 x 64, bf16, static kernel choice; frames are 2 of 96 x 128."""
import json
import os

import pytest
import torch

from conftest import GOLDEN, resnet_cfg

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "step_launch_lists.json")
B, SIZE, HS, WS = 2, 64, 96, 128
FRAMES = (2, HS, WS)
JITTER = (0.5, 0.5, 0.5, 0.5)
ROI_AUG = (30.0, 0.2, 0.1, 0.5)


def _nv12_tight():
    from lighthand_amd import topdown
    return topdown.nv12_layout(HS, WS)


# name -> (the step's class, its keyword arguments or a function that returns them)
CASES = {
    "infer": ("InferStep", {}),
    "infer_u8": ("InferStep", dict(input_u8=(HS, WS))),
    "infer_frames_rgb": ("InferStep", dict(frames=FRAMES)),
    "infer_frames_rgb_antialias4": ("InferStep", dict(frames=FRAMES, antialias=4)),
    "infer_frames_rgb_oriented": ("InferStep", dict(frames=FRAMES, oriented=True)),
    "infer_frames_nv12": ("InferStep", dict(frames=FRAMES, frame_format="nv12")),
    "infer_frames_nv12_tight_layout": ("InferStep", lambda: dict(frames=FRAMES, frame_format="nv12", frame_layout=_nv12_tight())),
    "infer_frames_p010": ("InferStep", dict(frames=FRAMES, frame_format="p010")),
    "infer_frames_rgb_surfaces": ("InferStep", dict(frames=FRAMES, surfaces=True)),
    "infer_frames_yuv420p_surfaces": ("InferStep", dict(frames=FRAMES, frame_format="yuv420p", surfaces=True)),
    "train": ("TrainStep", {}),
    "train_u8_jitter_warp": ("TrainStep", dict(input_u8=(HS, WS), color_jitter=JITTER, geometric_aug=(30.0, 0.25, 0.1))),
    "train_frames": ("TrainStep", dict(frames=FRAMES)),
    "train_frames_roi_aug": ("TrainStep", dict(frames=FRAMES, roi_aug=ROI_AUG)),
    "train_frames_crop_jitter": ("TrainStep", dict(frames=FRAMES, crop_jitter=JITTER)),
    "train_frames_nv21_surfaces_jitter_roi_aug": ("TrainStep", dict(frames=FRAMES, frame_format="nv21", surfaces=True, crop_jitter=JITTER,
                                                                   roi_aug=ROI_AUG)),
}


def build_step(name):
    from lighthand_amd import runtime
    from lighthand_amd.modeling.simplebaseline.pose_resnet import get_pose_net
    from lighthand_amd.options import PlanOptions
    kind, kwargs = CASES[name]
    torch.manual_seed(0)
    model = get_pose_net(resnet_cfg(18), True).cuda().set_precision("bf16")
    if kind == "InferStep":
        model.eval()
    return getattr(runtime, kind)(model, B, SIZE, SIZE, use_graph=False, plan_options=PlanOptions.from_env().replace(autotune=False),
                                  **(kwargs() if callable(kwargs) else kwargs))


def launch_list(step):
    """[entry or marker, description] of the step's forward list, as JSON keeps it (a fork / join marker has no entry: its type and kind)."""
    return [[c.fn.__name__, c.what] if hasattr(c, "fn") else [type(c).__name__, c.kind] for c in step.plan.fwd]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_the_table_and_the_file_name_the_same_steps(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_step_builds_the_recorded_launch_list(name, golden):
    got = launch_list(build_step(name))
    assert len(got) > 10 and got == golden[name]
