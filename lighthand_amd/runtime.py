"""hipGraph-captured training / inference steps: the fast path of the engine.

The reference's hot loop (src/utils/method.py:160-183) is, per iteration: H2D, forward,
JointsMSELoss, ``.item()``, full-heatmap D2H + NumPy arg-max, zero_grad, backward, Adam.
``TrainStep`` runs the same work as ONE replay of a captured HIP graph over static buffers:
weight packs -> forward -> Gaussian target render (from joints) -> MSE loss + dL/dheatmap ->
arg-max decode (kept on the device) -> backward -> [gradient all-reduce] -> fused Adam.
Loss and keypoints stay on the device; ``.loss`` / ``.preds`` are read only when the caller
asks (no per-iteration stream sync).

This module is the import surface; the code lives by role in ``draws`` (the host samplers), ``frame_input`` (the frame-crop
options and what the two steps share), ``train_step`` and ``infer_step``.
"""
from .draws import sample_affine, sample_color_jitter, sample_roi_aug  # noqa: F401
from .frame_input import (FrameInput, _antialias_taps, _check_manage_tracks, _check_motion, _check_smooth_gate,  # noqa: F401
                          _check_train_frames)
from .infer_step import InferPipeline, InferStep, ManagedInferPipeline, ManagedInferStep  # noqa: F401
from .train_step import TrainStep  # noqa: F401
