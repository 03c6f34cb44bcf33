"""Top-down inference on full frames: hand box -> crop matrix and keypoints -> next box, eagerly on device tensors (the C-ABI
entries lh_box_affine / lh_keypoints_to_boxes that runtime.InferStep(frames=...) captures into its graph) and restated in numpy.

Coordinates are pixel indices (pixel centres on the integers, an image spans [-0.5, size-0.5]); a box is (x0, y0, x1, y1) in them,
the box that encloses pixels i0..i1 is (i0-0.5, i1+0.5).  The matrix of a box takes a CROP pixel index to a FRAME pixel index: the
crop kernel (lh_frames_crop_to_nhwc4) samples through it and lh_affine_points takes the decoded keypoints back to the frame through
it.  The ``*_host`` functions follow the kernels operation by operation in fp32 (the library is built with -ffp-contract=off): the CPU
tests check the geometry on them, the GPU tests check the kernels against them."""
import numpy as np

F = np.float32


def box_affine_host(boxes, frame_index, n_frames, size, padding):
    """boxes [b][4], frame_index [b], size = (h, w) of the crop -> (mat fp32 [b][6], src_frame int32 [b]); lh_box_affine in numpy."""
    h, w = F(size[0]), F(size[1])
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    fi = np.asarray(frame_index, np.int32).reshape(-1)
    pad = F(padding)
    x0, y0, x1, y1 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    with np.errstate(all="ignore"):
        bw, bh = x1 - x0, y1 - y0
        ok = (fi >= 0) & (fi < n_frames) & np.isfinite(boxes).all(1) & (bw > 0) & (bh > 0)
        cx, cy = (x0 + x1) * F(0.5), (y0 + y1) * F(0.5)
        sw = pad * np.maximum(bw, bh * w / h)
        sh = sw * h / w
        a = sw / w
        zero = np.zeros_like(a)
        mat = np.stack([a, zero, (cx - sw * F(0.5)) + a * F(0.5), zero, a, (cy - sh * F(0.5)) + a * F(0.5)], 1).astype(np.float32)
    mat[~ok] = 0
    return mat, np.where(ok, fi, -1).astype(np.int32)


def boxes_from_keypoints_host(preds, maxvals, boxes, src_frame, min_score=0.1, min_joints=8, min_side=16.0):
    """preds [b][j][2] (frame coordinates), maxvals [b][j] or [b][j][1], boxes [b][4], src_frame [b] -> (next_boxes fp32 [b][4],
    lost int32 [b]); lh_keypoints_to_boxes in numpy: the joints are walked in order with the kernel's comparisons."""
    preds = np.asarray(preds, np.float32)
    b, j = preds.shape[:2]
    mv = np.asarray(maxvals, np.float32).reshape(b, j)
    boxes = np.asarray(boxes, np.float32).reshape(b, 4)
    src = np.asarray(src_frame, np.int32).reshape(b)
    lo_x, lo_y, hi_x, hi_y = (np.zeros(b, np.float32) for _ in range(4))
    n = np.zeros(b, np.int64)
    with np.errstate(all="ignore"):
        for k in range(j):
            take = mv[:, k] >= F(min_score)
            x, y = preds[:, k, 0], preds[:, k, 1]
            first = take & (n == 0)
            lo_x, hi_x = np.where(first, x, lo_x), np.where(first, x, hi_x)
            lo_y, hi_y = np.where(first, y, lo_y), np.where(first, y, hi_y)
            lo_x, hi_x = np.where(take & (x < lo_x), x, lo_x), np.where(take & (x > hi_x), x, hi_x)
            lo_y, hi_y = np.where(take & (y < lo_y), y, lo_y), np.where(take & (y > hi_y), y, hi_y)
            n += take
        half = F(min_side) * F(0.5)
        for lo, hi in ((lo_x, hi_x), (lo_y, hi_y)):
            narrow = hi - lo < F(min_side)
            c = (lo + hi) * F(0.5)
            lo[:], hi[:] = np.where(narrow, c - half, lo), np.where(narrow, c + half, hi)
    lost = (n < min_joints) | (src < 0)
    out = np.stack([lo_x, lo_y, hi_x, hi_y], 1).astype(np.float32)
    out[lost] = boxes[lost]
    return out, lost.astype(np.int32)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def box_affine(boxes, frame_index, n_frames, size, padding=1.25):
    """Device tensors boxes fp32 [b][4], frame_index int32 [b] -> (mat fp32 [b][6], src_frame int32 [b]) for an h x w = ``size`` crop
    (one lh_box_affine launch on the current stream)."""
    import torch
    from . import _lib
    if not padding > 0:
        raise ValueError(f"padding must be > 0, not {padding!r}")
    boxes = boxes.to(torch.float32).contiguous()
    frame_index = frame_index.to(torch.int32).contiguous()
    b = boxes.shape[0]
    if tuple(boxes.shape) != (b, 4) or tuple(frame_index.shape) != (b,) or not boxes.is_cuda or frame_index.device != boxes.device:
        raise _lib.LightHandError(f"box_affine: boxes [b, 4] and frame_index [b] on one device, got {tuple(boxes.shape)} / {tuple(frame_index.shape)}")
    mat = torch.empty(b, 6, dtype=torch.float32, device=boxes.device)
    src = torch.empty(b, dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        _lib.check(_lib.load().lh_box_affine(boxes.data_ptr(), frame_index.data_ptr(), b, int(n_frames), int(size[0]), int(size[1]),
                                             float(padding), mat.data_ptr(), src.data_ptr(), _stream()), "lh_box_affine")
    return mat, src


def boxes_from_keypoints(preds, maxvals, boxes, src_frame, min_score=0.1, min_joints=8, min_side=16.0):
    """Device tensors preds fp32 [b][j][2] (frame coordinates), maxvals [b][j] or [b][j][1], boxes [b][4], src_frame int32 [b] ->
    (next_boxes fp32 [b][4], lost int32 [b]) (one lh_keypoints_to_boxes launch on the current stream)."""
    import torch
    from . import _lib
    preds = preds.to(torch.float32).contiguous()
    b, j = preds.shape[:2]
    maxvals = maxvals.to(torch.float32).reshape(b, j).contiguous()
    boxes = boxes.to(torch.float32).contiguous()
    src_frame = src_frame.to(torch.int32).contiguous()
    if tuple(preds.shape) != (b, j, 2) or tuple(boxes.shape) != (b, 4) or tuple(src_frame.shape) != (b,) or not preds.is_cuda:
        raise _lib.LightHandError(f"boxes_from_keypoints: preds [b, j, 2], boxes [b, 4], src_frame [b] on the device, got "
                                  f"{tuple(preds.shape)} / {tuple(boxes.shape)} / {tuple(src_frame.shape)}")
    nxt = torch.empty(b, 4, dtype=torch.float32, device=preds.device)
    lost = torch.empty(b, dtype=torch.int32, device=preds.device)
    with torch.cuda.device(preds.device):
        _lib.check(_lib.load().lh_keypoints_to_boxes(preds.data_ptr(), maxvals.data_ptr(), boxes.data_ptr(), src_frame.data_ptr(), b, j,
                                                     float(min_score), int(min_joints), float(min_side), nxt.data_ptr(), lost.data_ptr(),
                                                     _stream()), "lh_keypoints_to_boxes")
    return nxt, lost
