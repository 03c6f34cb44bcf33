"""Seeded inputs and the comparison rule that tests/test_crop_jitter_host.py and tests/test_gpu_crop_jitter.py share: 28 hand ROIs on
three 96 x 128 frames, cropped to 64 x 64, and one ColorJitter draw per slot that covers every op order."""
import itertools

import numpy as np

F = np.float32
HS, WS, SIZE, B, N_FRAMES = 96, 128, 64, 28, 3
SEED = 20              # the frames and ROIs of every test here (test_crop_jitter_host.py: the fp32 / fp64 check this seed passes)
PERMS = list(itertools.permutations(range(4)))


def frames(seed=SEED):
    """uint8 [3][96][128][3]: two frames of noise and, as frame 1, one of grey pixels (r = g = b: the hue op is a no-op there)."""
    rng = np.random.RandomState(seed)
    out = rng.randint(0, 256, size=(N_FRAMES, HS, WS, 3)).astype(np.uint8)
    out[1] = out[1][..., :1]
    return out


def rois(seed=SEED, scale=(0.4, 1.1)):
    """(boxes fp32 [28][4], rot fp32 [28][2], mirror int32 [28], frame_index int32 [28]): centres anywhere on the frame (so many crops
    reach past its border: black pixels that count in the grey mean), ``scale`` frame pixels per crop pixel, the first four upright,
    the others turned by any angle (|m3| >= 0.25 for most: the tiled walk), every third mirrored, slot 5 empty (frame_index -1)."""
    rng = np.random.RandomState(seed + 1)
    s = rng.uniform(scale[0], scale[1], size=B)
    centre = np.stack([rng.uniform(10, WS - 10, B), rng.uniform(10, HS - 10, B)], 1)
    half = (s * SIZE / 2)[:, None] * np.ones((1, 2))
    boxes = np.concatenate([centre - half, centre + half], 1).astype(np.float32)
    ang = rng.uniform(-np.pi, np.pi, B)
    ang[:4] = 0.0
    rot = np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)
    mirror = (np.arange(B) % 3 == 2).astype(np.int32)
    index = (np.arange(B) % N_FRAMES).astype(np.int32)
    index[5] = -1
    return boxes, rot, mirror, index


def draw(seed=5):
    """(factors fp32 [28][4], order int32 [28][4]): runtime.sample_color_jitter's seeded draw with the orders replaced by all 24
    permutations, then no op at all, an order with skips, and the two ends of the reference's 0.5 ranges (the cases of
    test_color_jitter_input_pipeline_matches_oracle)."""
    import torch
    from lighthand_amd.runtime import sample_color_jitter
    factors, order = sample_color_jitter(B, generator=torch.Generator().manual_seed(seed))
    factors, order = factors.numpy().copy(), order.numpy().copy()
    order[:24] = np.array(PERMS, np.int32)
    order[24] = -1
    order[25] = (3, -1, 1, -1)
    factors[26] = (0.5, 0.5, 0.5, -0.5)
    factors[27] = (1.5, 1.5, 1.5, 0.5)
    return factors.astype(np.float32), order.astype(np.int32)


def mismatch(got, want):
    """The project's criterion for a jittered image against a restatement (test_color_jitter_input_pipeline_matches_oracle), per slot of
    [b][3][h][w]: (the largest share of values off by more than 1e-4 -- a pixel on a hue-sector or clamp boundary may take the other
    branch after a rounding --, the largest median difference).  The caller asserts share < 1e-3 and median < 1e-6."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).reshape(len(got), -1)
    return float((d > 1e-4).mean(1).max()), float(np.median(d, 1).max())


def half_outside_case(g=150, f=0.6):
    """The closed-form contrast case: a constant grey frame, an upright box whose 64 x 64 crop at scale 1 has its columns 0..31 left of
    the frame and 32..63 on it -> (frames uint8 [1][96][128][3], boxes [1][4], the expected un-normalised crop fp32 [3][64][64]).
    Inside, every sample is exactly g, c = g * (1/255); the grey mean is (2048 * gray(c)) / 4096 = 0.5 * gray(c) exactly (an fp64 sum of
    equal fp32 values, halved); with order (1, -1, -1, -1) and factor f the inside pixels are clamp(f*c + (1-f)*mean) and the outside
    ones clamp(f*0 + (1-f)*mean), in fp32."""
    fr = np.full((1, HS, WS, 3), g, np.uint8)
    boxes = F([[-32.5, 9.5, 31.5, 73.5]])                     # centre (-0.5, 41.5), 64 wide: m = (1, 0, -32, 0, 1, 10) under padding 1
    c = F(g) * (F(1) / F(255))
    gray = (F(0.2989) * c + F(0.587) * c) + F(0.114) * c
    mean = F(0.5) * gray
    inside = np.minimum(np.maximum(F(f) * c + (F(1) - F(f)) * mean, F(0)), F(1))
    outside = np.minimum(np.maximum(F(f) * F(0) + (F(1) - F(f)) * mean, F(0)), F(1))
    want = np.empty((3, SIZE, SIZE), np.float32)
    want[:, :, :32], want[:, :, 32:] = outside, inside
    return fr, boxes, want
