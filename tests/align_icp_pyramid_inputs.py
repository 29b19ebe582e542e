"""Inputs of the depth-pyramid tests (a helper, not a test module): two cameras whose level cameras are all integers, so
that they survive tf_set_camera's truncation; images that put one reading at each edge of the block rule; the noisy corner
of the experiment the pyramid was built for."""
import numpy as np

from tests import align_icp_inputs as II
from tests.align_inputs import hand_depth, hand_pose
from tests.align_icp_pyramid_ref import level_cam
from texturefusion_amd import synth

F = np.float32
CAM_A = synth.Camera(160, 120, 128.0, 128.0, 79.0, 59.0)  # levels 1, 2: 80 x 60, f 64, c (39, 29); 40 x 30, f 32, c (19, 14)
CAM_B = synth.Camera(160, 128, 128.0, 128.0, 79.0, 63.0)  # level 3: 20 x 16, f 16, c (9, 7)
JUMP = F(0.125)  # a power of two: 1 + JUMP and the float above it differ from 1 by exactly JUMP and JUMP + 2^-23
TINY = F(1e-40)  # a denormal: finite and > 0, so a reading like any other

# one 2 x 2 block each (a, b, c, d) and what the level-1 pixel must be under the jump JUMP (None: the block's mean)
BLOCKS = [
    ("spread_exact", (F(1), F(1), F(1) + JUMP, F(1)), None),
    ("spread_next", (F(1), F(1), np.nextafter(F(1) + JUMP, F(2)), F(1)), F(0)),
    ("nan", (F(1), F(np.nan), F(1), F(1)), F(0)),
    ("inf", (F(1), F(1), F(1), F(np.inf)), F(0)),
    ("zero", (F(0), F(1), F(1), F(1)), F(0)),
    ("negative", (F(1), F(1), F(-1), F(1)), F(0)),
    ("neg_inf", (F(1), F(-np.inf), F(1), F(1)), F(0)),
    ("denormal_among_ones", (F(1), F(1), F(1), TINY), F(0)),  # valid readings, but a spread of 1
    ("denormals", (TINY, TINY, F(3) * TINY, TINY), None),     # four valid readings: their mean, a denormal
    ("huge", (F(3e38), F(3e38), F(3e38), F(3e38)), None),     # a + b overflows: the mean is +inf, no reading for level 2
]


def edge_image(W, H, seed=0):
    """A W x H image (both even, W * H >= 64) of readings near 1 m, BLOCKS' blocks in its first level-1 pixels in row-major
    order, and -- where there is room -- two 4 x 4 patches that put level 2 at the spread's edge -> (image, {name: (X, Y)})"""
    img = (F(1) + F(0.01) * np.random.default_rng(seed).random((H, W), dtype=np.float32)).astype(np.float32)
    at = {}
    for i, (name, (a, b, c, d), _) in enumerate(BLOCKS):
        X, Y = i % (W // 2), i // (W // 2)
        img[2 * Y, 2 * X], img[2 * Y, 2 * X + 1], img[2 * Y + 1, 2 * X], img[2 * Y + 1, 2 * X + 1] = a, b, c, d
        at[name] = (X, Y)
    if W >= 16 and H >= 12:  # level-1 pixels 1, 1, 1, 1 + JUMP (exactly: constant blocks): kept at level 2; one ulp more: dropped
        for name, x0, top in (("l2_spread_exact", 0, F(1) + JUMP), ("l2_spread_next", 4, np.nextafter(F(1) + JUMP, F(2)))):
            img[8:12, x0:x0 + 4] = F(1)
            img[10:12, x0 + 2:x0 + 4] = top
            at[name] = (x0 // 4, 2)  # a level-2 pixel
    return img, at


def one_hole_per_block(W, H):
    """every 2 x 2 block has exactly one hole, in a corner that changes from block to block: level 1 is all zero"""
    img = np.full((H, W), F(1.5), np.float32)
    yy, xx = np.meshgrid(np.arange(H // 2), np.arange(W // 2), indexing="ij")
    k = (xx + 2 * yy) % 4
    img[2 * yy + k // 2, 2 * xx + k % 2] = F(0)
    return img


def noisy_corner(sigma, seed, cam=CAM_A):
    """hand_depth(hand_pose()) with Gaussian noise of `sigma` metres on every reading there is"""
    d = hand_depth(hand_pose(), cam)
    n = np.random.default_rng(seed).normal(0.0, sigma, d.shape)
    return np.where(d > 0, d + n, 0.0).astype(np.float32)


def analytic_maps(pose, cam, ks):
    """{k: hand_model_maps at level_cam(cam, k)} for k in ks"""
    return {k: II.hand_model_maps(pose, level_cam(cam, k)) for k in ks}
