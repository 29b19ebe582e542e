"""Inputs of the colour-aided alignment tests (a helper, not a test module): a smooth texture in world coordinates, the
hand-built plane of align_inputs.py with that texture in its voxels, and one wall of the S-room box seen from 1.2 m."""
import math

import numpy as np

from tests import align_inputs as I
from texturefusion_amd import synth

CAM = I.CAM
WALL_FRAMES, WALL_HELD = 11, 5
WALL_RES = np.float32(0.005)
HAND_COUNT = 100  # colour count of every hand-built voxel: the sums carry a hundredth of a grey level

# every iteration taken (eps 0), so that an end is a fixed point
PARAMS = dict(levels=[(2, 4), (1, 6)], eps_t=0.0, eps_r=0.0)
PHOTO = dict(photo_weight=0.1, max_photo_residual=0.25, huber_photo=0.05)

# Measured by tests/test_align_color_cpu.py with the restatement (tests/align_color_ref.py).
# Textured hand plane, four starts: the largest distance between two ends is 1.03e-7 m and 5.6e-8 rad, and the ends lie
# 1.046e-4 m and 3.67e-4 rad from the true pose (the trilinear field's smoothing of the texture and the u8 rounding of the
# frame: an offset, not noise).  The tests allow twice the latter.
HAND_SPREAD_T, HAND_SPREAD_R = 1.1e-7, 5.6e-8
HAND_TRUTH_T, HAND_TRUTH_R = 1.046e-4, 3.67e-4
# Textured wall, four starts: the largest distance between two ends, 1.24e-7 m and 7.8e-9 rad.  The device may differ from
# the restatement's fixed point by ten times it.
WALL_SPREAD_T, WALL_SPREAD_R = 1.3e-7, 8e-9


def intensity(p):
    """grey level of a world point [..., 3], f64; the shortest period is 0.17 m (17 voxels at 10 mm)"""
    y, z = p[..., 1], p[..., 2]
    return (128.0 + 55.0 * np.sin(2.0 * math.pi * y / 0.17 + 0.3) * np.cos(2.0 * math.pi * z / 0.23)
            + 45.0 * np.sin(2.0 * math.pi * (y + z) / 0.31 + 1.0))


def hit_points(depth, pose, cam=CAM):
    """world point of every pixel of a z-depth image, f64 [H, W, 3]"""
    P = np.asarray(pose, np.float64).reshape(3, 4)
    return P[:, 3] + (I.rays(cam) @ P[:, :3].T) * np.asarray(depth, np.float64)[..., None]


def texture_rgba(depth, pose, cam=CAM):
    """the texture at each pixel's hit point rounded to u8 in all three channels, alpha 1; 0 where there is no depth"""
    v = np.rint(intensity(hit_points(depth, pose, cam))).astype(np.uint8)
    rgba = np.stack([v, v, v, np.ones_like(v)], -1)
    rgba[~(np.asarray(depth) > 0)] = 0
    return rgba


# ---- the textured hand plane --------------------------------------------------------------------------------------------
def textured(vol):
    """a hand-built volume (ids, sdf, weight, colour) with the colour word (v, v, v, 100) in every voxel, v = rint(100 *
    intensity at the voxel's centre)"""
    ids, sdf, w, col = vol
    i = np.arange(8)
    z, y, x = np.meshgrid(i, i, i, indexing="ij")  # voxel = x + 8 y + 64 z
    col = col.reshape(len(ids), 512, 4).copy()
    for k, cid in enumerate(ids):
        c = np.stack([cid[0] * 8 + x + 0.5, cid[1] * 8 + y + 0.5, cid[2] * 8 + z + 0.5], -1) * float(I.HAND_RES)
        v = np.rint(HAND_COUNT * intensity(c)).astype(np.uint16).reshape(512)
        col[k, :, 0] = col[k, :, 1] = col[k, :, 2] = v
        col[k, :, 3] = HAND_COUNT
    return ids, sdf, w, col.reshape(len(ids), 2048)


def hand_plane_textured():
    return textured(I.hand_plane())


def hand_frame(pose, cam=CAM, edge_voxels=I.HAND_EDGE_VOXELS):
    """(depth, rgba) of the textured plane x = x0 from pose, rendered analytically"""
    depth = I.hand_depth(pose, cam, planes=1, edge_voxels=edge_voxels)
    return depth, texture_rgba(depth, pose, cam)


def hand_starts():
    """(dt, rotation vector) of the starts on the hand plane: the true pose, two in-plane shifts, one with 0.3 degrees; the
    farthest is (0, 15, 12) mm = 19.2 mm"""
    return [(np.zeros(3), np.zeros(3)), (np.array([0.0, 0.015, 0.012]), np.zeros(3)),
            (np.array([0.002, -0.008, 0.006]), np.zeros(3)),
            (np.array([-0.003, 0.006, -0.009]), np.radians(0.3) * np.array([0.6, -0.64, 0.48]))]


# ---- one wall of the S-room box ----------------------------------------------------------------------------------------
def wall_frames(cam=CAM):
    """the 11 frames (depth, rgba, pose) from x = 0.8 facing the wall x = +2, coloured by the texture at the hit points"""
    rng = np.random.default_rng(7)
    out = []
    for k in range(WALL_FRAMES):
        a = 2.0 * math.pi * k / WALL_FRAMES
        t = np.array([0.8, 0.0, 0.0]) + rng.uniform(-0.04, 0.04, 3)
        pose = synth.pose_euler(math.radians(90.0 + 5.0 * math.sin(a)), math.radians(4.0 * math.cos(2.0 * a + 0.4)),
                                math.radians(2.0 * math.sin(3.0 * a + 1.0)), t)
        depth, _ = I.render_box(pose, cam, hole_frac=0.02, seed=k)
        out.append((depth, texture_rgba(depth, pose, cam), pose))
    return out


def wall_starts():
    """(dt, rotation vector) of the starts on the wall (the wall is x = 2: y and z lie in it)"""
    return [(np.zeros(3), np.zeros(3)), (np.array([0.0, -0.012, 0.012]), np.zeros(3)),
            (np.array([0.0, 0.005, -0.016]), np.zeros(3)),
            (np.array([0.004, 0.010, -0.008]), np.radians(0.5) * np.array([0.6, -0.64, 0.48]))]
