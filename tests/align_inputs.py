"""Inputs of the alignment tests (a helper, not a test module): a ray / box renderer for an arbitrary pose, the corner
scene of the S-room box, and hand-built volumes whose SDF is known in closed form."""
import math

import numpy as np

from texturefusion_amd import synth

CAM = synth.Camera(160, 120, 131.25, 131.25, 79.5, 59.5)
HALF = (2.0, 1.5, 2.0)       # the S-room box
CORNER = (2.0, 1.5, 2.0)     # the corner the scene looks into
N_FRAMES, HELD = 13, 6


def rays(cam):
    """camera-frame rays through the pixel centres as the raycaster and the aligner form them (int-truncated intrinsics,
    cx + 0.5, cy + 0.5), z == 1, f64 [H, W, 3]"""
    u = (np.arange(cam.width, dtype=np.float64) - (int(cam.cx) + 0.5)) / int(cam.fx)
    v = (np.arange(cam.height, dtype=np.float64) - (int(cam.cy) + 0.5)) / int(cam.fy)
    uu, vv = np.meshgrid(u, v)
    return np.stack([uu, vv, np.ones_like(uu)], -1)


def render_box(pose, cam=CAM, half=HALF, hole_frac=0.02, seed=0):
    """z-depth [H, W] f32 and rgba of the inside of the box |x| <= half from any pose inside it (synth.room_frame renders
    the orbit only); hole_frac of the pixels are holes (depth 0), as the integrator's chunk selection needs"""
    P = np.asarray(pose, np.float64).reshape(3, 4)
    d = rays(cam) @ P[:, :3].T
    o = P[:, 3]
    hb = np.asarray(half, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(d > 0, (hb - o) / d, np.where(d < 0, (-hb - o) / d, np.inf)).min(-1)
    depth = s.astype(np.float32)
    if hole_frac:
        depth[np.random.default_rng(1000 + seed).random(depth.shape) < hole_frac] = 0.0
    rgba = np.empty(depth.shape + (4,), np.uint8)
    rgba[...] = (180, 120, 60, 1)
    return depth, rgba


def corner_pose(yaw_deg, pitch_deg, roll_deg, shift=(0.0, 0.0, 0.0), dist=1.2):
    """camera dist metres from CORNER along the base view (yaw 45, pitch -28), turned by the given angles, moved by shift"""
    base = synth.pose_euler(math.radians(45.0), math.radians(-28.0), 0.0)[:, 2].astype(np.float64)  # forward axis
    t = np.asarray(CORNER, np.float64) - dist * base + np.asarray(shift, np.float64)
    return synth.pose_euler(math.radians(yaw_deg), math.radians(pitch_deg), math.radians(roll_deg), t)


def corner_frames(cam=CAM):
    """the 13 frames (depth, rgba, pose) of the corner scene: yaw 45 +- 7, pitch -28 +- 6 degrees, a little roll, +- 5 cm"""
    rng = np.random.default_rng(42)
    out = []
    for k in range(N_FRAMES):
        a = 2.0 * math.pi * k / N_FRAMES
        pose = corner_pose(45.0 + 7.0 * math.sin(a), -28.0 + 6.0 * math.cos(2.0 * a + 0.4), 2.0 * math.sin(3.0 * a + 1.0),
                           rng.uniform(-0.05, 0.05, 3))
        depth, rgba = render_box(pose, cam, seed=k)
        out.append((depth, rgba, pose))
    return out


def perturb(pose, dt, axis_angle):
    """pose moved by dt (world) and turned about the camera centre by the rotation vector axis_angle (world), as f32"""
    from tests.align_ref import rodrigues
    P = np.asarray(pose, np.float64).reshape(3, 4).copy()
    P[:, :3] = rodrigues(np.asarray(axis_angle, np.float64)) @ P[:, :3]
    P[:, 3] += np.asarray(dt, np.float64)
    return P.astype(np.float32)


def held_perturbations():
    """(dt, rotation vector) of the starts the tests use; the first is the largest: 17.5 mm and 0.71 degrees"""
    big_t = np.array([0.010, -0.008, 0.0118])           # |.| = 17.5 mm
    big_r = np.radians(0.71) * np.array([0.6, -0.64, 0.48])
    return [(big_t, big_r), (-0.5 * big_t, 0.5 * big_r), (np.array([0.004, 0.006, -0.003]), -0.7 * big_r)]


# the corner scene's alignment: two levels, every iteration taken (eps 0), so that an end is a fixed point
SCENE_PARAMS = dict(levels=[(2, 4), (1, 6)], eps_t=0.0, eps_r=0.0)
# Ten times the distance between the restatement's two fixed points (from the integration pose and from the largest
# perturbation), measured by tests/test_align_cpu.py as 2.8e-8 m and 1.8e-8 rad: what the device may differ by
FIXED_TOL_T, FIXED_TOL_R = 2.9e-7, 1.9e-7


# ---- hand-built volumes: 10 mm voxels, weight 1, SDF in closed form ----------------------------------------------------
HAND_RES = np.float32(0.01)
# voxel 100 / 84 / 124 along x / y / z has its centre on the plane: index % 8 == 4, so one layer of chunks holds the
# voxels within 3.5 voxels of the plane on either side
X0 = np.array([1.005, 0.845, 1.245])
HAND_LAYER = (12, 10, 15)  # the chunk layer of each plane
HAND_SPAN = 7              # chunks along each in-plane axis, from the layer of the other planes upwards
HAND_DELTA = np.array([0.003, -0.002, 0.0025])
HAND_EDGE_VOXELS = 6.0     # pixels whose surface point is closer than this to a second plane are masked


def _chunk(cid, fn):
    i = np.arange(8)
    z, y, x = np.meshgrid(i, i, i, indexing="ij")  # voxel = x + 8 y + 64 z
    c = np.stack([(cid[0] * 8 + x + 0.5), (cid[1] * 8 + y + 0.5), (cid[2] * 8 + z + 0.5)], -1) * float(HAND_RES)
    return fn(c).astype(np.float32).reshape(512)


def _volume(ids, fn):
    ids = np.asarray(sorted(set(ids)), np.int32).reshape(-1, 3)
    sdf = np.stack([_chunk(c, fn) for c in ids])
    return ids, sdf, np.ones_like(sdf), np.zeros((len(ids), 2048), np.uint16)


def hand_corner(drop=None):
    """(ids, sdf, weight, colour) of the corner sdf = min(x - x0, y - y0, z - z0): one layer of chunks behind each of the
    three faces; drop = a chunk id to leave out"""
    ids = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for i in range(HAND_SPAN):
            for j in range(HAND_SPAN):
                cid = [0, 0, 0]
                cid[a], cid[b], cid[c] = HAND_LAYER[a], HAND_LAYER[b] + i, HAND_LAYER[c] + j
                ids.append(tuple(cid))
    if drop is not None:
        ids = [c for c in ids if c != tuple(drop)]
    return _volume(ids, lambda p: (p - X0).min(-1))


def hand_plane():
    """one plane alone, sdf = x - x0: the normal equations have rank 3"""
    ids = [(HAND_LAYER[0], HAND_LAYER[1] + i, HAND_LAYER[2] + j) for i in range(HAND_SPAN) for j in range(HAND_SPAN)]
    return _volume(ids, lambda p: p[..., 0] - X0[0])


def hand_pose():
    """looking into the corner along (-1, -1, -1) from 0.38 m"""
    f = -np.ones(3) / math.sqrt(3.0)
    right = np.cross([0.0, 1.0, 0.0], f)
    right /= np.linalg.norm(right)
    down = np.cross(f, right)
    R = np.stack([right, down, f], 1)
    t = X0 - 0.38 * f + np.array([0.01, -0.015, 0.02])
    return np.concatenate([R, t[:, None]], 1).astype(np.float32)


def hand_depth(pose, cam=CAM, planes=3, edge_voxels=HAND_EDGE_VOXELS):
    """z-depth of the corner (planes = 3) or of the plane x = x0 alone (planes = 1) from pose, rendered analytically; 0 where
    the ray misses or where the surface point is closer than edge_voxels voxels to a second plane"""
    P = np.asarray(pose, np.float64).reshape(3, 4)
    d = rays(cam) @ P[:, :3].T
    o = P[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d < 0, (X0 - o) / d, np.inf)[..., :planes]
    s = t.min(-1)
    hit = o + d * np.where(np.isfinite(s), s, 0.0)[..., None]
    dist = np.sort(hit - X0, -1)  # the smallest is the plane hit (0); the second the distance to the nearest edge
    ok = np.isfinite(s) & (s > 0)
    if planes == 3:
        ok &= dist[..., 1] >= edge_voxels * float(HAND_RES)
    return np.where(ok, s, 0.0).astype(np.float32)
