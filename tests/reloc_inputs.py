"""Inputs of the relocalisation tests (a helper, not a test module): the hand-built corner of tests/align_inputs.py seen from
a handful of keyframe poses that lie far apart, with a smooth colour painted on its faces so that the small images differ,
and the queries: keyframe poses moved by rungs of the ICP ladder."""
import math

import numpy as np

from tests.align_icp_inputs import LADDER_DIR_R, LADDER_DIR_T, hand_model_maps
from tests.align_inputs import CAM, HAND_LAYER, HAND_RES, HAND_SPAN, X0, hand_depth, perturb

# (tilt of the view axis away from the corner's diagonal, degrees; the direction of the tilt, degrees about the diagonal;
# roll about the view axis, degrees; distance from the corner, metres)
# (the third view stands 6 cm further back: from 0.36 m its 8 cm / 5 degree query, whose move happens to run along the image,
# scores its own keyframe at 955 and the first view's at 927; the descriptor has no invariance to such a shift, so the scene
# keeps its distance.  tests/test_reloc_cpu.py prints every margin.)
KEYFRAME_VIEWS = [(24.0, 0.0, 0.0, 0.36), (24.0, 120.0, 0.0, 0.36), (24.0, 240.0, 0.0, 0.42),
                  (0.0, 0.0, 35.0, 0.34), (0.0, 0.0, -35.0, 0.34)]
# Keyframes the tracker cannot start from: more than a metre further out.  On this scene the ICP returns to the true pose
# from every view above (40 to 70 degrees off; tests/test_reloc_cpu.py), so "far" has to mean that a frame's points, put
# into the world by the keyframe's pose, lie beyond the ICP's distance gate of every surface.
FAR_VIEWS = [(0.0, 0.0, 0.0, 1.50), (10.0, 120.0, 0.0, 1.40)]
QUERY_RUNGS = [(0.040, 2.0), (0.080, 5.0)]  # the ICP ladder's rungs the queries are moved by
MIN_APART_T, MIN_APART_R = 0.30, 20.0       # keyframes are at least this far from each other: metres OR degrees
# pixels whose surface point is closer than this to a second face are holes (align_inputs masks 6 voxels, which from these
# distances leaves a quarter to a half of the image: below tf_relocalise's default min_valid_fraction)
EDGE_VOXELS = 2.0


def _rot(axis, deg):
    from tests.align_ref import rodrigues
    a = np.asarray(axis, np.float64)
    return rodrigues(math.radians(deg) * a / np.linalg.norm(a))


def view_pose(tilt, about, roll, dist):
    """camera-to-world pose [3, 4] f32 looking into the corner: the diagonal view of align_inputs.hand_pose, its axis tilted,
    rolled, at dist from the corner along the axis"""
    diag = -np.ones(3) / math.sqrt(3.0)
    side = np.cross([0.0, 1.0, 0.0], diag)
    side = _rot(diag, about) @ (side / np.linalg.norm(side))
    f = _rot(side, tilt) @ diag
    right = np.cross([0.0, 1.0, 0.0], f)
    right /= np.linalg.norm(right)
    down = np.cross(f, right)
    R = _rot(f, roll) @ np.stack([right, down, f], 1)
    t = X0 - dist * f
    return np.concatenate([R, t[:, None]], 1).astype(np.float32)


def keyframe_poses():
    return [view_pose(*v) for v in KEYFRAME_VIEWS]


def far_poses():
    return [view_pose(*v) for v in FAR_VIEWS]


def apart(a, b):
    """(metres, degrees) between two poses"""
    A, B = np.asarray(a, np.float64).reshape(3, 4), np.asarray(b, np.float64).reshape(3, 4)
    c = (np.trace(A[:, :3].T @ B[:, :3]) - 1.0) / 2.0
    return float(np.linalg.norm(A[:, 3] - B[:, 3])), math.degrees(math.acos(min(1.0, max(-1.0, c))))


def query_pose(k, rung):
    """keyframe k's pose moved by QUERY_RUNGS[rung] along the ladder's directions"""
    m, deg = QUERY_RUNGS[rung]
    return perturb(keyframe_poses()[k], m * LADDER_DIR_T, np.radians(deg) * LADDER_DIR_R)


def all_rays_hit(pose, cam=CAM):
    """every ray from pose meets a face of the corner inside the hand-built layers, a voxel away from their rim at least: a
    raycast of the volume from there has a hit in every pixel"""
    V, N = hand_model_maps(pose, cam)
    if not (np.abs(N).sum(0) == 1.0).all():
        return False
    lo = np.asarray(HAND_LAYER, np.float64) * 8 * float(HAND_RES) + float(HAND_RES)
    hi = (np.asarray(HAND_LAYER, np.float64) + HAND_SPAN) * 8 * float(HAND_RES) - float(HAND_RES)
    P = V.astype(np.float64)
    return bool(all(((P[a] >= lo[a]) & (P[a] <= hi[a])).all() for a in range(3)))


def paint(pose, cam=CAM):
    """rgb u8 [H, W, 3]: a smooth function of the world point each ray meets"""
    V, _ = hand_model_maps(pose, cam)
    p = V.astype(np.float64) - X0[:, None, None]
    r = 128.0 + 110.0 * np.sin(7.0 * p[0] + 11.0 * p[1] + 0.3)
    g = 128.0 + 110.0 * np.sin(9.0 * p[1] - 8.0 * p[2] + 1.1)
    b = 128.0 + 110.0 * np.cos(10.0 * p[2] + 6.0 * p[0] - 0.7)
    return np.ascontiguousarray(np.clip(np.rint(np.stack([r, g, b], -1)), 0, 255).astype(np.uint8))


def frame(pose, cam=CAM):
    """(depth f32 [H, W] with the pixels near an edge of the corner masked as holes, rgb u8 [H, W, 3]) from pose"""
    return hand_depth(pose, cam, edge_voxels=EDGE_VOXELS), paint(pose, cam)


def rgba(rgb, alpha=255):
    """the same image with a pixel stride of 4"""
    out = np.full(rgb.shape[:2] + (4,), alpha, np.uint8)
    out[..., :3] = rgb
    return out


def pose_inv16(pose):
    """f32 of the inverse of [R t; 0 1] computed in f64: what tf_keyframe_set_pose takes"""
    T = np.eye(4)
    T[:3] = np.asarray(pose, np.float64).reshape(3, 4)
    return np.linalg.inv(T).astype(np.float32)


def rigid_inverse(T16):
    """tf_relocalise's pose of a keyframe: [R^T | -R^T t] of the stored f32 matrix, in f64, rounded to f32"""
    T = np.asarray(T16, np.float32).reshape(4, 4).astype(np.float64)
    out = np.zeros((3, 4), np.float32)
    for r in range(3):
        out[r, :3] = T[:3, r]
        out[r, 3] = np.float32(-((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3]))
    return out
