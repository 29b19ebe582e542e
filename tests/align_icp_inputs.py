"""Inputs of the projective-ICP tests (a helper, not a test module): analytic model maps of the hand-built corner from any
pose, the ladder of far starts, and the tolerances the tests hold the end pose to."""
import numpy as np

from tests.align_inputs import CAM, X0, hand_pose, perturb, rays

# the direction the ladder's starts are moved along and the rotation-vector direction they are turned about
LADDER_DIR_T = np.array([0.6, 0.53, 0.6]) / np.linalg.norm([0.6, 0.53, 0.6])
LADDER_DIR_R = np.array([0.6, -0.64, 0.48]) / np.linalg.norm([0.6, -0.64, 0.48])
LADDER = [(0.040, 2.0), (0.060, 3.0), (0.080, 5.0), (0.120, 8.0)]  # (metres, degrees)


def ladder_start(metres, degrees, pose=None):
    """hand_pose() (or pose) moved by `metres` along LADDER_DIR_T and turned by `degrees` about LADDER_DIR_R, as f32"""
    return perturb(hand_pose() if pose is None else pose, metres * LADDER_DIR_T, np.radians(degrees) * LADDER_DIR_R)


def hand_model_maps(pose, cam=CAM, planes=3):
    """(vertex, normal) f32 [3, H, W], world frame, of the corner (planes = 3) or of the plane x = x0 alone (planes = 1) as a
    raycast from pose would write them were it exact: the hit point, the hit plane's +axis normal, 0 on a miss.  No edge
    mask: a model map has a surface wherever a ray meets one."""
    P = np.asarray(pose, np.float64).reshape(3, 4)
    d = rays(cam) @ P[:, :3].T
    o = P[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d < 0, (X0 - o) / d, np.inf)[..., :planes]
    s = t.min(-1)
    ax = t.argmin(-1)
    ok = np.isfinite(s) & (s > 0)
    hit = o + d * np.where(ok, s, 0.0)[..., None]
    for a in range(planes):  # the hit lies on its plane exactly
        hit[..., a] = np.where(ax == a, X0[a], hit[..., a])
    nrm = np.eye(3)[ax]
    V = np.where(ok[..., None], hit, 0.0).astype(np.float32).transpose(2, 0, 1)
    N = np.where(ok[..., None], nrm, 0.0).astype(np.float32).transpose(2, 0, 1)
    return np.ascontiguousarray(V), np.ascontiguousarray(N)


# Ten times the largest distance between hand_pose() and the restatement's end pose over the 80 mm / 5 deg and the
# 120 mm / 8 deg starts, with the analytic maps rendered at the start pose and at the true pose, default parameters
# (tests/test_align_icp_cpu.py::test_capture_range prints them), taken on the f64 pose of the closing evaluation:
# 8.1e-8 m and 1.9e-7 rad at most.  The factor ten is for the f32 rounding of the pose between steps and of the result.
ICP_TOL_T, ICP_TOL_R = 8.1e-7, 1.9e-6

# tf_track_frame's device test starts from the 80 mm / 5 deg rung on the hand-built corner itself: every one of the 19 200
# rays of that start (and of every other rung) hits the hand-built layers (raycast_ref.RefVolume.raycast_depth, asserted by
# tests/test_align_icp_cpu.py), far more than min_valid, so the model can be raycast from there and no fused scene is needed;
# tf_align_frame alone finds no valid pixel from that rung.
TRACK_START = (0.080, 5.0)
