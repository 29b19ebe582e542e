"""Inputs of the group alignment tests (a helper, not a test module): three frames of the hand-built corner of
tests/align_inputs.py, the keyframe's depth masked to one face, and rigid perturbations of a whole group."""
import numpy as np

from tests import align_inputs as I
from tests.align_ref import rodrigues


def hand_group_poses():
    """the keyframe at hand_pose() and two local frames a few centimetres and degrees away"""
    T0 = I.hand_pose()
    T1 = I.perturb(T0, (0.03, -0.02, 0.01), np.radians([3.0, -2.0, 1.0]))
    T2 = I.perturb(T0, (-0.02, 0.03, 0.02), np.radians([-2.0, 3.5, -1.5]))
    return [T0, T1, T2]


def face_depth(pose, face=0, cam=I.CAM):
    """hand_depth(pose) kept only where the ray's surface point lies on the face x_face = x0: a frame facing one plane"""
    P = np.asarray(pose, np.float64).reshape(3, 4)
    d = I.rays(cam) @ P[:, :3].T
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d < 0, (I.X0 - P[:, 3]) / d, np.inf)
    return np.where(t.argmin(-1) == face, I.hand_depth(pose, cam), np.float32(0)).astype(np.float32)


def hand_group(masked=True):
    """(poses, depths) of the three-frame case: each frame's depth rendered at its own true pose; masked: the keyframe
    sees the face x = x0 only (alone it is singular)"""
    poses = hand_group_poses()
    depths = [I.hand_depth(P) for P in poses]
    if masked:
        depths[0] = face_depth(poses[0])
    return poses, depths


def move_group(poses, dt, axis_angle=(0.0, 0.0, 0.0)):
    """every frame moved by one rigid motion: turned about the first frame's camera centre by the rotation vector
    axis_angle (world), then moved by dt (world); as f32"""
    E = rodrigues(np.asarray(axis_angle, np.float64))
    Ps = [np.asarray(P, np.float64).reshape(3, 4) for P in poses]
    c = Ps[0][:, 3].copy()
    out = []
    for P in Ps:
        Q = P.copy()
        Q[:, :3] = E @ P[:, :3]
        Q[:, 3] = c + E @ (P[:, 3] - c) + np.asarray(dt, np.float64)
        out.append(Q.astype(np.float32))
    return out


# the multi-step rigid run: four steps at stride 1, every one taken (eps 0), then the closing evaluation
RIGID_PARAMS = dict(levels=[(1, 4)], huber=0.0, eps_t=0.0, eps_r=0.0)
# its two starts: the true poses moved as one body by HAND_DELTA, and turned by half a degree as well
RIGID_STARTS = [(I.HAND_DELTA, (0.0, 0.0, 0.0)), (I.HAND_DELTA, np.radians(0.5) * np.array([0.6, -0.64, 0.48]))]
# Ten times the distance between the restatement's two ends (the largest over the three frames), measured by
# tests/test_align_group_cpu.py as 2.62e-7 m and 6.58e-7 rad (the poses are rounded to f32 between steps, and the second start carries a rotation): what
# the device's end may differ from the restatement's by
GROUP_TOL_T, GROUP_TOL_R = 2.7e-6, 6.6e-6
