"""Inputs of the colour-ICP tests (a helper, not a test module): the textured hand plane of align_color_inputs.py seen from
far off its truncation band's capture range, the hand-built corner with the same texture in its voxels, analytic model maps
for both (align_icp_inputs.hand_model_maps), and the hand-built maps that put one pixel at each decision edge of the
photometric row."""
import numpy as np

from tests import align_color_inputs as CI
from tests import align_icp_inputs as II
from tests import align_inputs as I
from tests.raycast_ref import RefVolume
from tests.align_icp_gate_inputs import CAM_ODD  # 152 x 116: the last tiles of a row and of a column are partial

CAM = I.CAM

# the plane x = x0: y and z lie in it, x is its normal
IN_PLANE = np.array([0.0, 0.6, 0.8])
# (in-plane offset in metres, degrees about the normal) of the starts; the last is the one with a rotation
PLANE_RUNGS = [(0.010, 0.0), (0.020, 0.0), (0.030, 0.0), (0.010, 0.3)]

# Measured by tests/test_align_icp_color_cpu.py with the restatement (tests/align_icp_color_ref.py), default parameters,
# analytic model maps rendered at the start.  Textured hand plane, the four rungs above: every rung holds (status
# CONVERGED, the in-plane error far below a tenth of the offset); the ends lie at most 8.82e-5 m and 2.81e-4 rad from the
# true pose (the trilinear field's smoothing of the texture, the u8 rounding of the frame and the first-order model about
# the nearest model pixel: an offset, not noise) and at most 5.02e-6 m and 2.23e-5 rad from one another.  The tests allow twice each.
PLANE_TRUTH_T, PLANE_TRUTH_R = 8.82e-5, 2.81e-4
PLANE_SPREAD_T, PLANE_SPREAD_R = 5.02e-6, 2.23e-5
PLANE_HELD = 4  # rungs of PLANE_RUNGS the restatement holds, from the first
# Textured hand corner from the 40 mm / 2 degree rung of align_icp_inputs.LADDER: the colour call's end lies 3.84e-5 m and
# 2.17e-4 rad from the plain call's end of the same start (the geometry fixes the pose; the photometric row pulls it by a part
# of its own offset above).  The tests allow twice that.
CORNER_SHIFT_T, CORNER_SHIFT_R = 3.84e-5, 2.17e-4


def ref_of(vol):
    ids, s, w, c = vol
    return RefVolume(ids, s, w, c, I.HAND_RES)


def plane_start(metres, degrees):
    """hand_pose() moved by `metres` along IN_PLANE and turned by `degrees` about the plane's normal, as f32"""
    return I.perturb(I.hand_pose(), metres * IN_PLANE, np.radians(degrees) * np.array([1.0, 0.0, 0.0]))


def plane_frame():
    """(depth, rgba) of the textured plane from hand_pose()"""
    return CI.hand_frame(I.hand_pose())


def plane_maps(pose, cam=CAM):
    return II.hand_model_maps(pose, cam, planes=1)


def corner_textured():
    return CI.textured(I.hand_corner())


def corner_frame(pose=None):
    """(depth, rgba) of the textured corner from pose (hand_pose()), edges masked as align_inputs.hand_depth does"""
    pose = I.hand_pose() if pose is None else pose
    depth = I.hand_depth(pose, CAM, planes=3)
    return depth, CI.texture_rgba(depth, pose, CAM)


def upload(gv, vol):
    ids, s, w, c = vol
    for k in range(len(ids)):
        gv.set_chunk(ids[k], s[k], w[k], c[k])
    gv.sync()


# ---- hand-built cases: a fronto-parallel textured plane seen by the identity pose ------------------------------------------
# Camera at EDGE_POSE looks along -x at the plane x = x0 from EDGE_DIST: model pixel (u, v) hits a point whose y and z vary
# with v and u, so that L varies from pixel to pixel.  The model maps are the analytic ones; single pixels are then edited.
EDGE_DIST = 0.30


def edge_pose():
    """camera 0.30 m in front of the plane's middle, forward = -x, right = -z, as a 3 x 4 f32 pose"""
    f = np.array([-1.0, 0.0, 0.0])
    right = np.array([0.0, 0.0, -1.0])
    down = np.cross(f, right)
    Rm = np.stack([right, down, f], 1)
    mid = np.array([I.X0[0], (I.HAND_LAYER[1] * 8 + 28) * 0.01, (I.HAND_LAYER[2] * 8 + 28) * 0.01])
    t = mid - EDGE_DIST * f
    return np.concatenate([Rm, t[:, None]], 1).astype(np.float32)


def edge_scene(cam=CAM):
    """(depth, rgba, V, N, pose) of the fronto-parallel view: frame and model from the same pose"""
    pose = edge_pose()
    depth = I.hand_depth(pose, cam, planes=1)
    rgba = CI.texture_rgba(depth, pose, cam)
    V, N = II.hand_model_maps(pose, cam, planes=1)
    return depth, rgba, V, N, pose


NO_COUNT = ((12, 14, 19), 4)  # (chunk, voxel index) of the one voxel of edge_volume() whose colour count is 0: on the plane
MISS, JUMP, ALPHA0, RC_PIX, HALF = (40, 30), (100, 40), (60, 80), (50, 90), (90, 70)  # (x, y) of the edited pixels
JUMP_DX = 0.02       # the JUMP model pixel's vertex is moved this far along x: its model depth differs from its neighbours'
RC_GREY = 40         # the RC_PIX frame pixel is this many grey levels brighter


def edge_volume():
    """the textured plane with one voxel's colour count set to 0"""
    ids, s, w, c = CI.hand_plane_textured()
    c = c.copy()
    k = [tuple(i) for i in ids].index(NO_COUNT[0])
    c[k].reshape(512, 4)[NO_COUNT[1], 3] = 0
    return ids, s, w, c


def edge_cases(cam=CAM):
    """edge_scene with the edits: a model pixel that is a miss, one whose depth jumps, a frame pixel with alpha 0, one with a
    large photometric residual.  (Pixels of the first and last column and row, and the voxel without a colour count, need
    no edit.)"""
    depth, rgba, V, N, pose = edge_scene(cam)
    V, N, rgba = V.copy(), N.copy(), rgba.copy()
    N[:, MISS[1], MISS[0]] = 0
    V[0, JUMP[1], JUMP[0]] += np.float32(JUMP_DX)
    rgba[ALPHA0[1], ALPHA0[0], 3] = 0
    rgba[RC_PIX[1], RC_PIX[0], :3] += RC_GREY
    return depth, rgba, V, N, pose


def shifted(pose, right=0.0, down=0.0):
    """pose moved along its own right and down axes, as f32"""
    P = np.asarray(pose, np.float64).reshape(3, 4).copy()
    P[:, 3] += right * P[:, 0] + down * P[:, 1]
    return P.astype(np.float32)


def half_pixel_depth(pose, model_pose, cam, x, y, z0, span=4000):
    """a depth near z0 at which pixel (x, y) of a frame at `pose` projects into the model camera with uc exactly on a half
    (the tie of floorf(uc + 0.5f)), found by walking z over f32 neighbours with the row's own arithmetic; None if there is none"""
    F = np.float32
    P, M = np.asarray(pose, F).reshape(3, 4), np.asarray(model_pose, F).reshape(3, 4)
    fxi, cxs, cys, fyi = F(int(cam.fx)), F(int(cam.cx)) + F(0.5), F(int(cam.cy)) + F(0.5), F(int(cam.fy))
    z = np.full(2 * span + 1, F(z0), F)
    step = np.spacing(F(z0))
    z = (z + step * np.arange(-span, span + 1).astype(F)).astype(F)
    dcx, dcy = (F(x) - cxs) / fxi, (F(y) - cys) / fyi
    pcx, pcy = dcx * z, dcy * z
    q = [(P[r, 0] * pcx + P[r, 1] * pcy) + P[r, 2] * z for r in range(3)]
    d = [(P[r, 3] + q[r]) - M[r, 3] for r in range(3)]
    pm = [(M[0, c] * d[0] + M[1, c] * d[1]) + M[2, c] * d[2] for c in range(3)]
    uc = (fxi * pm[0]) / pm[2] + cxs
    hit = np.nonzero(uc - np.floor(uc) == F(0.5))[0]
    return None if len(hit) == 0 else z[hit[len(hit) // 2]]
