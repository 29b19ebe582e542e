"""Inputs of the gated projective-ICP tests (a helper, not a test module): the unmasked corner, the true plane of every pixel,
and a hand-built fronto-parallel plane that puts one case each at the gate's decision edges.

The plane: depth 1.0 in every pixel (a power of two: every product with it is exact), frame pose and model pose the
identity, the model maps the plane itself with the normal (0, 0, -1) that faces the camera.  There a = (ax, 0, 0),
b = (0, by, 0), so n = (0, 0, -by ax) exactly, nw = n, d = by ax, and d d == l2 m2 exactly: the pair passes at cosine 1.
Every case sits at a centre pixel whose coordinates are multiples of 8 (sampled at strides 1, 2 and 4), the depth it changes
at centre +- stride, so the image depends on the stride."""
import numpy as np

from tests.align_inputs import CAM, hand_depth, hand_pose
from tests.align_icp_inputs import hand_model_maps
from texturefusion_amd import synth

F = np.float32
CAM_ODD = synth.Camera(152, 116, 131.25, 131.25, 75.5, 57.5)  # no multiple of 8 * stride for stride 2 and 4: partial tiles
EYE = np.eye(3, 4, dtype=np.float32)
JUMP = F(0.125)  # a power of two: 1.0 + JUMP and the float above it differ from 1.0 by exactly JUMP and JUMP + 2^-23

# centre -> (side, the neighbour's depth): side is the offset in strides
DEPTH_CASES = {
    "zero": ((16, 56), (1, 0), F(0.0)),
    "nan": ((40, 56), (-1, 0), F(np.nan)),
    "inf": ((64, 56), (0, -1), F(np.inf)),
    "below_min": ((88, 56), (0, 1), F(0.04)),
    "above_max": ((112, 56), (1, 0), F(5.5)),
    "jump_exact": ((136, 56), (1, 0), F(1.0) + JUMP),
    "jump_next": ((16, 32), (1, 0), np.nextafter(F(1.0) + JUMP, F(2.0))),
    "jump_far": ((40, 32), (-1, 0), F(3.0)),
}
# centre -> the model normal at that model pixel
MODEL_CASES = {"perpendicular": ((64, 32), (1.0, 0.0, 0.0)), "away": ((88, 32), (0.0, 0.0, 1.0)), "miss": ((112, 32), (0.0, 0.0, 0.0))}
PLAIN = (136, 32)  # an interior pixel nothing touches

# the gates the plane is evaluated under, and the flags each case's centre must show (PLAIN shows 63 under all of them)
GATES = {
    "default_cos": dict(min_normal_cos=F(0.9396926), max_depth_jump=JUMP),
    "no_jump_test": dict(min_normal_cos=F(0.9396926), max_depth_jump=F(np.inf)),
    "cos_0": dict(min_normal_cos=F(0.0), max_depth_jump=JUMP),
    "cos_1": dict(min_normal_cos=F(1.0), max_depth_jump=JUMP),
}
_BAD = dict(zero=15, nan=15, inf=15, below_min=15, above_max=15)
EXPECT = {
    # a step of JUMP over one stride is far steeper than 20 degrees: the normal exists (16) and is not compatible
    "default_cos": dict(_BAD, jump_exact=31, jump_next=15, jump_far=15, perpendicular=31, away=31, miss=3),
    "no_jump_test": dict(_BAD, jump_exact=31, jump_next=31, jump_far=31, perpendicular=31, away=31, miss=3),
    # cosine 0: every normal with d > 0 passes; d == 0 (perpendicular) and d < 0 (away) do not
    "cos_0": dict(_BAD, jump_exact=63, jump_next=15, jump_far=15, perpendicular=31, away=31, miss=3),
    "cos_1": dict(_BAD, jump_exact=31, jump_next=15, jump_far=15, perpendicular=31, away=31, miss=3),
}


def plane(cam, stride):
    """(depth [H, W], V [3, H, W], N [3, H, W]) of the hand-built plane for this stride"""
    H, W = cam.height, cam.width
    depth = np.ones((H, W), np.float32)
    for (cx, cy), (sx, sy), z in DEPTH_CASES.values():
        depth[cy + sy * stride, cx + sx * stride] = z
    fxi, fyi, cxs, cys = F(int(cam.fx)), F(int(cam.fy)), F(int(cam.cx)) + F(0.5), F(int(cam.cy)) + F(0.5)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    V = np.stack([(xx.astype(np.float32) - cxs) / fxi, (yy.astype(np.float32) - cys) / fyi, np.ones((H, W), np.float32)])
    N = np.zeros((3, H, W), np.float32)
    N[2] = -1.0
    for (cx, cy), n in MODEL_CASES.values():
        N[:, cy, cx] = n
    return depth, np.ascontiguousarray(V, np.float32), N


def centres():
    out = {k: v[0] for k, v in DEPTH_CASES.items()}
    out.update({k: v[0] for k, v in MODEL_CASES.items()})
    return out


def border_masks(cam, stride):
    """(sampled, inner): the sampled pixels, and those of them whose four neighbours at +- stride lie inside the image"""
    H, W = cam.height, cam.width
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sampled = (yy % stride == 0) & (xx % stride == 0)
    inner = sampled & (xx - stride >= 0) & (xx + stride < W) & (yy - stride >= 0) & (yy + stride < H)
    return sampled, inner


def corner_unmasked(cam=CAM):
    """the hand-built corner from hand_pose() with no edge mask: a depth in every pixel, the edges in the image"""
    return hand_depth(hand_pose(), cam, edge_voxels=0.0)


def true_axis(cam=CAM):
    """the axis of the plane each pixel of the frame really lies on: read from the analytic maps at the true pose"""
    return hand_model_maps(hand_pose(), cam)[1].argmax(0)
