"""Projective ICP without a GPU: the capture range of the numpy restatement (tests/align_icp_ref.py) on the hand-built corner
against tf_align_frame's, a known answer, every flag on hand-made pixels, degenerate scenes and the ABI."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import align_icp_inputs as II
from tests import align_icp_ref as K
from tests import align_inputs as I
from tests import align_ref as R
from tests.raycast_ref import RefVolume
from texturefusion_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++")
F = np.float32


@pytest.fixture(scope="module")
def frame():
    return I.hand_pose(), I.hand_depth(I.hand_pose())


# ---- 1. capture range ----------------------------------------------------------------------------------------------------
def test_the_sdf_alignment_does_not_capture_the_far_starts(frame):
    """the premise: tf_align_frame restated ends SINGULAR from 40 mm / 2 deg and TOO_FEW from 80 mm / 5 deg"""
    true, depth = frame
    ids, s, w, c = I.hand_corner()
    ref = RefVolume(ids, s, w, c, I.HAND_RES)
    res, log = R.align(ref, depth, II.ladder_start(0.040, 2.0), I.CAM, R.params())
    assert res["status"] == R.SINGULAR and len(log) == 1 and log[0]["n_valid"] == 124
    assert np.array_equal(res["pose"], II.ladder_start(0.040, 2.0))
    res, log = R.align(ref, depth, II.ladder_start(*II.TRACK_START), I.CAM, R.params())
    assert res["status"] == R.TOO_FEW and log[0]["n_valid"] == 0
    # ... while a raycast from that start sees the hand-built layers in every pixel: tf_track_frame's device test can
    # render its model from there
    cam = I.CAM
    hits = ref.raycast_depth(II.ladder_start(*II.TRACK_START), cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, 0.05, 5.0, 1024)
    assert (hits > 0).sum() == cam.width * cam.height >= 100


def test_capture_range(frame):
    """from 80 mm / 5 deg and 120 mm / 8 deg, maps rendered at the start pose and at the true pose: the true pose, every
    pixel with depth valid at the end"""
    true, depth = frame
    n_depth = int((depth > 0).sum())
    assert n_depth == 10357
    worst_t = worst_r = 0.0
    for metres, degrees in ((0.080, 5.0), (0.120, 8.0)):
        start = II.ladder_start(metres, degrees)
        for at in (start, true):
            V, N = II.hand_model_maps(at)
            res, log = K.align(depth, start, V, N, at, I.CAM, K.params())
            dt, dr = R.pose_distance(res["pose"], true)
            dt64, dr64 = R.pose_distance(log[-1]["pose"], true)
            worst_t, worst_r = max(worst_t, dt64), max(worst_r, dr64)
            print("%.0f mm / %.0f deg, maps at the %s pose: status %d, %d evaluations, f32 end %.3g m %.3g rad, f64 end %.3g m "
                  "%.3g rad" % (1e3 * metres, degrees, "start" if at is start else "true", res["status"], len(log), dt, dr,
                                dt64, dr64))
            assert res["status"] == R.CONVERGED
            assert dt <= II.ICP_TOL_T and dr <= II.ICP_TOL_R
            assert res["n_valid_last"] == n_depth == log[-1]["n_valid"]
    # (the provenance of ICP_TOL_*: ten times these, rounded up in the second digit)
    print("largest f64 end distance: %.3g m, %.3g rad" % (worst_t, worst_r))


# ---- 2. one step from a small displacement --------------------------------------------------------------------------------
def test_one_step_returns_the_true_pose(frame):
    true, depth = frame
    V, N = II.hand_model_maps(true)
    start = I.perturb(true, I.HAND_DELTA, np.zeros(3))
    res, log = K.align(depth, start, V, N, true, I.CAM, K.params(levels=[(1, 1)], huber=0.0))
    dt, dr = R.pose_distance(res["pose"], true)
    print("one step: dt %.3g m, dr %.3g rad, valid %d" % (dt, dr, log[0]["n_valid"]))
    assert res["status"] == R.MAX_ITERS and res["evaluations"] == 2
    assert dt <= 1e-5 and dr <= 1e-5
    assert np.abs(log[0]["xi"][:3] + I.HAND_DELTA).max() <= 1e-5 and np.abs(log[0]["xi"][3:]).max() <= 1e-5


# ---- 3. flags on hand-made pixels -----------------------------------------------------------------------------------------
# fx = fy = 16, cx + 0.5 = 7.5, cy + 0.5 = 5.5: with z = 1 and identity poses every product below is exact in f32
TINY = synth.Camera(16, 12, 16.0, 16.0, 7.0, 5.0)
EYE = np.eye(3, 4, dtype=np.float32)


def _pixel(x, y, z=1.0, tm=(0.0, 0.0, 0.0), hit=True, dv=(0.0, 0.0, 0.0), at=None, **kw):
    """(flags, assoc, r) of pixel (x, y) with depth z under the identity pose, the model camera at tm (no rotation).  The
    model maps hold, at pixel `at` (default: where the point projects by hand: (x, y) moved by -16 tm.xy / z), the point
    itself moved by dv and the normal (0, 0, 1) (hit) or 0 (miss)."""
    H, W = TINY.height, TINY.width
    depth = np.zeros((H, W), np.float32)
    depth[y, x] = z
    M = EYE.copy()
    M[:, 3] = tm
    pw = np.array([(x - 7.5) / 16.0 * z, (y - 5.5) / 16.0 * z, z])
    V, N = np.zeros((3, H, W), np.float32), np.zeros((3, H, W), np.float32)
    if at is None:
        at = (x, y) if not (np.isfinite(z) and z > 0) else (int(round(x - 16.0 * tm[0] / z)), int(round(y - 16.0 * tm[1] / z)))
    if 0 <= at[0] < W and 0 <= at[1] < H:
        V[:, at[1], at[0]] = pw + np.asarray(dv)
        N[2, at[1], at[0]] = 1.0 if hit else 0.0
    p = K.params(min_depth=0.05, max_depth=5.0, max_distance=0.1, max_residual=1.0)
    p.update(kw)
    rw = K.rows(depth, EYE, V, N, M, TINY, 1, p)
    others = np.ones((H, W), bool)
    others[y, x] = False
    assert not rw["flags"][others].any() and (rw["assoc"][others] == -1).all() and not rw["r"][others].any()
    return int(rw["flags"][y, x]), int(rw["assoc"][y, x]), float(rw["r"][y, x])


def test_flags_depth_range():
    assert _pixel(3, 4) == (15, 4 * 16 + 3, 0.0)
    for z in (0.0, 0.04, 5.5, np.nan, np.inf, -1.0):
        assert _pixel(3, 4, z=z) == (0, -1, 0.0), z
    # the bounds are inside (at z = min_depth the point is not above min_depth in the model camera: bit 1 stays clear)
    assert _pixel(3, 4, z=0.05) == (1, -1, 0.0) and _pixel(3, 4, z=5.0)[0] == 15


def test_flags_behind_the_model_camera():
    assert _pixel(3, 4, tm=(0.0, 0.0, 2.0)) == (1, -1, 0.0)     # pm.z = -1
    assert _pixel(3, 4, tm=(0.0, 0.0, 1.0)) == (1, -1, 0.0)     # pm.z = 0: not above min_depth, no division looked at
    assert _pixel(3, 4, tm=(0.0, 0.0, 0.95)) == (1, -1, 0.0)    # pm.z = 0.05 is not above min_depth = 0.05


def test_flags_projection_at_the_four_borders():
    px = 1.0 / 16.0  # one pixel at z = 1
    # left: pixel x = 0 moved by 0.4 of a pixel stays in column 0, by 0.6 leaves
    assert _pixel(0, 4, tm=(0.4 * px, 0.0, 0.0), at=(0, 4))[:2] == (15, 4 * 16 + 0)
    assert _pixel(0, 4, tm=(0.6 * px, 0.0, 0.0)) == (1, -1, 0.0)
    # right
    assert _pixel(15, 4, tm=(-0.4 * px, 0.0, 0.0), at=(15, 4))[:2] == (15, 4 * 16 + 15)
    assert _pixel(15, 4, tm=(-0.6 * px, 0.0, 0.0)) == (1, -1, 0.0)
    # top
    assert _pixel(3, 0, tm=(0.0, 0.4 * px, 0.0), at=(3, 0))[:2] == (15, 3)
    assert _pixel(3, 0, tm=(0.0, 0.6 * px, 0.0)) == (1, -1, 0.0)
    # bottom
    assert _pixel(3, 11, tm=(0.0, -0.4 * px, 0.0), at=(3, 11))[:2] == (15, 11 * 16 + 3)
    assert _pixel(3, 11, tm=(0.0, -0.6 * px, 0.0)) == (1, -1, 0.0)


def test_flags_projection_on_a_rounding_boundary():
    """the model camera half a pixel to the left: the point projects to u + 0.5 exactly, which rounds up (floor(. + 0.5))"""
    half = 0.5 / 16.0
    assert _pixel(3, 4, tm=(-half, 0.0, 0.0), at=(4, 4))[:2] == (15, 4 * 16 + 4)
    assert _pixel(3, 4, tm=(0.0, -half, 0.0), at=(3, 5))[:2] == (15, 5 * 16 + 3)
    assert _pixel(15, 4, tm=(-half, 0.0, 0.0)) == (1, -1, 0.0)   # ... and out of the image from the last column
    assert _pixel(0, 4, tm=(half, 0.0, 0.0), at=(0, 4))[:2] == (15, 4 * 16 + 0)  # -0.5 rounds up to 0


def test_flags_model_miss():
    assert _pixel(3, 4, hit=False) == (3, 4 * 16 + 3, 0.0)


def test_flags_distance_gate():
    fl, _, r = _pixel(3, 4, dv=(0.0, 0.0, 0.0999))
    assert fl == 15 and abs(r + 0.0999) < 1e-6
    fl, _, r = _pixel(3, 4, dv=(0.0, 0.0, 0.1001))
    assert fl == 7 and abs(r + 0.1001) < 1e-6   # r is written where the model pixel is a hit
    # the gate is on |e|, not on r: a point 0.1001 off inside the plane has r = 0
    assert _pixel(3, 4, dv=(0.1001, 0.0, 0.0)) == (7, 4 * 16 + 3, 0.0)
    # |e|^2 == max_distance^2 exactly is inside
    e = F(1.0) - F(0.9)
    assert _pixel(3, 4, dv=(0.0, 0.0, -0.1), max_distance=e)[0] == 15
    assert _pixel(3, 4, dv=(0.0, 0.0, -0.1), max_distance=np.nextafter(e, F(0)))[0] == 7


def test_flags_residual_gate_below_the_distance_gate():
    e = F(1.0) - F(0.95)  # r as the rows form it: 1 * (1 - f32(0.95))
    fl, _, r = _pixel(3, 4, dv=(0.0, 0.0, -0.05), max_residual=e)
    assert fl == 15 and F(r) == e
    assert _pixel(3, 4, dv=(0.0, 0.0, -0.05), max_residual=np.nextafter(e, F(0)))[0] == 7


def test_rows_at_a_stride_leave_the_other_pixels_alone(frame):
    true, depth = frame
    V, N = II.hand_model_maps(true)
    rw = K.rows(depth, II.ladder_start(0.040, 2.0), V, N, true, I.CAM, 3, K.params())
    m = np.zeros(depth.shape, bool)
    m[::3, ::3] = True
    assert not rw["flags"][~m].any() and (rw["assoc"][~m] == -1).all() and (rw["flags"][m] == 15).sum() > 500
    assert len(rw["fl"]) == 40 * 54


# ---- 4. degenerate scenes -------------------------------------------------------------------------------------------------
def test_one_plane_alone_is_singular():
    true = I.hand_pose()
    depth = I.hand_depth(true, planes=1)
    V, N = II.hand_model_maps(true, planes=1)
    res, log = K.align(depth, I.perturb(true, I.HAND_DELTA, np.zeros(3)), V, N, true, I.CAM, K.params())
    assert res["status"] == R.SINGULAR and len(log) == 1 and log[0]["n_valid"] >= 100


def test_an_empty_depth_image_is_too_few(frame):
    true, depth = frame
    V, N = II.hand_model_maps(true)
    res, log = K.align(np.zeros_like(depth), true, V, N, true, I.CAM, K.params())
    assert res["status"] == R.TOO_FEW and len(log) == 1 and log[0]["n_valid"] == 0 and np.array_equal(res["pose"], true)


# ---- 5. ABI ---------------------------------------------------------------------------------------------------------------
ICP_SYMBOLS = ("tf_align_icp_default_params", "tf_align_frame_icp", "tf_align_frame_icp_device", "tf_align_icp_log",
               "tf_align_icp_residuals", "tf_align_icp_residuals_device", "tf_track_frame")


def test_icp_symbols_are_exported_and_bound():
    L = capi.lib()
    for s in ICP_SYMBOLS:
        assert s in capi.SYMBOLS and hasattr(L, s) and getattr(L, s).argtypes is not None, s
    for m in ("align_frame_icp", "align_frame_icp_device", "align_icp_log", "align_icp_residuals", "track_frame"):
        assert callable(getattr(capi.Volume, m))


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_struct_sizes_match_a_compiled_probe(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tf_fusion.h"\nint main() {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(tf_align_icp_params), offsetof(tf_align_icp_params, max_distance),\n'
                   '         offsetof(tf_align_icp_params, ray_max_steps), sizeof(tf_track_result), offsetof(tf_track_result, stage),\n'
                   '         offsetof(tf_track_result, pose));\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    r = subprocess.run([CXX, "-std=c++14", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    P, T = capi.AlignIcpParamsC, capi.TrackResult
    assert got == [C.sizeof(P), P.max_distance.offset, P.ray_max_steps.offset, C.sizeof(T), T.stage.offset, T.pose.offset]
    assert C.sizeof(P) == 68 + 16 and C.sizeof(T) == 2 * 76 + 4 + 48


def test_default_params_round_trip():
    p = capi.AlignIcpParams()
    g = p.geo
    assert g.n_levels == 3 and list(g.stride)[:3] == [4, 2, 1] and list(g.iters)[:3] == [6, 4, 3]
    assert (g.min_depth, g.max_depth, g.damping, g.min_valid) == (F(0.05), F(5.0), 0.0, 100)
    assert (g.max_residual, g.huber, g.eps_t, g.eps_r) == (F(0.15), F(0.02), F(1e-5), F(1e-5))
    assert (p.max_distance, p.ray_near, p.ray_far, p.ray_max_steps) == (F(0.15), F(0.05), F(5.0), 1024)
    d = K.params()
    assert d["levels"] == [(4, 6), (2, 4), (1, 3)] and F(d["max_distance"]) == p.max_distance and F(d["huber"]) == g.huber
    q = capi.AlignIcpParams(levels=[(3, 2)], max_distance=0.3, huber=0.0, ray_max_steps=64, min_valid=7)
    assert q.geo.n_levels == 1 and q.geo.stride[0] == 3 and q.geo.iters[0] == 2 and q.max_distance == F(0.3)
    assert q.geo.huber == 0.0 and q.ray_max_steps == 64 and q.geo.min_valid == 7
    with pytest.raises(TypeError):
        capi.AlignIcpParams(no_such_field=1)
    assert capi.lib().tf_align_icp_default_params(None) == capi.TF_ERR_INVALID


def test_invalid_arguments_are_refused_ahead_of_the_device():
    """the checks that come before the handle is touched return TF_ERR_INVALID without a GPU"""
    L = capi.lib()
    res, trk = capi.AlignResult(), capi.TrackResult()
    p, sp = capi.AlignIcpParams(), capi.AlignParams()
    z = (C.c_float * 12)()
    assert L.tf_align_frame_icp(None, z, z, None, C.byref(p), C.byref(res)) == capi.TF_ERR_INVALID
    assert L.tf_align_frame_icp_device(None, None, z, None, None, z, C.byref(p), None) == capi.TF_ERR_INVALID
    assert L.tf_track_frame(None, z, z, C.byref(p), C.byref(sp), C.byref(trk)) == capi.TF_ERR_INVALID
    n = C.c_int64(5)
    assert L.tf_align_icp_log(None, None, 0, C.byref(n)) == capi.TF_ERR_INVALID
