"""Frame-to-model alignment without a GPU: the numpy restatement (tests/align_ref.py) on the hand-built volumes and on
the oracle's volume of the corner scene, tf_align_solve.h on its own against numpy, and the ABI."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import api as O
from tests import align_inputs as I
from tests import align_ref as R
from tests.raycast_ref import RefVolume
from texturefusion_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++")
ONE_STEP = dict(levels=[(1, 1)], huber=0.0, damping=0.0)


def _hand(vol):
    ids, s, w, c = vol
    return RefVolume(ids, s, w, c, I.HAND_RES)


@pytest.fixture(scope="module")
def corner():
    return _hand(I.hand_corner()), I.hand_pose(), I.hand_depth(I.hand_pose())


def test_known_answer_on_the_hand_built_corner(corner):
    """away from the edges the SDF is linear, so xi = (-delta, 0) solves the linearised system exactly: one step from the
    true pose moved by delta returns it (1e-5 m, 1e-5 rad: f32 coordinates near 1-2 m carry 1.2e-7 m, about 20 roundings
    per sample, amplified by cond(A))"""
    ref, pose, depth = corner
    start = pose.astype(np.float64)
    start[:, 3] += I.HAND_DELTA
    res, log = R.align(ref, depth, start.astype(np.float32), I.CAM, R.params(**ONE_STEP))
    dt, dr = R.pose_distance(res["pose"], pose)
    print("known answer: dt %.3g m, dr %.3g rad, cond %.3g, valid %d" % (dt, dr, np.linalg.cond(log[0]["A"]), log[0]["n_valid"]))
    assert res["status"] == R.MAX_ITERS and res["evaluations"] == 2
    assert dt <= 1e-5 and dr <= 1e-5
    assert np.abs(log[0]["xi"][:3] + I.HAND_DELTA).max() <= 1e-5 and np.abs(log[0]["xi"][3:]).max() <= 1e-5
    assert log[0]["n_valid"] > 5000 and res["rms_last"] < 1e-6


def test_single_plane_is_singular_and_returns_the_input_pose(corner):
    _, pose, _ = corner
    ref = _hand(I.hand_plane())
    depth = I.hand_depth(pose, planes=1)
    res, log = R.align(ref, depth, pose, I.CAM, R.params(**ONE_STEP))
    assert res["status"] == R.SINGULAR and len(log) == 1 and log[0]["n_valid"] > 1000
    assert np.array_equal(res["pose"].view(np.uint32), pose.view(np.uint32))
    assert np.linalg.matrix_rank(log[0]["A"], tol=1e-9 * log[0]["A"].diagonal().max()) == 3


def test_empty_volume_reports_too_few(corner):
    _, pose, depth = corner
    ref = RefVolume(np.zeros((0, 3), np.int32), np.zeros((0, 512)), np.zeros((0, 512)), np.zeros((0, 2048)), I.HAND_RES)
    res, log = R.align(ref, depth, pose, I.CAM, R.params(**ONE_STEP))
    assert res["status"] == R.TOO_FEW and len(log) == 1 and log[0]["n_valid"] == 0 and res["rms_first"] == 0
    assert np.array_equal(res["pose"].view(np.uint32), pose.view(np.uint32))


def test_bad_depth_pixels_are_skipped(corner):
    ref, pose, depth = corner
    p = R.params(**ONE_STEP)
    d = depth.copy()
    good = np.argwhere(R.rows(ref, depth, pose, I.CAM, 1, p)["flags"] == 15)
    pick = good[:: len(good) // 8][:8]
    for k, (y, x) in enumerate(pick):
        d[y, x] = (0.0, np.nan, np.inf, -np.inf, -0.3, 0.04, 5.5, 1e30)[k]
    rw = R.rows(ref, d, pose, I.CAM, 1, p)
    for y, x in pick:
        assert rw["flags"][y, x] == 0 and rw["r"][y, x] == 0 and not rw["grad"][:, y, x].any()
    assert R.sums(rw, p)["n_valid"] == len(good) - 8
    assert np.isfinite(R.sums(rw, p)["A21"]).all()


def test_a_tap_in_an_absent_chunk_gives_flags_3(corner):
    """the chunk that holds the centre sample stays, a neighbour one tap reaches is left out"""
    _, pose, depth = corner
    drop = (I.HAND_LAYER[0], I.HAND_LAYER[1] + 2, I.HAND_LAYER[2] + 2)
    ref = _hand(I.hand_corner(drop=drop))
    p = R.params(**ONE_STEP)
    rw = R.rows(ref, depth, pose, I.CAM, 1, p)
    full = R.rows(_hand(I.hand_corner()), depth, pose, I.CAM, 1, p)
    three = (rw["flags"] == 3) & (full["flags"] == 15)
    assert three.sum() > 10
    assert np.all(rw["r"][three] == full["r"][three]) and not rw["grad"][:, three].any()
    sm = R.sums(rw, p)
    assert sm["n_valid"] == int((rw["flags"] == 15).sum()) < R.sums(full, p)["n_valid"]


def test_stride_3_samples_exactly_the_pixels_of_the_rule(corner):
    ref, pose, depth = corner
    p = R.params(**ONE_STEP)
    rw = R.rows(ref, depth, pose, I.CAM, 3, p)
    yy, xx = np.mgrid[0:I.CAM.height, 0:I.CAM.width]
    sampled = (yy % 3 == 0) & (xx % 3 == 0)
    assert len(rw["fl"]) == sampled.sum() == 54 * 40
    assert not rw["flags"][~sampled].any() and not rw["r"][~sampled].any() and not rw["grad"][:, ~sampled].any()
    one = R.rows(ref, depth, pose, I.CAM, 1, p)
    assert np.array_equal(rw["flags"][sampled], one["flags"][sampled])
    assert np.array_equal(rw["r"][sampled].view(np.uint32), one["r"][sampled].view(np.uint32))


@pytest.fixture(scope="module")
def scene():
    frames = I.corner_frames()
    res = np.float32(0.005)
    ov = O.Volume(res, O.camera_from(I.CAM), O.default_integrator())
    for depth, rgba, pose in frames:
        ov.integrate_frame(depth, rgba, pose)
    ref = RefVolume.from_volume(ov, ov.list_chunks(), res)
    ov.close()
    return ref, frames[I.HELD][0], frames[I.HELD][2]


def test_corner_scene_reaches_one_fixed_point(scene):
    """from the integration pose and from 17.5 mm / 0.71 degrees away the restatement ends at the same pose; the distance
    between the two ends is the measurement behind I.FIXED_TOL_T / I.FIXED_TOL_R (ten times it)"""
    ref, depth, pose = scene
    p = R.params(**I.SCENE_PARAMS)
    start = I.perturb(pose, *I.held_perturbations()[0])
    dt0, dr0 = R.pose_distance(start, pose)
    assert 0.017 < dt0 < 0.018 and abs(np.degrees(dr0) - 0.71) < 0.01
    ends = []
    for st in (pose, start):
        res, log = R.align(ref, depth, st, I.CAM, p)
        ends.append(log[-1]["pose"])
        assert res["status"] == R.MAX_ITERS and res["evaluations"] == 11
        assert res["n_valid_last"] >= 0.9 * res["n_sampled"], (res["n_valid_last"], res["n_sampled"])
        assert np.linalg.cond(log[-1]["A"]) < 1e3
        dt, _ = R.pose_distance(res["pose"], pose)
        assert dt < 0.005  # one voxel: the model's zero level is offset from the input depth by a fraction of a voxel
    assert res["rms_last"] < res["rms_first"] / 5, (res["rms_first"], res["rms_last"])
    dt, dr = R.pose_distance(ends[0], ends[1])
    print("fixed points: %.3g m, %.3g rad apart" % (dt, dr))
    assert dt <= I.FIXED_TOL_T and dr <= I.FIXED_TOL_R


# ---- tf_align_solve.h on its own ------------------------------------------------------------------------------------
def _solve_print(tmp_path, extra):
    exe = str(tmp_path / "align_solve_print")
    cmd = [CXX, "-std=c++14", "-O2", "-Wall", "-ffp-contract=off"] + extra + \
          [os.path.join(ROOT, "tests", "cpp_align", "align_solve_print.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    out = {"S": [], "R": [], "U": []}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "S":
            out["S"].append((int(w[1]), np.array([int(x, 16) for x in w[2:]], np.uint64).view(np.float64)))
        else:
            out[w[0]].append(np.array([int(x, 16) for x in w[1:]], np.uint64).view(np.float64))
    return out


def _check_solve_output(out):
    assert len(out["S"]) == 55 and len(out["R"]) == 18 and len(out["U"]) == 6
    n_singular = 0
    for ok, v in out["S"]:
        A21, b, damping, xi = v[:21], v[21:27], v[27], v[28:34]
        A = R.full(A21)
        M = A + damping * np.diag(A.diagonal())
        assert ok == int(R.pivots_ok(M))
        if not ok:
            n_singular += 1
            assert not xi.any()
            continue
        # backward error; Cholesky's bound for n = 6 is about 4e-14, 1e-12 leaves a margin of about 25x
        assert np.linalg.norm(M @ xi + b) <= 1e-12 * (np.linalg.norm(M, 2) * np.linalg.norm(xi) + np.linalg.norm(b))
    assert n_singular == 4  # rank 3 undamped, rank 5, all zero, a negative diagonal entry
    for v in out["R"]:
        w, E = v[:3], v[3:].reshape(3, 3)
        want = _expm_so3(w)
        # I + a K + b K^2 with |a K| <= 1, |b K^2| <= 2: a and b carry a few roundings each (sin, a divide, a square), the
        # entry of K^2 two, the two sums two more -- under 8 roundings of 1.1e-16 on terms of size <= 2
        assert np.abs(E - want).max() <= 2e-15, (w, np.abs(E - want).max())
        assert np.abs(E @ E.T - np.eye(3)).max() <= 1e-15
    for v in out["U"]:
        pose, xi, got = v[:12].reshape(3, 4), v[12:18], v[18:].reshape(3, 4)
        want = pose.copy()
        want[:, :3] = _expm_so3(xi[3:]) @ pose[:, :3]
        want[:, 3] += xi[:3]
        assert np.abs(got - want).max() <= 4e-15  # (the same, through a 3-term product with |R| <= 1)


def _expm_so3(w):
    """exp([w]x) without scipy: the Taylor series of the matrix exponential in 60-digit decimals, rounded to f64 once"""
    import decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        D = decimal.Decimal
        x, y, z = (D(float(c)) for c in w)
        K = [[D(0), -z, y], [z, D(0), -x], [-y, x, D(0)]]
        E = [[D(int(i == j)) for j in range(3)] for i in range(3)]
        term = [row[:] for row in E]
        for n in range(1, 80):
            term = [[sum(term[i][k] * K[k][j] for k in range(3)) / n for j in range(3)] for i in range(3)]
            E = [[E[i][j] + term[i][j] for j in range(3)] for i in range(3)]
        return np.array([[float(E[i][j]) for j in range(3)] for i in range(3)])


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_shared_solve_against_numpy(tmp_path):
    _check_solve_output(_solve_print(tmp_path, []))


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_shared_solve_under_sanitizers(tmp_path):
    _check_solve_output(_solve_print(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]))


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_align_symbols_are_exported_and_bound():
    L = capi.lib()
    for s in ("tf_align_default_params", "tf_align_frame", "tf_align_frame_device", "tf_align_log", "tf_align_residuals",
              "tf_align_residuals_device"):
        assert s in capi.SYMBOLS and hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert C.sizeof(capi.AlignParamsC) == 68 and C.sizeof(capi.AlignResult) == 76 and C.sizeof(capi.AlignIter) == 392


def test_default_params_round_trip():
    p = capi.AlignParams()
    assert p.n_levels == 3 and list(p.stride)[:3] == [4, 2, 1] and list(p.iters)[:3] == [4, 3, 2]
    d = R.DEFAULTS
    assert [(p.stride[i], p.iters[i]) for i in range(p.n_levels)] == d["levels"]
    for k in ("min_depth", "max_depth", "max_residual", "huber", "damping", "eps_t", "eps_r"):
        assert getattr(p, k) == np.float32(d[k]), k
    assert p.min_valid == d["min_valid"]
    q = capi.AlignParams(levels=[(3, 5)], huber=0.0, min_valid=7)
    assert q.n_levels == 1 and q.stride[0] == 3 and q.iters[0] == 5 and q.huber == 0.0 and q.min_valid == 7
    assert capi.lib().tf_align_default_params(None) == capi.TF_ERR_INVALID
    with pytest.raises(TypeError):
        capi.AlignParams(no_such_field=1)
