"""Group alignment without a GPU: the numpy restatement (tests/align_group_ref.py) on the three-frame case of the
hand-built corner, partitions and stops, tf_align_group_solve.h on its own against a 60-digit reference, and the ABI."""
import ctypes as C
import decimal
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import align_group_inputs as GI
from tests import align_group_ref as G
from tests import align_inputs as I
from tests import align_ref as R
from tests.raycast_ref import RefVolume
from texturefusion_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++")
ONE_STEP = dict(levels=[(1, 1)], huber=0.0, damping=0.0)


@pytest.fixture(scope="module")
def case():
    ids, s, w, c = I.hand_corner()
    poses, depths = GI.hand_group()
    return RefVolume(ids, s, w, c, I.HAND_RES), poses, depths


@pytest.fixture(scope="module")
def singles(case):
    """align_ref.align of each frame alone from its moved pose: computed once, shared"""
    ref, poses, depths = case
    start = GI.move_group(poses, I.HAND_DELTA)
    p = R.params(levels=[(2, 2), (1, 1)], huber=0.0, eps_t=0.0, eps_r=0.0)
    return start, p, [R.align(ref, depths[k], start[k], I.CAM, p) for k in range(3)]


def test_known_answer_of_the_rigid_group(case):
    """the keyframe sees one face and is singular alone; the three frames as one body are not, and one step from the true
    poses moved by HAND_DELTA returns every frame (the bound of the single-frame known-answer test, tests/test_align_cpu.py)"""
    ref, poses, depths = case
    p = R.params(**ONE_STEP)
    res, log = R.align(ref, depths[0], poses[0], I.CAM, p)
    assert res["status"] == R.SINGULAR and log[0]["n_valid"] == 3445
    out = G.align_group(ref, depths, GI.move_group(poses, I.HAND_DELTA), I.CAM, p)
    body, rec = out["body"][0], out["log"][0][0]
    dt, dr = G.group_distance(out["pose64"], poses)
    print("rigid known answer: dt %.3g m, dr %.3g rad, cond %.3g, valid %d" % (dt, dr, np.linalg.cond(rec["A"]), rec["n_valid"]))
    assert out["n_bodies"] == 1 and body["status"] == R.MAX_ITERS and body["evaluations"] == 2
    assert dt <= 1e-5 and dr <= 1e-5
    assert rec["n_valid"] == 25473 == out["frame_valid_first"].sum() and out["frame_valid_first"][0] == 3445
    assert np.linalg.cond(rec["A"]) < 1e3
    assert np.abs(rec["xi"][:3] + I.HAND_DELTA).max() <= 1e-5 and np.abs(rec["xi"][3:]).max() <= 1e-5
    assert np.array_equal(out["body"][0]["pose"], out["pose"][0])


def _same_log(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for key in x:
            assert np.array_equal(np.asarray(x[key]), np.asarray(y[key])), key


def test_every_frame_its_own_body_is_align_per_frame(case, singles):
    ref, poses, depths = case
    start, p, alone = singles
    out = G.align_group(ref, depths, start, I.CAM, p, body=[0, 1, 2])
    assert out["n_bodies"] == 3
    for k in range(3):
        res, log = alone[k]
        assert {key: v for key, v in out["body"][k].items() if key != "pose"} == {key: v for key, v in res.items() if key != "pose"}
        assert np.array_equal(out["body"][k]["pose"].view(np.uint32), res["pose"].view(np.uint32))
        assert np.array_equal(out["pose"][k].view(np.uint32), res["pose"].view(np.uint32))
        _same_log(out["log"][k], log)
        assert out["frame_valid_first"][k] == res["n_valid_first"] and out["frame_valid_last"][k] == res["n_valid_last"]
    assert out["body"][0]["status"] == R.SINGULAR and out["body"][1]["status"] == R.MAX_ITERS


def test_mixed_partition(case, singles):
    """[0, 0, 1]: the first two frames move as one body (the keyframe is held by the local frame), the third is
    align_ref.align on its own"""
    ref, poses, depths = case
    start, p, alone = singles
    out = G.align_group(ref, depths, start, I.CAM, p, body=[0, 0, 1])
    assert out["n_bodies"] == 2 and [b["status"] for b in out["body"]] == [R.MAX_ITERS, R.MAX_ITERS]
    _same_log(out["log"][1], alone[2][1])
    assert np.array_equal(out["pose"][2].view(np.uint32), alone[2][0]["pose"].view(np.uint32))
    rec = out["log"][0][0]
    assert rec["n_valid"] == out["frame_valid_first"][0] + out["frame_valid_first"][1] and rec["n_sampled"] == 2 * 80 * 60
    dt, dr = G.group_distance(out["pose64"][:2], poses[:2])
    assert dt <= 1e-5 and dr <= 1e-5
    # the two frames moved by one rigid motion: their relative pose is the start's (f64 products: 1e-12 is ample)
    rel = lambda a, b: a[:, :3].T @ (b[:, 3] - a[:, 3])
    s64 = [np.asarray(s, np.float64) for s in start]
    assert np.abs(rel(out["pose64"][0], out["pose64"][1]) - rel(s64[0], s64[1])).max() <= 1e-12


def test_an_empty_body_ends_too_few_while_the_other_goes_on(case):
    ref, poses, depths = case
    empty = np.zeros_like(depths[1])
    start = GI.move_group(poses, I.HAND_DELTA)
    p = R.params(**ONE_STEP)
    out = G.align_group(ref, [depths[1], empty, empty, depths[2]], [start[1], start[0], start[2], start[2]], I.CAM, p,
                        body=[0, 1, 1, 0])
    a, b = out["body"]
    assert b["status"] == R.TOO_FEW and b["evaluations"] == 1 and b["n_valid_first"] == 0 and b["rms_first"] == 0
    assert np.array_equal(out["pose"][1], start[0]) and np.array_equal(out["pose"][2], start[2])
    assert a["status"] == R.MAX_ITERS and a["evaluations"] == 2
    dt, dr = G.group_distance(out["pose64"][[0, 3]], [poses[1], poses[2]])
    assert dt <= 1e-5 and dr <= 1e-5
    assert list(out["frame_valid_first"][1:3]) == [0, 0] and out["frame_valid_first"][0] > 5000


def test_rigid_run_reaches_one_end_from_two_starts(case):
    """four steps at stride 1 from the two starts of GI.RIGID_STARTS; the distance between the two ends is the measurement
    behind GI.GROUP_TOL_T / GROUP_TOL_R (ten times it)"""
    ref, poses, depths = case
    p = R.params(**GI.RIGID_PARAMS)
    ends = []
    for dt, aa in GI.RIGID_STARTS:
        out = G.align_group(ref, depths, GI.move_group(poses, dt, aa), I.CAM, p)
        assert out["body"][0]["status"] == R.MAX_ITERS and out["body"][0]["evaluations"] == 5
        d = G.group_distance(out["pose64"], poses)
        assert d[0] <= 1e-5 and d[1] <= 1e-5
        ends.append(out["pose64"])
    dt, dr = G.group_distance(ends[0], ends[1])
    print("rigid ends: %.3g m, %.3g rad apart" % (dt, dr))
    assert dt <= GI.GROUP_TOL_T and dr <= GI.GROUP_TOL_R


# ---- tf_align_group_solve.h on its own -----------------------------------------------------------------------------------
def _solve_print(tmp_path, extra):
    exe = str(tmp_path / "group_solve_print")
    cmd = [CXX, "-std=c++14", "-O2", "-Wall", "-ffp-contract=off"] + extra + \
          [os.path.join(ROOT, "tests", "cpp_align_group", "group_solve_print.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    out = {"G": [], "A": []}
    for line in r.stdout.splitlines():
        w = line.split()
        out[w[0]].append(np.array([int(x, 16) for x in w[1:]], np.uint64).view(np.float64))
    return out


def _moved_exactly(pose, xi, c):
    """[E R | c + E (t - c) + v] with E = exp([w]x) by its Taylor series in 60-digit decimals, rounded to f64 once"""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        D = decimal.Decimal
        x, y, z = (D(float(a)) for a in xi[3:])
        K = [[D(0), -z, y], [z, D(0), -x], [-y, x, D(0)]]
        E = [[D(int(i == j)) for j in range(3)] for i in range(3)]
        term = [row[:] for row in E]
        for n in range(1, 80):
            term = [[sum(term[i][k] * K[k][j] for k in range(3)) / n for j in range(3)] for i in range(3)]
            E = [[E[i][j] + term[i][j] for j in range(3)] for i in range(3)]
        P = [[D(float(pose[i, j])) for j in range(4)] for i in range(3)]
        cc, v = [D(float(a)) for a in c], [D(float(a)) for a in xi[:3]]
        out = np.zeros((3, 4))
        for i in range(3):
            for j in range(3):
                out[i, j] = float(sum(E[i][k] * P[k][j] for k in range(3)))
            out[i, 3] = float(cc[i] + sum(E[i][k] * (P[k][3] - cc[k]) for k in range(3)) + v[i])
        return out


def _check_solve_output(out):
    assert len(out["G"]) == 18 and len(out["A"]) == 12
    for v in out["G"]:
        pose, xi, c, got = v[:12].reshape(3, 4), v[12:18], v[18:21], v[21:].reshape(3, 4)
        want = _moved_exactly(pose, xi, c)
        # the rotation: the bound of tests/test_align_cpu.py (E within 2e-15 of exp([w]x), through a 3-term product with |R| <= 1)
        assert np.abs(got[:, :3] - want[:, :3]).max() <= 4e-15
        # the translation: E's 2e-15 per entry against |d|_1, and six roundings (d, two products' sums, c +, + v, the
        # reference's own) of 2^-53 relative on values no larger than |c| + |d|_1 + |v|
        d1 = np.abs(pose[:, 3] - c).sum()
        bound = 2e-15 * d1 + 6 * 2.0 ** -53 * (np.abs(c).max() + d1 + np.abs(xi[:3]).max())
        assert np.abs(got[:, 3] - want[:, 3]).max() <= bound, (np.abs(got[:, 3] - want[:, 3]).max(), bound)
    for v in out["A"]:
        upd, about = v[18:30], v[30:42]
        assert np.array_equal(upd.view(np.uint64), about.view(np.uint64))  # the anchor case is align_update, bit for bit


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_group_update_against_a_60_digit_reference(tmp_path):
    _check_solve_output(_solve_print(tmp_path, []))


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_group_update_under_sanitizers(tmp_path):
    _check_solve_output(_solve_print(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]))


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_group_symbols_are_exported_and_bound():
    L = capi.lib()
    for s in ("tf_align_group", "tf_align_group_device", "tf_align_group_log", "tf_align_unit_group"):
        assert s in capi.SYMBOLS and hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert capi.TF_ALIGN_GROUP_MAX_FRAMES == 7
    assert C.sizeof(capi.AlignGroupResult) == 8 + 7 * 76 + 7 * 48 + 2 * 7 * 4 == 932
    text = open(os.path.join(ROOT, "include", "tf_fusion.h")).read()
    assert "#define TF_ALIGN_GROUP_MAX_FRAMES 7" in text
