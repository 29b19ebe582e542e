"""Exposure compensation in the photometric aligners without a GPU: tf_align_exposure_solve.h against the restatement
(tests/align_exposure_ref.py) bit for bit, the eliminated step against the direct solve of the full 8 x 8 system, the
measurement on the textured hand plane that the device tests rest on, and the ABI."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import align_color_inputs as CI
from tests import align_color_ref as CR
from tests import align_exposure_inputs as EI
from tests import align_exposure_ref as E
from tests import align_icp_color_inputs as XI
from tests import align_icp_color_ref as X
from tests import align_inputs as I
from tests import align_ref as R
from texturefusion_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++")
u64 = lambda a: np.asarray(a, np.float64).view(np.uint64)


# ---- 1. tf_align_exposure_solve.h on its own --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("exposure") / "exposure_solve_print")
    cmd = [CXX, "-std=c++14", "-O2", "-Wall", "-ffp-contract=off",
           os.path.join(ROOT, "tests", "cpp_align_exposure", "exposure_solve_print.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    out = []
    for line in r.stdout.splitlines():
        w = line.split()
        assert w[0] == "E"
        v = np.array([int(x, 16) for x in w[3:]], np.uint64).view(np.float64)
        out.append(dict(unknowns=int(w[1]), rank=int(w[2]), min_gain=v[0], max_gain=v[1], pair=v[2:4], S=v[4:21], Ac=v[21:42],
                        bc=v[42:48], xi=v[48:54], Ac2=v[54:75], bc2=v[75:81], de=v[81:83], pair2=v[83:85]))
    return out


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_header_equals_the_restatement_bit_for_bit(printed):
    seen, clamped = set(), set()
    for c in printed:
        A2, b2, el = E.eliminate(c["S"], c["unknowns"], c["Ac"], c["bc"])
        assert el["rank"] == c["rank"] <= c["unknowns"]
        assert np.array_equal(u64(A2), u64(c["Ac2"])) and np.array_equal(u64(b2), u64(c["bc2"]))
        de = E.step(c["S"], el, c["xi"])
        assert np.array_equal(u64(de), u64(c["de"]))
        pair = E.apply(c["pair"], el["rank"], de, c["min_gain"], c["max_gain"])
        assert np.array_equal(u64(pair), u64(c["pair2"]))
        seen.add((c["unknowns"], c["rank"]))
        if el["rank"] == 0:  # the joined system is the existing one, the pair stays
            assert np.array_equal(u64(A2), u64(c["Ac"])) and np.array_equal(u64(b2), u64(c["bc"]))
            assert not np.any(c["de"]) and np.array_equal(u64(c["pair2"]), u64(c["pair"]))
        if el["rank"] < 2:
            assert c["pair2"][0] == c["pair"][0] and c["de"][1] == 0.0
        if el["rank"] == 2 and c["pair"][0] + c["de"][1] != c["pair2"][0]:
            clamped.add("min" if c["pair2"][0] == c["min_gain"] else "max" if c["pair2"][0] == c["max_gain"] else "?")
    # every rank under every setting it can occur under, a constant Lf (unknowns 2, rank 1), the clamp at both ends
    assert seen == {(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)}, seen
    assert clamped == {"min", "max"}, clamped


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_eliminated_step_is_the_joint_gauss_newton_step(printed):
    """the 6 x 6 solve of the eliminated system and the pair's step against numpy.linalg.solve of the full 8 x 8 system on the
    same sums, damping 0: the algebra is the joint step, not merely self-consistent"""
    rng = np.random.default_rng(3)
    n = 0
    for c in printed:
        if c["rank"] != 2:
            continue
        G = rng.normal(size=(40, 6)) * np.array([3.0, 3.0, 3.0, 1.0, 1.0, 1.0])
        geo = dict(A21=(G.T @ G)[R.IU], b=rng.normal(size=6))
        pho = dict(A21=c["Ac"], b=c["bc"])
        for l2 in (1.0, 0.01):
            want_xi, want_do, want_dg = E.solve_joint(geo, pho, c["S"], l2, 0.0)
            A2, b2, el = E.eliminate(c["S"], 2, c["Ac"], c["bc"])
            M21, bM = geo["A21"] + l2 * A2, geo["b"] + l2 * b2
            if np.linalg.cond(R.full(M21)) > 1e4:
                continue
            xi = X.solve_exact(M21, bM, 0.0)
            do, dg = E.step(c["S"], el, xi)
            got, want = np.concatenate([xi, [do, dg]]), np.concatenate([want_xi, [want_do, want_dg]])
            assert np.linalg.norm(got - want) <= 1e-9 * np.linalg.norm(want), (np.linalg.norm(got - want), np.linalg.norm(want))
            n += 1
    assert n >= 20


# ---- 2. the measurement on the hand plane ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plane():
    return XI.ref_of(CI.hand_plane_textured())


def _conditions(log, xlog, what):
    """what keeps the known-answer tests honest"""
    assert log[0]["n_photo"] >= 300, what
    assert all(x["rank"] == 2 for x in xlog), what
    assert np.linalg.cond(R.full(log[-1]["M21"])) < 1e5, what


def _sdf_runs(ref, exposure):
    depth, rgba = EI.plane_frame(exposure)
    p = CR.params(**CI.PARAMS)
    return [E.align_sdf(ref, depth, rgba, EI.sdf_start(k), I.CAM, p, E.setting()) for k in EI.SDF_STARTS]


def _icp_runs(ref, exposure):
    depth, rgba = EI.plane_frame(exposure)
    out = []
    for rung in EI.ICP_STARTS:
        start = EI.icp_start(rung)
        V, N = XI.plane_maps(start)
        out.append(E.align_icp(ref, depth, rgba, start, V, N, start, I.CAM, X.params(), E.setting()))
    return out


@pytest.mark.parametrize("form", ["sdf", "icp"])
def test_measurement_compensated_runs_end_next_to_the_true_pose(plane, form):
    runs = _sdf_runs if form == "sdf" else _icp_runs
    truth_t, truth_r = (CI.HAND_TRUTH_T, CI.HAND_TRUTH_R) if form == "sdf" else (XI.PLANE_TRUTH_T, XI.PLANE_TRUTH_R)
    ident = runs(plane, None)
    for res, log, xlog, pair in ident:
        _conditions(log, xlog, (form, "identity"))
    g_id, o_id = np.mean([r[3][0] for r in ident]), np.mean([r[3][1] for r in ident])
    print("%s: the unmodified frame gives gain %.6f offset %.6f (per start: %s)" % (
        form, g_id, o_id, ", ".join("%.6f %.6f" % r[3] for r in ident)))
    dev_g = dev_o = 0.0
    for g, o in EI.EXPOSURES:
        for k, (res, log, xlog, pair) in enumerate(runs(plane, (g, o))):
            _conditions(log, xlog, (form, g, o, k))
            dt, dr = R.pose_distance(res["pose"], I.hand_pose())
            pg, po = EI.predicted((g_id, o_id), g, o)
            print("%s gain %.1f offset %+.2f start %d: status %d, %d evaluations, %.4g m %.3g rad from the true pose; pair "
                  "%.6f %.6f, predicted %.6f %.6f" % (form, g, o, k, res["status"], res["evaluations"], dt, dr, pair[0], pair[1],
                                                     pg, po))
            assert res["status"] <= R.MAX_ITERS
            assert dt <= 2 * truth_t and dr <= 2 * truth_r
            dev_g, dev_o = max(dev_g, abs(pair[0] - pg)), max(dev_o, abs(pair[1] - po))
    print("%s: largest deviation from the prediction: gain %.3g offset %.3g" % (form, dev_g, dev_o))
    rec_id, rec_g, rec_o = (EI.SDF_ID, EI.SDF_DEV_G, EI.SDF_DEV_O) if form == "sdf" else (EI.ICP_ID, EI.ICP_DEV_G, EI.ICP_DEV_O)
    # what align_exposure_inputs.py records is what this prints
    assert abs(g_id - rec_id[0]) <= 1e-6 and abs(o_id - rec_id[1]) <= 1e-6
    assert dev_g <= rec_g and dev_o <= rec_o and dev_g >= 0.9 * rec_g and dev_o >= 0.9 * rec_o


@pytest.mark.parametrize("form", ["sdf", "icp"])
def test_measurement_uncompensated_runs_end_far_from_the_true_pose(plane, form):
    """the existing restatements, unchanged, on the frame exposed by (0.8, +0.06)"""
    depth, rgba = EI.plane_frame(EI.EXPOSURES[0])
    if form == "sdf":
        start = EI.sdf_start(EI.SDF_STARTS[0])
        res, log = CR.align(plane, depth, rgba, start, I.CAM, CR.params(**CI.PARAMS))
        truth_t, truth_r = CI.HAND_TRUTH_T, CI.HAND_TRUTH_R
    else:
        start = EI.icp_start(EI.ICP_STARTS[0])
        V, N = XI.plane_maps(start)
        res, log = X.align(plane, depth, rgba, start, V, N, start, I.CAM, X.params())
        truth_t, truth_r = XI.PLANE_TRUTH_T, XI.PLANE_TRUTH_R
    dt, dr = R.pose_distance(res["pose"], I.hand_pose())
    print("%s uncompensated on gain 0.8 offset +0.06: status %d, %.4g m %.3g rad from the true pose (%.0f x, %.0f x)" % (
        form, res["status"], dt, dr, dt / truth_t, dr / truth_r))
    assert log[0]["n_photo"] >= 300 and res["status"] <= R.MAX_ITERS
    assert dt >= 10 * truth_t and dr >= 10 * truth_r


def test_the_exposures_do_not_clip_the_texture():
    _, rgba = EI.plane_frame()
    v = rgba[..., 0][rgba[..., 3] != 0]
    assert 28 <= v.min() and v.max() <= 228
    for g, o in EI.EXPOSURES:
        lo, hi = g * 28 + 255 * o, g * 228 + 255 * o
        assert 0 < lo and hi < 255, (g, o)


def test_the_start_pair_one_zero_gives_the_existing_rows(plane):
    depth, rgba = EI.plane_frame()
    p = CR.params(**CI.PARAMS)
    at = EI.sdf_start(1)
    a, b = E.rows_sdf(plane, depth, rgba, at, I.CAM, 2, p, (1.0, 0.0)), CR.rows(plane, depth, rgba, at, I.CAM, 2, p)
    for k in ("rc", "gradc", "flags"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    V, N = XI.plane_maps(at)
    pi = X.params()
    maps = X.model_maps(plane, V, N, at, I.CAM, pi)
    a = E.rows_icp(maps, depth, rgba, at, V, N, at, I.CAM, 2, pi, (1.0, 0.0))
    b = X.rows(maps, depth, rgba, at, V, N, at, I.CAM, 2, pi)
    for k in ("rc", "gradc", "flags"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


# ---- 3. ABI -----------------------------------------------------------------------------------------------------------
def test_exposure_symbols_are_exported_and_bound():
    L = capi.lib()
    for s in ("tf_align_exposure_default", "tf_align_set_exposure", "tf_align_get_exposure", "tf_align_exposure_log",
              "tf_align_exposure_estimate"):
        assert s in capi.SYMBOLS and hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert C.sizeof(capi.AlignExposureC) == 24 and C.sizeof(capi.AlignExposureIter) == 176
    assert capi.ALIGN_EXPOSURE_ITER_DTYPE.itemsize == 176


def test_defaults_round_trip():
    e = capi.AlignExposure()
    for k, v in E.DEFAULT.items():
        assert getattr(e, k) == v, k
    q = capi.AlignExposure(unknowns=1, carry=1, gain0=1.25, offset0=-0.07, min_gain=0.5, max_gain=2.0)
    assert (q.unknowns, q.carry, q.gain0, q.min_gain, q.max_gain) == (1, 1, 1.25, 0.5, 2.0) and q.offset0 == np.float32(-0.07)
    assert capi.lib().tf_align_exposure_default(None) == capi.TF_ERR_INVALID
    with pytest.raises(TypeError):
        capi.AlignExposure(no_such_field=1)
