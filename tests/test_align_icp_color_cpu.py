"""The colour ICP's method, checked on the CPU with the numpy restatement (tests/align_icp_color_ref.py): on the textured
hand plane, where the plain projective ICP is singular, it ends next to the true pose from in-plane starts of 10, 20 and
30 mm and from one with 0.3 degrees about the normal; on the textured corner it ends where the plain call ends; without
weight it is the plain restatement bit for bit.  The measurements recorded in tests/align_icp_color_inputs.py are printed
here."""
import numpy as np
import pytest

from tests import align_icp_color_inputs as XI
from tests import align_icp_color_ref as X
from tests import align_icp_gate_ref as G
from tests import align_icp_inputs as II
from tests import align_icp_ref as K
from tests import align_inputs as I
from tests import align_ref as R


@pytest.fixture(scope="module")
def plane():
    depth, rgba = XI.plane_frame()
    return XI.ref_of(XI.CI.hand_plane_textured()), depth, rgba


@pytest.fixture(scope="module")
def plane_runs(plane):
    ref, depth, rgba = plane
    out = []
    for metres, degrees in XI.PLANE_RUNGS:
        start = XI.plane_start(metres, degrees)
        V, N = XI.plane_maps(start)
        res, log = X.align(ref, depth, rgba, start, V, N, start, I.CAM, X.params())
        out.append((metres, degrees, res, log))
    return out


def _in_plane(pose):
    d = np.asarray(pose, np.float64).reshape(3, 4)[:, 3] - np.asarray(I.hand_pose(), np.float64)[:, 3]
    return float(np.linalg.norm(d[1:]))  # x is the plane's normal


def test_plain_icp_is_singular_on_the_textured_plane(plane):
    _, depth, _ = plane
    start = XI.plane_start(*XI.PLANE_RUNGS[0])
    V, N = XI.plane_maps(start)
    res, log = K.align(depth, start, V, N, start, I.CAM, K.params())
    assert res["status"] == R.SINGULAR and log[0]["n_valid"] > 1000


def test_colour_icp_holds_the_plane_from_every_rung(plane_runs):
    """the condition the device tests rest on: every rung ends with status <= MAX_ITERS and an in-plane error of at most a
    tenth of the start's offset"""
    held, broken = 0, False
    for metres, degrees, res, log in plane_runs:
        err = _in_plane(log[-1]["pose"])
        dt, dr = R.pose_distance(log[-1]["pose"], I.hand_pose())
        ok = res["status"] <= R.MAX_ITERS and err <= 0.1 * metres
        print("plane from %.0f mm, %.1f deg: status %d, %d evaluations, %d photometric of %d valid first, in-plane error %.4g m, "
              "%.4g m %.3g rad from the true pose, cond %.3g -> %s" % (
                  1e3 * metres, degrees, res["status"], res["evaluations"], log[0]["n_photo"], log[0]["n_valid"], err, dt, dr,
                  np.linalg.cond(R.full(log[-1]["M21"])), "held" if ok else "NOT held"))
        broken = broken or not ok
        held += 0 if broken else 1
    assert held >= 1, "the 10 mm rung must hold"
    assert held == XI.PLANE_HELD  # the device tests use every rung the restatement holds
    for metres, degrees, res, log in plane_runs[:held]:
        assert log[0]["n_photo"] > 300 and np.linalg.cond(R.full(log[-1]["M21"])) < 1e5
        dt, dr = R.pose_distance(log[-1]["pose"], I.hand_pose())
        assert dt <= 2 * XI.PLANE_TRUTH_T and dr <= 2 * XI.PLANE_TRUTH_R
    ends = [log[-1]["pose"] for _, _, _, log in plane_runs[:held]]
    d = [R.pose_distance(a, b) for a in ends for b in ends]
    truth = [R.pose_distance(e, I.hand_pose()) for e in ends]
    print("plane: ends %.3g m, %.3g rad apart; at most %.4g m, %.3g rad from the true pose" % (
        max(x[0] for x in d), max(x[1] for x in d), max(t[0] for t in truth), max(t[1] for t in truth)))
    assert max(x[0] for x in d) <= 2 * XI.PLANE_SPREAD_T and max(x[1] for x in d) <= 2 * XI.PLANE_SPREAD_R


def test_on_the_corner_the_colour_call_ends_where_the_plain_call_ends():
    ref = XI.ref_of(XI.corner_textured())
    depth, rgba = XI.corner_frame()
    start = II.ladder_start(*II.LADDER[0])
    V, N = II.hand_model_maps(start)
    plain, plog = K.align(depth, start, V, N, start, I.CAM, K.params())
    res, log = X.align(ref, depth, rgba, start, V, N, start, I.CAM, X.params())
    dt, dr = R.pose_distance(log[-1]["pose"], plog[-1]["pose"])
    print("corner from 40 mm / 2 deg: colour status %d, %d evaluations, %d photometric of %d valid; plain status %d, %d evaluations; "
          "ends %.3g m, %.3g rad apart" % (res["status"], res["evaluations"], log[-1]["n_photo"], log[-1]["n_valid"],
                                          plain["status"], plain["evaluations"], dt, dr))
    assert res["status"] <= R.MAX_ITERS and plain["status"] <= R.MAX_ITERS and log[-1]["n_photo"] > 1000
    assert dt <= 2 * XI.CORNER_SHIFT_T and dr <= 2 * XI.CORNER_SHIFT_R


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_without_weight_it_is_the_plain_restatement(gated):
    """the geometric rows, counts and flags are the plain restatement's bit for bit; so is every step once the sums are taken
    the same way (the plain restatement's are exact sums, so poses are compared after one evaluation's rows)"""
    ref = XI.ref_of(XI.corner_textured())
    depth, rgba = XI.corner_frame()
    start = II.ladder_start(*II.LADDER[0])
    V, N = II.hand_model_maps(start)
    g = G.gate() if gated else None
    p = X.params(photo_weight=0.0)
    maps = X.model_maps(ref, V, N, start, I.CAM, p)
    for stride in (4, 1):
        rw = X.rows(maps, depth, rgba, start, V, N, start, I.CAM, stride, p, g)
        want = G.rows(depth, start, V, N, start, I.CAM, stride, p, g) if gated else K.rows(depth, start, V, N, start, I.CAM, stride, p)
        assert np.array_equal(rw["flags"] & 255, want["flags"]) and np.array_equal(rw["assoc"], want["assoc"])
        assert np.array_equal(rw["r"].view(np.uint32), want["r"].view(np.uint32))
        sg, _ = X.sums(rw, p)
        sw = R.sums(want, p)
        assert np.array_equal(sg["A21"], sw["A21"]) and np.array_equal(sg["b"], sw["b"]) and sg["n_valid"] == sw["n_valid"]
    res, log = X.align(ref, depth, rgba, start, V, N, start, I.CAM, p, g)
    none, nlog = X.align(None, depth, rgba, start, V, N, start, I.CAM, X.params(), g)  # a volume without colour
    assert nlog[0]["n_photo"] == 0 and log[0]["n_photo"] > 0
    assert res["status"] == none["status"] and np.array_equal(res["pose"], none["pose"]) and len(log) == len(nlog)
    for a, b in zip(log, nlog):
        assert np.array_equal(a["A21"], b["A21"]) and np.array_equal(a["xi"], b["xi"]) and np.array_equal(a["pose"], b["pose"])
