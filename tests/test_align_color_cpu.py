"""Alignment by colour as well as depth without a GPU: the numpy restatement (tests/align_color_ref.py) on the textured
hand-built plane and on the oracle's volume of one textured wall, its degenerate cases against tests/align_ref.py, the
flag bits on hand-made pixels, and the ABI."""
import ctypes as C

import numpy as np
import pytest

from oracle import api as O
from tests import align_color_inputs as CI
from tests import align_color_ref as CR
from tests import align_inputs as I
from tests import align_ref as R
from tests.raycast_ref import RefVolume
from texturefusion_amd import capi


def _ref(vol):
    ids, s, w, c = vol
    return RefVolume(ids, s, w, c, I.HAND_RES)


def _spread(ends):
    d = [R.pose_distance(a, b) for a in ends for b in ends]
    return max(x[0] for x in d), max(x[1] for x in d)


def _runs(ref, depth, rgba, pose, starts, what):
    p = CR.params(**CI.PARAMS)
    out = []
    for dt, rv in starts:
        res, log = CR.align(ref, depth, rgba, I.perturb(pose, dt, rv), I.CAM, p)
        print("%s from %s mm: %d photometric of %d valid of %d sampled first, %d of %d last, cond %.3g" % (
            what, np.round(1e3 * dt, 1), log[0]["n_photo"], log[0]["n_valid"], log[0]["n_sampled"], log[-1]["n_photo"],
            log[-1]["n_valid"], np.linalg.cond(R.full(log[-1]["M21"]))))
        out.append((res, log))
    return out


def _check_conditions(runs):
    """what keeps the fixed-point tests from hiding a failure: the colour term is there from the first evaluation on and
    the joined system is well conditioned"""
    for res, log in runs:
        assert res["status"] == R.MAX_ITERS and res["evaluations"] == 11
        assert log[-1]["n_valid"] > 1000 and log[-1]["n_photo"] >= 0.95 * log[-1]["n_valid"]
        assert log[0]["n_photo"] >= 0.8 * log[0]["n_valid"]
        assert np.linalg.cond(R.full(log[-1]["M21"])) < 1e4


@pytest.fixture(scope="module")
def plane():
    pose = I.hand_pose()
    depth, rgba = CI.hand_frame(pose)
    return _ref(CI.hand_plane_textured()), pose, depth, rgba


@pytest.fixture(scope="module")
def plane_runs(plane):
    ref, pose, depth, rgba = plane
    return _runs(ref, depth, rgba, pose, CI.hand_starts(), "plane")


def test_geometric_alone_is_singular_on_the_textured_plane(plane):
    ref, pose, depth, _ = plane
    res, log = R.align(ref, depth, pose, I.CAM, R.params(levels=[(1, 1)], huber=0.0))
    assert res["status"] == R.SINGULAR and log[0]["n_valid"] > 1000


def test_textured_plane_ends_at_one_pose_next_to_the_true_one(plane, plane_runs):
    """four starts up to (0, 15, 12) mm and 0.3 degrees away end at one pose; the two measurements recorded in
    align_color_inputs.py (the ends' spread, their distance to the true pose) are printed here"""
    _, pose, _, _ = plane
    far = max(np.linalg.norm(dt) for dt, _ in CI.hand_starts())
    assert abs(far - 0.0192) < 1e-4 and any(np.linalg.norm(rv) > 0.005 for _, rv in CI.hand_starts())
    _check_conditions(plane_runs)
    ends = [log[-1]["pose"] for _, log in plane_runs]
    st, sr = _spread(ends)
    truth = [R.pose_distance(e, pose) for e in ends]
    print("plane: ends %.3g m, %.3g rad apart; %.4g m, %.3g rad from the true pose" % (
        st, sr, max(t[0] for t in truth), max(t[1] for t in truth)))
    assert st <= CI.HAND_SPREAD_T and sr <= CI.HAND_SPREAD_R
    for dt, dr in truth:
        assert dt <= 2 * CI.HAND_TRUTH_T and dr <= 2 * CI.HAND_TRUTH_R


@pytest.fixture(scope="module")
def wall():
    frames = CI.wall_frames()
    ov = O.Volume(CI.WALL_RES, O.camera_from(I.CAM), O.default_integrator())
    for depth, rgba, pose in frames:
        ov.integrate_frame(depth, rgba, pose)
    ref = RefVolume.from_volume(ov, ov.list_chunks(), CI.WALL_RES)
    ov.close()
    depth, rgba, pose = frames[CI.WALL_HELD]
    return ref, pose, depth, rgba


def test_textured_wall_ends_at_one_pose(wall):
    """the spread of the four ends is the measurement behind CI.WALL_SPREAD_T / _R"""
    ref, pose, depth, rgba = wall
    runs = _runs(ref, depth, rgba, pose, CI.wall_starts(), "wall")
    _check_conditions(runs)
    st, sr = _spread([log[-1]["pose"] for _, log in runs])
    print("wall: ends %.3g m, %.3g rad apart, %s m from the integration pose" % (st, sr, runs[0][1][-1]["pose"][:, 3] - pose[:, 3]))
    assert st <= CI.WALL_SPREAD_T and sr <= CI.WALL_SPREAD_R
    assert R.pose_distance(runs[0][1][-1]["pose"], pose)[0] < 2 * float(CI.WALL_RES)


def test_geometric_alone_on_the_wall_depends_on_its_start(wall):
    ref, pose, depth, _ = wall
    ends = []
    for dt, rv in CI.wall_starts()[:2]:
        res, log = R.align(ref, depth, I.perturb(pose, dt, rv), I.CAM, R.params(**CI.PARAMS))
        assert res["status"] == R.MAX_ITERS
        ends.append(log[-1]["pose"])
    apart = np.abs(ends[0][:, 3] - ends[1][:, 3])
    print("geometric alone: ends (%.2f, %.2f, %.2f) mm apart" % tuple(1e3 * apart))
    assert apart[1] > 0.005 and apart[2] > 0.005  # y and z lie in the wall


def _assert_logs_equal(clog, glog):
    assert len(clog) == len(glog)
    for a, b in zip(clog, glog):
        for k in ("level", "stride", "n_sampled", "n_valid", "sum_r2", "sum_wr2", "A21", "b", "xi", "pose"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_no_weight_and_no_colour_reproduce_the_geometric_alignment():
    pose = I.hand_pose()
    depth = I.hand_depth(pose)
    rgba = CI.texture_rgba(depth, pose)
    start = I.perturb(pose, I.HAND_DELTA, np.radians(0.2) * np.array([0.6, -0.64, 0.48]))
    levels = dict(levels=[(2, 2), (1, 2)], eps_t=0.0, eps_r=0.0)
    coloured, plain = _ref(CI.textured(I.hand_corner())), _ref(I.hand_corner())
    gres, glog = R.align(plain, depth, start, I.CAM, R.params(**levels))
    assert gres["status"] == R.MAX_ITERS and len(glog) == 5
    # photo_weight 0 on a coloured volume: the photometric sums are there and weigh nothing
    res, log = CR.align(coloured, depth, rgba, start, I.CAM, CR.params(photo_weight=0.0, **levels))
    assert log[0]["n_photo"] > 1000 and log[0]["Ac21"].any()
    _assert_logs_equal(log, glog)
    assert np.array_equal(res["pose"].view(np.uint32), gres["pose"].view(np.uint32)) and res["status"] == gres["status"]
    # every colour count 0: no pixel is photometrically valid
    res, log = CR.align(plain, depth, rgba, start, I.CAM, CR.params(**levels))
    assert all(r["n_photo"] == 0 and not r["Ac21"].any() and not r["bc"].any() for r in log)
    _assert_logs_equal(log, glog)
    assert np.array_equal(res["pose"].view(np.uint32), gres["pose"].view(np.uint32)) and res["status"] == gres["status"]
    # and with colour the step differs
    res, log = CR.align(coloured, depth, rgba, start, I.CAM, CR.params(**levels))
    assert not np.array_equal(log[0]["xi"], glog[0]["xi"])


def test_flags_on_hand_made_pixels(plane):
    ref, pose, depth, rgba = plane
    p = CR.params(**CI.PARAMS)
    base = CR.rows(ref, depth, rgba, pose, I.CAM, 1, p)
    good = np.argwhere(base["flags"] == 127)
    assert len(good) > 5000 and not np.isin(base["flags"], (15, 31, 63)).any()
    (ya, xa), (yb, xb), (yc, xc) = good[len(good) // 4], good[len(good) // 2], good[3 * len(good) // 4]
    c2 = rgba.copy()
    c2[ya, xa, 3] = 0                                        # colour not valid
    c2[yb, xb, :3] = (c2[yb, xb, :3].astype(int) + 100) % 256  # 100 grey levels off: |rc| = 0.39 > 0.25
    # the voxel two to the +x side of pixel c's base corner: a corner of the +x tap alone
    P = np.asarray(pose, np.float32).reshape(3, 4)
    k = yc * I.CAM.width + xc
    pw = (P[:, 3] + base["q"][k]).astype(np.float64)
    vox = np.floor(pw / float(I.HAND_RES) - 0.5).astype(int) + np.array([2, 0, 0])
    ids, s, w, c = CI.hand_plane_textured()
    row = int(np.nonzero((ids == vox >> 3).all(1))[0][0])
    c = c.reshape(len(ids), 512, 4).copy()
    c[row, ((vox[2] & 7) * 8 + (vox[1] & 7)) * 8 + (vox[0] & 7), 3] = 0
    rw = CR.rows(_ref((ids, s, w, c.reshape(len(ids), 2048))), depth, c2, pose, I.CAM, 1, p)
    assert rw["flags"][ya, xa] == 15 and rw["rc"][ya, xa] == 0 and not rw["gradc"][:, ya, xa].any()
    assert rw["flags"][yb, xb] == 63 and abs(rw["rc"][yb, xb]) > 0.25 and rw["gradc"][:, yb, xb].any()
    assert rw["flags"][yc, xc] == 31 and rw["rc"][yc, xc] == base["rc"][yc, xc] and not rw["gradc"][:, yc, xc].any()
    for y, x in ((ya, xa), (yb, xb), (yc, xc)):  # the geometric row does not see any of it
        assert rw["r"][y, x] == base["r"][y, x] and np.array_equal(rw["grad"][:, y, x], base["grad"][:, y, x])
    sg, sc = CR.sums(rw, p)
    bg, bc = CR.sums(base, p)
    assert sg["n_valid"] == bg["n_valid"] and sc["n_valid"] < bc["n_valid"] and sc["n_valid"] == int((rw["flags"] == 127).sum())


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_align_color_symbols_are_exported_and_bound():
    L = capi.lib()
    for s in ("tf_align_color_default_params", "tf_align_frame_color", "tf_align_frame_color_device", "tf_align_color_log",
              "tf_align_color_residuals", "tf_align_color_residuals_device"):
        assert s in capi.SYMBOLS and hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert C.sizeof(capi.AlignColorParamsC) == 80 and C.sizeof(capi.AlignColorResult) == 92
    assert C.sizeof(capi.AlignColorIter) == 632


def test_default_params_round_trip():
    p = capi.AlignColorParams()
    assert bytes(p.geo) == bytes(capi.AlignParams())
    for k in ("photo_weight", "max_photo_residual", "huber_photo"):
        assert getattr(p, k) == np.float32(CR.DEFAULTS[k]) == np.float32(CI.PHOTO[k]), k
    q = capi.AlignColorParams(levels=[(3, 5)], huber=0.0, photo_weight=0.3, huber_photo=0.0)
    assert q.geo.n_levels == 1 and q.geo.stride[0] == 3 and q.geo.iters[0] == 5 and q.geo.huber == 0.0
    assert q.photo_weight == np.float32(0.3) and q.huber_photo == 0.0 and q.max_photo_residual == 0.25
    assert capi.lib().tf_align_color_default_params(None) == capi.TF_ERR_INVALID
    with pytest.raises(TypeError):
        capi.AlignColorParams(no_such_field=1)
