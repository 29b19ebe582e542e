"""Exposure compensation in the photometric aligners on the MI355X (tf_align_exposure.hip): the maps of one evaluation and
the whole alignment -- colour log, exposure log, result -- against the restatement (tests/align_exposure_ref.py) bit for bit,
the known answer on the textured hand plane seen at another exposure, the degenerate frames, the clamp, the cell, the device
forms, the read-only guarantee, invalid settings and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import align_color_inputs as CI
from tests import align_color_ref as CR
from tests import align_exposure_inputs as EI
from tests import align_exposure_ref as E
from tests import align_icp_color_inputs as XI
from tests import align_icp_color_ref as X
from tests import align_icp_inputs as II
from tests import align_inputs as I
from tests import align_ref as R
from tests.util import HipBuffer, make_pair, assert_chunks_equal
from texturefusion_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = capi.TF_ERR_INVALID
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
u64 = lambda a: np.asarray(a, np.float64).view(np.uint64)
SMALL = synth.Camera(13, 9, 11.0, 11.0, 6.5, 4.5)


def _volume(vol):
    gv = capi.Volume(I.HAND_RES, I.CAM, max_chunks=1 << 10, max_keyframes=8)
    XI.upload(gv, vol)
    return gv


@pytest.fixture(scope="module")
def plane(gpu_required):
    vol = CI.hand_plane_textured()
    gv = _volume(vol)
    yield gv, XI.ref_of(vol)
    gv.align_set_exposure(None)
    gv.close()


@pytest.fixture(scope="module")
def edge(gpu_required):
    vol = XI.edge_volume()
    gv = _volume(vol)
    yield gv, XI.ref_of(vol)
    gv.close()


@pytest.fixture(scope="module")
def corner(gpu_required):
    """the textured corner and the same corner without colour"""
    gc, gp = _volume(XI.corner_textured()), _volume(I.hand_corner())
    yield gc, gp
    gc.close()
    gp.close()


@pytest.fixture(autouse=True)
def _setting_off_afterwards(request):
    yield
    for name in ("plane", "edge"):
        if name in request.fixturenames:
            request.getfixturevalue(name)[0].align_set_exposure(None)
    if "corner" in request.fixturenames:
        for gv in request.getfixturevalue("corner"):
            gv.align_set_exposure(None)
            gv.align_icp_set_gate(None)


def _on(gv, **kw):
    gv.align_set_exposure(capi.AlignExposure(**kw))
    return E.setting(**kw)


def _sdf_device(gv, depth, rgba, start, pc):
    bufs = [HipBuffer(a.nbytes).from_host(np.ascontiguousarray(a)) for a in (depth, rgba)]
    d_res = HipBuffer(C.sizeof(capi.AlignColorResult))
    try:
        gv.align_frame_color_device(bufs[0].ptr, bufs[1].ptr, start, pc, d_res.ptr)
        gv.sync()
        return gv.align_color_result(d_res.to_host())
    finally:
        for b in bufs + [d_res]:
            b.free()


def _icp_device(gv, depth, rgba, start, V, N, pc):
    bufs = [HipBuffer(a.nbytes).from_host(np.ascontiguousarray(a)) for a in (depth, rgba, V, N)]
    d_res = HipBuffer(C.sizeof(capi.AlignColorResult))
    try:
        gv.align_frame_icp_color_device(bufs[0].ptr, bufs[1].ptr, start, bufs[2].ptr, bufs[3].ptr, start, pc, d_res.ptr)
        gv.sync()
        return gv.align_color_result(d_res.to_host())
    finally:
        for b in bufs + [d_res]:
            b.free()


def _same_logs(log, xlog, wlog, wxlog):
    """the colour log and the exposure log against the restatement's, bit for bit"""
    assert len(log) == len(wlog) == len(xlog) == len(wxlog)
    for k, (a, b) in enumerate(zip(log, wlog)):
        for key in ("level", "stride", "n_sampled", "n_valid", "n_photo", "sum_r2", "sum_wr2", "sum_rc2", "sum_wrc2"):
            assert a[key] == b[key], (k, key)
        for key in ("A21", "b", "Ac21", "bc", "xi", "pose"):
            assert np.array_equal(u64(a[key]), u64(b[key])), (k, key)
    for k, (a, b) in enumerate(zip(xlog, wxlog)):
        assert a["rank"] == b["rank"] and a["n_photo"] == b["n_photo"], k
        got = np.concatenate([a["P"], a["Q"], [a["S_w"], a["S_l"], a["S_ll"], a["S_r"], a["S_lr"]]])
        assert np.array_equal(u64(got), u64(b["S"])), (k, "sums")
        for key in ("gain", "offset", "d_offset", "d_gain"):
            assert u64(a[key]) == u64(b[key]), (k, key, a[key], b[key])


def _same_result(res, want):
    assert np.array_equal(bits(res["pose"]), bits(want["pose"]))
    for key in ("status", "evaluations", "n_sampled", "n_valid_first", "n_valid_last", "n_photo_first", "n_photo_last", "rms_first",
                "rms_last", "rms_photo_first", "rms_photo_last"):
        assert res[key] == want[key], key


# ---- 1. maps --------------------------------------------------------------------------------------------------------------
def _sdf_maps_equal(got, want, what):
    assert np.array_equal(got["flags"], want["flags"]), what
    for k in ("r", "grad", "rc", "gradc"):
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k)


def test_sdf_maps_follow_the_compensated_luma(plane):
    gv, ref = plane
    pose = I.hand_pose()
    depth, rgba = EI.plane_frame()
    # the 13 x 9 camera: partial tiles over both borders
    gv.raycast_camera(SMALL)
    try:
        d, c = CI.hand_frame(pose, SMALL, edge_voxels=0.0)
        for stride in (1, 2):
            pd, pc = CR.params(levels=[(stride, 1)], min_valid=1), capi.AlignColorParams(levels=[(stride, 1)], min_valid=1)
            off = gv.align_color_residuals(d, c, pose, pc)
            _on(gv, gain0=EI.MAP_PAIR[0], offset0=EI.MAP_PAIR[1])
            want = E.rows_sdf(ref, d, c, pose, SMALL, stride, pd, EI.MAP_PAIR)
            _sdf_maps_equal(gv.align_color_residuals(d, c, pose, pc), want, "13 x 9 stride %d" % stride)
            assert (want["flags"] & 16).any() and not np.array_equal(bits(want["rc"]), bits(off["rc"]))
            _on(gv)  # the start pair (1, 0): every map is the setting-off call's
            _sdf_maps_equal(gv.align_color_residuals(d, c, pose, pc), off, "13 x 9 stride %d at (1, 0)" % stride)
            gv.align_set_exposure(None)
    finally:
        gv.raycast_camera(None)
    # the full camera with hand-made pixels: bad depths, alpha 0, |rc| above the bound, and one pixel whose |rc| is above the
    # bound uncompensated and below it compensated
    pd, pc = CR.params(levels=[(1, 1)]), capi.AlignColorParams(levels=[(1, 1)])
    base = CR.rows(ref, depth, rgba, pose, I.CAM, 1, pd)
    good = np.argwhere(base["flags"] == 127)
    d, c = depth.copy(), rgba.copy()
    for k, (y, x) in enumerate(good[:: len(good) // 8][:8]):
        d[y, x] = (0.0, np.nan, np.inf, -np.inf, -0.3, 0.04, 5.5, 1e30)[k]
    (ya, xa), (yb, xb) = good[len(good) // 4 + 1], good[len(good) // 2 + 1]
    c[ya, xa, 3] = 0
    c[yb, xb, :3] = (c[yb, xb, :3].astype(int) + 100) % 256
    bright = [(y, x) for y, x in good if rgba[y, x, 0] >= 212 and (y, x) not in ((ya, xa), (yb, xb)) and d[y, x] == depth[y, x]]
    yc, xc = bright[len(bright) // 2]
    c[yc, xc, :3] = rgba[yc, xc, :3] - 74  # 0.29 darker: rc = +0.29 as it is, -0.25 L + 0.43 <= 0.23 compensated (L >= 0.83)
    at = pose.astype(np.float64)
    at[:, 3] += (0.0, 0.004, -0.003)
    for stride in (1, 2):
        pd, pc = CR.params(levels=[(stride, 1)]), capi.AlignColorParams(levels=[(stride, 1)])
        for pp in (at.astype(np.float32), pose):
            gv.align_set_exposure(None)
            off = gv.align_color_residuals(d, c, pp, pc)
            _sdf_maps_equal(off, CR.rows(ref, d, c, pp, I.CAM, stride, pd), "off")
            _on(gv, gain0=EI.MAP_PAIR[0], offset0=EI.MAP_PAIR[1])
            want = E.rows_sdf(ref, d, c, pp, I.CAM, stride, pd, EI.MAP_PAIR)
            got = gv.align_color_residuals(d, c, pp, pc)
            _sdf_maps_equal(got, want, "full camera stride %d" % stride)
            _on(gv)
            _sdf_maps_equal(gv.align_color_residuals(d, c, pp, pc), off, "full camera at (1, 0)")
            if stride == 1:
                assert got["flags"][ya, xa] == 15 and got["flags"][yb, xb] == 63 and (got["flags"] == 127).sum() > 5000
        if stride == 1:  # (at the last pose) bit 6 follows the compensated value
            assert off["flags"][yc, xc] == 63 and got["flags"][yc, xc] == 127
            assert abs(off["rc"][yc, xc]) > 0.25 >= abs(got["rc"][yc, xc]) > 0.15


def _icp_maps_equal(got, want, what):
    assert np.array_equal(got["flags"], want["flags"]), what
    assert np.array_equal(got["assoc"], want["assoc"]), what
    for k in ("r", "rc", "gradc"):
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k)


@pytest.mark.parametrize("stride", [1, 2])
def test_icp_maps_follow_the_compensated_luma(edge, stride):
    gv, ref = edge
    pd, pc = X.params(levels=[(stride, 1)]), capi.AlignIcpColorParams(levels=[(stride, 1)])
    # the 13 x 9 camera
    gv.raycast_camera(SMALL)
    try:
        depth, rgba, V, N, pose = XI.edge_scene(SMALL)
        at = XI.shifted(pose, 0.002, -0.001)
        maps = X.model_maps(ref, V, N, pose, SMALL, pd)
        off = gv.align_icp_color_residuals(depth, rgba, at, pose, pc, vertex=V, normal=N)
        _icp_maps_equal(off, X.rows(maps, depth, rgba, at, V, N, pose, SMALL, stride, pd), "13 x 9 off")
        _on(gv, gain0=EI.MAP_PAIR[0], offset0=EI.MAP_PAIR[1])
        want = E.rows_icp(maps, depth, rgba, at, V, N, pose, SMALL, stride, pd, EI.MAP_PAIR)
        _icp_maps_equal(gv.align_icp_color_residuals(depth, rgba, at, pose, pc, vertex=V, normal=N), want, "13 x 9")
        assert (want["flags"] & 256).any()
        _on(gv)
        _icp_maps_equal(gv.align_icp_color_residuals(depth, rgba, at, pose, pc, vertex=V, normal=N), off, "13 x 9 at (1, 0)")
        gv.align_set_exposure(None)
    finally:
        gv.raycast_camera(None)
    # the full camera with the existing hand-made pixels and one whose bit 9 depends on the compensation
    cam = XI.CAM
    depth, rgba, V, N, pose = XI.edge_cases(cam)
    maps = X.model_maps(ref, V, N, pose, cam, pd)
    at = XI.shifted(pose, 0.0021, -0.0013)
    base = X.rows(maps, depth, rgba, at, V, N, pose, cam, stride, pd)
    bright = [(y, x) for y, x in np.argwhere(base["flags"] == 783) if rgba[y, x, 0] >= 212 and (x, y) != XI.RC_PIX]
    yc, xc = bright[len(bright) // 2]
    rgba = rgba.copy()
    rgba[yc, xc, :3] -= 74
    off = gv.align_icp_color_residuals(depth, rgba, at, pose, pc, vertex=V, normal=N)
    _icp_maps_equal(off, X.rows(maps, depth, rgba, at, V, N, pose, cam, stride, pd), "off")
    _on(gv, gain0=EI.MAP_PAIR[0], offset0=EI.MAP_PAIR[1])
    want = E.rows_icp(maps, depth, rgba, at, V, N, pose, cam, stride, pd, EI.MAP_PAIR)
    got = gv.align_icp_color_residuals(depth, rgba, at, pose, pc, vertex=V, normal=N)
    _icp_maps_equal(got, want, "full camera")
    assert off["flags"][yc, xc] == 271 and got["flags"][yc, xc] == 783
    assert abs(off["rc"][yc, xc]) > 0.25 >= abs(got["rc"][yc, xc]) > 0.15
    n = (cam.width // stride) * (cam.height // stride)
    assert (got["flags"] == 783).sum() > 0.5 * n and (got["flags"] == 15).sum() > 0
    _on(gv)
    _icp_maps_equal(gv.align_icp_color_residuals(depth, rgba, at, pose, pc, vertex=V, normal=N), off, "full camera at (1, 0)")


# ---- 2. sums and log ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unknowns", [0, 1, 2])
@pytest.mark.parametrize("huber_photo", [0.05, 0.0])
def test_sdf_alignment_follows_the_restatement(plane, huber_photo, unknowns):
    gv, ref = plane
    depth, rgba = EI.plane_frame(EI.EXPOSURES[0])
    start = EI.sdf_start(EI.SDF_STARTS[0])
    kw = dict(CI.PARAMS, huber_photo=huber_photo)
    e = _on(gv, unknowns=unknowns)
    want, wlog, wxlog, wpair = E.align_sdf(ref, depth, rgba, start, I.CAM, CR.params(**kw), e)
    res = _sdf_device(gv, depth, rgba, start, capi.AlignColorParams(**kw))
    _same_logs(gv.align_color_log(), gv.align_exposure_log(0), wlog, wxlog)
    _same_result(res, want)
    g, o, valid = gv.align_exposure_estimate(0)
    assert valid and (g, o) == wpair
    assert [x["rank"] for x in wxlog] == [unknowns] * len(wxlog)
    if unknowns == 0:
        assert (g, o) == (1.0, 0.0)
    elif unknowns == 1:
        assert g == 1.0 and o != 0.0


@pytest.mark.parametrize("unknowns", [0, 1, 2])
@pytest.mark.parametrize("huber_photo", [0.05, 0.0])
def test_icp_alignment_follows_the_restatement(plane, huber_photo, unknowns):
    gv, ref = plane
    depth, rgba = EI.plane_frame(EI.EXPOSURES[0])
    start = EI.icp_start(EI.ICP_STARTS[0])
    V, N = XI.plane_maps(start)
    e = _on(gv, unknowns=unknowns)
    want, wlog, wxlog, wpair = E.align_icp(ref, depth, rgba, start, V, N, start, I.CAM, X.params(huber_photo=huber_photo), e)
    res = _icp_device(gv, depth, rgba, start, V, N, capi.AlignIcpColorParams(huber_photo=huber_photo))
    _same_logs(gv.align_icp_color_log(), gv.align_exposure_log(1), wlog, wxlog)
    _same_result(res, want)
    g, o, valid = gv.align_exposure_estimate(1)
    assert (g, o) == wpair and valid == (want["status"] <= R.MAX_ITERS)


# ---- 3. the known answer on the device --------------------------------------------------------------------------------------
def _check_known(form, res, pair, exposure, log, xlog):
    truth_t, truth_r = (CI.HAND_TRUTH_T, CI.HAND_TRUTH_R) if form == "sdf" else (XI.PLANE_TRUTH_T, XI.PLANE_TRUTH_R)
    ident, dg, do = (EI.SDF_ID, EI.SDF_DEV_G, EI.SDF_DEV_O) if form == "sdf" else (EI.ICP_ID, EI.ICP_DEV_G, EI.ICP_DEV_O)
    dt, dr = R.pose_distance(res["pose"], I.hand_pose())
    pg, po = EI.predicted(ident, *exposure)
    print("%s on, gain %.1f offset %+.2f: status %d, %.4g m %.3g rad from the true pose, pair %.6f %.6f (predicted %.6f %.6f)" % (
        form, exposure[0], exposure[1], res["status"], dt, dr, pair[0], pair[1], pg, po))
    assert res["status"] <= capi.TF_ALIGN_MAX_ITERS and pair[2]
    assert log[0]["n_photo"] >= 300 and all(x["rank"] == 2 for x in xlog)
    x = xlog[-1]
    S = np.concatenate([x["P"], x["Q"], [x["S_w"], x["S_l"], x["S_ll"], x["S_r"], x["S_lr"]]])
    A2, _, _ = E.eliminate(S, 2, log[-1]["Ac21"], log[-1]["bc"])
    l2 = float(np.float32(0.1)) ** 2  # both calls' default photo_weight
    assert np.linalg.cond(R.full(log[-1]["A21"] + l2 * A2)) < 1e5  # the joined system
    assert dt <= 2 * truth_t and dr <= 2 * truth_r
    assert abs(pair[0] - pg) <= 2 * dg and abs(pair[1] - po) <= 2 * do


def test_known_answer_sdf(plane):
    gv, _ = plane
    pc = capi.AlignColorParams(**CI.PARAMS)
    for exposure in EI.EXPOSURES:
        depth, rgba = EI.plane_frame(exposure)
        for k in EI.SDF_STARTS:
            _on(gv)
            res = gv.align_frame_color(depth, rgba, EI.sdf_start(k), pc)
            _check_known("sdf", res, gv.align_exposure_estimate(0), exposure, gv.align_color_log(), gv.align_exposure_log(0))
    # off, on the same frame
    gv.align_set_exposure(None)
    depth, rgba = EI.plane_frame(EI.EXPOSURES[0])
    res = gv.align_frame_color(depth, rgba, EI.sdf_start(EI.SDF_STARTS[0]), pc)
    dt, dr = R.pose_distance(res["pose"], I.hand_pose())
    print("sdf off, gain 0.8 offset +0.06: %.4g m %.3g rad from the true pose" % (dt, dr))
    assert res["n_photo_first"] >= 300 and dt >= 10 * CI.HAND_TRUTH_T and dr >= 10 * CI.HAND_TRUTH_R
    assert len(gv.align_exposure_log(0)) == 0 and not gv.align_exposure_estimate(0)[2]


def test_known_answer_icp(plane):
    gv, _ = plane
    pc = capi.AlignIcpColorParams()
    for exposure in EI.EXPOSURES:
        depth, rgba = EI.plane_frame(exposure)
        for rung in EI.ICP_STARTS:
            start = EI.icp_start(rung)
            V, N = XI.plane_maps(start)
            _on(gv)
            res = _icp_device(gv, depth, rgba, start, V, N, pc)
            _check_known("icp", res, gv.align_exposure_estimate(1), exposure, gv.align_icp_color_log(), gv.align_exposure_log(1))
    gv.align_set_exposure(None)
    depth, rgba = EI.plane_frame(EI.EXPOSURES[0])
    start = EI.icp_start(EI.ICP_STARTS[0])
    V, N = XI.plane_maps(start)
    res = _icp_device(gv, depth, rgba, start, V, N, pc)
    dt, dr = R.pose_distance(res["pose"], I.hand_pose())
    print("icp off, gain 0.8 offset +0.06: status %d, %.4g m %.3g rad from the true pose" % (res["status"], dt, dr))
    assert res["n_photo_first"] >= 300 and dt >= 10 * XI.PLANE_TRUTH_T and dr >= 10 * XI.PLANE_TRUTH_R
    # the host form, which raycasts the model itself, holds the same bounds with the setting on
    _on(gv)
    res = gv.align_frame_icp_color(depth, rgba, start)
    _check_known("icp", res, gv.align_exposure_estimate(1), EI.EXPOSURES[0], gv.align_icp_color_log(), gv.align_exposure_log(1))


# ---- 4. degenerate frames -------------------------------------------------------------------------------------------------
def test_a_grey_frame_leaves_the_gain_alone(plane):
    gv, _ = plane
    depth, grey = EI.grey_frame()
    _on(gv, gain0=1.125)
    start = EI.sdf_start(EI.SDF_STARTS[0])
    gv.align_frame_color(depth, grey, start, capi.AlignColorParams(**CI.PARAMS))
    xlog = gv.align_exposure_log(0)
    assert len(xlog) == 11 and (xlog["rank"] == 1).all() and (xlog["gain"] == 1.125).all() and (xlog["d_gain"] == 0).all()
    assert xlog["n_photo"][0] >= 300 and xlog["d_offset"][:-1].all() and gv.align_exposure_estimate(0)[0] == 1.125
    start = EI.icp_start(EI.ICP_STARTS[0])
    V, N = XI.plane_maps(start)
    _icp_device(gv, depth, grey, start, V, N, capi.AlignIcpColorParams())
    xlog = gv.align_exposure_log(1)
    assert len(xlog) >= 2 and (xlog["rank"] == 1).all() and (xlog["gain"] == 1.125).all() and (xlog["n_photo"] > 100).all()


def test_alpha_zero_everywhere_is_the_setting_off_call(plane):
    gv, _ = plane
    depth, rgba = EI.plane_frame(EI.EXPOSURES[0])
    rgba = rgba.copy()
    rgba[..., 3] = 0
    start = EI.sdf_start(EI.SDF_STARTS[0])
    pc = capi.AlignColorParams(**CI.PARAMS)
    off = gv.align_frame_color(depth, rgba, start, pc)
    offlog = gv.align_color_log()
    _on(gv, gain0=1.25, offset0=-0.07)
    res = gv.align_frame_color(depth, rgba, start, pc)
    log, xlog = gv.align_color_log(), gv.align_exposure_log(0)
    assert bytes(res.pop("pose")) == bytes(off.pop("pose")) and res == off
    assert len(log) == len(offlog) == len(xlog) and (xlog["rank"] == 0).all() and (xlog["n_photo"] == 0).all()
    for a, b in zip(log, offlog):
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    assert (xlog["gain"] == 1.25).all() and (xlog["offset"] == np.float64(np.float32(-0.07))).all()


@pytest.mark.parametrize("gated", [False, True], ids=["gate off", "gate on"])
def test_no_weight_and_no_colour_equal_the_plain_calls(corner, gated):
    gc, gp = corner
    depth, rgba = XI.corner_frame()
    rgba = E.expose(rgba, *EI.EXPOSURES[0])
    for gv in (gc, gp):
        gv.align_icp_set_gate(capi.AlignIcpGate() if gated else None)
        _on(gv)
    # the projective form against tf_align_frame_icp
    start = II.ladder_start(*II.LADDER[0])
    V, N = II.hand_model_maps(start)
    pc, p0 = capi.AlignIcpColorParams(), capi.AlignIcpColorParams(photo_weight=0.0)
    bufs = [HipBuffer(a.nbytes).from_host(np.ascontiguousarray(a)) for a in (depth, V, N)]
    d_res = HipBuffer(C.sizeof(capi.AlignResult))
    try:
        gp.align_frame_icp_device(bufs[0].ptr, start, bufs[1].ptr, bufs[2].ptr, start, pc.icp, d_res.ptr)
        gp.sync()
        geo = gp.align_result(d_res.to_host())
        glog = gp.align_icp_log()
    finally:
        for b in bufs + [d_res]:
            b.free()
    assert geo["status"] <= capi.TF_ALIGN_MAX_ITERS and geo["evaluations"] >= 4
    for gv, par, photo in ((gp, pc, False), (gc, p0, True)):
        res = _icp_device(gv, depth, rgba, start, V, N, par)
        log = gv.align_icp_color_log()
        assert bytes(res["pose"]) == bytes(geo["pose"]) and all(res[k] == geo[k] for k in geo if k != "pose")
        assert len(log) == len(glog)
        for a, b in zip(log, glog):
            for key in b:
                assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
        assert (res["n_photo_first"] > 300) == photo and len(gv.align_exposure_log(1)) == len(glog)
    if gated:
        return
    # the SDF form against tf_align_frame
    near = I.perturb(I.hand_pose(), I.HAND_DELTA, np.radians(0.2) * np.array([0.6, -0.64, 0.48]))
    geo = gp.align_frame(depth, near)
    glog = gp.align_log()
    for gv, par, photo in ((gp, capi.AlignColorParams(), False), (gc, capi.AlignColorParams(photo_weight=0.0), True)):
        res = gv.align_frame_color(depth, rgba, near, par)
        log = gv.align_color_log()
        assert bytes(res["pose"]) == bytes(geo["pose"]) and all(res[k] == geo[k] for k in geo if k != "pose")
        assert len(log) == len(glog)
        for a, b in zip(log, glog):
            for key in b:
                assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
        assert (res["n_photo_first"] > 300) == photo


# ---- 5. the clamp -------------------------------------------------------------------------------------------------------
def test_the_gain_is_clamped_after_every_update(plane):
    gv, ref = plane
    depth, rgba = EI.plane_frame(EI.EXPOSURES[0])
    start = EI.sdf_start(EI.SDF_STARTS[0])
    e = _on(gv, max_gain=1.1)
    want, wlog, wxlog, wpair = E.align_sdf(ref, depth, rgba, start, I.CAM, CR.params(**CI.PARAMS), e)
    res = gv.align_frame_color(depth, rgba, start, capi.AlignColorParams(**CI.PARAMS))
    xlog = gv.align_exposure_log(0)
    _same_logs(gv.align_color_log(), xlog, wlog, wxlog)
    _same_result(res, want)
    top = np.float64(np.float32(1.1))
    assert xlog["gain"][0] == 1.0 and (xlog["gain"][1:] == top).all() and (xlog["d_gain"][:-1] > 0).all()
    assert gv.align_exposure_estimate(0)[0] == top


# ---- 6. the cell ----------------------------------------------------------------------------------------------------------
def test_the_cell_carries_the_estimate_only_where_it_is_told_to(plane):
    gv, _ = plane
    depth, rgba = EI.plane_frame(EI.EXPOSURES[0])
    start = EI.sdf_start(EI.SDF_STARTS[0])
    pc = capi.AlignColorParams(**CI.PARAMS)
    gv.align_set_exposure(None)
    old = gv.align_frame_color(depth, rgba, start, pc)
    oldlog = gv.align_color_log()
    _on(gv, carry=1)
    gv.align_frame_color(depth, rgba, start, pc)
    g1, o1, valid = gv.align_exposure_estimate(0)
    assert valid and abs(g1 - 1.2336) < 0.01
    # a call stopped as TOO_FEW leaves the cell as it was
    few = gv.align_frame_color(depth, rgba, start, capi.AlignColorParams(**dict(CI.PARAMS, min_valid=10 ** 6)))
    assert few["status"] == capi.TF_ALIGN_TOO_FEW and not gv.align_exposure_estimate(0)[2]
    gv.align_frame_color(depth, rgba, start, pc)
    x = gv.align_exposure_log(0)
    assert (x["gain"][0], x["offset"][0]) == (g1, o1)
    # the other aligner reads the same cell
    st = EI.icp_start(EI.ICP_STARTS[0])
    V, N = XI.plane_maps(st)
    g2, o2, _ = gv.align_exposure_estimate(0)
    _icp_device(gv, depth, rgba, st, V, N, capi.AlignIcpColorParams())
    x = gv.align_exposure_log(1)
    assert (x["gain"][0], x["offset"][0]) == (g2, o2)
    # carry off: every call starts at (gain0, offset0), and so do the residual maps
    _on(gv, gain0=1.125, offset0=-0.03125)
    for _ in range(2):
        gv.align_frame_color(depth, rgba, start, pc)
        x = gv.align_exposure_log(0)
        assert (x["gain"][0], x["offset"][0]) == (1.125, -0.03125) and x["gain"][-1] != 1.125
    # the tracker: the second stage starts at the first stage's estimate, and with carry off the cell is the start pair after
    res = gv.track_frame_color(depth, rgba, st, capi.AlignIcpColorParams(), pc)
    assert res["stage"] == 2
    g_icp, o_icp, v_icp = gv.align_exposure_estimate(1)
    x = gv.align_exposure_log(0)
    assert v_icp and (x["gain"][0], x["offset"][0]) == (g_icp, o_icp) and g_icp != 1.125
    gv.align_frame_color(depth, rgba, start, pc)
    x = gv.align_exposure_log(0)
    assert (x["gain"][0], x["offset"][0]) == (1.125, -0.03125)
    _on(gv, carry=1)
    gv.track_frame_color(depth, rgba, st, capi.AlignIcpColorParams(), pc)
    g_sdf, o_sdf, _ = gv.align_exposure_estimate(0)
    gv.align_frame_color(depth, rgba, start, pc)
    x = gv.align_exposure_log(0)
    assert (x["gain"][0], x["offset"][0]) == (g_sdf, o_sdf)
    # NULL: the old results bit for bit
    gv.align_set_exposure(None)
    again = gv.align_frame_color(depth, rgba, start, pc)
    assert bytes(again.pop("pose")) == bytes(old["pose"]) and again == {k: v for k, v in old.items() if k != "pose"}
    for a, b in zip(gv.align_color_log(), oldlog):
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    assert gv.align_get_exposure()[0] is False


def test_reset_turns_the_setting_off(gpu_required):
    vol = CI.hand_plane_textured()
    gv = _volume(vol)
    try:
        depth, rgba = EI.plane_frame(EI.EXPOSURES[0])
        start = EI.sdf_start(EI.SDF_STARTS[0])
        pc = capi.AlignColorParams(**CI.PARAMS)
        old = gv.align_frame_color(depth, rgba, start, pc)
        _on(gv, carry=1)
        on = gv.align_frame_color(depth, rgba, start, pc)
        assert bytes(on["pose"]) != bytes(old["pose"])
        gv.reset()
        assert gv.align_get_exposure()[0] is False and len(gv.align_exposure_log(0)) == 0
        gv.set_camera(I.CAM)
        XI.upload(gv, vol)
        again = gv.align_frame_color(depth, rgba, start, pc)
        assert bytes(again.pop("pose")) == bytes(old["pose"]) and again == {k: v for k, v in old.items() if k != "pose"}
    finally:
        gv.close()


# ---- 7. the device forms ----------------------------------------------------------------------------------------------------
def test_device_forms_equal_the_host_forms(plane):
    gv, _ = plane
    depth, rgba = EI.plane_frame(EI.EXPOSURES[0])
    start = EI.sdf_start(EI.SDF_STARTS[0])
    pc = capi.AlignColorParams(**CI.PARAMS)
    _on(gv, gain0=1.25, offset0=-0.07)
    host = gv.align_frame_color(depth, rgba, start, pc)
    hlog, hx = gv.align_color_log(), gv.align_exposure_log(0)
    dev = _sdf_device(gv, depth, rgba, start, pc)
    assert bytes(np.asarray(dev.pop("pose"))) == bytes(host["pose"]) and dev == {k: v for k, v in host.items() if k != "pose"}
    assert gv.align_exposure_log(0).tobytes() == hx.tobytes() and len(hx) == host["evaluations"]
    for a, b in zip(gv.align_color_log(), hlog):
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    P = depth.size
    bufs = [HipBuffer(depth.nbytes).from_host(depth), HipBuffer(rgba.nbytes).from_host(rgba)]
    maps = [HipBuffer(4 * P), HipBuffer(12 * P), HipBuffer(4 * P), HipBuffer(12 * P), HipBuffer(4 * P)]
    st = EI.icp_start(EI.ICP_STARTS[0])
    V, N = XI.plane_maps(st)
    vn = [HipBuffer(a.nbytes).from_host(np.ascontiguousarray(a)) for a in (V, N)]
    imaps = [HipBuffer(4 * P), HipBuffer(4 * P), HipBuffer(4 * P), HipBuffer(4 * P), HipBuffer(12 * P)]
    try:
        gv.align_color_residuals_device(bufs[0].ptr, bufs[1].ptr, start, pc, *[b.ptr for b in maps])
        gv.sync()
        hostmap = gv.align_color_residuals(depth, rgba, start, pc)
        for b, k in zip(maps, ("r", "grad", "rc", "gradc", "flags")):
            assert np.array_equal(b.to_host().view(np.uint32), hostmap[k].view(np.uint32).reshape(-1)), k
        pi = capi.AlignIcpColorParams()
        gv.align_icp_color_residuals_device(bufs[0].ptr, bufs[1].ptr, st, vn[0].ptr, vn[1].ptr, st, pi, *[b.ptr for b in imaps])
        gv.sync()
        hostmap = gv.align_icp_color_residuals(depth, rgba, st, st, pi, vertex=V, normal=N)
        for b, k in zip(imaps, ("r", "rc", "flags", "assoc", "gradc")):
            assert np.array_equal(b.to_host().view(np.uint32), hostmap[k].view(np.uint32).reshape(-1)), k
        assert (hostmap["flags"] & 512).sum() > 1000
    finally:
        for b in bufs + maps + vn + imaps:
            b.free()


# ---- 8. readers -----------------------------------------------------------------------------------------------------------
def _log_raw(gv, name, rec):
    n = C.c_int64(0)
    buf = (rec * capi.TF_ALIGN_MAX_EVALUATIONS)()
    args = (gv.h, 0, buf) if name == "tf_align_group_log" else (gv.h, buf)
    assert getattr(gv.L, name)(*args, capi.TF_ALIGN_MAX_EVALUATIONS, C.byref(n)) == capi.TF_OK
    return bytes(buf)[:n.value * C.sizeof(rec)]


def test_the_calls_are_readers_and_leave_the_other_logs_alone(gpu_required):
    ov, gv, cam, _ = make_pair(res=CI.WALL_RES, cam=I.CAM, max_chunks=1 << 14)
    frames = CI.wall_frames()
    try:
        for k, (depth, rgba, pose) in enumerate(frames[:3]):
            ov.integrate_frame(depth, rgba, pose)
            gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, k)
        gv.update_meshes()
        ov.update_meshes()
        gv.sync()
        depth, rgba, pose = frames[1]
        rgba = E.expose(rgba, 0.8, 0.06)
        start = I.perturb(pose, *CI.wall_starts()[1])
        gv.align_frame(depth, start)
        gv.align_frame_icp(depth, start)
        gv.align_group([depth], [start])
        gv.align_frame_color(depth, rgba, start)
        gv.align_frame_icp_color(depth, rgba, start)
        names = [("tf_align_log", capi.AlignIter), ("tf_align_icp_log", capi.AlignIter), ("tf_align_group_log", capi.AlignIter),
                 ("tf_align_color_log", capi.AlignColorIter), ("tf_align_icp_color_log", capi.AlignColorIter)]
        before = [_log_raw(gv, *n) for n in names]
        assert all(len(b) > 0 for b in before)
        _on(gv)
        res = gv.align_frame_color(depth, rgba, start)
        assert res["n_photo_first"] > 1000 and len(gv.align_exposure_log(0)) == res["evaluations"]
        gv.align_color_residuals(depth, rgba, start)
        after = [_log_raw(gv, *n) for n in names]
        assert after[:3] == before[:3] and after[4] == before[4] and after[3] != before[3]  # the colour log is this call's
        x0 = gv.align_exposure_log(0).tobytes()
        res = gv.align_frame_icp_color(depth, rgba, start)
        gv.align_icp_color_residuals(depth, rgba, start)
        assert len(gv.align_exposure_log(1)) == res["evaluations"] and gv.align_exposure_log(0).tobytes() == x0
        last = [_log_raw(gv, *n) for n in names]
        assert last[:4] == after[:4] and last[4] != after[4]
        gv.align_set_exposure(None)
        depth, rgba, pose = frames[3]
        ov.integrate_frame(depth, rgba, pose)
        gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, 3)
        gv.sync()
        assert_chunks_equal(ov, gv, ov.list_chunks(), "after alignments with exposure compensation")
    finally:
        gv.close()
        ov.close()


# ---- 9. invalid settings --------------------------------------------------------------------------------------------------
def test_invalid_settings_are_refused_and_change_nothing(plane):
    gv, _ = plane
    _on(gv, unknowns=1, gain0=1.125, offset0=0.03125)
    kept = bytes(gv.align_get_exposure()[1])
    bad = [dict(unknowns=-1), dict(unknowns=3), dict(gain0=np.nan), dict(offset0=np.inf), dict(min_gain=np.nan),
           dict(max_gain=np.inf), dict(min_gain=0.0), dict(min_gain=-1.0), dict(min_gain=2.0, max_gain=1.5, gain0=1.75),
           dict(gain0=0.2), dict(gain0=4.5)]
    for kw in bad:
        e = capi.AlignExposure(**kw)
        assert gv.L.tf_align_set_exposure(gv.h, C.byref(e)) == INV, kw
        on, cur = gv.align_get_exposure()
        assert on and bytes(cur) == kept, kw
    # ... and the cell still holds the pair that was set
    depth, rgba = EI.plane_frame()
    gv.align_frame_color(depth, rgba, EI.sdf_start(1), capi.AlignColorParams(levels=[(2, 1)]))
    x = gv.align_exposure_log(0)
    assert (x["gain"][0], x["offset"][0]) == (1.125, 0.03125) and (x["rank"] == 1).all()
    n = C.c_int64(0)
    go, valid = (C.c_double * 2)(), C.c_int32(0)
    for which in (-1, 2):
        assert gv.L.tf_align_exposure_log(gv.h, which, None, 0, C.byref(n)) == INV
        assert gv.L.tf_align_exposure_estimate(gv.h, which, go, C.byref(valid)) == INV
    assert gv.L.tf_align_get_exposure(gv.h, None, None) == INV
    e = capi.AlignExposure(min_gain=1.0, max_gain=1.0)  # an empty interval is allowed: the gain is fixed
    assert gv.L.tf_align_set_exposure(gv.h, C.byref(e)) == capi.TF_OK


# ---- 10. the C++ mirror ---------------------------------------------------------------------------------------------------
def test_host_mirror_align_exposure(gpu_required, tmp_path):
    exe = str(tmp_path / "mirror_align_exposure")
    src = os.path.join(ROOT, "tests", "cpp_align_exposure", "mirror_align_exposure.cpp")
    lib = os.path.join(ROOT, "texturefusion_amd")
    subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", src, "-o", exe, "-L" + lib, "-ltexfusion_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "mirror ok" in r.stdout, r.stdout + r.stderr
