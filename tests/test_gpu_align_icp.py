"""Projective ICP on the MI355X (tf_align_icp.hip): the maps of one evaluation against the restatement bit for bit, the
first evaluation's sums against exact sums, the known answer from 120 mm / 8 degrees, a multi-step run on raycast maps
against the restatement, host and device forms, tf_track_frame from a start tf_align_frame cannot capture, invalid
arguments, the read-only guarantee and the C++ mirror.  Everything runs on the hand-built corner at 160 x 120 or smaller."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import align_icp_inputs as II
from tests import align_icp_ref as K
from tests import align_inputs as I
from tests import align_ref as R
from tests.util import HipBuffer, sorted_ids
from texturefusion_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = synth.Camera(13, 9, 11.0, 11.0, 6.5, 4.5)
NEAR, FAR, STEPS = 0.05, 5.0, 1024  # the default ray parameters
f32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))


def _params(**kw):
    """the same parameters for the restatement (dict) and the library (tf_align_icp_params)"""
    return K.params(**kw), capi.AlignIcpParams(**kw)


@pytest.fixture(scope="module")
def hand(gpu_required):
    gv = capi.Volume(I.HAND_RES, I.CAM, max_chunks=1 << 10)
    ids, s, w, c = I.hand_corner()
    for k in range(len(ids)):
        gv.set_chunk(ids[k], s[k], w[k], c[k])
    gv.sync()
    true = I.hand_pose()
    yield gv, true, I.hand_depth(true)
    gv.close()


@pytest.fixture(scope="module")
def ray_maps(hand):
    """the device's own maps of the hand-built corner from the 80 mm / 5 deg start: raycast once, shared, left unchanged"""
    gv, _, _ = hand
    at = II.ladder_start(0.080, 5.0)
    m = gv.raycast(at, NEAR, FAR, STEPS)
    assert (m["depth"] > 0).sum() >= 100
    return at, m["vertex"], m["normal"]


def _same_maps(got, want):
    assert np.array_equal(got["flags"], want["flags"])
    assert np.array_equal(got["assoc"], want["assoc"])
    assert np.array_equal(got["r"].view(np.uint32), want["r"].view(np.uint32))


def _log_raw(gv, fn="tf_align_icp_log", ty=capi.AlignIter, *lead):
    n = C.c_int64(0)
    buf = (ty * capi.TF_ALIGN_MAX_EVALUATIONS)()
    assert getattr(gv.L, fn)(gv.h, *lead, buf, capi.TF_ALIGN_MAX_EVALUATIONS, C.byref(n)) == capi.TF_OK
    return bytes(buf)[:n.value * C.sizeof(ty)]


# ---- 1. the maps of one evaluation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 3])
def test_maps_equal_the_restatement_on_raycast_maps(hand, ray_maps, stride):
    gv, true, depth = hand
    at, V, N = ray_maps
    pose = II.ladder_start(0.040, 2.0)  # the frame elsewhere than the model camera: pixels associate across columns and rows
    pd, pc = _params(levels=[(stride, 1)], max_distance=0.03)  # about half of the pixels inside the gate
    want = K.rows(depth, pose, V, N, at, I.CAM, stride, pd)
    assert (want["flags"] == 15).sum() > 3000 // stride ** 2 and (want["flags"] == 7).sum() > 3000 // stride ** 2
    assert (want["assoc"] >= 0).sum() > (want["flags"] == 15).sum()
    _same_maps(gv.align_icp_residuals(depth, pose, at, pc, vertex=V, normal=N), want)  # host maps
    _same_maps(gv.align_icp_residuals(depth, pose, at, pc), want)                      # the call's own raycast
    bufs = [HipBuffer(a.nbytes).from_host(a) for a in (depth, V, N)]
    outs = [HipBuffer(depth.nbytes) for _ in range(3)]
    try:  # everything on the device; the raycast written there too
        gv.raycast_device(at, NEAR, FAR, STEPS, d_normal=bufs[2].ptr, d_vertex=bufs[1].ptr)
        gv.align_icp_residuals_device(bufs[0].ptr, pose, bufs[1].ptr, bufs[2].ptr, at, pc, outs[0].ptr, outs[1].ptr, outs[2].ptr)
        gv.sync()
        got = dict(r=outs[0].to_host().view(np.float32).reshape(depth.shape), flags=outs[1].to_host().view(np.uint32).reshape(depth.shape),
                   assoc=outs[2].to_host().view(np.int32).reshape(depth.shape))
        _same_maps(got, want)
    finally:
        for b in bufs + outs:
            b.free()


@pytest.mark.parametrize("stride", [1, 3])
def test_maps_equal_the_restatement_with_tiles_over_both_borders(hand, stride):
    """a 13 x 9 camera: one full tile column and a partial one, one full tile row and a partial one"""
    gv, true, _ = hand
    gv.raycast_camera(SMALL)
    try:
        depth = I.hand_depth(true, SMALL, edge_voxels=0.0)
        at = II.ladder_start(0.040, 2.0)
        m = gv.raycast(at, NEAR, FAR, STEPS)
        pd, pc = _params(levels=[(stride, 1)])
        want = K.rows(depth, true, m["vertex"], m["normal"], at, SMALL, stride, pd)
        assert (want["flags"] == 15).sum() > 3
        _same_maps(gv.align_icp_residuals(depth, true, at, pc, vertex=m["vertex"], normal=m["normal"]), want)
        _same_maps(gv.align_icp_residuals(depth, true, at, pc), want)
    finally:
        gv.raycast_camera(None)


@pytest.mark.parametrize("stride", [1, 3])
def test_maps_equal_the_restatement_on_analytic_maps(hand, stride):
    gv, true, depth = hand
    """the model camera 120 mm and 20 degrees away, a block of its pixels blanked: every flag value occurs"""
    at = II.ladder_start(0.120, 20.0)
    V, N = II.hand_model_maps(at)
    N = N.copy()
    N[:, 40:60, 50:90] = 0.0
    pose = II.ladder_start(0.080, 5.0)
    pd, pc = _params(levels=[(stride, 1)], max_distance=0.08, max_residual=0.05)
    want = K.rows(depth, pose, V, N, at, I.CAM, stride, pd)
    for fl, least in ((0, 1000), (1, 200), (3, 10), (7, 150), (15, 500)):
        assert (want["flags"] == fl).sum() > least, fl
    _same_maps(gv.align_icp_residuals(depth, pose, at, pc, vertex=V, normal=N), want)


# ---- 2. the first evaluation's sums ---------------------------------------------------------------------------------------
def _check_sums(rec, sm):
    assert rec["n_valid"] == sm["n_valid"] and rec["n_sampled"] == sm["n_sampled"]
    got = np.concatenate([rec["A21"], rec["b"], [rec["sum_r2"], rec["sum_wr2"]]])
    want = np.concatenate([sm["A21"], sm["b"], [sm["sum_r2"], sm["sum_wr2"]]])
    bound = sm["n_valid"] * 2.0 ** -52 * sm["mag"]  # an f64 sum of exact terms in any order
    print("sums: largest |delta| / bound = %.3g" % np.max(np.abs(got - want) / np.maximum(bound, 1e-300)))
    assert np.all(np.abs(got - want) <= bound), np.abs(got - want) / bound


@pytest.mark.parametrize("huber", [0.0, 0.02])
def test_first_evaluation_sums_against_exact_sums(hand, ray_maps, huber):
    gv, true, depth = hand
    at, V, N = ray_maps
    for stride in (1, 3):
        pd, pc = _params(levels=[(stride, 1)], huber=huber)
        res = gv.align_frame_icp(depth, at, at, pc)  # the model raycast at the start, as ray_maps
        rw = K.rows(depth, at, V, N, at, I.CAM, stride, pd)
        assert res["n_valid_first"] == int((rw["fl"] == 15).sum()) > 500
        _check_sums(gv.align_icp_log()[0], R.sums(rw, pd))


# ---- 3. the known answer --------------------------------------------------------------------------------------------------
def test_known_answer_from_120_mm_and_8_degrees(hand):
    gv, true, depth = hand
    start = II.ladder_start(0.120, 8.0)
    V, N = II.hand_model_maps(start)
    bufs = [HipBuffer(a.nbytes).from_host(a) for a in (depth, V, N)]
    d_res = HipBuffer(C.sizeof(capi.AlignResult))
    try:
        gv.align_frame_icp_device(bufs[0].ptr, start, bufs[1].ptr, bufs[2].ptr, start, capi.AlignIcpParams(), d_res.ptr)
        gv.sync()
        res = gv.align_result(d_res.to_host())
    finally:
        for b in bufs + [d_res]:
            b.free()
    dt, dr = R.pose_distance(res["pose"], true)
    print("120 mm / 8 deg: status %d, %d evaluations, %.3g m and %.3g rad from the true pose" % (
        res["status"], res["evaluations"], dt, dr))
    assert res["status"] == capi.TF_ALIGN_CONVERGED
    assert dt <= II.ICP_TOL_T and dr <= II.ICP_TOL_R
    assert res["n_valid_last"] == int((depth > 0).sum()) == 10357
    log = gv.align_icp_log()
    assert len(log) == res["evaluations"] and [r["stride"] for r in log][:1] == [4] and log[-1]["stride"] == 1
    assert np.array_equal(log[0]["pose"].astype(np.float32), start)


# ---- 4. a multi-step run on raycast maps ----------------------------------------------------------------------------------
def test_run_on_raycast_maps_follows_the_restatement(hand, ray_maps):
    gv, true, depth = hand
    at, V, N = ray_maps
    pd, pc = _params()
    want, wlog = K.align(depth, at, V, N, at, I.CAM, pd)
    res = gv.align_frame_icp(depth, at, None, pc)  # the model raycast at the start pose
    log = gv.align_icp_log()
    dt, dr = R.pose_distance(res["pose"], want["pose"])
    print("80 mm / 5 deg on raycast maps: status %d, %d evaluations, %.3g m and %.3g rad from the restatement's end, %.3g m "
          "from the true pose" % (res["status"], res["evaluations"], dt, dr, R.pose_distance(res["pose"], true)[0]))
    assert res["status"] == want["status"] and res["evaluations"] == want["evaluations"] == len(log)
    assert [(r["level"], r["stride"], r["n_sampled"], r["n_valid"]) for r in log] == \
           [(r["level"], r["stride"], r["n_sampled"], r["n_valid"]) for r in wlog]
    assert dt <= II.ICP_TOL_T and dr <= II.ICP_TOL_R
    assert res["n_valid_first"] == wlog[0]["n_valid"] and res["n_valid_last"] == wlog[-1]["n_valid"] > 9000


# ---- 5. forms and repeatability -------------------------------------------------------------------------------------------
def test_host_form_equals_the_device_form_and_runs_repeat_bit_for_bit(hand):
    gv, true, depth = hand
    start = II.ladder_start(0.060, 3.0)
    pc = capi.AlignIcpParams(damping=1e-4)
    host = capi.AlignResult()
    sp = np.ascontiguousarray(start, np.float32)
    assert gv.L.tf_align_frame_icp(gv.h, f32p(depth), f32p(sp), None, C.byref(pc), C.byref(host)) == capi.TF_OK
    host_log = _log_raw(gv)
    assert host.status <= capi.TF_ALIGN_MAX_ITERS and host.evaluations >= 4 and len(host_log) == host.evaluations * 392
    bufs = [HipBuffer(depth.nbytes).from_host(depth), HipBuffer(3 * depth.nbytes), HipBuffer(3 * depth.nbytes)]
    d_res = HipBuffer(C.sizeof(capi.AlignResult))
    try:
        gv.raycast_device(start, NEAR, FAR, STEPS, d_normal=bufs[2].ptr, d_vertex=bufs[1].ptr)
        for _ in range(2):
            gv.align_frame_icp_device(bufs[0].ptr, start, bufs[1].ptr, bufs[2].ptr, start, pc, d_res.ptr)
            gv.sync()
            assert bytes(d_res.to_host()) == bytes(host)
            assert _log_raw(gv) == host_log
    finally:
        for b in bufs + [d_res]:
            b.free()
    again = capi.AlignResult()
    assert gv.L.tf_align_frame_icp(gv.h, f32p(depth), f32p(sp), f32p(sp), C.byref(pc), C.byref(again)) == capi.TF_OK
    assert bytes(again) == bytes(host) and _log_raw(gv) == host_log


# ---- 6. tf_track_frame ----------------------------------------------------------------------------------------------------
def test_track_frame_from_a_start_the_sdf_alignment_cannot_capture(hand):
    """every ray of the 80 mm / 5 deg start hits the hand-built layers (tests/align_icp_inputs.py), so the model is raycast
    from there; tf_align_frame alone finds no valid pixel"""
    gv, true, depth = hand
    start = II.ladder_start(*II.TRACK_START)
    sp = capi.AlignParams(**I.SCENE_PARAMS)
    alone = gv.align_frame(depth, start, sp)
    assert alone["status"] == capi.TF_ALIGN_TOO_FEW and alone["n_valid_first"] == 0
    want = gv.align_frame(depth, true, sp)  # the SDF stage owns the fixed point
    assert want["status"] <= capi.TF_ALIGN_MAX_ITERS
    out = gv.track_frame(depth, start, None, sp)
    dt, dr = R.pose_distance(out["pose"], want["pose"])
    it, ir = R.pose_distance(out["icp"]["pose"], true)
    print("track: stage %d, icp status %d (%d evaluations, %.3g m %.3g rad from the true pose), sdf status %d; %.3g m and "
          "%.3g rad from tf_align_frame's end from the true pose" % (out["stage"], out["icp"]["status"], out["icp"]["evaluations"],
                                                                    it, ir, out["sdf"]["status"], dt, dr))
    assert out["stage"] == 2 and out["icp"]["status"] <= capi.TF_ALIGN_MAX_ITERS and out["sdf"]["status"] <= capi.TF_ALIGN_MAX_ITERS
    assert np.array_equal(out["pose"], out["sdf"]["pose"])
    assert dt <= I.FIXED_TOL_T and dr <= I.FIXED_TOL_R
    # the stages' logs are the stages' own
    assert len(gv.align_icp_log()) == out["icp"]["evaluations"] and len(gv.align_log()) == out["sdf"]["evaluations"]
    # an ICP that cannot start: stage 0, the caller's pose, the SDF stage not run
    out = gv.track_frame(np.zeros_like(depth), start, None, sp)
    assert out["stage"] == 0 and out["icp"]["status"] == capi.TF_ALIGN_TOO_FEW and out["sdf"]["status"] == -1
    assert np.array_equal(out["pose"], start)


# ---- 7. invalid arguments -------------------------------------------------------------------------------------------------
def _other_logs(gv):
    return (_log_raw(gv, "tf_align_log"), _log_raw(gv, "tf_align_color_log", capi.AlignColorIter),
            _log_raw(gv, "tf_align_group_log", capi.AlignIter, 0))


def _run_the_other_aligners(gv, depth, pose):
    rgba = np.full(depth.shape + (4,), 200, np.uint8)
    gv.align_frame(depth, pose)
    gv.align_frame_color(depth, rgba, pose)
    gv.align_group([depth], [pose])
    logs = _other_logs(gv)
    assert all(len(x) > 0 for x in logs)
    return logs


def test_invalid_arguments_launch_nothing(hand):
    gv, true, depth = hand
    L = gv.L
    start = np.ascontiguousarray(II.ladder_start(0.040, 2.0), np.float32)
    others = _run_the_other_aligners(gv, depth, I.perturb(true, I.HAND_DELTA, np.zeros(3)))
    gv.align_frame_icp(depth, start)
    good_log = _log_raw(gv)
    assert len(good_log) >= 2 * 392
    res, trk = capi.AlignResult(), capi.TrackResult()
    C.memset(C.byref(res), 0x5A, C.sizeof(res))
    C.memset(C.byref(trk), 0x5A, C.sizeof(trk))
    preset, preset_trk = bytes(res), bytes(trk)
    d_res = HipBuffer(C.sizeof(res)).from_host(np.frombuffer(preset, np.uint8))
    V, N = II.hand_model_maps(start)
    bufs = [HipBuffer(a.nbytes).from_host(a) for a in (depth, V, N)]
    sdf = capi.AlignParams()
    INV = capi.TF_ERR_INVALID
    scratch = np.full(depth.shape, 7.0, np.float32)
    d_out = HipBuffer(depth.nbytes).from_host(scratch)

    def call(pc=None, pose=start, mpose=start, ray=False, iters=False, track=True, host=True):
        """every entry point with one thing wrong.  ray: only the forms that raycast themselves refuse it; iters: the
        residual forms do not read them; track: tf_track_frame takes the argument at all"""
        pc = pc or capi.AlignIcpParams()
        pp, mp = f32p(pose) if pose is not None else None, f32p(mpose) if mpose is not None else None
        if host:
            assert L.tf_align_frame_icp(gv.h, f32p(depth), pp, mp, C.byref(pc), C.byref(res)) == INV
            if track:
                assert L.tf_track_frame(gv.h, f32p(depth), pp, C.byref(pc), C.byref(sdf), C.byref(trk)) == INV
            if not iters:
                assert L.tf_align_icp_residuals(gv.h, f32p(depth), pp, None, None, mp, C.byref(pc), f32p(scratch), None, None) == INV
        if not ray:
            assert L.tf_align_frame_icp_device(gv.h, bufs[0].ptr, pp, bufs[1].ptr, bufs[2].ptr, mp, C.byref(pc), d_res.ptr) == INV
            if not iters:
                assert L.tf_align_icp_residuals_device(gv.h, bufs[0].ptr, pp, bufs[1].ptr, bufs[2].ptr, mp, C.byref(pc), None, None,
                                                       d_out.ptr) == INV

    try:
        for kw in (dict(n_levels=0), dict(n_levels=5), dict(stride=[0, 1, 1, 1]), dict(min_depth=np.nan),
                   dict(min_depth=2.0, max_depth=1.0), dict(huber=-0.1), dict(damping=-1e-3), dict(eps_t=-1e-6), dict(eps_r=np.inf),
                   dict(max_residual=np.nan), dict(max_distance=-0.01), dict(max_distance=np.nan), dict(max_distance=np.inf)):
            call(capi.AlignIcpParams(**kw))
        for kw in (dict(iters=[30, 30, 5, 0]), dict(iters=[-1, 3, 2, 0])):
            call(capi.AlignIcpParams(**kw), iters=True)
        for kw in (dict(ray_near=-0.1), dict(ray_near=1.0, ray_far=1.0), dict(ray_far=np.inf), dict(ray_near=np.nan), dict(ray_max_steps=0)):
            call(capi.AlignIcpParams(**kw), ray=True)
        for entry, bad in ((0, np.nan), (3, np.inf), (11, -np.inf)):
            q = start.copy()
            q.reshape(12)[entry] = bad
            call(pose=q)                # the frame's pose
            call(mpose=q, track=False)  # the model's
        call(pose=None)
        call(mpose=None, host=False)    # the device forms need a model pose
        pc = capi.AlignIcpParams()
        sp = f32p(start)
        # null images, maps, parameters and results
        assert L.tf_align_frame_icp(gv.h, None, sp, None, C.byref(pc), C.byref(res)) == INV
        assert L.tf_align_frame_icp(gv.h, f32p(depth), sp, None, None, C.byref(res)) == INV
        assert L.tf_align_frame_icp(gv.h, f32p(depth), sp, None, C.byref(pc), None) == INV
        assert L.tf_align_frame_icp_device(gv.h, None, sp, bufs[1].ptr, bufs[2].ptr, sp, C.byref(pc), d_res.ptr) == INV
        assert L.tf_align_frame_icp_device(gv.h, bufs[0].ptr, sp, None, bufs[2].ptr, sp, C.byref(pc), d_res.ptr) == INV
        assert L.tf_align_frame_icp_device(gv.h, bufs[0].ptr, sp, bufs[1].ptr, None, sp, C.byref(pc), d_res.ptr) == INV
        assert L.tf_align_frame_icp_device(gv.h, bufs[0].ptr, sp, bufs[1].ptr, bufs[2].ptr, sp, C.byref(pc), None) == INV
        assert L.tf_align_frame_icp_device(gv.h, bufs[0].ptr, sp, bufs[1].ptr, bufs[2].ptr, sp, None, d_res.ptr) == INV
        assert L.tf_align_icp_residuals(gv.h, f32p(depth), sp, f32p(V), None, sp, C.byref(pc), None, None, None) == INV  # one map of two
        assert L.tf_align_icp_residuals_device(gv.h, bufs[0].ptr, sp, None, bufs[2].ptr, sp, C.byref(pc), None, None, None) == INV
        assert L.tf_track_frame(gv.h, None, sp, C.byref(pc), C.byref(sdf), C.byref(trk)) == INV
        assert L.tf_track_frame(gv.h, f32p(depth), sp, None, C.byref(sdf), C.byref(trk)) == INV
        assert L.tf_track_frame(gv.h, f32p(depth), sp, C.byref(pc), None, C.byref(trk)) == INV
        assert L.tf_track_frame(gv.h, f32p(depth), sp, C.byref(pc), C.byref(sdf), None) == INV
        for kw in (dict(n_levels=0), dict(huber=-1.0), dict(iters=[60, 30, 0, 0])):  # the SDF stage's parameters
            bad = capi.AlignParams(**kw)
            assert L.tf_track_frame(gv.h, f32p(depth), sp, C.byref(pc), C.byref(bad), C.byref(trk)) == INV
        n = C.c_int64(0)
        assert L.tf_align_icp_log(gv.h, None, 3, C.byref(n)) == INV and L.tf_align_icp_log(gv.h, None, 0, None) == INV
        # nothing was written, on the host or on the device, and nothing ran: the four logs are still the good calls'
        assert bytes(res) == preset and bytes(trk) == preset_trk and bytes(d_res.to_host()) == preset
        assert (scratch == 7.0).all() and bytes(d_out.to_host()) == scratch.tobytes()
        assert _log_raw(gv) == good_log and _other_logs(gv) == others
    finally:
        for b in bufs + [d_res, d_out]:
            b.free()


# ---- 8. read-only ---------------------------------------------------------------------------------------------------------
def _snapshot(gv):
    ids = sorted_ids(gv.list_chunks())
    s, w, c = gv.get_chunks(ids)
    return (bytes(gv.stats()), sorted_ids(gv.dirty()).tobytes(), ids.tobytes(), s.tobytes(), w.tobytes(), c.tobytes(),
            gv.check_summaries(), gv.check_neighbours().tobytes(), gv.model_stream_stats())


def test_read_only_and_the_other_logs_keep_their_meaning(hand):
    gv, true, depth = hand
    others = _run_the_other_aligners(gv, depth, I.perturb(true, I.HAND_DELTA, np.zeros(3)))
    before = _snapshot(gv)
    start = II.ladder_start(0.080, 5.0)
    assert gv.align_frame_icp(depth, start)["n_valid_last"] > 9000
    gv.align_icp_residuals(depth, start)
    V, N = II.hand_model_maps(start)
    bufs = [HipBuffer(a.nbytes).from_host(a) for a in (depth, V, N)]
    d_res, d_out = HipBuffer(C.sizeof(capi.AlignResult)), HipBuffer(depth.nbytes)
    try:
        gv.align_frame_icp_device(bufs[0].ptr, start, bufs[1].ptr, bufs[2].ptr, start, capi.AlignIcpParams(), d_res.ptr)
        gv.align_icp_residuals_device(bufs[0].ptr, start, bufs[1].ptr, bufs[2].ptr, start, capi.AlignIcpParams(), d_assoc=d_out.ptr)
        gv.sync()
    finally:
        for b in bufs + [d_res, d_out]:
            b.free()
    assert _snapshot(gv) == before and _other_logs(gv) == others
    color_group = others[1:]
    assert gv.track_frame(depth, start)["stage"] == 2  # its SDF stage is a tf_align_frame call: that log is its own
    after = _snapshot(gv)
    assert after == before and _other_logs(gv)[1:] == color_group


# ---- 9. the C++ mirror ----------------------------------------------------------------------------------------------------
def test_host_mirror_align_icp(gpu_required, tmp_path):
    exe = str(tmp_path / "mirror_align_icp")
    src = os.path.join(ROOT, "tests", "cpp_align_icp", "mirror_align_icp.cpp")
    lib = os.path.join(ROOT, "texturefusion_amd")
    subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", src,
                    "-o", exe, "-L" + lib, "-ltexfusion_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                    "-lamdhip64"], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mirror ok" in r.stdout, r.stdout + r.stderr
