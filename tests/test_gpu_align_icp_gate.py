"""The ICP's normal-compatibility gate on the MI355X (tf_align_icp_gate.hip): the frame normals and the gated maps of one
evaluation against the restatement bit for bit -- on the unmasked corner and on the hand-built plane that puts one case at
each decision edge (tests/align_icp_gate_inputs.py), at strides 1, 2 and 4, at 160 x 120 and at 152 x 116 whose last tiles
are partial -- the tie to the ungated kernel, a gate set and cleared, the whole alignment from 120 mm / 8 degrees, the
entry points that share the path, invalid arguments."""
import ctypes as C

import numpy as np
import pytest

from tests import align_icp_gate_inputs as GI
from tests import align_icp_gate_ref as G
from tests import align_icp_inputs as II
from tests import align_icp_ref as K
from tests import align_inputs as I
from tests import align_ref as R
from tests import reloc_inputs as QI
from tests.util import HipBuffer
from texturefusion_amd import capi

pytestmark = pytest.mark.gpu
INV = capi.TF_ERR_INVALID
TRK = C.sizeof(capi.TrackResult)
f32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))


@pytest.fixture(scope="module")
def hand(gpu_required):
    """the hand-built corner; every test leaves the gate off"""
    gv = capi.Volume(I.HAND_RES, I.CAM, max_chunks=1 << 10, max_keyframes=8)
    ids, s, w, c = I.hand_corner()
    for k in range(len(ids)):
        gv.set_chunk(ids[k], s[k], w[k], c[k])
    gv.sync()
    yield gv
    gv.close()


@pytest.fixture()
def gated(hand):
    """the handle with a gate to set, off again afterwards"""
    yield hand
    hand.align_icp_set_gate(None)
    hand.raycast_camera(None)


def _same_maps(got, want):
    assert np.array_equal(got["flags"], want["flags"])
    assert np.array_equal(got["assoc"], want["assoc"])
    assert np.array_equal(got["r"].view(np.uint32), want["r"].view(np.uint32))


def _log_raw(gv):
    n = C.c_int64(0)
    buf = (capi.AlignIter * capi.TF_ALIGN_MAX_EVALUATIONS)()
    assert gv.L.tf_align_icp_log(gv.h, buf, capi.TF_ALIGN_MAX_EVALUATIONS, C.byref(n)) == capi.TF_OK
    return bytes(buf)[:n.value * C.sizeof(capi.AlignIter)]


def _check_tie(gated_maps, plain_maps):
    """r, assoc and bits 0 to 3 are the ungated kernel's (everywhere, so also wherever bit 5 is set or a low bit is clear)"""
    assert np.array_equal(gated_maps["flags"] & 15, plain_maps["flags"]) and plain_maps["flags"].max() <= 15
    assert np.array_equal(gated_maps["assoc"], plain_maps["assoc"])
    assert np.array_equal(gated_maps["r"].view(np.uint32), plain_maps["r"].view(np.uint32))
    fl = gated_maps["flags"]
    assert not (fl[(fl & 15) != 15] & 48).any() and not (fl[(fl & 16) == 0] & 32).any()  # each bit only above the lower ones


# ---- 1. the maps of one evaluation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2, 4])
def test_corner_maps_equal_the_restatement(gated, stride):
    gv = gated
    depth = GI.corner_unmasked()
    at = II.ladder_start(0.120, 8.0)
    V, N = II.hand_model_maps(at)
    pose = II.ladder_start(0.040, 2.0)  # the frame elsewhere than the model camera
    pd, pc = K.params(levels=[(stride, 1)]), capi.AlignIcpParams(levels=[(stride, 1)])
    gd = G.gate()
    want = G.rows(depth, pose, V, N, at, I.CAM, stride, pd, gd)
    for fl, least in ((15, 50 // stride), (31, 100 // stride), (63, 10000 // stride ** 2)):
        assert (want["flags"] == fl).sum() > least, fl
    plain = gv.align_icp_residuals(depth, pose, at, pc, vertex=V, normal=N)
    gv.align_icp_set_gate(capi.AlignIcpGate())
    got = gv.align_icp_residuals(depth, pose, at, pc, vertex=V, normal=N)
    _same_maps(got, want)
    _check_tie(got, plain)
    n = gv.align_icp_frame_normals(depth, pc)
    fn = G.frame_normals(depth, I.CAM, stride, pd, gd)
    assert np.array_equal(n.view(np.uint32), fn["n"].view(np.uint32))
    bufs = [HipBuffer(a.nbytes).from_host(a) for a in (depth, V, N)]
    outs = [HipBuffer(depth.nbytes) for _ in range(3)] + [HipBuffer(3 * depth.nbytes)]
    try:  # everything on the device
        gv.align_icp_residuals_device(bufs[0].ptr, pose, bufs[1].ptr, bufs[2].ptr, at, pc, outs[0].ptr, outs[1].ptr, outs[2].ptr)
        gv.align_icp_frame_normals_device(bufs[0].ptr, pc, capi.AlignIcpGate(), outs[3].ptr)
        gv.sync()
        dev = dict(r=outs[0].to_host().view(np.float32).reshape(depth.shape), flags=outs[1].to_host().view(np.uint32).reshape(depth.shape),
                   assoc=outs[2].to_host().view(np.int32).reshape(depth.shape))
        _same_maps(dev, want)
        assert np.array_equal(outs[3].to_host().view(np.uint32), fn["n"].view(np.uint32).reshape(-1))
    finally:
        for b in bufs + outs:
            b.free()


@pytest.mark.parametrize("cam", [GI.CAM, GI.CAM_ODD], ids=["160x120", "152x116"])
@pytest.mark.parametrize("stride", [1, 2, 4])
def test_plane_maps_equal_the_restatement_at_every_edge(gated, cam, stride):
    gv = gated
    gv.raycast_camera(cam)  # the camera of the aligners' images too
    depth, V, N = GI.plane(cam, stride)
    pd, pc = K.params(levels=[(stride, 1)]), capi.AlignIcpParams(levels=[(stride, 1)])
    plain = gv.align_icp_residuals(depth, GI.EYE, GI.EYE, pc, vertex=V, normal=N)
    sampled, inner = GI.border_masks(cam, stride)
    for name, gk in GI.GATES.items():
        want = G.rows(depth, GI.EYE, V, N, GI.EYE, cam, stride, pd, G.gate(**gk))
        gv.align_icp_set_gate(capi.AlignIcpGate(**gk))
        got = gv.align_icp_residuals(depth, GI.EYE, GI.EYE, pc, vertex=V, normal=N)
        _same_maps(got, want)
        _check_tie(got, plain)
        fl = got["flags"]
        for case, (x, y) in GI.centres().items():
            assert fl[y, x] == GI.EXPECT[name][case], (name, case, int(fl[y, x]))
        assert fl[GI.PLAIN[1], GI.PLAIN[0]] == 63, name
        assert not (fl[sampled & ~inner] & 16).any() and (fl[sampled & ~inner] == 15).sum() > 20
        n = gv.align_icp_frame_normals(depth, pc, capi.AlignIcpGate(**gk))
        fn = G.frame_normals(depth, cam, stride, pd, G.gate(**gk))
        assert np.array_equal(n.view(np.uint32), fn["n"].view(np.uint32)), name
        assert not n[:, ~inner].any()


# ---- 2. a gate set and cleared --------------------------------------------------------------------------------------------
def _run(gv, bufs, start, pc, d_res):
    """one alignment on device maps -> (the tf_align_result's bytes, the log's bytes)"""
    gv.align_frame_icp_device(bufs[0].ptr, start, bufs[1].ptr, bufs[2].ptr, start, pc, d_res.ptr)
    gv.sync()
    return bytes(d_res.to_host()), _log_raw(gv)


def test_a_gate_set_and_cleared_leaves_no_trace(gpu_required):
    depth = GI.corner_unmasked()
    start = II.ladder_start(0.060, 3.0)
    V, N = II.hand_model_maps(start)
    pc = capi.AlignIcpParams()
    bufs = [HipBuffer(a.nbytes).from_host(a) for a in (depth, V, N)]
    d_res = HipBuffer(C.sizeof(capi.AlignResult))
    never, other = capi.Volume(I.HAND_RES, I.CAM, max_chunks=64), capi.Volume(I.HAND_RES, I.CAM, max_chunks=64)
    try:
        want_res, want_log = _run(never, bufs, start, pc, d_res)
        want_maps = never.align_icp_residuals(depth, start, start, pc, vertex=V, normal=N)
        assert never.align_icp_get_gate()[0] is False and len(want_log) >= 4 * 392

        def same():
            res, log = _run(other, bufs, start, pc, d_res)
            assert res == want_res and log == want_log
            _same_maps(other.align_icp_residuals(depth, start, start, pc, vertex=V, normal=N), want_maps)

        g = capi.AlignIcpGate(min_normal_cos=0.5, max_depth_jump=0.25)
        other.align_icp_set_gate(g)
        on, back = other.align_icp_get_gate()
        assert on is True and bytes(back) == bytes(g)
        res, log = _run(other, bufs, start, pc, d_res)
        assert res != want_res and log != want_log  # the gate is read
        other.align_icp_set_gate(None)
        on, back = other.align_icp_get_gate()
        assert on is False and bytes(back) == bytes(capi.AlignIcpGate())
        same()
        other.align_icp_set_gate(g)
        other.reset()  # the ICP's state is made anew: the gate is off
        assert other.align_icp_get_gate()[0] is False
        same()
    finally:
        for b in bufs + [d_res]:
            b.free()
        never.close()
        other.close()


# ---- 3. the whole alignment -----------------------------------------------------------------------------------------------
def test_gated_alignment_from_120_mm_and_8_degrees_follows_the_restatement(gated):
    """held as tests/test_gpu_align_icp.py holds the ungated call (its tests 3 and 4): status, evaluations and every record's
    level, stride and counts are the restatement's, the end pose within ICP_TOL_* of the restatement's and of the true pose"""
    gv = gated
    true, depth = I.hand_pose(), GI.corner_unmasked()
    start = II.ladder_start(0.120, 8.0)
    V, N = II.hand_model_maps(start)
    pd, pc = K.params(), capi.AlignIcpParams()
    want, wlog = G.align(depth, start, V, N, start, I.CAM, pd, G.gate())
    bufs = [HipBuffer(a.nbytes).from_host(a) for a in (depth, V, N)]
    d_res = HipBuffer(C.sizeof(capi.AlignResult))
    try:
        gv.align_frame_icp_device(bufs[0].ptr, start, bufs[1].ptr, bufs[2].ptr, start, pc, d_res.ptr)
        gv.sync()
        plain = gv.align_result(d_res.to_host())
        gv.align_icp_set_gate(capi.AlignIcpGate())
        gv.align_frame_icp_device(bufs[0].ptr, start, bufs[1].ptr, bufs[2].ptr, start, pc, d_res.ptr)
        gv.sync()
        res = gv.align_result(d_res.to_host())
    finally:
        for b in bufs + [d_res]:
            b.free()
    log = gv.align_icp_log()
    dt, dr = R.pose_distance(res["pose"], true)
    wt, wr = R.pose_distance(res["pose"], want["pose"])
    pt, pr = R.pose_distance(plain["pose"], true)
    print("120 mm / 8 deg, unmasked corner: gated status %d, %d evaluations, %.3g m %.3g rad from the true pose, %.3g m %.3g rad "
          "from the restatement's end; ungated %d evaluations, %.3g m %.3g rad from the true pose" % (
              res["status"], res["evaluations"], dt, dr, wt, wr, plain["evaluations"], pt, pr))
    assert res["status"] == want["status"] == capi.TF_ALIGN_CONVERGED and res["evaluations"] == want["evaluations"] == len(log)
    assert [(r["level"], r["stride"], r["n_sampled"], r["n_valid"]) for r in log] == \
           [(r["level"], r["stride"], r["n_sampled"], r["n_valid"]) for r in wlog]
    assert wt <= II.ICP_TOL_T and wr <= II.ICP_TOL_R
    assert dt <= II.ICP_TOL_T and dr <= II.ICP_TOL_R
    assert res["n_valid_first"] == wlog[0]["n_valid"] and res["n_valid_last"] == wlog[-1]["n_valid"]
    assert np.array_equal(log[0]["pose"].astype(np.float32), start)
    assert plain["status"] <= capi.TF_ALIGN_MAX_ITERS and pt > II.ICP_TOL_T  # the ungated call on the same image
    assert res["evaluations"] <= plain["evaluations"]


# ---- 4. the entry points that share the path ------------------------------------------------------------------------------
def test_the_trackers_read_the_gate(gated):
    gv = gated
    true = I.hand_pose()
    depth = GI.corner_unmasked()
    start = np.ascontiguousarray(II.ladder_start(*II.TRACK_START), np.float32)
    icp, sdf = capi.AlignIcpParams(), capi.AlignParams(**I.SCENE_PARAMS)
    plain = capi.TrackResult()
    assert gv.L.tf_track_frame(gv.h, f32p(depth), f32p(start), C.byref(icp), C.byref(sdf), C.byref(plain)) == capi.TF_OK
    gv.align_icp_set_gate(capi.AlignIcpGate())
    alone = capi.AlignResult()
    assert gv.L.tf_align_frame_icp(gv.h, f32p(depth), f32p(start), None, C.byref(icp), C.byref(alone)) == capi.TF_OK
    alone_log = _log_raw(gv)
    host = capi.TrackResult()
    assert gv.L.tf_track_frame(gv.h, f32p(depth), f32p(start), C.byref(icp), C.byref(sdf), C.byref(host)) == capi.TF_OK
    assert bytes(host.icp) == bytes(alone) and _log_raw(gv) == alone_log
    assert host.stage >= 1 and alone.n_valid_first < plain.icp.n_valid_first  # the gate was read
    cell = capi.DevicePose()
    cell.pose[:] = [float(x) for x in start.reshape(12)]
    cell.valid = 1
    d_depth, d_start = HipBuffer(depth.nbytes).from_host(depth), HipBuffer(64).from_host(np.frombuffer(bytes(cell), np.uint8))
    d_out, d_pose = HipBuffer(256), HipBuffer(64)
    try:
        gv.track_frame_device(d_depth.ptr, d_start.ptr, icp, sdf, None, d_out.ptr, d_pose.ptr)
        gv.sync()
        assert bytes(d_out.to_host(TRK)) == bytes(host)
        assert _log_raw(gv) == alone_log
    finally:
        for b in (d_depth, d_start, d_out, d_pose):
            b.free()
    print("track, gated: ICP %d evaluations, %.3g m from the true pose; first valid %d gated, %d ungated" % (
        alone.evaluations, R.pose_distance(np.array(alone.pose, np.float32).reshape(3, 4), true)[0], alone.n_valid_first,
        plain.icp.n_valid_first))


def test_relocalise_reads_the_gate(gated):
    gv = gated
    kf_pose = QI.keyframe_poses()[3]
    kd, krgb = QI.frame(kf_pose)
    depth, rgb = QI.frame(QI.query_pose(3, 1))
    sp = capi.AlignParams(**I.SCENE_PARAMS)
    gv.keyframe_cache(5, krgb, kd, QI.pose_inv16(kf_pose))
    try:
        gv.reloc_configure()
        gv.reloc_index_add([5])
        plain = gv.relocalise(depth, rgb, capi.RelocaliseParams(sdf=sp))
        gv.align_icp_set_gate(capi.AlignIcpGate())
        res = gv.relocalise(depth, rgb, capi.RelocaliseParams(sdf=sp))
        assert res["status"] == plain["status"] == capi.TF_RELOC_FOUND and res["n_tried"] == 1 and res["kf_id"] == 5
        pose_k = np.ascontiguousarray(QI.rigid_inverse(QI.pose_inv16(kf_pose)))
        alone = capi.AlignResult()
        assert gv.L.tf_align_frame_icp(gv.h, f32p(depth), f32p(pose_k), None, C.byref(capi.AlignIcpParams()), C.byref(alone)) == capi.TF_OK
        t = res["tries"][0]
        assert t["raw"][:C.sizeof(capi.AlignResult)] == bytes(alone)
        assert t["track"]["icp"]["n_valid_first"] < plain["tries"][0]["track"]["icp"]["n_valid_first"]
    finally:
        gv.keyframe_release(5)


# ---- 5. invalid arguments -------------------------------------------------------------------------------------------------
def test_invalid_arguments_change_nothing(gated):
    gv = gated
    L = gv.L
    good = capi.AlignIcpGate(min_normal_cos=0.75, max_depth_jump=0.5)
    gv.align_icp_set_gate(good)
    for kw in (dict(min_normal_cos=np.nan), dict(min_normal_cos=-0.01), dict(min_normal_cos=np.nextafter(np.float32(1), np.float32(2))),
               dict(max_depth_jump=np.nan), dict(max_depth_jump=0.0), dict(max_depth_jump=-1.0), dict(max_depth_jump=-np.inf)):
        bad = capi.AlignIcpGate(**kw)
        assert L.tf_align_icp_set_gate(gv.h, C.byref(bad)) == INV, kw
        on, back = gv.align_icp_get_gate()
        assert on is True and bytes(back) == bytes(good)
    for ok in (dict(min_normal_cos=0.0), dict(min_normal_cos=1.0), dict(max_depth_jump=np.inf)):
        gv.align_icp_set_gate(capi.AlignIcpGate(**ok))
    on = C.c_int32(0)
    assert L.tf_align_icp_get_gate(gv.h, None, C.byref(on)) == INV and L.tf_align_icp_get_gate(gv.h, C.byref(good), None) == INV
    # the frame normals: nothing is written for a call that is refused
    depth = GI.corner_unmasked()
    out = np.full((3,) + depth.shape, 7.0, np.float32)
    pc, g = capi.AlignIcpParams(), capi.AlignIcpGate()
    d_depth, d_out = HipBuffer(depth.nbytes).from_host(depth), HipBuffer(out.nbytes).from_host(out)
    try:
        calls = [(None, pc, g, True), (depth, None, g, True), (depth, pc, None, True), (depth, pc, g, False),
                 (depth, capi.AlignIcpParams(n_levels=0), g, True), (depth, capi.AlignIcpParams(stride=[0, 1, 1, 1]), g, True),
                 (depth, capi.AlignIcpParams(min_depth=np.nan), g, True), (depth, capi.AlignIcpParams(min_depth=2.0, max_depth=1.0), g, True),
                 (depth, pc, capi.AlignIcpGate(max_depth_jump=0.0), True), (depth, pc, capi.AlignIcpGate(max_depth_jump=np.nan), True),
                 (depth, pc, capi.AlignIcpGate(min_normal_cos=2.0), True)]
        for d, p, gg, with_out in calls:
            pp, gp = (None if p is None else C.byref(p)), (None if gg is None else C.byref(gg))
            assert L.tf_align_icp_frame_normals(gv.h, None if d is None else f32p(d), pp, gp, f32p(out) if with_out else None) == INV
            assert L.tf_align_icp_frame_normals_device(gv.h, None if d is None else d_depth.ptr, pp, gp,
                                                       d_out.ptr if with_out else None) == INV
        gv.sync()
        assert (out == 7.0).all() and bytes(d_out.to_host()) == out.tobytes()
    finally:
        d_depth.free()
        d_out.free()


def test_the_new_entry_points_are_readers(gated):
    """none of them advances the model generation: the resident model stream stays current"""
    gv = gated
    depth = GI.corner_unmasked()
    pose = I.hand_pose()
    gv.render_model(pose, 0.1, 3.0, 4)  # the stream is packed and current
    before = gv.model_stream_stats()
    gv.align_icp_set_gate(capi.AlignIcpGate())
    gv.align_icp_get_gate()
    gv.align_icp_frame_normals(depth)
    d_depth, d_out = HipBuffer(depth.nbytes).from_host(depth), HipBuffer(3 * depth.nbytes)
    try:
        gv.align_icp_frame_normals_device(d_depth.ptr, capi.AlignIcpParams(), capi.AlignIcpGate(), d_out.ptr)
        gv.sync()
    finally:
        d_depth.free()
        d_out.free()
    gv.render_model(pose, 0.1, 3.0, 4)
    after = gv.model_stream_stats()
    assert (after["packs"], after["hits"]) == (before["packs"], before["hits"] + 1)  # a hit: nothing was repacked
