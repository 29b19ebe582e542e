"""The projective ICP's depth pyramid on the MI355X (tf_align_icp_pyramid.hip): the level images against the restatement bit
for bit at sizes with one tile, partial tiles and three levels and at every edge of the block rule; what a call is refused
for; the setting set, read and cleared; a level of a call with the setting on against a plain call of a second handle
whose camera is the level's, bit for bit; the default schedule against the restatement; the residual maps; the gate on
top of it; the device tracker.  Everything runs on the hand-built corner at 160 x 128 or smaller."""
import ctypes as C

import numpy as np
import pytest

from tests import align_icp_gate_ref as G
from tests import align_icp_inputs as II
from tests import align_icp_pyramid_inputs as PI
from tests import align_icp_pyramid_ref as Y
from tests import align_icp_ref as K
from tests import align_inputs as I
from tests import align_ref as R
from tests.util import HipBuffer
from texturefusion_amd import capi, synth

pytestmark = pytest.mark.gpu
INV = capi.TF_ERR_INVALID
TRK = C.sizeof(capi.TrackResult)
REC = C.sizeof(capi.AlignIter)
NEAR, FAR, STEPS = 0.05, 5.0, 1024  # the default ray parameters
f32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))


def _corner(cam):
    gv = capi.Volume(I.HAND_RES, cam, max_chunks=1 << 10)
    ids, s, w, c = I.hand_corner()
    for k in range(len(ids)):
        gv.set_chunk(ids[k], s[k], w[k], c[k])
    gv.sync()
    return gv


@pytest.fixture(scope="module")
def pair(gpu_required):
    """handle A, on which the pyramid is set, and handle B with the same chunks, which never has it on and whose raycast
    camera is set to a level's; every test leaves A's settings off and both raycast cameras unset"""
    a, b = _corner(PI.CAM_A), _corner(PI.CAM_A)
    yield a, b
    a.close()
    b.close()


@pytest.fixture()
def ab(pair):
    yield pair
    a, b = pair
    a.align_icp_set_pyramid(None)
    a.align_icp_set_gate(None)
    a.raycast_camera(None)
    b.raycast_camera(None)


def _log_raw(gv):
    n = C.c_int64(0)
    buf = (capi.AlignIter * capi.TF_ALIGN_MAX_EVALUATIONS)()
    assert gv.L.tf_align_icp_log(gv.h, buf, capi.TF_ALIGN_MAX_EVALUATIONS, C.byref(n)) == capi.TF_OK
    return bytes(buf)[:n.value * REC]


def _without_stride(log):
    a = np.frombuffer(log, np.uint8).reshape(-1, REC).copy()
    a[:, 4:8] = 0
    return a.tobytes()


def _same_maps(got, want):
    assert np.array_equal(got["flags"], want["flags"])
    assert np.array_equal(got["assoc"], want["assoc"])
    assert np.array_equal(got["r"].view(np.uint32), want["r"].view(np.uint32))


def _level_maps(b, cam, k, at):
    """handle B's raycast at the camera of level k of cam -> (V, N)"""
    b.raycast_camera(Y.level_cam(cam, k))
    m = b.raycast(at, NEAR, FAR, STEPS)
    b.raycast_camera(None)
    return m["vertex"], m["normal"]


# ---- 1. the level images --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,n", [(8, 8, 3), (16, 8, 3), (20, 12, 2), (36, 28, 2), (160, 128, 3)])
def test_level_images_equal_the_restatement(ab, W, H, n):
    gv, _ = ab
    gv.raycast_camera(synth.Camera(W, H, 16.0, 16.0, W / 2 - 1.0, H / 2 - 1.0))
    img, at = PI.edge_image(W, H)
    for jump in (PI.JUMP, np.float32(np.inf), np.float32(0.004)):
        want = Y.levels(img, n, jump)[1:]
        for m in range(1, n + 1):  # every count of levels: the launch stops after level m
            got = gv.align_icp_pyramid_depth(img, m, capi.AlignIcpPyramid(max_depth_jump=jump))
            assert len(got) == m
            for l in range(m):
                assert got[l].shape == want[l].shape
                assert np.array_equal(got[l].view(np.uint32), want[l].view(np.uint32)), (float(jump), m, l + 1)
    l1 = gv.align_icp_pyramid_depth(img, 1, capi.AlignIcpPyramid(max_depth_jump=PI.JUMP))[0]
    for name, _, want in PI.BLOCKS:  # each edge by its name
        X, Y_ = at[name]
        assert (l1[Y_, X] == 0) == (want is not None and want == 0), name
    for other in (PI.one_hole_per_block(W, H), np.zeros((H, W), np.float32)):
        assert not any(x.any() for x in gv.align_icp_pyramid_depth(other, n))
    # everything on the device, into buffers that are exactly as large as the levels
    want = Y.levels(img, n, PI.JUMP)[1:]
    d_img = HipBuffer(img.nbytes).from_host(img)
    outs = [HipBuffer(w.nbytes + 64).from_host(np.full(w.size + 16, 7.0, np.float32)) for w in want]
    try:
        gv.align_icp_pyramid_depth_device(d_img.ptr, n, capi.AlignIcpPyramid(max_depth_jump=PI.JUMP), [o.ptr for o in outs])
        gv.sync()
        for o, w in zip(outs, want):
            back = o.to_host().view(np.float32)
            assert np.array_equal(back[:w.size].view(np.uint32), w.reshape(-1).view(np.uint32))
            assert (back[w.size:] == 7.0).all()  # nothing past the level's last pixel
    finally:
        for x in [d_img] + outs:
            x.free()


def test_level_cameras(ab):
    gv, _ = ab
    for cam, top in ((PI.CAM_A, 2), (PI.CAM_B, 3)):
        gv.raycast_camera(cam)
        for l in range(top + 1):
            c4, w, h = gv.align_icp_pyramid_camera(l)
            lc = Y.level_cam(cam, l)
            assert (w, h) == (lc.width, lc.height) and list(c4) == [lc.fx, lc.fy, lc.cx, lc.cy]
    gv.raycast_camera(synth.Camera(160, 120, 131.25, 131.25, 79.5, 59.5))  # from the int-truncated intrinsics, not truncated again
    c4, w, h = gv.align_icp_pyramid_camera(2)
    assert list(c4) == [32.75, 32.75, 19.0, 14.0] and (w, h) == (40, 30)


# ---- 2. what a call is refused for ----------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(ab):
    gv, _ = ab
    L = gv.L
    depth = I.hand_depth(I.hand_pose(), PI.CAM_A)
    start = np.ascontiguousarray(II.ladder_start(0.040, 2.0), np.float32)
    V, N = II.hand_model_maps(start, PI.CAM_A)
    sdf = capi.AlignParams(**I.SCENE_PARAMS)
    plain3 = gv.align_icp_residuals(depth, start, start, capi.AlignIcpParams(levels=[(3, 1)]), vertex=V, normal=N)
    gv.align_icp_set_pyramid(capi.AlignIcpPyramid())
    cell = capi.DevicePose()
    cell.pose[:] = [float(x) for x in start.reshape(12)]
    cell.valid = 1
    d_depth, d_start = HipBuffer(depth.nbytes).from_host(depth), HipBuffer(64).from_host(np.frombuffer(bytes(cell), np.uint8))
    d_out, d_pose = HipBuffer(256).from_host(np.full(256, 7, np.uint8)), HipBuffer(64).from_host(np.full(64, 7, np.uint8))
    try:
        cases = [("stride 3", PI.CAM_A, [(4, 2), (3, 2), (1, 1)]), ("stride 16", PI.CAM_A, [(16, 2), (1, 1)]),
                 ("stride 8 does not divide 124", synth.Camera(160, 124, 128.0, 128.0, 79.0, 61.0), [(8, 2), (1, 1)]),
                 ("stride 0", PI.CAM_A, [(0, 1)])]
        for name, cam, levels in cases:
            gv.raycast_camera(None if cam is PI.CAM_A else cam)
            img = np.ascontiguousarray(np.resize(depth, (cam.height, cam.width)))
            pc = capi.AlignIcpParams(levels=levels)
            res = capi.AlignResult()
            res.status = 77
            assert L.tf_align_frame_icp(gv.h, f32p(img), f32p(start), None, C.byref(pc), C.byref(res)) == INV, name
            assert res.status == 77 and res.evaluations == 0
            trk = capi.TrackResult()
            trk.stage = 77
            assert L.tf_track_frame(gv.h, f32p(img), f32p(start), C.byref(pc), C.byref(sdf), C.byref(trk)) == INV, name
            assert trk.stage == 77
            if levels[0][0] not in (1, 2, 4, 8) or cam.height % levels[0][0]:
                r = np.full(img.shape, 7.0, np.float32)
                assert L.tf_align_icp_residuals(gv.h, f32p(img), f32p(start), None, None, None, C.byref(pc), f32p(r), None, None) == INV
                assert (r == 7.0).all()
            if cam is PI.CAM_A:
                assert L.tf_track_frame_device(gv.h, d_depth.ptr, d_start.ptr, C.byref(pc), C.byref(sdf), None, d_out.ptr, d_pose.ptr) == INV
        gv.raycast_camera(None)
        gv.sync()
        assert (d_out.to_host() == 7).all() and (d_pose.to_host() == 7).all()
        # the forms that take the caller's maps do not read the setting: stride 3 is theirs as ever
        _same_maps(gv.align_icp_residuals(depth, start, start, capi.AlignIcpParams(levels=[(3, 1)]), vertex=V, normal=N), plain3)
    finally:
        for x in (d_depth, d_start, d_out, d_pose):
            x.free()
    # bad settings: nothing changes
    good = capi.AlignIcpPyramid(max_depth_jump=0.5)
    gv.align_icp_set_pyramid(good)
    for jump in (np.nan, 0.0, -1.0, -np.inf):
        bad = capi.AlignIcpPyramid(max_depth_jump=jump)
        assert L.tf_align_icp_set_pyramid(gv.h, C.byref(bad)) == INV, jump
        on, back = gv.align_icp_get_pyramid()
        assert on is True and bytes(back) == bytes(good)
    gv.align_icp_set_pyramid(capi.AlignIcpPyramid(max_depth_jump=np.inf))
    # null pointers and sizes
    on, w = C.c_int32(0), C.c_int32(0)
    c4 = (C.c_float * 4)()
    assert L.tf_align_icp_get_pyramid(gv.h, None, C.byref(on)) == INV and L.tf_align_icp_get_pyramid(gv.h, C.byref(good), None) == INV
    assert L.tf_align_icp_pyramid_camera(gv.h, 1, None, C.byref(w), C.byref(w)) == INV
    assert L.tf_align_icp_pyramid_camera(gv.h, 1, c4, None, C.byref(w)) == INV
    assert L.tf_align_icp_pyramid_camera(gv.h, 4, c4, C.byref(w), C.byref(w)) == INV
    assert L.tf_align_icp_pyramid_camera(gv.h, -1, c4, C.byref(w), C.byref(w)) == INV
    gv.raycast_camera(synth.Camera(20, 12, 16.0, 16.0, 9.0, 5.0))
    depth = np.ones((12, 20), np.float32)
    assert L.tf_align_icp_pyramid_camera(gv.h, 2, c4, C.byref(w), C.byref(w)) == capi.TF_OK
    assert L.tf_align_icp_pyramid_camera(gv.h, 3, c4, C.byref(w), C.byref(w)) == INV  # 8 does not divide 12
    out = np.full((6, 10), 7.0, np.float32)
    ptrs = (C.POINTER(C.c_float) * 3)(f32p(out), f32p(out), f32p(out))
    none = (C.POINTER(C.c_float) * 3)()
    for d, n, p, lv in ((None, 1, good, ptrs), (depth, 1, None, ptrs), (depth, 1, good, None), (depth, 1, good, none),
                        (depth, 0, good, ptrs), (depth, 4, good, ptrs), (depth, 3, good, ptrs),
                        (depth, 1, capi.AlignIcpPyramid(max_depth_jump=0.0), ptrs), (depth, 1, capi.AlignIcpPyramid(max_depth_jump=np.nan), ptrs)):
        assert L.tf_align_icp_pyramid_depth(gv.h, None if d is None else f32p(d), n, None if p is None else C.byref(p), lv) == INV
    gv.sync()
    assert (out == 7.0).all()


# ---- 3. set, get, reset; off, on, off -------------------------------------------------------------------------------------
def test_a_pyramid_set_and_cleared_leaves_no_trace(gpu_required):
    depth = I.hand_depth(I.hand_pose(), PI.CAM_A)
    start = np.ascontiguousarray(II.ladder_start(0.060, 3.0), np.float32)
    pc = capi.AlignIcpParams()
    gv = _corner(PI.CAM_A)
    try:
        def run():
            res = capi.AlignResult()
            assert gv.L.tf_align_frame_icp(gv.h, f32p(depth), f32p(start), None, C.byref(pc), C.byref(res)) == capi.TF_OK
            return bytes(res), _log_raw(gv), gv.align_icp_residuals(depth, start, start, pc)

        on, back = gv.align_icp_get_pyramid()
        assert on is False and bytes(back) == bytes(capi.AlignIcpPyramid())
        off_res, off_log, off_maps = run()
        assert len(off_log) >= 4 * REC
        g = capi.AlignIcpPyramid(max_depth_jump=0.25)
        gv.align_icp_set_pyramid(g)
        on, back = gv.align_icp_get_pyramid()
        assert on is True and bytes(back) == bytes(g)
        on_res, on_log, on_maps = run()
        assert on_res != off_res and on_log != off_log  # the setting is read
        assert not on_maps["flags"][1::2].any() and (on_maps["assoc"] >= 0).sum() > 100
        gv.align_icp_set_pyramid(None)
        on, back = gv.align_icp_get_pyramid()
        assert on is False and bytes(back) == bytes(capi.AlignIcpPyramid())
        res, log, maps = run()
        assert res == off_res and log == off_log
        _same_maps(maps, off_maps)
        gv.align_icp_set_pyramid(g)
        gv.reset()  # the ICP's state is made anew: the setting is off
        assert gv.align_icp_get_pyramid()[0] is False
    finally:
        gv.close()


# ---- 4. a level of a call with the setting on is a plain call at the level camera -----------------------------------------
@pytest.mark.parametrize("stride", [2, 4, 8])
def test_a_pyramid_level_equals_a_plain_call_at_the_level_camera(ab, stride):
    a, b = ab
    k = stride.bit_length() - 1
    cam = PI.CAM_B if stride == 8 else PI.CAM_A
    a.raycast_camera(None if cam is PI.CAM_A else cam)
    depth = I.hand_depth(I.hand_pose(), cam)
    start = np.ascontiguousarray(II.ladder_start(0.040, 2.0), np.float32)
    kw = dict(min_valid=20 if stride == 8 else 100)
    pa, pb = capi.AlignIcpParams(levels=[(stride, 5)], **kw), capi.AlignIcpParams(levels=[(1, 5)], **kw)
    a.align_icp_set_pyramid(capi.AlignIcpPyramid())
    res_a = capi.AlignResult()
    assert a.L.tf_align_frame_icp(a.h, f32p(depth), f32p(start), None, C.byref(pa), C.byref(res_a)) == capi.TF_OK
    log_a = _log_raw(a)
    level = a.align_icp_pyramid_depth(depth, k)[k - 1]  # A's level image
    lc = Y.level_cam(cam, k)
    b.raycast_camera(lc)
    bufs = [HipBuffer(level.nbytes).from_host(level), HipBuffer(3 * level.nbytes), HipBuffer(3 * level.nbytes)]
    d_res = HipBuffer(C.sizeof(capi.AlignResult))
    try:
        b.raycast_device(start, NEAR, FAR, STEPS, d_normal=bufs[2].ptr, d_vertex=bufs[1].ptr)
        b.align_frame_icp_device(bufs[0].ptr, start, bufs[1].ptr, bufs[2].ptr, start, pb, d_res.ptr)
        b.sync()
        res_b, log_b = bytes(d_res.to_host()), _log_raw(b)
    finally:
        for x in bufs + [d_res]:
            x.free()
    recs = a.align_icp_log()
    print("stride %d: status %d, %d evaluations, %d of %d valid at the end" % (stride, res_a.status, res_a.evaluations,
                                                                              res_a.n_valid_last, res_a.n_sampled))
    assert res_a.status <= capi.TF_ALIGN_MAX_ITERS and res_a.evaluations >= 3
    assert res_a.n_sampled == lc.width * lc.height and res_a.n_valid_last > 0.3 * res_a.n_sampled
    assert all(r["stride"] == stride and r["n_sampled"] == lc.width * lc.height for r in recs)
    assert bytes(res_a) == res_b
    assert len(log_a) == len(log_b) == res_a.evaluations * REC and _without_stride(log_a) == _without_stride(log_b)


# ---- 5. the default schedule against the restatement ----------------------------------------------------------------------
def test_default_schedule_follows_the_restatement(ab):
    a, b = ab
    true = I.hand_pose()
    depth = I.hand_depth(true, PI.CAM_A)
    start = II.ladder_start(0.080, 5.0)
    maps = {k: _level_maps(b, PI.CAM_A, k, start) for k in (0, 1, 2)}
    pd, pc = K.params(), capi.AlignIcpParams()
    want, wlog = Y.align(depth, start, maps, start, PI.CAM_A, pd)
    a.align_icp_set_pyramid(capi.AlignIcpPyramid())
    res = a.align_frame_icp(depth, start, None, pc)
    log = a.align_icp_log()
    dt, dr = R.pose_distance(res["pose"], want["pose"])
    print("80 mm / 5 deg, pyramid {4, 2, 1}: status %d, %d evaluations, %.3g m %.3g rad from the restatement's end, %.3g m from "
          "the true pose" % (res["status"], res["evaluations"], dt, dr, R.pose_distance(res["pose"], true)[0]))
    assert res["status"] == want["status"] and res["evaluations"] == want["evaluations"] == len(log)
    assert [(r["level"], r["stride"], r["n_sampled"], r["n_valid"]) for r in log] == \
           [(r["level"], r["stride"], r["n_sampled"], r["n_valid"]) for r in wlog]
    assert [r["n_sampled"] for r in log][0] == 40 * 30 and log[-1]["n_sampled"] == 160 * 120
    assert dt <= II.ICP_TOL_T and dr <= II.ICP_TOL_R
    assert res["n_valid_first"] == wlog[0]["n_valid"] and res["n_valid_last"] == wlog[-1]["n_valid"]
    # the first evaluation is at the same f32 pose: its sums against exact sums, as tests/test_gpu_align_icp.py holds them
    rec, sm = log[0], R.sums(Y.level_rows(Y.levels(depth, 2), start, maps, start, PI.CAM_A, 4, pd), pd)
    got = np.concatenate([rec["A21"], rec["b"], [rec["sum_r2"], rec["sum_wr2"]]])
    exact = np.concatenate([sm["A21"], sm["b"], [sm["sum_r2"], sm["sum_wr2"]]])
    bound = sm["n_valid"] * 2.0 ** -52 * sm["mag"]
    assert np.all(np.abs(got - exact) <= bound)
    assert np.array_equal(log[0]["pose"].astype(np.float32), start)


# ---- 6. the residual maps -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [2, 4, 8])
def test_residual_maps_are_the_levels_spread_over_the_image(ab, stride):
    a, b = ab
    k = stride.bit_length() - 1
    cam = PI.CAM_B if stride == 8 else PI.CAM_A
    a.raycast_camera(None if cam is PI.CAM_A else cam)
    depth = I.hand_depth(I.hand_pose(), cam)
    at = II.ladder_start(0.080, 5.0)
    pose = II.ladder_start(0.040, 2.0)  # the frame elsewhere than the model camera
    V, N = _level_maps(b, cam, k, at)
    pd, pc = K.params(levels=[(stride, 1)], max_distance=0.03), capi.AlignIcpParams(levels=[(stride, 1)], max_distance=0.03)
    lc = Y.level_cam(cam, k)
    rw = K.rows(Y.levels(depth, k)[k], pose, V, N, at, lc, 1, pd)
    want = Y.spread(rw, cam, stride)
    assert (rw["flags"] == 15).sum() > 2000 // stride ** 2 and (rw["assoc"] >= 0).sum() > (rw["flags"] == 15).sum()
    assert rw["assoc"].max() < lc.width * lc.height
    a.align_icp_set_pyramid(capi.AlignIcpPyramid())
    got = a.align_icp_residuals(depth, pose, at, pc)
    _same_maps(got, want)
    off = np.ones(depth.shape, bool)
    off[::stride, ::stride] = False
    assert not got["r"][off].any() and not got["flags"][off].any() and (got["assoc"][off] == -1).all()
    _same_maps(a.align_icp_residuals(depth, pose, at, pc), want)  # twice: the level buffers are reused


# ---- 7. the gate on top ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [2, 4])
def test_the_gate_reads_the_level_image(ab, stride):
    a, b = ab
    k = stride.bit_length() - 1
    depth = I.hand_depth(I.hand_pose(), PI.CAM_A, edge_voxels=0.0)  # the unmasked corner: edges in the image
    at = II.ladder_start(0.080, 5.0)
    pose = II.ladder_start(0.040, 2.0)
    V, N = _level_maps(b, PI.CAM_A, k, at)
    pd, pc = K.params(levels=[(stride, 1)]), capi.AlignIcpParams(levels=[(stride, 1)])
    lc = Y.level_cam(PI.CAM_A, k)
    rw = G.rows(Y.levels(depth, k)[k], pose, V, N, at, lc, 1, pd, G.gate())
    for fl, least in ((15, 5), (31, 5), (63, 4000 // stride ** 2)):
        assert (rw["flags"] == fl).sum() > least, fl
    a.align_icp_set_pyramid(capi.AlignIcpPyramid())
    a.align_icp_set_gate(capi.AlignIcpGate())
    _same_maps(a.align_icp_residuals(depth, pose, at, pc), Y.spread(rw, PI.CAM_A, stride))


# ---- 8. the device tracker ------------------------------------------------------------------------------------------------
def test_the_device_tracker_reads_the_pyramid(ab):
    gv, _ = ab
    depth = I.hand_depth(I.hand_pose(), PI.CAM_A)
    start = np.ascontiguousarray(II.ladder_start(*II.TRACK_START), np.float32)
    icp, sdf = capi.AlignIcpParams(), capi.AlignParams(**I.SCENE_PARAMS)
    plain = capi.TrackResult()
    assert gv.L.tf_track_frame(gv.h, f32p(depth), f32p(start), C.byref(icp), C.byref(sdf), C.byref(plain)) == capi.TF_OK
    gv.align_icp_set_pyramid(capi.AlignIcpPyramid())
    host = capi.TrackResult()
    assert gv.L.tf_track_frame(gv.h, f32p(depth), f32p(start), C.byref(icp), C.byref(sdf), C.byref(host)) == capi.TF_OK
    host_log = _log_raw(gv)
    first = capi.AlignIter.from_buffer_copy(host_log[:REC])
    assert host.stage >= 1 and (first.stride, first.n_sampled) == (4, 40 * 30)  # the setting was read
    assert bytes(host.icp) != bytes(plain.icp)
    cell = capi.DevicePose()
    cell.pose[:] = [float(x) for x in start.reshape(12)]
    cell.valid = 1
    d_depth, d_start = HipBuffer(depth.nbytes).from_host(depth), HipBuffer(64).from_host(np.frombuffer(bytes(cell), np.uint8))
    d_out, d_pose = HipBuffer(256), HipBuffer(64)
    try:
        gv.track_frame_device(d_depth.ptr, d_start.ptr, icp, sdf, None, d_out.ptr, d_pose.ptr)
        gv.sync()
        assert bytes(d_out.to_host(TRK)) == bytes(host)
        assert _log_raw(gv) == host_log
        # a cell that holds no pose: nothing runs -- no records, the result says so, the output cell is the start's floats
        cell.valid = 0
        d_start.from_host(np.frombuffer(bytes(cell), np.uint8))
        d_out.from_host(np.full(256, 7, np.uint8))
        gv.track_frame_device(d_depth.ptr, d_start.ptr, icp, sdf, None, d_out.ptr, d_pose.ptr)
        gv.sync()
        out = capi.TrackResult.from_buffer_copy(bytes(d_out.to_host(TRK)))
        back = capi.DevicePose.from_buffer_copy(bytes(d_pose.to_host(64)))
        assert (out.icp.status, out.sdf.status, out.stage, out.icp.evaluations) == (-1, -1, 0, 0)
        assert list(out.pose) == list(cell.pose) and back.valid == 0 and list(back.pose) == list(cell.pose)
        assert _log_raw(gv) == b""
        assert (d_out.to_host()[TRK:] == 7).all()
    finally:
        for x in (d_depth, d_start, d_out, d_pose):
            x.free()
    print("track, pyramid: ICP %d evaluations, stage %d; without: %d evaluations" % (host.icp.evaluations, host.stage,
                                                                                    plain.icp.evaluations))
