"""The colour ICP on the MI355X (tf_align_icp_color.hip): the model maps and the maps of one evaluation against the
restatement bit for bit -- on the hand-built cases of tests/align_icp_color_inputs.py, at strides 1, 2 and 4, at 160 x 120
and at 152 x 116 whose last tiles are partial -- the whole alignment on the textured plane where the plain call is singular,
the tie to the plain and to the gated call, the tracker, the other aligners' logs, the volume, invalid arguments."""
import ctypes as C

import numpy as np
import pytest

from tests import align_color_inputs as CI
from tests import align_icp_color_inputs as XI
from tests import align_icp_color_ref as X
from tests import align_icp_gate_ref as G
from tests import align_icp_inputs as II
from tests import align_inputs as I
from tests import align_ref as R
from tests.util import HipBuffer
from texturefusion_amd import capi

pytestmark = pytest.mark.gpu
INV = capi.TF_ERR_INVALID
f32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
PHOTO = ("photo_weight", "max_photo_residual", "huber_photo", "max_depth_jump")


def _params(**kw):
    """(the restatement's dict, the library's struct) of the same parameters"""
    pd = X.params(**kw)
    pc = capi.AlignIcpColorParams(**kw)
    return pd, pc


def _volume(vol):
    gv = capi.Volume(I.HAND_RES, I.CAM, max_chunks=1 << 10, max_keyframes=8)
    XI.upload(gv, vol)
    return gv


@pytest.fixture(scope="module")
def edge(gpu_required):
    """the textured plane with one voxel without a colour count, and the restatement's volume of it"""
    vol = XI.edge_volume()
    gv = _volume(vol)
    yield gv, XI.ref_of(vol)
    gv.close()


@pytest.fixture(scope="module")
def plane(gpu_required):
    vol = CI.hand_plane_textured()
    gv = _volume(vol)
    yield gv, XI.ref_of(vol)
    gv.close()


@pytest.fixture(scope="module")
def corner(gpu_required):
    """the textured corner, the same corner without colour, the restatement's volume of the first"""
    vol = XI.corner_textured()
    gc, gp = _volume(vol), _volume(I.hand_corner())
    yield gc, gp, XI.ref_of(vol)
    gc.close()
    gp.close()


def _same_maps(got, want):
    assert np.array_equal(got["flags"], want["flags"])
    assert np.array_equal(got["assoc"], want["assoc"])
    for k in ("r", "rc", "gradc"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k


def _same_model_maps(got, want):
    for k in ("L", "Gu", "Gv"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k


def _log_raw(gv, name, rec):
    n = C.c_int64(0)
    buf = (rec * capi.TF_ALIGN_MAX_EVALUATIONS)()
    args = (gv.h, 0, buf) if name == "tf_align_group_log" else (gv.h, buf)
    assert getattr(gv.L, name)(*args, capi.TF_ALIGN_MAX_EVALUATIONS, C.byref(n)) == capi.TF_OK
    return bytes(buf)[:n.value * C.sizeof(rec)]


# ---- 1. the model maps and the maps of one evaluation ---------------------------------------------------------------------
@pytest.mark.parametrize("cam", [XI.CAM, XI.CAM_ODD], ids=["160x120", "152x116"])
def test_model_maps_equal_the_restatement_at_every_edge(edge, cam):
    gv, ref = edge
    gv.raycast_camera(cam)
    try:
        depth, rgba, V, N, pose = XI.edge_cases(cam)
        pd, pc = _params()
        want = X.model_maps(ref, V, N, pose, cam, pd)
        got = gv.align_icp_color_model_maps(V, N, pose, pc)
        _same_model_maps(got, want)
        L, Gu, Gv = got["L"], got["Gu"], got["Gv"]
        hit = np.square(N).sum(0) > 0.5
        # no gradient in the first and last column and row
        assert np.isnan(Gu[:, 0]).all() and np.isnan(Gu[:, -1]).all() and np.isnan(Gv[0]).all() and np.isnan(Gv[-1]).all()
        assert (~np.isnan(Gu[:, 1:-1])).sum() > 0.9 * Gu[:, 1:-1].size
        # a neighbour that is a miss
        x, y = XI.MISS
        assert L[y, x] == -1 and L[y, x - 1] >= 0 and np.isnan(Gu[y, x - 1]) and np.isnan(Gu[y, x + 1]) and np.isnan(Gv[y - 1, x])
        assert not np.isnan(Gv[y, x - 1])
        # a voxel without a colour count: hits without intensity, and their neighbours without a gradient
        dark = hit & (L < 0)
        dark[y, x] = False
        ys, xs = np.nonzero(dark)
        assert 20 < len(ys) < 400 and ys.min() > 2 and xs.min() > 2
        assert np.isnan(Gu[ys, xs + 1]).all() and np.isnan(Gv[ys + 1, xs]).all()
        # a neighbour at exactly max_depth_jump, at the next float below it, and no limit at all
        x, y = XI.JUMP
        jump = np.abs(want["Z"][y, x] - want["Z"][y, x - 1])
        assert 0.9 * XI.JUMP_DX < jump < 1.1 * XI.JUMP_DX and jump == np.abs(want["Z"][y, x] - want["Z"][y - 1, x])
        for mj, there in ((jump, True), (np.nextafter(jump, np.float32(0)), False), (np.inf, True)):
            pd, pc = _params(max_depth_jump=mj)
            got = gv.align_icp_color_model_maps(V, N, pose, pc)
            _same_model_maps(got, X.model_maps(ref, V, N, pose, cam, pd))
            for g in (got["Gu"][y, x - 1], got["Gu"][y, x + 1], got["Gv"][y - 1, x], got["Gv"][y + 1, x]):
                assert np.isnan(g) != there, (mj, g)
            assert np.isnan(got["Gu"][y, x]) != there  # its own neighbours lie the same jump away from it
        # the device form, one output at a time
        bufs = [HipBuffer(a.nbytes).from_host(a) for a in (V, N)]
        outs = [HipBuffer(4 * cam.width * cam.height) for _ in range(3)]
        try:
            pd, pc = _params()
            gv.align_icp_color_model_maps_device(bufs[0].ptr, bufs[1].ptr, pose, pc, outs[0].ptr, outs[1].ptr, outs[2].ptr)
            gv.sync()
            for o, k in zip(outs, ("L", "Gu", "Gv")):
                assert np.array_equal(o.to_host().view(np.uint32), bits(want[k]).reshape(-1)), k
        finally:
            for b in bufs + outs:
                b.free()
    finally:
        gv.raycast_camera(None)


@pytest.mark.parametrize("cam", [XI.CAM, XI.CAM_ODD], ids=["160x120", "152x116"])
@pytest.mark.parametrize("stride", [1, 2, 4])
def test_evaluation_maps_equal_the_restatement(edge, cam, stride):
    gv, ref = edge
    gv.raycast_camera(cam)
    try:
        depth, rgba, V, N, pose = XI.edge_cases(cam)
        pd, pc = _params(levels=[(stride, 1)])
        maps = X.model_maps(ref, V, N, pose, cam, pd)
        at = XI.shifted(pose, 0.0021, -0.0013)  # the frame about a pixel off the model camera
        want = X.rows(maps, depth, rgba, at, V, N, pose, cam, stride, pd)
        got = gv.align_icp_color_residuals(depth, rgba, at, pose, pc, vertex=V, normal=N)
        _same_maps(got, want)
        fl = got["flags"]
        n = (cam.width // stride) * (cam.height // stride)
        assert (fl == 783).sum() > 0.8 * n and (fl == 15).sum() > 32 // stride ** 2  # both kinds of pixel are there
        assert not (fl[(fl & 15) != 15] & 768).any() and not (fl[(fl & 256) == 0] & 512).any()
        assert not got["rc"][(fl & 256) == 0].any() and not got["gradc"][:, (fl & 256) == 0].any()
        plain = gv.align_icp_residuals(depth, at, pose, pc.icp, vertex=V, normal=N)
        assert np.array_equal(fl & 255, plain["flags"]) and np.array_equal(got["assoc"], plain["assoc"])
        assert np.array_equal(bits(got["r"]), bits(plain["r"]))
        if stride > 1:  # pixels that are not sampled
            un = np.ones(fl.shape, bool)
            un[::stride, ::stride] = False
            assert not fl[un].any() and (got["assoc"][un] == -1).all() and not got["rc"][un].any() and not got["gradc"][:, un].any()
    finally:
        gv.raycast_camera(None)


def test_hand_built_pixels_of_the_row(edge):
    gv, ref = edge
    cam = XI.CAM
    depth, rgba, V, N, pose = XI.edge_cases(cam)
    pd, pc = _params(levels=[(1, 1)])
    maps = X.model_maps(ref, V, N, pose, cam, pd)

    def both(at, pd, pc, depth=depth):
        want = X.rows(maps, depth, rgba, at, V, N, pose, cam, 1, pd)
        got = gv.align_icp_color_residuals(depth, rgba, at, pose, pc, vertex=V, normal=N)
        _same_maps(got, want)
        return got

    # the frame at the model's own pose: every pixel is associated with itself
    got = both(pose, pd, pc)
    fl, H, W = got["flags"], cam.height, cam.width
    assert np.array_equal(got["assoc"][fl != 0], np.arange(H * W).reshape(H, W)[fl != 0])
    # the associated pixel in the first and last column and row: valid geometrically, no gradient
    border = np.ones((H, W), bool)
    border[1:-1, 1:-1] = False
    assert (fl[border] == 15).sum() > 400 and not (fl[border] & 256).any()
    x, y = XI.ALPHA0
    assert fl[y, x] == 15 and fl[y, x + 1] == 783  # frame alpha 0
    x, y = XI.MISS
    assert fl[y, x] == 3 and fl[y, x - 1] == 15 and fl[y - 1, x] == 15  # a miss, and its neighbours without a gradient
    dark = (np.square(N).sum(0) > 0.5) & (maps["L"] < 0)
    assert (fl[dark] == 15).all() and dark.sum() > 20  # valid geometrically, no intensity
    # |rc| exactly max_photo_residual, and the next float below it
    x, y = XI.RC_PIX
    rc = np.abs(got["rc"][y, x])
    assert fl[y, x] == 783 and 0.1 < rc < 0.25
    for lim, want_fl in ((rc, 783), (np.nextafter(rc, np.float32(0)), 271)):
        pd2, pc2 = _params(levels=[(1, 1)], max_photo_residual=lim)
        assert both(pose, pd2, pc2)["flags"][y, x] == want_fl
    # uc exactly on x.5: the tie goes up
    x, y = XI.HALF
    at = XI.shifted(pose, 0.5 * XI.EDGE_DIST / int(cam.fx))
    z = XI.half_pixel_depth(at, pose, cam, x, y, depth[y, x])
    assert z is not None
    d2 = depth.copy()
    d2[y, x] = z
    got = both(at, pd, pc, d2)
    assert got["flags"][y, x] == 783 and got["assoc"][y, x] == y * W + x + 1


# ---- 2. the whole alignment ---------------------------------------------------------------------------------------------
def _align_device(gv, depth, rgba, start, V, N, pc, plain=False):
    bufs = [HipBuffer(a.nbytes).from_host(np.ascontiguousarray(a)) for a in (depth, rgba, V, N)]
    d_res = HipBuffer(C.sizeof(capi.AlignColorResult))
    try:
        if plain:
            gv.align_frame_icp_device(bufs[0].ptr, start, bufs[2].ptr, bufs[3].ptr, start, pc, d_res.ptr)
            gv.sync()
            return gv.align_result(d_res.to_host(C.sizeof(capi.AlignResult)))
        gv.align_frame_icp_color_device(bufs[0].ptr, bufs[1].ptr, start, bufs[2].ptr, bufs[3].ptr, start, pc, d_res.ptr)
        gv.sync()
        return gv.align_color_result(d_res.to_host())
    finally:
        for b in bufs + [d_res]:
            b.free()


@pytest.mark.parametrize("huber_photo", [0.05, 0.0])
def test_alignment_on_the_textured_plane_follows_the_restatement(plane, huber_photo):
    """from the largest rung the restatement holds (tests/test_align_icp_color_cpu.py): pose and log bit for bit"""
    gv, ref = plane
    metres, degrees = max(XI.PLANE_RUNGS[:XI.PLANE_HELD])
    depth, rgba = XI.plane_frame()
    start = XI.plane_start(metres, degrees)
    V, N = XI.plane_maps(start)
    pd, pc = _params(huber_photo=huber_photo)
    want, wlog = X.align(ref, depth, rgba, start, V, N, start, I.CAM, pd)
    plain = _align_device(gv, depth, rgba, start, V, N, pc.icp, plain=True)
    assert plain["status"] == capi.TF_ALIGN_SINGULAR  # the plain call on the same input
    res = _align_device(gv, depth, rgba, start, V, N, pc)
    log = gv.align_icp_color_log()
    dt, dr = R.pose_distance(res["pose"], I.hand_pose())
    d = np.asarray(res["pose"], np.float64)[:, 3] - np.asarray(I.hand_pose(), np.float64)[:, 3]
    print("plane from %.0f mm, huber_photo %g: status %d, %d evaluations, %.4g m %.3g rad from the true pose, in-plane %.4g m; "
          "restatement status %d, %d evaluations" % (1e3 * metres, huber_photo, res["status"], res["evaluations"], dt, dr,
                                                     np.linalg.norm(d[1:]), want["status"], want["evaluations"]))
    assert res["status"] == want["status"] <= capi.TF_ALIGN_MAX_ITERS and res["evaluations"] == want["evaluations"] == len(log)
    for k, (a, b) in enumerate(zip(log, wlog)):
        for key in ("level", "stride", "n_sampled", "n_valid", "n_photo"):
            assert a[key] == b[key], (k, key)
        for key in ("A21", "b", "Ac21", "bc", "xi", "pose"):
            assert np.array_equal(np.asarray(a[key], np.float64).view(np.uint64), np.asarray(b[key], np.float64).view(np.uint64)), (k, key)
        for key in ("sum_r2", "sum_wr2", "sum_rc2", "sum_wrc2"):
            assert a[key] == b[key], (k, key)
    assert np.array_equal(bits(res["pose"]), bits(want["pose"]))
    for key in ("n_sampled", "n_valid_first", "n_valid_last", "n_photo_first", "n_photo_last", "rms_first", "rms_last",
                "rms_photo_first", "rms_photo_last"):
        assert res[key] == want[key], key
    assert np.linalg.norm(d[1:]) <= 0.1 * metres and dt <= 2 * XI.PLANE_TRUTH_T and dr <= 2 * XI.PLANE_TRUTH_R


@pytest.mark.parametrize("gated", [False, True], ids=["gate off", "gate on"])
def test_no_weight_and_no_colour_equal_the_plain_call_bit_for_bit(corner, gated):
    gc, gp, _ = corner
    depth, rgba = XI.corner_frame()
    start = II.ladder_start(*II.LADDER[0])
    V, N = II.hand_model_maps(start)
    _, pc = _params()
    _, p0 = _params(photo_weight=0.0)
    try:
        for gv in (gc, gp):
            gv.align_icp_set_gate(capi.AlignIcpGate() if gated else None)
        geo = _align_device(gp, depth, rgba, start, V, N, pc.icp, plain=True)
        glog = _log_raw(gp, "tf_align_icp_log", capi.AlignIter)
        assert geo["status"] <= capi.TF_ALIGN_MAX_ITERS and geo["evaluations"] >= 4

        def same(gv, res):
            assert bytes(res["pose"]) == bytes(geo["pose"])
            assert {k: res[k] for k in geo if k != "pose"} == {k: v for k, v in geo.items() if k != "pose"}
            raw = _log_raw(gv, "tf_align_icp_color_log", capi.AlignColorIter)
            n, a, b = geo["evaluations"], C.sizeof(capi.AlignColorIter), C.sizeof(capi.AlignIter)
            assert len(raw) == n * a and b"".join(raw[k * a:k * a + b] for k in range(n)) == glog

        res = _align_device(gp, depth, rgba, start, V, N, pc)  # every colour count 0, default weight
        same(gp, res)
        assert res["n_photo_first"] == 0 == res["n_photo_last"]
        res = _align_device(gc, depth, rgba, start, V, N, p0)  # a coloured volume, weight 0
        same(gc, res)
        assert res["n_photo_first"] > 300 and res["n_photo_last"] > 5000 and gc.align_icp_color_log()[0]["Ac21"].any()
        res = _align_device(gc, depth, rgba, start, V, N, pc)  # ... and with the default weight the step differs
        assert not np.array_equal(gc.align_icp_color_log()[0]["xi"], gp.align_icp_log()[0]["xi"])
        if gated:  # bits 4 and 5 are tf_align_icp_residuals', the photometric bits lie above pixels with 63
            _, p1 = _params(levels=[(1, 1)])
            got = gc.align_icp_color_residuals(depth, rgba, start, start, p1, vertex=V, normal=N)
            ref = gc.align_icp_residuals(depth, start, start, p1.icp, vertex=V, normal=N)
            assert np.array_equal(got["flags"] & 255, ref["flags"]) and (ref["flags"] == 31).sum() + (ref["flags"] == 15).sum() > 0
            assert (got["flags"] == 63 + 768).sum() > 1000 and not (got["flags"][(got["flags"] & 63) != 63] & 768).any()
    finally:
        for gv in (gc, gp):
            gv.align_icp_set_gate(None)


def test_gated_maps_equal_the_restatement(corner):
    gc, _, ref = corner
    depth, rgba = XI.corner_frame()
    start = II.ladder_start(*II.LADDER[0])
    at = II.ladder_start(0.02, 1.0)
    V, N = II.hand_model_maps(start)
    try:
        gc.align_icp_set_gate(capi.AlignIcpGate())
        for stride in (1, 2):
            pd, pc = _params(levels=[(stride, 1)])
            maps = X.model_maps(ref, V, N, start, I.CAM, pd)
            want = X.rows(maps, depth, rgba, at, V, N, start, I.CAM, stride, pd, G.gate())
            _same_maps(gc.align_icp_color_residuals(depth, rgba, at, start, pc, vertex=V, normal=N), want)
            assert (want["flags"] == 63 + 768).sum() > 1000 // stride ** 2
    finally:
        gc.align_icp_set_gate(None)


# ---- 3. the tracker, the other logs, the volume -------------------------------------------------------------------------
def test_the_colour_tracker_holds_the_plane_where_the_plain_one_does_not(plane):
    gv, _ = plane
    depth, rgba = XI.plane_frame()
    start = XI.plane_start(*XI.PLANE_RUNGS[0])
    sdf = dict(CI.PARAMS)
    plain = gv.track_frame(depth, start, capi.AlignIcpParams(), capi.AlignParams(**sdf))
    assert plain["stage"] == 0 and plain["icp"]["status"] == capi.TF_ALIGN_SINGULAR and plain["sdf"]["status"] == -1
    res = gv.track_frame_color(depth, rgba, start, capi.AlignIcpColorParams(), capi.AlignColorParams(**sdf))
    d = np.asarray(res["pose"], np.float64)[:, 3] - np.asarray(I.hand_pose(), np.float64)[:, 3]
    print("track, colour: stage %d, icp status %d (%d evaluations, %d photometric), sdf status %d, in-plane error %.4g m" % (
        res["stage"], res["icp"]["status"], res["icp"]["evaluations"], res["icp"]["n_photo_last"], res["sdf"]["status"],
        np.linalg.norm(d[1:])))
    assert res["stage"] == 2 and res["icp"]["status"] <= capi.TF_ALIGN_MAX_ITERS and res["sdf"]["status"] <= capi.TF_ALIGN_MAX_ITERS
    assert np.array_equal(res["pose"], res["sdf"]["pose"]) and np.linalg.norm(d[1:]) <= 0.1 * XI.PLANE_RUNGS[0][0]
    alone = gv.align_frame_icp_color(depth, rgba, start)  # the first stage is the call on its own
    assert bytes(alone["pose"]) == bytes(res["icp"]["pose"]) and alone["evaluations"] == res["icp"]["evaluations"]


def _digest(gv):
    ids = gv.list_chunks()
    ids = ids[np.lexsort((ids[:, 2], ids[:, 1], ids[:, 0]))]
    s, w, c = gv.get_chunks(ids)
    return bytes(gv.stats()), ids.tobytes(), s.tobytes(), w.tobytes(), c.tobytes(), np.asarray(gv.dirty()).tobytes()


def test_the_calls_are_readers_and_leave_the_other_logs_alone(corner):
    gc, _, _ = corner
    depth, rgba = XI.corner_frame()
    pose = I.hand_pose()
    start = II.ladder_start(*II.LADDER[0])
    V, N = II.hand_model_maps(start)
    near = I.perturb(pose, I.HAND_DELTA, np.zeros(3))
    gc.align_frame(depth, near)
    gc.align_frame_color(depth, rgba, near)
    gc.align_frame_icp(depth, start)
    gc.align_group([depth], [near])
    logs = [("tf_align_log", capi.AlignIter), ("tf_align_color_log", capi.AlignColorIter), ("tf_align_icp_log", capi.AlignIter),
            ("tf_align_group_log", capi.AlignIter)]
    before = [_log_raw(gc, *l) for l in logs]
    assert all(len(b) > 0 for b in before)
    digest = _digest(gc)
    gc.render_model(pose, 0.1, 3.0, 4)  # the model stream is packed and current
    stats = gc.model_stream_stats()
    res = gc.align_frame_icp_color(depth, rgba, start)
    assert res["status"] <= capi.TF_ALIGN_MAX_ITERS and res["n_photo_first"] > 300 and res["n_photo_last"] > 5000
    gc.align_icp_color_residuals(depth, rgba, start)
    gc.align_icp_color_model_maps(V, N, start)
    _align_device(gc, depth, rgba, start, V, N, capi.AlignIcpColorParams())
    gc.track_frame_color(depth, rgba, start)
    icp_after = _log_raw(gc, "tf_align_icp_log", capi.AlignIter)
    assert icp_after == before[2] and _log_raw(gc, "tf_align_group_log", capi.AlignIter) == before[3]
    assert _log_raw(gc, "tf_align_log", capi.AlignIter) == before[0]
    # (tf_track_frame_color's second stage is tf_align_frame_color: that log is its own stage's now, and only then)
    gc.render_model(pose, 0.1, 3.0, 4)
    after = gc.model_stream_stats()
    assert (after["packs"], after["hits"]) == (stats["packs"], stats["hits"] + 1)  # a hit: nothing was repacked
    assert _digest(gc) == digest  # (the downloads are no readers: taken after the stream's check)
    gc.align_frame_color(depth, rgba, near)
    assert _log_raw(gc, "tf_align_color_log", capi.AlignColorIter) == before[1]  # and a colour ICP leaves it as it finds it
    gc.align_frame_icp_color(depth, rgba, start)
    assert _log_raw(gc, "tf_align_color_log", capi.AlignColorIter) == before[1]


# ---- 4. invalid arguments -----------------------------------------------------------------------------------------------
def test_invalid_arguments_change_nothing(corner):
    gc, _, _ = corner
    L = gc.L
    depth, rgba = XI.corner_frame()
    start = np.ascontiguousarray(II.ladder_start(*II.LADDER[0]), np.float32)
    V, N = II.hand_model_maps(start)
    d, c = np.ascontiguousarray(depth, np.float32), np.ascontiguousarray(rgba)
    good = gc.align_frame_icp_color(depth, rgba, start)
    log = _log_raw(gc, "tf_align_icp_color_log", capi.AlignColorIter)
    bad = [dict(n_levels=0), dict(stride=[0, 1, 1, 1]), dict(iters=[30, 30, 5, 0]), dict(min_depth=np.nan), dict(huber=-0.1),
           dict(max_distance=-1.0), dict(max_distance=np.inf), dict(ray_near=-1.0), dict(ray_max_steps=0),
           dict(photo_weight=-0.1), dict(photo_weight=np.nan), dict(photo_weight=np.inf), dict(max_photo_residual=-1.0),
           dict(max_photo_residual=np.nan), dict(huber_photo=-0.01), dict(huber_photo=np.inf), dict(max_depth_jump=0.0),
           dict(max_depth_jump=-1.0), dict(max_depth_jump=np.nan), dict(max_depth_jump=-np.inf)]
    res = capi.AlignColorResult()
    res.geo.status = 77
    trk = capi.TrackColorResult()
    trk.stage = 77
    outs = {k: np.full(depth.shape, 7, t) for k, t in (("r", np.float32), ("rc", np.float32), ("flags", np.uint32), ("assoc", np.int32))}
    gcm = np.full((3,) + depth.shape, 7, np.float32)
    sdf = capi.AlignColorParams()
    i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    u32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))

    def calls(dp, cp, pp, mp, par, own=True):
        """every host entry point with these arguments -> their return codes"""
        rcs = [L.tf_align_frame_icp_color(gc.h, dp, cp, pp, mp, par, C.byref(res)),
               L.tf_track_frame_color(gc.h, dp, cp, pp, par, C.byref(sdf), C.byref(trk))]
        if own:
            rcs.append(L.tf_align_icp_color_residuals(gc.h, dp, cp, pp, f32p(V), f32p(N), mp, par, f32p(outs["r"]), f32p(outs["rc"]),
                                                      u32p(outs["flags"]), i32p(outs["assoc"]), f32p(gcm)))
        return rcs

    for kw in bad:
        pc = capi.AlignIcpColorParams(**kw)
        with_res = "iters" not in kw and "ray_near" not in kw and "ray_max_steps" not in kw
        assert set(calls(f32p(d), u8p(c), f32p(start), None, C.byref(pc), with_res)) == {INV}, kw
        if any(k in kw for k in PHOTO):
            assert L.tf_align_icp_color_model_maps(gc.h, f32p(V), f32p(N), f32p(start), C.byref(pc), f32p(outs["r"]), None, None) == INV, kw
    pc = capi.AlignIcpColorParams()
    q = start.copy()
    q.reshape(-1)[7] = np.nan
    assert set(calls(f32p(d), u8p(c), f32p(q), None, C.byref(pc))) == {INV}
    assert set(calls(f32p(d), None, f32p(start), None, C.byref(pc))) == {INV}  # a null rgba
    assert set(calls(None, u8p(c), f32p(start), None, C.byref(pc))) == {INV}
    assert set(calls(f32p(d), u8p(c), f32p(start), None, None)) == {INV}
    assert L.tf_align_frame_icp_color(gc.h, f32p(d), u8p(c), f32p(start), f32p(q), C.byref(pc), C.byref(res)) == INV  # model pose
    assert L.tf_align_frame_icp_color(gc.h, f32p(d), u8p(c), f32p(start), None, C.byref(pc), None) == INV
    assert L.tf_track_frame_color(gc.h, f32p(d), u8p(c), f32p(start), C.byref(pc), None, C.byref(trk)) == INV
    assert L.tf_track_frame_color(gc.h, f32p(d), u8p(c), f32p(start), C.byref(pc), C.byref(capi.AlignColorParams(photo_weight=-1.0)),
                                  C.byref(trk)) == INV
    assert L.tf_align_icp_color_residuals(gc.h, f32p(d), u8p(c), f32p(start), f32p(V), None, None, C.byref(pc), f32p(outs["r"]),
                                          None, None, None, None) == INV  # one map without the other
    assert L.tf_align_icp_color_model_maps(gc.h, None, f32p(N), f32p(start), C.byref(pc), f32p(outs["r"]), None, None) == INV
    assert L.tf_align_icp_color_model_maps(gc.h, f32p(V), f32p(N), None, C.byref(pc), f32p(outs["r"]), None, None) == INV
    # the device forms: a null pointer of each kind, an rgba image off a word boundary
    bufs = [HipBuffer(a.nbytes).from_host(a) for a in (d, c, V, N)]
    d_res = HipBuffer(C.sizeof(capi.AlignColorResult)).from_host(np.full(C.sizeof(capi.AlignColorResult), 7, np.uint8))
    try:
        ptrs = [bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, d_res.ptr]
        for k in range(5):
            a = list(ptrs)
            a[k] = None
            assert L.tf_align_frame_icp_color_device(gc.h, a[0], a[1], f32p(start), a[2], a[3], f32p(start), C.byref(pc), a[4]) == INV, k
        assert L.tf_align_frame_icp_color_device(gc.h, ptrs[0], ptrs[1], f32p(start), ptrs[2], ptrs[3], None, C.byref(pc), ptrs[4]) == INV
        assert L.tf_align_frame_icp_color_device(gc.h, ptrs[0], ptrs[1] + 1, f32p(start), ptrs[2], ptrs[3], f32p(start), C.byref(pc),
                                                 ptrs[4]) == INV
        assert L.tf_align_icp_color_residuals_device(gc.h, ptrs[0], None, f32p(start), ptrs[2], ptrs[3], f32p(start), C.byref(pc),
                                                     ptrs[4], None, None, None, None) == INV
        assert L.tf_align_icp_color_model_maps_device(gc.h, ptrs[2], None, f32p(start), C.byref(pc), ptrs[4], None, None) == INV
        gc.sync()
        assert (d_res.to_host() == 7).all()
    finally:
        for b in bufs + [d_res]:
            b.free()
    assert res.geo.status == 77 and trk.stage == 77  # nothing was written
    assert all((o == 7).all() for o in outs.values()) and (gcm == 7).all()
    assert _log_raw(gc, "tf_align_icp_color_log", capi.AlignColorIter) == log and len(log) == good["evaluations"] * C.sizeof(capi.AlignColorIter)
