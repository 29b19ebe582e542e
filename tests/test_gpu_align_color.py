"""Alignment by colour as well as depth on the MI355X (tf_align_color.hip): the five maps against the numpy restatement bit
for bit, both sets of sums against exact sums, every logged step against the logged joined system, the known answer on
the textured hand-built plane, the textured wall's fixed point, the degenerate cases against tf_align_frame, levels and
stops, invalid parameters, the read-only guarantee, the device forms and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import align_color_inputs as CI
from tests import align_color_ref as CR
from tests import align_inputs as I
from tests import align_ref as R
from tests.raycast_ref import RefVolume
from tests.util import HipBuffer, assert_chunks_equal, make_pair, sorted_ids
from texturefusion_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = ("r", "grad", "rc", "gradc")
GEO_KEYS = ("level", "stride", "n_sampled", "n_valid", "sum_r2", "sum_wr2", "A21", "b", "xi", "pose")


def _params(**kw):
    """the same parameters for the restatement (dict) and the library (tf_align_color_params)"""
    return CR.params(**kw), capi.AlignColorParams(**kw)


def _hand_volume(chunks):
    gv = capi.Volume(I.HAND_RES, I.CAM, max_chunks=1 << 10)
    ids, s, w, c = chunks
    for k in range(len(ids)):
        gv.set_chunk(ids[k], s[k], w[k], c[k])
    gv.sync()
    return gv, RefVolume(ids, s, w, c, I.HAND_RES)


@pytest.fixture(scope="module")
def plane(gpu_required):
    gv, ref = _hand_volume(CI.hand_plane_textured())
    pose = I.hand_pose()
    depth, rgba = CI.hand_frame(pose)
    yield gv, ref, pose, depth, rgba
    gv.close()


@pytest.fixture(scope="module")
def corner(gpu_required):
    """the hand-built corner twice: with the texture in its voxels, and with every colour count 0"""
    gc, rc = _hand_volume(CI.textured(I.hand_corner()))
    gp, rp = _hand_volume(I.hand_corner())
    pose = I.hand_pose()
    depth = I.hand_depth(pose)
    yield gc, gp, pose, depth, CI.texture_rgba(depth, pose)
    gc.close()
    gp.close()


@pytest.fixture(scope="module")
def wall(gpu_required):
    """the textured wall integrated on the device; the restatement reads the device's own chunks"""
    frames = CI.wall_frames()
    gv = capi.Volume(CI.WALL_RES, I.CAM, max_chunks=1 << 14)
    for k, (depth, rgba, pose) in enumerate(frames):
        gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, k)
    gv.update_meshes()  # the neighbour table filled in: the sampler reads it
    gv.sync()
    ref = RefVolume.from_volume(gv, gv.list_chunks(), gv.res)
    depth, rgba, pose = frames[CI.WALL_HELD]
    yield gv, ref, pose, depth, rgba
    gv.close()


@pytest.fixture(scope="module")
def wall_fixed_point(wall):
    """the restatement's fixed point from the integration pose: computed once, shared"""
    _, ref, pose, depth, rgba = wall
    return CR.align(ref, depth, rgba, pose, I.CAM, CR.params(**CI.PARAMS))


def _assert_maps_equal(got, exp, what):
    assert np.array_equal(got["flags"], exp["flags"]), "%s: flags differ at %d pixels" % (what, (got["flags"] != exp["flags"]).sum())
    for k in MAPS:
        assert np.array_equal(got[k].view(np.uint32), exp[k].view(np.uint32)), "%s: %s differs at %d" % (
            what, k, (got[k].view(np.uint32) != exp[k].view(np.uint32)).sum())


@pytest.mark.parametrize("stride", [1, 3])
def test_maps_bit_exact_on_the_textured_wall(wall, stride):
    gv, ref, pose, depth, rgba = wall
    pd, pc = _params(levels=[(stride, 1)])
    for k, start in enumerate([pose, I.perturb(pose, *CI.wall_starts()[3])]):
        got = gv.align_color_residuals(depth, rgba, start, pc)
        exp = CR.rows(ref, depth, rgba, start, I.CAM, stride, pd)
        _assert_maps_equal(got, exp, "pose %d stride %d" % (k, stride))
        n = len(exp["fl"])
        print("pose %d stride %d: %d of %d photometrically valid, %d geometrically" % (
            k, stride, (exp["fl"] == 127).sum(), n, ((exp["fl"] & 15) == 15).sum()))
        assert (exp["fl"] == 127).sum() > 0.75 * n and exp["gradc"].any() and exp["rc"].any()
        assert (exp["fl"] == 0).sum() > 0  # the holes
    # the perturbed pose leaves the coloured band at the image's border: geometrically valid pixels without a colour term
    assert np.isin(exp["fl"], (15, 31)).sum() > 0


def test_maps_with_tiles_over_both_borders_and_hand_made_pixels(plane):
    """a 13 x 9 camera: one full tile column and a partial one, one full tile row and a partial one; and on the full
    camera hand-made pixels: alpha 0, |rc| above the bound, bad depths (a tap with a colourless corner, flags 31, comes by
    itself on the integrated wall)"""
    gv, ref, pose, depth, rgba = plane
    small = synth.Camera(13, 9, 11.0, 11.0, 6.5, 4.5)
    gv.raycast_camera(small)
    try:
        d, c = CI.hand_frame(pose, small, edge_voxels=0.0)
        for stride in (1, 2):
            pd, pc = _params(levels=[(stride, 1)], min_valid=1)
            exp = CR.rows(ref, d, c, pose, small, stride, pd)
            _assert_maps_equal(gv.align_color_residuals(d, c, pose, pc), exp, "13 x 9 stride %d" % stride)
            assert (exp["flags"] == 127).sum() > 10
            gv.align_frame_color(d, c, pose, pc)
            rec = gv.align_color_log()[0]
            assert rec["n_sampled"] == len(exp["fl"]) and rec["n_valid"] == int(((exp["flags"] & 15) == 15).sum())
            assert rec["n_photo"] == int((exp["flags"] == 127).sum())
    finally:
        gv.raycast_camera(None)
    pd, pc = _params(levels=[(1, 1)])
    good = np.argwhere(CR.rows(ref, depth, rgba, pose, I.CAM, 1, pd)["flags"] == 127)
    d, c = depth.copy(), rgba.copy()
    for k, (y, x) in enumerate(good[:: len(good) // 8][:8]):
        d[y, x] = (0.0, np.nan, np.inf, -np.inf, -0.3, 0.04, 5.5, 1e30)[k]
    (ya, xa), (yb, xb) = good[len(good) // 4 + 1], good[len(good) // 2 + 1]
    c[ya, xa, 3] = 0
    c[yb, xb, :3] = (c[yb, xb, :3].astype(int) + 100) % 256
    start = pose.astype(np.float64)
    start[:, 3] += (0.0, 0.004, -0.003)
    for pp in (pose, start.astype(np.float32)):
        exp = CR.rows(ref, d, c, pp, I.CAM, 1, pd)
        _assert_maps_equal(gv.align_color_residuals(d, c, pp, pc), exp, "hand-made pixels")
        assert exp["flags"][ya, xa] == 15 and exp["flags"][yb, xb] == 63 and (exp["flags"] == 127).sum() > 5000


def _check_sums(rec, sg, sc):
    assert rec["n_valid"] == sg["n_valid"] and rec["n_sampled"] == sg["n_sampled"] and rec["n_photo"] == sc["n_valid"]
    for what, got, sm in (("geometric", np.concatenate([rec["A21"], rec["b"], [rec["sum_r2"], rec["sum_wr2"]]]), sg),
                          ("photometric", np.concatenate([rec["Ac21"], rec["bc"], [rec["sum_rc2"], rec["sum_wrc2"]]]), sc)):
        want = np.concatenate([sm["A21"], sm["b"], [sm["sum_r2"], sm["sum_wr2"]]])
        bound = sm["n_valid"] * 2.0 ** -52 * sm["mag"]  # an f64 sum of exact terms in any order
        print("%s sums: largest |delta| / bound = %.3g" % (what, np.max(np.abs(got - want) / np.maximum(bound, 1e-300))))
        assert np.all(np.abs(got - want) <= bound), (what, np.abs(got - want) / bound)


@pytest.mark.parametrize("huber", [0.0, 0.002])
def test_first_evaluation_sums_against_exact_sums(wall, plane, huber):
    for (gv, ref, pose, depth, rgba), stride, pert in ((wall, 1, CI.wall_starts()[3]), (wall, 3, CI.wall_starts()[1]),
                                                       (plane, 1, CI.hand_starts()[3])):
        pd, pc = _params(levels=[(stride, 1)], huber=huber, huber_photo=10 * huber)
        start = I.perturb(pose, *pert)
        gv.align_frame_color(depth, rgba, start, pc)
        rec = gv.align_color_log()[0]
        sg, sc = CR.sums(CR.rows(ref, depth, rgba, start, I.CAM, stride, pd), pd)
        assert sc["n_valid"] > 1000 and sc["A21"].any()
        _check_sums(rec, sg, sc)


def _check_steps(log, damping, photo_weight):
    """every step against the logged joined system, by tf_align_solve.h's backward-error bound"""
    l2 = float(np.float32(photo_weight)) ** 2
    n = 0
    for rec in log:
        if not rec["xi"].any():
            continue
        A, b = rec["A"] + l2 * rec["Ac"], rec["b"] + l2 * rec["bc"]
        M = A + damping * np.diag(A.diagonal())
        lhs = np.linalg.norm(M @ rec["xi"] + b)
        rhs = 1e-12 * (np.linalg.norm(M, 2) * np.linalg.norm(rec["xi"]) + np.linalg.norm(b))
        assert lhs <= rhs, (lhs, rhs)
        n += 1
    return n


def test_known_answer_on_the_textured_plane(plane):
    gv, ref, pose, depth, rgba = plane
    _, pc = _params(**CI.PARAMS)
    geo = gv.align_frame(depth, pose, pc.geo)
    assert geo["status"] == capi.TF_ALIGN_SINGULAR
    ends = []
    for dt, rv in CI.hand_starts():
        res = gv.align_frame_color(depth, rgba, I.perturb(pose, dt, rv), pc)
        log = gv.align_color_log()
        dtr, drr = R.pose_distance(log[-1]["pose"], pose)
        print("from %s mm: %.4g m, %.3g rad from the true pose; photometric rms %.3g -> %.3g, cond %.3g" % (
            np.round(1e3 * dt, 1), dtr, drr, res["rms_photo_first"], res["rms_photo_last"],
            np.linalg.cond(log[-1]["A"] + 0.1 ** 2 * log[-1]["Ac"])))
        assert res["status"] == capi.TF_ALIGN_MAX_ITERS and res["evaluations"] == 11 == len(log)
        assert dtr <= 2 * CI.HAND_TRUTH_T and drr <= 2 * CI.HAND_TRUTH_R
        assert res["n_photo_last"] == res["n_valid_last"] > 5000 and res["n_photo_first"] >= 0.8 * res["n_valid_first"]
        assert _check_steps(log, 0.0, 0.1) == 10
        ends.append(log[-1]["pose"])
    # one pose from all four starts: ten times the spread the restatement's own ends have (its sums are exact; the
    # device's differ from them by the order of summation)
    for e in ends[1:]:
        dt, dr = R.pose_distance(e, ends[0])
        assert dt <= 10 * CI.HAND_SPREAD_T and dr <= 10 * CI.HAND_SPREAD_R, (dt, dr)


def test_textured_wall_reaches_the_restatements_fixed_point(wall, wall_fixed_point):
    gv, ref, pose, depth, rgba = wall
    want, want_log = wall_fixed_point
    _, pc = _params(**CI.PARAMS)
    for k, (dt_, rv) in enumerate(CI.wall_starts()):
        res = gv.align_frame_color(depth, rgba, I.perturb(pose, dt_, rv), pc)
        log = gv.align_color_log()
        dt, dr = R.pose_distance(log[-1]["pose"], want_log[-1]["pose"])
        print("start %d: %.3g m, %.3g rad from the restatement's fixed point; %d of %d photometric" % (
            k, dt, dr, res["n_photo_last"], res["n_valid_last"]))
        assert res["status"] == capi.TF_ALIGN_MAX_ITERS and res["evaluations"] == 11 == len(log)
        assert dt <= 10 * CI.WALL_SPREAD_T and dr <= 10 * CI.WALL_SPREAD_R
        assert res["n_photo_last"] >= 0.95 * res["n_valid_last"] and res["n_valid_last"] >= 0.9 * res["n_sampled"]
        assert np.linalg.cond(log[-1]["A"] + 0.1 ** 2 * log[-1]["Ac"]) < 1e4
        _check_steps(log, 0.0, 0.1)
    res = gv.align_frame_color(depth, rgba, pose, pc)
    assert (res["n_valid_first"], res["n_photo_first"], res["n_sampled"]) == (want["n_valid_first"], want["n_photo_first"], want["n_sampled"])
    assert (res["n_valid_last"], res["n_photo_last"]) == (want["n_valid_last"], want["n_photo_last"])


def _assert_logs_equal(a, b, keys=None):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for key in (keys or x):
            assert np.array_equal(np.asarray(x[key]), np.asarray(y[key])), key


def test_device_form_equals_the_host_form_and_runs_repeat_bit_for_bit(wall):
    gv, _, pose, depth, rgba = wall
    _, pc = _params(damping=1e-4)
    start = I.perturb(pose, *CI.wall_starts()[1])
    host = gv.align_frame_color(depth, rgba, start, pc)
    log = gv.align_color_log()
    bufs = [HipBuffer(depth.nbytes).from_host(depth), HipBuffer(rgba.nbytes).from_host(rgba), HipBuffer(C.sizeof(capi.AlignColorResult))]
    d_depth, d_rgba, d_res = bufs
    P = depth.size
    maps = [HipBuffer(4 * P), HipBuffer(12 * P), HipBuffer(4 * P), HipBuffer(12 * P), HipBuffer(4 * P)]
    try:
        for _ in range(2):
            gv.align_frame_color_device(d_depth.ptr, d_rgba.ptr, start, pc, d_res.ptr)
            gv.sync()
            dev = gv.align_color_result(d_res.to_host())
            assert bytes(np.asarray(dev.pop("pose"))) == bytes(host["pose"]) and dev == {k: v for k, v in host.items() if k != "pose"}
            log2 = gv.align_color_log()
            assert len(log2) == host["evaluations"]
            _assert_logs_equal(log, log2)
        assert _check_steps(log, 1e-4, 0.1) >= 1
        gv.align_color_residuals_device(d_depth.ptr, d_rgba.ptr, start, pc, *[b.ptr for b in maps])
        gv.sync()
        hostmap = gv.align_color_residuals(depth, rgba, start, pc)
        for b, k in zip(maps, ("r", "grad", "rc", "gradc", "flags")):
            assert np.array_equal(b.to_host().view(np.uint32), hostmap[k].view(np.uint32).reshape(-1)), k
    finally:
        for b in bufs + maps:
            b.free()


def test_no_weight_and_no_colour_equal_the_geometric_call_bit_for_bit(corner, wall):
    gc, gp, pose, depth, rgba = corner
    start = I.perturb(pose, I.HAND_DELTA, np.radians(0.2) * np.array([0.6, -0.64, 0.48]))
    levels = dict(levels=[(2, 2), (1, 2)], eps_t=0.0, eps_r=0.0)
    _, pc = _params(**levels)
    _, p0 = _params(photo_weight=0.0, **levels)
    geo = gp.align_frame(depth, start, pc.geo)
    glog = gp.align_log()
    assert geo["status"] == capi.TF_ALIGN_MAX_ITERS and len(glog) == 5

    def same(res, log):
        assert bytes(res["pose"]) == bytes(geo["pose"])
        assert {k: res[k] for k in geo if k != "pose"} == {k: v for k, v in geo.items() if k != "pose"}
        _assert_logs_equal(log, glog, GEO_KEYS)

    # every colour count 0, default weight
    res = gp.align_frame_color(depth, rgba, start, pc)
    log = gp.align_color_log()
    same(res, log)
    assert res["n_photo_first"] == 0 == res["n_photo_last"] and all(not r["Ac21"].any() and not r["bc"].any() for r in log)
    # a coloured volume, weight 0: the photometric sums are there and weigh nothing
    res = gc.align_frame_color(depth, rgba, start, p0)
    log = gc.align_color_log()
    same(res, log)
    assert res["n_photo_first"] > 1000 and log[0]["Ac21"].any()
    # ... and with the default weight the step differs
    gc.align_frame_color(depth, rgba, start, pc)
    assert not np.array_equal(gc.align_color_log()[0]["xi"], glog[0]["xi"])
    # the same on the integrated wall, default levels
    gv, _, wpose, wdepth, wrgba = wall
    wstart = I.perturb(wpose, *CI.wall_starts()[1])
    geo = gv.align_frame(wdepth, wstart)
    glog = gv.align_log()
    res = gv.align_frame_color(wdepth, wrgba, wstart, capi.AlignColorParams(photo_weight=0.0))
    same(res, gv.align_color_log())


def test_levels_and_stops(wall):
    gv, _, pose, depth, rgba = wall
    start = I.perturb(pose, *CI.wall_starts()[1])
    _, pc = _params(levels=[(4, 2), (2, 2), (1, 2)], eps_t=0.0, eps_r=0.0)
    res = gv.align_frame_color(depth, rgba, start, pc)
    log = gv.align_color_log()
    assert res["evaluations"] == 7 and res["status"] == capi.TF_ALIGN_MAX_ITERS
    assert [(r["level"], r["stride"]) for r in log] == [(0, 4), (0, 4), (1, 2), (1, 2), (2, 1), (2, 1), (2, 1)]
    assert [r["n_sampled"] for r in log] == [40 * 30] * 2 + [80 * 60] * 2 + [160 * 120] * 3
    assert all(r["n_photo"] > 0.5 * r["n_sampled"] for r in log)
    # eps above any step: the first step ends the (only) level, then the closing evaluation
    _, pc = _params(levels=[(1, 5)], eps_t=1.0, eps_r=1.0)
    res = gv.align_frame_color(depth, rgba, start, pc)
    assert res["evaluations"] == 2 == len(gv.align_color_log()) and res["status"] == capi.TF_ALIGN_CONVERGED
    # ... at a level that is not the last one, the next level still runs
    _, pc = _params(levels=[(2, 5), (1, 1)], eps_t=1.0, eps_r=1.0)
    res = gv.align_frame_color(depth, rgba, start, pc)
    assert res["evaluations"] == 3 and res["status"] == capi.TF_ALIGN_CONVERGED
    assert [(r["level"], r["stride"]) for r in gv.align_color_log()] == [(0, 2), (1, 1), (1, 1)]
    # too few goes by the geometric count
    _, pc = _params(min_valid=160 * 120 + 1)
    res = gv.align_frame_color(depth, rgba, start, pc)
    assert res["status"] == capi.TF_ALIGN_TOO_FEW and res["evaluations"] == 1
    assert np.array_equal(res["pose"].view(np.uint32), start.view(np.uint32))
    # ... and few photometric pixels are no stop: no alpha anywhere
    none = rgba.copy()
    none[..., 3] = 0
    res = gv.align_frame_color(depth, none, start, capi.AlignColorParams())
    assert res["status"] in (capi.TF_ALIGN_CONVERGED, capi.TF_ALIGN_MAX_ITERS) and res["n_photo_first"] == 0 == res["n_photo_last"]
    assert res["rms_photo_first"] == 0 and res["n_valid_last"] > 0.9 * res["n_sampled"]
    empty = capi.Volume(CI.WALL_RES, I.CAM, max_chunks=1 << 10)
    try:
        res = empty.align_frame_color(depth, rgba, start)
        assert res["status"] == capi.TF_ALIGN_TOO_FEW and res["n_valid_first"] == 0 == res["n_photo_first"]
        assert not empty.align_color_residuals(depth, rgba, start)["flags"].any() & 2
    finally:
        empty.close()


def test_invalid_parameters_launch_nothing(wall):
    gv, _, pose, depth, rgba = wall
    good = gv.align_frame_color(depth, rgba, pose)
    n_log = len(gv.align_color_log())
    bad = [dict(n_levels=0), dict(n_levels=5), dict(stride=[0, 1, 1, 1]), dict(iters=[30, 30, 5, 0]), dict(iters=[-1, 3, 2, 0]),
           dict(min_depth=np.nan), dict(max_residual=np.nan), dict(huber=-0.1), dict(damping=-1e-3), dict(eps_t=-1e-6),
           dict(min_depth=2.0, max_depth=1.0), dict(photo_weight=-0.1), dict(photo_weight=np.nan), dict(photo_weight=np.inf),
           dict(max_photo_residual=-1.0), dict(max_photo_residual=np.nan), dict(huber_photo=-0.01), dict(huber_photo=np.inf)]
    res = capi.AlignColorResult()
    res.geo.status = 77
    f32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    d, c, p = np.ascontiguousarray(depth, np.float32), np.ascontiguousarray(rgba), np.ascontiguousarray(pose, np.float32)
    for kw in bad:
        pc = capi.AlignColorParams(**kw)
        assert gv.L.tf_align_frame_color(gv.h, f32p(d), u8p(c), f32p(p), C.byref(pc), C.byref(res)) == capi.TF_ERR_INVALID, kw
        if "iters" not in kw:
            assert gv.L.tf_align_color_residuals(gv.h, f32p(d), u8p(c), f32p(p), C.byref(pc), None, None, None, None,
                                                 None) == capi.TF_ERR_INVALID, kw
    pc = capi.AlignColorParams()
    q = p.copy()
    q.reshape(-1)[7] = np.nan
    assert gv.L.tf_align_frame_color(gv.h, f32p(d), u8p(c), f32p(q), C.byref(pc), C.byref(res)) == capi.TF_ERR_INVALID
    assert gv.L.tf_align_frame_color(gv.h, f32p(d), None, f32p(p), C.byref(pc), C.byref(res)) == capi.TF_ERR_INVALID
    assert gv.L.tf_align_frame_color(gv.h, None, u8p(c), f32p(p), C.byref(pc), C.byref(res)) == capi.TF_ERR_INVALID
    assert res.geo.status == 77  # nothing was written
    assert len(gv.align_color_log()) == n_log == good["evaluations"]  # ... and nothing ran


def _snapshot(gv):
    ids = sorted_ids(gv.list_chunks())
    s, w, c = gv.get_chunks(ids)
    mids = sorted_ids(gv.list_meshes())
    meshes = gv.get_meshes(mids)
    return (bytes(gv.stats()), sorted_ids(gv.dirty()).tobytes(), ids.tobytes(), s.tobytes(), w.tobytes(), c.tobytes(),
            mids.tobytes(), b"".join(np.ascontiguousarray(m).tobytes() for m in meshes), gv.check_neighbours().tobytes())


def test_read_only_and_the_geometric_log_and_integration_stay_bit_exact(gpu_required):
    ov, gv, cam, _ = make_pair(res=CI.WALL_RES, cam=I.CAM, max_chunks=1 << 14)
    frames = CI.wall_frames()
    try:
        for k, (depth, rgba, pose) in enumerate(frames[:4]):
            ov.integrate_frame(depth, rgba, pose)
            gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, k)
        gv.update_meshes()
        ov.update_meshes()
        gv.sync()
        depth, rgba, pose = frames[2]
        start = I.perturb(pose, *CI.wall_starts()[1])
        gv.align_frame(depth, start)
        glog = gv.align_log()
        before = _snapshot(gv)
        res = gv.align_frame_color(depth, rgba, start)
        assert res["n_photo_first"] > 1000
        gv.align_color_residuals(depth, rgba, pose)
        assert len(gv.align_color_log()) == res["evaluations"]
        assert _snapshot(gv) == before
        _assert_logs_equal(gv.align_log(), glog)
        depth, rgba, pose = frames[4]
        ov.integrate_frame(depth, rgba, pose)
        gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, 4)
        gv.sync()
        assert_chunks_equal(ov, gv, ov.list_chunks(), "after a colour alignment")
        # tf_volume_reset gives the state block back: an empty log, and the next call allocates it again
        gv.reset()
        assert gv.align_color_log() == []
        gv.set_camera(I.CAM)
        assert gv.align_frame_color(depth, rgba, pose)["status"] == capi.TF_ALIGN_TOO_FEW
    finally:
        gv.close()
        ov.close()


def test_host_mirror_align_color(gpu_required, tmp_path):
    exe = str(tmp_path / "mirror_align_color")
    src = os.path.join(ROOT, "tests", "cpp_align_color", "mirror_align_color.cpp")
    lib = os.path.join(ROOT, "texturefusion_amd")
    subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", src, "-o", exe, "-L" + lib, "-ltexfusion_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mirror ok" in r.stdout, r.stdout + r.stderr
