"""Group alignment on the MI355X (tf_align_group.hip): a body of one frame against tf_align_frame byte for byte, bodies that
stop beside bodies that go on, the rigid known answer, a two-frame body's sums against exact sums, the multi-step rigid
run against the restatement's end, device and host forms, a camera whose tiles hang over both borders, invalid arguments,
the read-only guarantee, tf_align_unit_group feeding the keyframe unit, and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import align_group_inputs as GI
from tests import align_group_ref as G
from tests import align_inputs as I
from tests import align_ref as R
from tests.raycast_ref import RefVolume
from tests.util import RES5, HipBuffer, sorted_ids
from texturefusion_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_STEP = dict(levels=[(1, 1)], huber=0.0, damping=0.0)
f32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))


def _params(**kw):
    """the same parameters for the restatement (dict) and the library (tf_align_params)"""
    return R.params(**kw), capi.AlignParams(**kw)


@pytest.fixture(scope="module")
def hand(gpu_required):
    gv = capi.Volume(I.HAND_RES, I.CAM, max_chunks=1 << 10)
    ids, s, w, c = I.hand_corner()
    for k in range(len(ids)):
        gv.set_chunk(ids[k], s[k], w[k], c[k])
    gv.sync()
    poses, depths = GI.hand_group()
    yield gv, RefVolume(ids, s, w, c, I.HAND_RES), poses, depths
    gv.close()


@pytest.fixture(scope="module")
def scene(gpu_required):
    """the corner scene integrated on the device, built once; the restatement reads the device's own chunks"""
    frames = I.corner_frames()
    gv = capi.Volume(RES5, I.CAM, max_chunks=1 << 14)
    for k, (depth, rgba, pose) in enumerate(frames):
        gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, k)
    gv.update_meshes()  # the neighbour table filled in: the sampler reads it
    gv.sync()
    ref = RefVolume.from_volume(gv, gv.list_chunks(), gv.res)
    yield gv, ref, frames
    gv.close()


@pytest.fixture(scope="module")
def rigid_end(hand):
    """the restatement's end of the multi-step rigid run from the first start: computed once, shared"""
    _, ref, poses, depths = hand
    dt, aa = GI.RIGID_STARTS[0]
    return G.align_group(ref, depths, GI.move_group(poses, dt, aa), I.CAM, R.params(**GI.RIGID_PARAMS))


def _frame_raw(gv, depth, pose, pc):
    """tf_align_frame -> (the result's bytes, the log's bytes)"""
    d, p = np.ascontiguousarray(depth, np.float32), np.ascontiguousarray(pose, np.float32)
    res = capi.AlignResult()
    assert gv.L.tf_align_frame(gv.h, f32p(d), f32p(p), C.byref(pc), C.byref(res)) == capi.TF_OK
    n = C.c_int64(0)
    buf = (capi.AlignIter * capi.TF_ALIGN_MAX_EVALUATIONS)()
    assert gv.L.tf_align_log(gv.h, buf, capi.TF_ALIGN_MAX_EVALUATIONS, C.byref(n)) == capi.TF_OK
    return bytes(res), bytes(buf)[:n.value * C.sizeof(capi.AlignIter)]


def _group_log_raw(gv, body):
    n = C.c_int64(0)
    buf = (capi.AlignIter * capi.TF_ALIGN_MAX_EVALUATIONS)()
    assert gv.L.tf_align_group_log(gv.h, body, buf, capi.TF_ALIGN_MAX_EVALUATIONS, C.byref(n)) == capi.TF_OK
    return bytes(buf)[:n.value * C.sizeof(capi.AlignIter)]


def _group_raw(gv, depths, poses, body, pc):
    """tf_align_group -> (the AlignGroupResult, [the log's bytes per body])"""
    ds = [np.ascontiguousarray(d, np.float32) for d in depths]
    ps = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 12))
    ptrs = (C.c_void_p * len(ds))(*[d.ctypes.data for d in ds])
    b = None if body is None else np.ascontiguousarray(body, np.int32)
    res = capi.AlignGroupResult()
    rc = gv.L.tf_align_group(gv.h, len(ds), ptrs, f32p(ps), None if b is None else b.ctypes.data_as(C.POINTER(C.c_int32)),
                             C.byref(pc), C.byref(res))
    assert rc == capi.TF_OK
    return res, [_group_log_raw(gv, k) for k in range(res.n_bodies)]


def _scene_starts(frames, ks):
    """frames ks of the corner scene, each at its integration pose moved by one of the tests' perturbations"""
    pert = I.held_perturbations()
    return [frames[k][0] for k in ks], [I.perturb(frames[k][2], *pert[i % len(pert)]) for i, k in enumerate(ks)]


def test_one_frame_is_align_frame_byte_for_byte(scene):
    gv, _, frames = scene
    _, pc = _params()
    depths, starts = _scene_starts(frames, [I.HELD])
    want_res, want_log = _frame_raw(gv, depths[0], starts[0], pc)
    res, logs = _group_raw(gv, depths, starts, None, pc)
    assert (res.n_frames, res.n_bodies) == (1, 1)
    assert bytes(res.body[0]) == want_res and logs[0] == want_log and len(want_log) >= 2 * C.sizeof(capi.AlignIter)
    out = gv.align_group_result(res)
    assert np.array_equal(out["pose"][0], out["body"][0]["pose"])
    assert out["frame_valid_first"][0] == out["body"][0]["n_valid_first"] > 1000
    assert out["frame_valid_last"][0] == out["body"][0]["n_valid_last"]
    # the entries past the call's frames and bodies are zero
    assert not any(bytes(res.body[1])) and not np.array(res.pose)[1:].any() and not any(res.frame_valid_first[1:])


def test_three_bodies_equal_three_calls_and_a_stopped_body_stops_alone(scene, hand):
    # the corner scene: the middle frame's depth is all zero, TF_ALIGN_TOO_FEW at its first evaluation
    gv, _, frames = scene
    _, pc = _params()
    depths, starts = _scene_starts(frames, [I.HELD - 1, I.HELD, I.HELD + 1])
    depths[1] = np.zeros_like(depths[1])
    want = [_frame_raw(gv, depths[k], starts[k], pc) for k in range(3)]
    res, logs = _group_raw(gv, depths, starts, [0, 1, 2], pc)
    assert (res.n_frames, res.n_bodies) == (3, 3)
    for k in range(3):
        assert bytes(res.body[k]) == want[k][0] and logs[k] == want[k][1], k
        assert bytes(res.pose[k]) == bytes(res.body[k].pose)
    assert res.body[1].status == capi.TF_ALIGN_TOO_FEW and res.body[1].evaluations == 1
    assert bytes(res.pose[1]) == starts[1].tobytes()
    for k in (0, 2):
        assert res.body[k].status <= capi.TF_ALIGN_MAX_ITERS and res.body[k].evaluations >= 4
        assert res.body[k].rms_last < res.body[k].rms_first
    # the hand-built corner: the keyframe sees one face, TF_ALIGN_SINGULAR at its first evaluation
    hv, _, poses, hdepths = hand
    _, pc = _params(levels=[(2, 2), (1, 2)], huber=0.0, eps_t=0.0, eps_r=0.0)
    start = GI.move_group(poses, I.HAND_DELTA)
    want = [_frame_raw(hv, hdepths[k], start[k], pc) for k in range(3)]
    res, logs = _group_raw(hv, hdepths, start, [0, 1, 2], pc)
    for k in range(3):
        assert bytes(res.body[k]) == want[k][0] and logs[k] == want[k][1], k
    assert res.body[0].status == capi.TF_ALIGN_SINGULAR and res.body[0].evaluations == 1
    assert bytes(res.pose[0]) == start[0].tobytes() and res.frame_valid_first[0] > 500
    for k in (1, 2):
        assert res.body[k].status == capi.TF_ALIGN_MAX_ITERS and res.body[k].evaluations == 5
        dt, dr = R.pose_distance(np.array(res.pose[k], np.float32), poses[k])
        assert dt <= 1e-5 and dr <= 1e-5


def test_known_answer_of_the_rigid_group(hand):
    gv, _, poses, depths = hand
    _, pc = _params(**ONE_STEP)
    assert gv.align_frame(depths[0], poses[0], pc)["status"] == capi.TF_ALIGN_SINGULAR
    out = gv.align_group(depths, GI.move_group(poses, I.HAND_DELTA), None, pc)
    log = gv.align_group_log(0)
    dt, dr = G.group_distance(out["pose"], poses)
    print("rigid known answer on the device: dt %.3g m, dr %.3g rad" % (dt, dr))
    body = out["body"][0]
    assert out["n_bodies"] == 1 and body["status"] == capi.TF_ALIGN_MAX_ITERS and body["evaluations"] == 2 == len(log)
    assert dt <= 1e-5 and dr <= 1e-5
    assert log[0]["n_valid"] == 25473 and list(out["frame_valid_first"]) == [3445, 11219, 10809]
    assert body["rms_last"] < 1e-6 < body["rms_first"]
    assert np.abs(log[0]["xi"][:3] + I.HAND_DELTA).max() <= 1e-5 and np.abs(log[0]["xi"][3:]).max() <= 1e-5
    assert np.array_equal(log[1]["pose"].astype(np.float32), out["pose"][0]) and gv.align_group_log(1) == []


def _check_sums(rec, sm):
    assert rec["n_valid"] == sm["n_valid"] and rec["n_sampled"] == sm["n_sampled"]
    got = np.concatenate([rec["A21"], rec["b"], [rec["sum_r2"], rec["sum_wr2"]]])
    want = np.concatenate([sm["A21"], sm["b"], [sm["sum_r2"], sm["sum_wr2"]]])
    bound = sm["n_valid"] * 2.0 ** -52 * sm["mag"]  # an f64 sum of exact terms in any order
    print("sums: largest |delta| / bound = %.3g" % np.max(np.abs(got - want) / np.maximum(bound, 1e-300)))
    assert np.all(np.abs(got - want) <= bound), np.abs(got - want) / bound


@pytest.mark.parametrize("huber", [0.0, 0.002])
def test_two_frame_body_sums_against_exact_sums(scene, hand, huber):
    gv, ref, frames = scene
    hv, href, hposes, hdepths = hand
    depths, _ = _scene_starts(frames, [I.HELD, I.HELD + 1])
    moved = GI.move_group([frames[I.HELD][2], frames[I.HELD + 1][2]], *I.held_perturbations()[2])
    hmoved = GI.move_group(hposes[1:], I.HAND_DELTA, np.radians(0.3) * np.array([0.6, -0.64, 0.48]))
    for v, rf, dd, pp, stride in ((gv, ref, depths, moved, 1), (gv, ref, depths, moved, 3), (hv, href, hdepths[1:], hmoved, 1)):
        pd, pc = _params(levels=[(stride, 1)], huber=huber)
        out = v.align_group(dd, pp, None, pc)
        rw = G.body_rows(rf, dd, pp, I.CAM, stride, pd)
        assert list(out["frame_valid_first"]) == rw["per_frame"] and min(rw["per_frame"]) > 1000
        _check_sums(v.align_group_log(0)[0], R.sums(rw, pd))


def test_rigid_run_ends_at_the_restatements_end_from_two_starts(hand, rigid_end):
    gv, _, poses, depths = hand
    _, pc = _params(**GI.RIGID_PARAMS)
    for k, (dt, aa) in enumerate(GI.RIGID_STARTS):
        out = gv.align_group(depths, GI.move_group(poses, dt, aa), None, pc)
        log = gv.align_group_log(0)
        assert out["body"][0]["status"] == capi.TF_ALIGN_MAX_ITERS and out["body"][0]["evaluations"] == 5 == len(log)
        d = G.group_distance(out["pose"], rigid_end["pose64"])
        print("start %d: %.3g m, %.3g rad from the restatement's end; %.3g m from the truth" % (
            k, d[0], d[1], G.group_distance(out["pose"], poses)[0]))
        assert d[0] <= GI.GROUP_TOL_T and d[1] <= GI.GROUP_TOL_R
        assert [r["n_sampled"] for r in log] == [3 * 160 * 120] * 5 and log[-1]["n_valid"] == rigid_end["log"][0][-1]["n_valid"]


def test_device_form_equals_the_host_form_and_runs_repeat_bit_for_bit(scene):
    gv, _, frames = scene
    _, pc = _params(damping=1e-4)
    ks = list(range(I.HELD - 3, I.HELD + 4))
    body = [0, 0, 1, 0, 1, 2, 2]
    depths = [frames[k][0] for k in ks]
    starts = GI.move_group([frames[k][2] for k in ks], *I.held_perturbations()[1])
    host, host_logs = _group_raw(gv, depths, starts, body, pc)
    assert (host.n_frames, host.n_bodies) == (7, 3) and all(host.body[b].evaluations >= 4 for b in range(3))
    assert all(host.body[b].rms_last < host.body[b].rms_first / 2 for b in range(3))
    bufs = [HipBuffer(d.nbytes).from_host(d) for d in depths]
    d_res = HipBuffer(C.sizeof(capi.AlignGroupResult))
    try:
        for _ in range(2):
            gv.align_group_device([b.ptr for b in bufs], starts, body, pc, d_res.ptr)
            gv.sync()
            assert bytes(d_res.to_host()) == bytes(host)
            assert [_group_log_raw(gv, b) for b in range(3)] == host_logs
    finally:
        for b in bufs + [d_res]:
            b.free()
    # the frames of a body moved by one rigid motion: their relative poses are the start's (four f32 poses near 2 m, half an ulp of
    # 1.2e-7 m in each coordinate of each: 2e-6)
    out = gv.align_group_result(host)
    rel = lambda a, b: a[:, :3].T.astype(np.float64) @ (b[:, 3].astype(np.float64) - a[:, 3])
    for a, b in ((0, 1), (0, 3), (2, 4), (5, 6)):
        assert np.abs(rel(out["pose"][a], out["pose"][b]) - rel(starts[a], starts[b])).max() <= 2e-6


def test_tiles_over_both_borders_with_two_frames_and_stride_3(hand):
    """a 13 x 9 camera: one full tile column and a partial one, one full tile row and a partial one; at stride 3 a 5 x 3
    grid of samples in one tile per frame"""
    gv, ref, poses, _ = hand
    small = synth.Camera(13, 9, 11.0, 11.0, 6.5, 4.5)
    gv.raycast_camera(small)  # (tf_set_camera takes widths that are multiples of 8 only; the readers' camera any)
    try:
        depths = [I.hand_depth(P, small, edge_voxels=0.0) for P in poses[:2]]
        for stride in (3, 1):
            pd, pc = _params(levels=[(stride, 1)], huber=0.0, min_valid=1)
            out = gv.align_group(depths, poses[:2], None, pc)
            rw = G.body_rows(ref, depths, poses[:2], small, stride, pd)
            rec = gv.align_group_log(0)[0]
            assert rec["n_sampled"] == len(rw["fl"]) == 2 * len(range(0, 13, stride)) * len(range(0, 9, stride))
            assert list(out["frame_valid_first"]) == rw["per_frame"] and sum(rw["per_frame"]) > 3
            _check_sums(rec, R.sums(rw, pd))
    finally:
        gv.raycast_camera(None)


def test_invalid_arguments_launch_nothing(scene):
    gv, _, frames = scene
    L = gv.L
    depths, starts = _scene_starts(frames, [I.HELD, I.HELD + 1, I.HELD + 2])
    good, good_logs = _group_raw(gv, depths, starts, [0, 0, 1], capi.AlignParams())
    ds = [np.ascontiguousarray(d, np.float32) for d in depths] * 3
    ps = np.ascontiguousarray(np.tile(np.asarray(starts, np.float32).reshape(3, 12), (3, 1)))
    res = capi.AlignGroupResult()
    C.memset(C.byref(res), 0x5A, C.sizeof(res))
    preset = bytes(res)
    d_res = HipBuffer(C.sizeof(res)).from_host(np.frombuffer(preset, np.uint8))
    bufs = [HipBuffer(d.nbytes).from_host(d) for d in ds[:3]] * 3

    def call(n, body=None, pc=None, images=None, poses=ps, null_result=False):
        pc = pc or capi.AlignParams()
        b = None if body is None else np.ascontiguousarray(body, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
        m = max(n, 1)
        host = (C.c_void_p * m)(*(images if images is not None else [d.ctypes.data for d in ds[:m]]))
        dev = (C.c_void_p * m)(*(images if images is not None else [x.ptr for x in bufs[:m]]))
        rc = [L.tf_align_group(gv.h, n, host, f32p(poses), b, C.byref(pc), None if null_result else C.byref(res)),
              L.tf_align_group_device(gv.h, n, dev, f32p(poses), b, C.byref(pc), None if null_result else d_res.ptr)]
        assert rc == [capi.TF_ERR_INVALID] * 2, (n, body, rc)

    try:
        for kw in (dict(n_levels=0), dict(n_levels=5), dict(stride=[0, 1, 1, 1]), dict(iters=[30, 30, 5, 0]), dict(iters=[-1, 3, 2, 0]),
                   dict(min_depth=np.nan), dict(min_depth=2.0, max_depth=1.0), dict(huber=-0.1), dict(damping=-1e-3),
                   dict(eps_t=-1e-6), dict(eps_r=np.inf)):
            call(3, [0, 0, 1], capi.AlignParams(**kw))
        for frame, entry in ((0, 0), (1, 3), (2, 11)):  # a pose that is not finite, in any frame
            q = ps.copy()
            q[frame, entry] = (np.nan, np.inf, -np.inf)[frame]
            call(3, None, poses=q)
        call(0)
        call(-1)
        call(8)
        call(3, images=[ds[0].ctypes.data, None, ds[2].ctypes.data])       # a null image
        call(3, images=[ds[0].ctypes.data, ds[1].ctypes.data, None])
        for body in ([1, 0, 0], [0, 2, 1], [0, -1, 0], [0, 0, 2], [0, 1, 3]):  # not numbered by first appearance
            call(3, body)
        call(7, [0, 1, 2, 3, 4, 5, 7])
        call(3, null_result=True)
        assert L.tf_align_group(gv.h, 3, None, f32p(ps), None, C.byref(capi.AlignParams()), C.byref(res)) == capi.TF_ERR_INVALID
        assert L.tf_align_group(gv.h, 3, (C.c_void_p * 3)(*[d.ctypes.data for d in ds[:3]]), None, None,
                                C.byref(capi.AlignParams()), C.byref(res)) == capi.TF_ERR_INVALID
        n = C.c_int64(0)
        for body in (-1, 7):
            assert L.tf_align_group_log(gv.h, body, None, 0, C.byref(n)) == capi.TF_ERR_INVALID
        # tf_align_unit_group: a null group, a null result, n_local out of range, a local frame without an image
        grp = capi.Volume.unit_group(1, (bufs[0].ptr, None, None, starts[0]), [(bufs[1].ptr, starts[1]), (bufs[2].ptr, starts[2])])
        before = bytes(grp)
        pc = capi.AlignParams()
        assert L.tf_align_unit_group(gv.h, None, 1, C.byref(pc), C.byref(res)) == capi.TF_ERR_INVALID
        assert L.tf_align_unit_group(gv.h, C.byref(grp), 1, C.byref(pc), None) == capi.TF_ERR_INVALID
        assert L.tf_align_unit_group(gv.h, C.byref(grp), 1, None, C.byref(res)) == capi.TF_ERR_INVALID
        grp.n_local = 7
        assert L.tf_align_unit_group(gv.h, C.byref(grp), 1, C.byref(pc), C.byref(res)) == capi.TF_ERR_INVALID
        grp.n_local = 2
        grp.local[1].d_depth = None
        assert L.tf_align_unit_group(gv.h, C.byref(grp), 0, C.byref(pc), C.byref(res)) == capi.TF_ERR_INVALID
        grp.local[1].d_depth = bufs[2].ptr
        assert bytes(grp) == before
        # nothing was written, on the host or on the device, and nothing ran: the logs are still the good call's
        assert bytes(res) == preset and bytes(d_res.to_host()) == preset
        assert [_group_log_raw(gv, b) for b in range(2)] == good_logs and _group_log_raw(gv, 2) == b""
        assert good.n_bodies == 2
    finally:
        for b in bufs[:3] + [d_res]:
            b.free()


def _snapshot(gv):
    ids = sorted_ids(gv.list_chunks())
    s, w, c = gv.get_chunks(ids)
    return (bytes(gv.stats()), sorted_ids(gv.dirty()).tobytes(), ids.tobytes(), s.tobytes(), w.tobytes(), c.tobytes(),
            gv.check_summaries(), gv.check_neighbours().tobytes())


def test_read_only_and_the_frame_log_keeps_its_meaning(scene):
    gv, _, frames = scene
    _, pc = _params()
    depths, starts = _scene_starts(frames, [I.HELD, I.HELD + 1, I.HELD + 2])
    _, frame_log = _frame_raw(gv, depths[0], starts[0], pc)
    before = _snapshot(gv)
    assert before[6][0] > 1000 and before[6][1:] == (0, 0)
    out = gv.align_group(depths, starts, [0, 0, 1], pc)
    assert out["body"][0]["n_valid_first"] > 1000
    bufs = [HipBuffer(d.nbytes).from_host(d) for d in depths]
    try:
        grp = capi.Volume.unit_group(3, (bufs[0].ptr, None, None, starts[0]), [(bufs[1].ptr, starts[1]), (bufs[2].ptr, starts[2])])
        gv.align_unit_group(grp, rigid=False, params=pc)
    finally:
        for b in bufs:
            b.free()
    assert len(gv.align_group_log(2)) >= 2  # the unit group's three bodies
    assert _snapshot(gv) == before
    n = C.c_int64(0)
    buf = (capi.AlignIter * capi.TF_ALIGN_MAX_EVALUATIONS)()
    assert gv.L.tf_align_log(gv.h, buf, capi.TF_ALIGN_MAX_EVALUATIONS, C.byref(n)) == capi.TF_OK
    assert bytes(buf)[:n.value * C.sizeof(capi.AlignIter)] == frame_log and n.value >= 2


def test_unit_group_comes_back_aligned_and_feeds_the_keyframe_unit(gpu_required):
    """tf_align_unit_group writes result.pose into the struct, and tf_keyframe_unit_device on that struct leaves the chunks
    it leaves on a struct filled with those poses by hand"""
    frames = I.corner_frames()
    a = capi.Volume(RES5, I.CAM, max_chunks=1 << 14)
    b = capi.Volume(RES5, I.CAM, max_chunks=1 << 14)
    ks = [I.HELD, I.HELD + 1, I.HELD + 2]
    dd = [HipBuffer(frames[k][0].nbytes).from_host(frames[k][0]) for k in ks]
    dc = HipBuffer(frames[ks[0]][1].nbytes).from_host(frames[ks[0]][1])
    try:
        for k, (depth, rgba, pose) in enumerate(frames[:5]):
            for v in (a, b):
                v.integrate_frame_host(depth, rgba, pose.reshape(12), None, k)
        for v in (a, b):
            v.update_meshes()
        truth = [frames[k][2] for k in ks]
        start = GI.move_group(truth, *I.held_perturbations()[1])
        mk = lambda poses: capi.Volume.unit_group(40, (dd[0].ptr, dc.ptr, None, poses[0]), [(dd[1].ptr, poses[1]), (dd[2].ptr, poses[2])],
                                                  old_keyframe_pose=truth[0], old_local_poses=truth[1:])
        grp = mk(start)
        out = a.align_unit_group(grp, rigid=True)
        body = out["body"][0]
        assert out["n_frames"] == 3 and out["n_bodies"] == 1 and body["status"] <= capi.TF_ALIGN_MAX_ITERS
        assert body["rms_last"] < body["rms_first"] / 2 and G.group_distance(out["pose"], truth)[0] < float(RES5)
        got = [np.array(f.pose, np.float32) for f in (grp.keyframe, grp.local[0], grp.local[1])]
        for k in range(3):
            assert got[k].tobytes() == out["pose"][k].tobytes() != start[k].tobytes()
        assert bytes(grp.old_keyframe_pose) == truth[0].astype(np.float32).tobytes()
        assert bytes(grp.old_local_pose[1]) == truth[2].astype(np.float32).tobytes()
        a.keyframe_unit(fresh=grp, texture=False)
        b.keyframe_unit(fresh=mk(out["pose"]), texture=False)
        a.sync()
        b.sync()
        ids = sorted_ids(a.list_chunks())
        assert np.array_equal(ids, sorted_ids(b.list_chunks())) and len(ids) > 1000
        for x, y in zip(a.get_chunks(ids), b.get_chunks(ids)):
            assert x.tobytes() == y.tobytes()
    finally:
        for h in dd + [dc]:
            h.free()
        a.close()
        b.close()


def test_host_mirror_align_group(gpu_required, tmp_path):
    exe = str(tmp_path / "mirror_align_group")
    src = os.path.join(ROOT, "tests", "cpp_align_group", "mirror_align_group.cpp")
    lib = os.path.join(ROOT, "texturefusion_amd")
    subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", src,
                    "-o", exe, "-L" + lib, "-ltexfusion_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                    "-lamdhip64"], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mirror ok" in r.stdout, r.stdout + r.stderr
