"""Frame-to-model alignment on the MI355X (tf_align.hip): the residual maps against the numpy restatement bit for bit, the
sums against exact sums, every logged step against a numpy solve, the known answer on the hand-built corner, the corner
scene's fixed point, levels and stops, invalid parameters, the read-only guarantee, the device forms and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import align_inputs as I
from tests import align_ref as R
from tests.raycast_ref import RefVolume
from tests.util import RES5, HipBuffer, assert_chunks_equal, make_pair, sorted_ids
from texturefusion_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_STEP = dict(levels=[(1, 1)], huber=0.0, damping=0.0)


def _params(**kw):
    """the same parameters for the restatement (dict) and the library (tf_align_params)"""
    return R.params(**kw), capi.AlignParams(**kw)


def _hand_volume(chunks):
    gv = capi.Volume(I.HAND_RES, I.CAM, max_chunks=1 << 10)
    ids, s, w, c = chunks
    for k in range(len(ids)):
        gv.set_chunk(ids[k], s[k], w[k], c[k])
    gv.sync()
    return gv, RefVolume(ids, s, w, c, I.HAND_RES)


@pytest.fixture(scope="module")
def hand(gpu_required):
    gv, ref = _hand_volume(I.hand_corner())
    pose = I.hand_pose()
    yield gv, ref, pose, I.hand_depth(pose)
    gv.close()


@pytest.fixture(scope="module")
def scene(gpu_required):
    """the corner scene integrated on the device; the restatement reads the device's own chunks"""
    frames = I.corner_frames()
    gv = capi.Volume(RES5, I.CAM, max_chunks=1 << 14)
    for k, (depth, rgba, pose) in enumerate(frames):
        gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, k)
    gv.update_meshes()  # the neighbour table filled in: the sampler reads it
    gv.sync()
    st = gv.stats()
    # parked chunks exist (GarbageCollect parks what a frame selected and did not update: the chunks just off the surface
    # band, which the neighbour table still names).  The restatement knows the alive chunks only and counts the rest absent.
    assert st.n_slots > st.n_chunks, (st.n_slots, st.n_chunks)
    ref = RefVolume.from_volume(gv, gv.list_chunks(), gv.res)
    depth, _, pose = frames[I.HELD]
    yield gv, ref, pose, depth
    gv.close()


@pytest.fixture(scope="module")
def scene_fixed_point(scene):
    """the restatement's fixed point from the integration pose: computed once, shared"""
    _, ref, pose, depth = scene
    return R.align(ref, depth, pose, I.CAM, R.params(**I.SCENE_PARAMS))


def _assert_maps_equal(got, exp, what):
    assert np.array_equal(got["flags"], exp["flags"]), "%s: flags differ at %d pixels" % (what, (got["flags"] != exp["flags"]).sum())
    for k in ("r", "grad"):
        assert np.array_equal(got[k].view(np.uint32), exp[k].view(np.uint32)), "%s: %s differs at %d" % (
            what, k, (got[k].view(np.uint32) != exp[k].view(np.uint32)).sum())


def _samples_in_chunks_that_are_not_alive(ref, rw, pose, depth, stride):
    """how many of the in-range pixels have one of their seven sample points in a chunk that is not alive (the chunk that
    holds the point; the restatement's slot lookup is -1 there): such a chunk was never created, or it is parked"""
    P = np.asarray(pose, np.float32).reshape(3, 4)
    ok = rw["fl"] >= 1
    pw = (P[:, 3][None, :] + rw["q"])[ok]
    e = np.float32(8) * ref.res
    hit = np.zeros(len(pw), bool)
    for off in ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        c = np.floor((pw + np.asarray(off, np.float32) * ref.res) / e).astype(np.int64)
        hit |= ref.slot(c[:, 0], c[:, 1], c[:, 2]) < 0
    return int(hit.sum())


@pytest.mark.parametrize("stride", [1, 3])
def test_residual_maps_bit_exact_on_the_corner_scene(scene, stride):
    gv, ref, pose, depth = scene
    st = gv.stats()
    print("corner scene: %d chunks in %d slots" % (st.n_chunks, st.n_slots))
    pd, pc = _params(levels=[(stride, 1)])
    for k, start in enumerate([pose] + [I.perturb(pose, *pp) for pp in I.held_perturbations()[:2]]):
        got = gv.align_residuals(depth, start, pc)
        exp = R.rows(ref, depth, start, I.CAM, stride, pd)
        _assert_maps_equal(got, exp, "pose %d stride %d" % (k, stride))
        assert (exp["flags"] == 15).sum() > 0.8 * len(exp["fl"])
        # pixels whose centre or taps leave the alive chunks (flags 1 or 3): into absent and into parked ones
        assert ((exp["flags"] == 1) | (exp["flags"] == 3)).sum() > 0
        assert _samples_in_chunks_that_are_not_alive(ref, exp, start, depth, stride) > 0


def test_residual_maps_edge_cases_on_the_hand_built_corner(hand):
    gv, ref, pose, depth = hand
    pd, pc = _params(**ONE_STEP)
    d = depth.copy()
    good = np.argwhere(R.rows(ref, depth, pose, I.CAM, 1, pd)["flags"] == 15)
    for k, (y, x) in enumerate(good[:: len(good) // 8][:8]):
        d[y, x] = (0.0, np.nan, np.inf, -np.inf, -0.3, 0.04, 5.5, 1e30)[k]
    start = pose.astype(np.float64)
    start[:, 3] += I.HAND_DELTA
    for dd, pp in ((d, pose), (depth, start.astype(np.float32))):
        exp = R.rows(ref, dd, pp, I.CAM, 1, pd)
        _assert_maps_equal(gv.align_residuals(dd, pp, pc), exp, "hand-built")
        assert (exp["flags"] == 15).sum() > 5000 and (exp["flags"] == 0).sum() > 1000
    # a tap in an absent chunk: flags 3, the residual written, no gradient, no part of the sums
    drop = (I.HAND_LAYER[0], I.HAND_LAYER[1] + 2, I.HAND_LAYER[2] + 2)
    g2, r2 = _hand_volume(I.hand_corner(drop=drop))
    try:
        exp = R.rows(r2, depth, pose, I.CAM, 1, pd)
        got = g2.align_residuals(depth, pose, pc)
        _assert_maps_equal(got, exp, "absent chunk")
        assert (got["flags"] == 3).sum() > 10
        g2.align_frame(depth, pose, pc)
        assert g2.align_log()[0]["n_valid"] == int((exp["flags"] == 15).sum())
    finally:
        g2.close()


def test_residual_maps_with_tiles_over_both_borders(hand):
    """a 13 x 9 camera: one full tile column and a partial one, one full tile row and a partial one"""
    gv, ref, pose, _ = hand
    small = synth.Camera(13, 9, 11.0, 11.0, 6.5, 4.5)
    gv.raycast_camera(small)  # (tf_set_camera takes widths that are multiples of 8 only; the readers' camera any)
    try:
        depth = I.hand_depth(pose, small, edge_voxels=0.0)
        for stride in (1, 2):
            pd, pc = _params(levels=[(stride, 1)], huber=0.0, min_valid=1)
            exp = R.rows(ref, depth, pose, small, stride, pd)
            _assert_maps_equal(gv.align_residuals(depth, pose, pc), exp, "13 x 9 stride %d" % stride)
            assert (exp["flags"] == 15).sum() > 10
            gv.align_frame(depth, pose, pc)
            rec = gv.align_log()[0]
            assert rec["n_sampled"] == len(exp["fl"]) and rec["n_valid"] == int((exp["flags"] == 15).sum())
    finally:
        gv.raycast_camera(None)


def _check_sums(rec, sm):
    assert rec["n_valid"] == sm["n_valid"] and rec["n_sampled"] == sm["n_sampled"]
    got = np.concatenate([rec["A21"], rec["b"], [rec["sum_r2"], rec["sum_wr2"]]])
    want = np.concatenate([sm["A21"], sm["b"], [sm["sum_r2"], sm["sum_wr2"]]])
    bound = sm["n_valid"] * 2.0 ** -52 * sm["mag"]  # an f64 sum of exact terms in any order
    print("sums: largest |delta| / bound = %.3g" % np.max(np.abs(got - want) / np.maximum(bound, 1e-300)))
    assert np.all(np.abs(got - want) <= bound), np.abs(got - want) / bound


@pytest.mark.parametrize("huber", [0.0, 0.002])
def test_first_evaluation_sums_against_exact_sums(scene, hand, huber):
    for (gv, ref, pose, depth), stride in ((scene, 1), (scene, 3), (hand, 1)):
        pd, pc = _params(levels=[(stride, 1)], huber=huber)
        start = I.perturb(pose, *I.held_perturbations()[2])
        gv.align_frame(depth, start, pc)
        _check_sums(gv.align_log()[0], R.sums(R.rows(ref, depth, start, I.CAM, stride, pd), pd))


def _check_steps(log, damping):
    for rec in log:
        if not rec["xi"].any():
            continue
        M = rec["A"] + damping * np.diag(rec["A"].diagonal())
        lhs = np.linalg.norm(M @ rec["xi"] + rec["b"])
        rhs = 1e-12 * (np.linalg.norm(M, 2) * np.linalg.norm(rec["xi"]) + np.linalg.norm(rec["b"]))
        assert lhs <= rhs, (lhs, rhs)


def test_known_answer_on_the_hand_built_corner(hand):
    gv, ref, pose, depth = hand
    pd, pc = _params(**ONE_STEP)
    start = pose.astype(np.float64)
    start[:, 3] += I.HAND_DELTA
    res = gv.align_frame(depth, start.astype(np.float32), pc)
    log = gv.align_log()
    dt, dr = R.pose_distance(res["pose"], pose)
    print("known answer on the device: dt %.3g m, dr %.3g rad" % (dt, dr))
    assert res["status"] == capi.TF_ALIGN_MAX_ITERS and res["evaluations"] == 2 and len(log) == 2
    assert dt <= 1e-5 and dr <= 1e-5
    assert res["rms_last"] < 1e-6 < res["rms_first"]
    _check_steps(log, 0.0)
    assert not log[1]["xi"].any() and np.array_equal(log[1]["pose"].astype(np.float32), res["pose"])


def test_corner_scene_reaches_the_restatements_fixed_point(scene, scene_fixed_point):
    gv, ref, pose, depth = scene
    want, want_log = scene_fixed_point
    pd, pc = _params(**I.SCENE_PARAMS)
    for k, start in enumerate([pose] + [I.perturb(pose, *pp) for pp in I.held_perturbations()]):
        res = gv.align_frame(depth, start, pc)
        log = gv.align_log()
        dt, dr = R.pose_distance(log[-1]["pose"], want_log[-1]["pose"])
        print("start %d: %.3g m, %.3g rad from the restatement's fixed point; rms %.3g -> %.3g" % (
            k, dt, dr, res["rms_first"], res["rms_last"]))
        assert res["status"] == capi.TF_ALIGN_MAX_ITERS and res["evaluations"] == 11 == len(log)
        assert dt <= I.FIXED_TOL_T and dr <= I.FIXED_TOL_R
        assert res["n_valid_last"] >= 0.9 * res["n_sampled"] and np.linalg.cond(log[-1]["A"]) < 1e3
        assert R.pose_distance(res["pose"], pose)[0] < float(RES5)
        if k > 0:
            assert res["rms_last"] < res["rms_first"] / 5
        _check_steps(log, 0.0)
    # the last start was the integration pose's third perturbation; the first evaluation of the restatement from the
    # integration pose and the device's agree in their counts
    res = gv.align_frame(depth, pose, pc)
    assert (res["n_valid_first"], res["n_sampled"]) == (want["n_valid_first"], want["n_sampled"])


def test_device_form_equals_the_host_form_and_runs_repeat_bit_for_bit(scene):
    gv, _, pose, depth = scene
    _, pc = _params(damping=1e-4)
    start = I.perturb(pose, *I.held_perturbations()[1])
    host = gv.align_frame(depth, start, pc)
    log = gv.align_log()
    d_depth, d_res = HipBuffer(depth.nbytes).from_host(depth), HipBuffer(C.sizeof(capi.AlignResult))
    try:
        for _ in range(2):
            gv.align_frame_device(d_depth.ptr, start, pc, d_res.ptr)
            gv.sync()
            dev = gv.align_result(d_res.to_host())
            assert bytes(np.asarray(dev.pop("pose"))) == bytes(host["pose"]) and dev == {k: v for k, v in host.items() if k != "pose"}
            log2 = gv.align_log()
            assert len(log2) == len(log) == host["evaluations"]
            for a, b in zip(log, log2):
                for key in a:
                    assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
        _check_steps(log, 1e-4)
        # the residual maps' device form
        P = depth.size
        bufs = [HipBuffer(4 * P), HipBuffer(12 * P), HipBuffer(4 * P)]
        gv.align_residuals_device(d_depth.ptr, start, pc, *[b.ptr for b in bufs])
        gv.sync()
        hostmap = gv.align_residuals(depth, start, pc)
        assert np.array_equal(bufs[0].to_host().view(np.uint32), hostmap["r"].view(np.uint32).reshape(-1))
        assert np.array_equal(bufs[1].to_host().view(np.uint32), hostmap["grad"].view(np.uint32).reshape(-1))
        assert np.array_equal(bufs[2].to_host().view(np.uint32), hostmap["flags"].reshape(-1))
        for b in bufs:
            b.free()
    finally:
        d_depth.free()
        d_res.free()


def test_levels_and_stops(scene, hand):
    gv, _, pose, depth = scene
    start = I.perturb(pose, *I.held_perturbations()[1])
    _, pc = _params(levels=[(4, 2), (2, 2), (1, 2)], eps_t=0.0, eps_r=0.0)
    res = gv.align_frame(depth, start, pc)
    log = gv.align_log()
    assert res["evaluations"] == 7 and res["status"] == capi.TF_ALIGN_MAX_ITERS
    assert [(r["level"], r["stride"]) for r in log] == [(0, 4), (0, 4), (1, 2), (1, 2), (2, 1), (2, 1), (2, 1)]
    assert [r["n_sampled"] for r in log] == [40 * 30] * 2 + [80 * 60] * 2 + [160 * 120] * 3
    # eps above any step: the first step ends the (only) level, then the closing evaluation
    _, pc = _params(levels=[(1, 5)], eps_t=1.0, eps_r=1.0)
    res = gv.align_frame(depth, start, pc)
    assert res["evaluations"] == 2 == len(gv.align_log()) and res["status"] == capi.TF_ALIGN_CONVERGED
    # ... at a level that is not the last one, the next level still runs and the call ends as MAX_ITERS
    _, pc = _params(levels=[(2, 5), (1, 1)], eps_t=1.0, eps_r=0.0)
    _, pc2 = _params(levels=[(2, 5), (1, 1)], eps_t=1.0, eps_r=1.0)
    assert gv.align_frame(depth, start, pc)["evaluations"] == 7
    res = gv.align_frame(depth, start, pc2)
    assert res["evaluations"] == 3 and res["status"] == capi.TF_ALIGN_CONVERGED
    assert [(r["level"], r["stride"]) for r in gv.align_log()] == [(0, 2), (1, 1), (1, 1)]
    # too few
    _, pc = _params(min_valid=160 * 120 + 1)
    res = gv.align_frame(depth, start, pc)
    assert res["status"] == capi.TF_ALIGN_TOO_FEW and res["evaluations"] == 1
    assert np.array_equal(res["pose"].view(np.uint32), start.view(np.uint32))
    empty = capi.Volume(RES5, I.CAM, max_chunks=1 << 10)
    try:
        res = empty.align_frame(depth, start)
        assert res["status"] == capi.TF_ALIGN_TOO_FEW and res["n_valid_first"] == 0 and res["rms_first"] == 0
        assert not empty.align_residuals(depth, start)["flags"].any() & 2
    finally:
        empty.close()
    # a plane alone
    hv, href, hpose, _ = hand
    pv, pref = _hand_volume(I.hand_plane())
    try:
        _, pc = _params(**ONE_STEP)
        res = pv.align_frame(I.hand_depth(hpose, planes=1), hpose, pc)
        assert res["status"] == capi.TF_ALIGN_SINGULAR and res["evaluations"] == 1 and res["n_valid_first"] > 1000
        assert np.array_equal(res["pose"].view(np.uint32), hpose.view(np.uint32))
    finally:
        pv.close()


def test_invalid_parameters_launch_nothing(scene):
    gv, _, pose, depth = scene
    good = gv.align_frame(depth, pose)
    n_log = len(gv.align_log())
    bad = [dict(n_levels=0), dict(n_levels=5), dict(stride=[0, 1, 1, 1]), dict(stride=[4, -2, 1, 1]), dict(iters=[30, 30, 5, 0]),
           dict(iters=[-1, 3, 2, 0]), dict(min_depth=np.nan), dict(max_depth=np.inf), dict(max_residual=np.nan),
           dict(huber=np.inf), dict(damping=np.nan), dict(eps_t=np.nan), dict(eps_r=-np.inf), dict(min_depth=2.0, max_depth=1.0),
           dict(huber=-0.1), dict(damping=-1e-3), dict(eps_t=-1e-6), dict(eps_r=-1e-6)]
    res = capi.AlignResult()
    res.status = 77
    f32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    d, p = np.ascontiguousarray(depth, np.float32), np.ascontiguousarray(pose, np.float32)
    for kw in bad:
        pc = capi.AlignParams(**kw)
        assert gv.L.tf_align_frame(gv.h, f32p(d), f32p(p), C.byref(pc), C.byref(res)) == capi.TF_ERR_INVALID, kw
        if "iters" not in kw:
            assert gv.L.tf_align_residuals(gv.h, f32p(d), f32p(p), C.byref(pc), None, None, None) == capi.TF_ERR_INVALID, kw
    for k in (0, 3, 7, 11):
        q = p.copy()
        q.reshape(-1)[k] = (np.nan, np.inf, -np.inf, np.nan)[k % 4]
        pc = capi.AlignParams()
        assert gv.L.tf_align_frame(gv.h, f32p(d), f32p(q), C.byref(pc), C.byref(res)) == capi.TF_ERR_INVALID
    assert res.status == 77  # nothing was written
    log = gv.align_log()  # ... and nothing ran: the log is still the good call's
    assert len(log) == n_log == good["evaluations"]


def _snapshot(gv):
    ids = sorted_ids(gv.list_chunks())
    s, w, c = gv.get_chunks(ids)
    mids = sorted_ids(gv.list_meshes())
    meshes = gv.get_meshes(mids)
    return (bytes(gv.stats()), sorted_ids(gv.dirty()).tobytes(), ids.tobytes(), s.tobytes(), w.tobytes(), c.tobytes(),
            mids.tobytes(), b"".join(np.ascontiguousarray(m).tobytes() for m in meshes), gv.check_neighbours().tobytes())


def test_read_only_and_integration_stays_bit_exact(gpu_required):
    ov, gv, cam, _ = make_pair(cam=I.CAM, max_chunks=1 << 14)
    frames = I.corner_frames()
    try:
        for k, (depth, rgba, pose) in enumerate(frames[:4]):
            ov.integrate_frame(depth, rgba, pose)
            gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, k)
        gv.update_meshes()
        ov.update_meshes()
        gv.sync()
        before = _snapshot(gv)
        depth, rgba, pose = frames[2]
        res = gv.align_frame(depth, I.perturb(pose, *I.held_perturbations()[1]))
        assert res["n_valid_first"] > 1000
        gv.align_residuals(depth, pose)
        gv.align_log()
        assert _snapshot(gv) == before
        depth, rgba, pose = frames[4]
        ov.integrate_frame(depth, rgba, pose)
        gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, 4)
        gv.sync()
        assert_chunks_equal(ov, gv, ov.list_chunks(), "after an alignment")
    finally:
        gv.close()
        ov.close()


def test_aligned_pose_feeds_the_device_integrator(gpu_required):
    """the depth image stays on the device: aligned there, then integrated from the same buffer with the aligned pose (the
    76-byte result is all that is read back); the volume equals the one the host path builds from the same pose"""
    frames = I.corner_frames()
    a = capi.Volume(RES5, I.CAM, max_chunks=1 << 14)
    b = capi.Volume(RES5, I.CAM, max_chunks=1 << 14)
    depth, rgba, pose = frames[I.HELD]
    d_depth, d_rgba, d_res = HipBuffer(depth.nbytes).from_host(depth), HipBuffer(rgba.nbytes).from_host(rgba), HipBuffer(76)
    try:
        for k, (dd, cc, pp) in enumerate(frames[:5]):
            for v in (a, b):
                v.integrate_frame_host(dd, cc, pp.reshape(12), None, k)
        a.update_meshes()
        b.update_meshes()
        start = I.perturb(pose, *I.held_perturbations()[1])
        a.align_frame_device(d_depth.ptr, start, capi.AlignParams(), d_res.ptr)
        a.sync()
        res = a.align_result(d_res.to_host())
        assert res["status"] in (capi.TF_ALIGN_CONVERGED, capi.TF_ALIGN_MAX_ITERS) and res["rms_last"] < res["rms_first"] / 5
        assert R.pose_distance(res["pose"], pose)[0] < float(RES5)
        a.integrate_frames_device([d_depth.ptr], [d_rgba.ptr], res["pose"].reshape(1, 12))
        a.sync()
        b.integrate_frame_host(depth, rgba, res["pose"].reshape(12), None, 5)
        b.sync()
        ids = sorted_ids(a.list_chunks())
        assert np.array_equal(ids, sorted_ids(b.list_chunks()))
        for x, y in zip(a.get_chunks(ids), b.get_chunks(ids)):
            assert x.tobytes() == y.tobytes()
    finally:
        for h in (d_depth, d_rgba, d_res):
            h.free()
        a.close()
        b.close()


def test_host_mirror_align(gpu_required, tmp_path):
    exe = str(tmp_path / "mirror_align")
    src = os.path.join(ROOT, "tests", "cpp_align", "mirror_align.cpp")
    lib = os.path.join(ROOT, "texturefusion_amd")
    subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", src, "-o", exe, "-L" + lib, "-ltexfusion_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mirror ok" in r.stdout, r.stdout + r.stderr
