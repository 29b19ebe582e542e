"""Tracking and integrating with the pose kept in device memory (tf_devpose.hip), on the MI355X.  Every comparison is bit
for bit: the constants block against the restatement, the device tracker against tf_track_frame, its acceptance test against
tf_relocalise's, the posed integrate against tf_integrate_frames_device, the loop on the stream against the host loop, and
what a gated or refused call leaves behind.  160 x 120 frames throughout.

What a skipped frame does to tf_get_stats: the handle moves on to the next selection set in any case (the host cannot know
the gate), and that set is left as an empty frame's.  So after a skipped frame the figures that describe the volume
(n_chunks, n_slots, n_dirty) are what they were, and those that describe the last frame (n_selected, n_listed, n_coarse,
n_updated, the rows, the id range) are 0 -- tests 5 and 6 hold both."""
import ctypes as C

import numpy as np
import pytest

from tests import align_icp_inputs as II
from tests import align_inputs as I
from tests import pose_consts_ref as PR
from tests import reloc_inputs as QI
from tests.util import RES5, HipBuffer, sorted_ids
from texturefusion_amd import capi, synth

pytestmark = pytest.mark.gpu
INV = capi.TF_ERR_INVALID
TRK = C.sizeof(capi.TrackResult)  # 204
VOLUME_STATS = ("n_chunks", "n_slots", "n_dirty")
FRAME_STATS = ("n_coarse", "n_selected", "n_updated", "rows_tsdf", "rows_color", "n_listed")


def _cell(pose, valid=1):
    c = capi.DevicePose()
    c.pose[:] = [float(x) for x in np.asarray(pose, np.float32).reshape(12)]
    c.valid = valid
    return c


def _cell_buf(pose, valid=1):
    return HipBuffer(64).from_host(np.frombuffer(bytes(_cell(pose, valid)), np.uint8))


def _read_cell(buf):
    return capi.DevicePose.from_buffer_copy(bytes(buf.to_host()))


def _log_raw(gv, fn):
    n = C.c_int64(0)
    buf = (capi.AlignIter * capi.TF_ALIGN_MAX_EVALUATIONS)()
    assert getattr(gv.L, fn)(gv.h, buf, capi.TF_ALIGN_MAX_EVALUATIONS, C.byref(n)) == capi.TF_OK
    return bytes(buf)[:n.value * C.sizeof(capi.AlignIter)]


def _logs(gv):
    return _log_raw(gv, "tf_align_icp_log"), _log_raw(gv, "tf_align_log")


def _track_host(gv, depth, pose, icp, sdf):
    out = capi.TrackResult()
    d = np.ascontiguousarray(depth, np.float32)
    p = np.ascontiguousarray(pose, np.float32).reshape(12)
    f32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert gv.L.tf_track_frame(gv.h, f32p(d), f32p(p), C.byref(icp), C.byref(sdf), C.byref(out)) == capi.TF_OK
    return out


def _accepted(t, acc):
    """tf_devpose.h's track_accepted in np.float32; acc None: stage >= 1"""
    if acc is None:
        return t.stage >= 1
    a = t.sdf if t.stage == 2 else t.icp
    F = np.float32
    return bool(t.stage >= acc.min_stage and a.n_sampled > 0 and
                F(a.n_valid_last) >= F(F(acc.min_valid_fraction) * F(a.n_sampled)) and F(a.rms_last) <= F(acc.max_rms))


def _not_run():
    r = capi.AlignResult()
    r.status = -1
    return r


def _skipped(pose):
    """the tf_track_result of a call whose start cell held no pose"""
    t = capi.TrackResult()
    t.icp, t.sdf, t.stage = _not_run(), _not_run(), 0
    t.pose[:] = [float(x) for x in np.asarray(pose, np.float32).reshape(12)]
    return t


@pytest.fixture(scope="module")
def hand(gpu_required):
    gv = capi.Volume(I.HAND_RES, I.CAM, max_chunks=1 << 10)
    ids, s, w, c = I.hand_corner()
    for k in range(len(ids)):
        gv.set_chunk(ids[k], s[k], w[k], c[k])
    gv.sync()
    true = I.hand_pose()
    depth = I.hand_depth(true)
    d_depth = HipBuffer(depth.nbytes).from_host(depth)
    yield gv, true, depth, d_depth
    d_depth.free()
    gv.close()


SDF = dict(I.SCENE_PARAMS)


# ---- 1. the constants --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", PR.RESOLUTIONS)
def test_constants_equal_the_restatement(gpu_required, res):
    gv = capi.Volume(res, I.CAM, max_chunks=1 << 8)
    try:
        for name, pose in PR.poses().items():
            buf = _cell_buf(pose)
            try:
                pc = gv.pose_consts_download(buf.ptr)
            finally:
                buf.free()
            got = np.concatenate([np.array(getattr(pc, k), np.float32).reshape(-1) for k in PR.FIELDS]).view(np.uint32)
            want = PR.words(PR.consts(pose, res))
            assert np.array_equal(got, want), (name, float(res), np.flatnonzero(got != want))
            assert pc.step == PR.step_of(res) and np.float32(pc.res) == res and pc.plain == 0 and pc.gate == 1
            assert np.array_equal(np.array(pc.P, np.float32).view(np.uint32), np.asarray(pose, np.float32).view(np.uint32))
        # a cell that holds no pose: the gate word says so
        bad = PR.poses()["generic"].copy()
        bad[6] = np.nan
        for cell in (_cell(PR.poses()["generic"], 0), _cell(bad, 1)):
            buf = HipBuffer(64).from_host(np.frombuffer(bytes(cell), np.uint8))
            try:
                assert gv.pose_consts_download(buf.ptr).gate == 0
            finally:
                buf.free()
    finally:
        gv.close()


# ---- 2. the tracker chain ----------------------------------------------------------------------------------------------------
def _track_both(gv, depth, d_depth, start, icp, sdf, acc, aliased=False):
    """tf_track_frame, then tf_track_frame_device, on the same frame -> (host result, its logs, device result bytes, its
    logs, the output cell)"""
    host = _track_host(gv, depth, start, icp, sdf)
    host_logs = _logs(gv)
    d_start, d_out = _cell_buf(start), HipBuffer(256).from_host(np.full(256, 0x5A, np.uint8))
    d_pose = d_start if aliased else HipBuffer(64).from_host(np.full(64, 0x5A, np.uint8))
    try:
        gv.track_frame_device(d_depth.ptr, d_start.ptr, icp, sdf, acc, d_out.ptr, d_pose.ptr)
        gv.sync()
        dev, cell = bytes(d_out.to_host(TRK)), _read_cell(d_pose)
        if not aliased:  # the start cell is read only
            assert bytes(d_start.to_host()) == bytes(_cell(start))
    finally:
        for b in {d_start, d_out, d_pose}:
            b.free()
    return host, host_logs, dev, _logs(gv), cell


@pytest.mark.parametrize("aliased", [False, True])
def test_device_tracker_equals_track_frame(hand, aliased):
    gv, true, depth, d_depth = hand
    start = II.ladder_start(*II.TRACK_START)
    icp, sdf = capi.AlignIcpParams(), capi.AlignParams(**SDF)
    host, hl, dev, dl, cell = _track_both(gv, depth, d_depth, start, icp, sdf, None, aliased)
    assert host.stage == 2 and host.icp.evaluations >= 4 and host.sdf.evaluations >= 4
    assert dev == bytes(host) and dl == hl and len(hl[0]) == host.icp.evaluations * 392 and len(hl[1]) == host.sdf.evaluations * 392
    assert cell.valid == 1 and bytes(cell.pose) == bytes(host.pose) and list(cell.reserved) == [0, 0, 0]


def test_device_tracker_where_a_stage_does_not_hold(hand):
    gv, true, depth, d_depth = hand
    start = II.ladder_start(*II.TRACK_START)
    icp, sdf = capi.AlignIcpParams(), capi.AlignParams(**SDF)
    _track_host(gv, depth, start, icp, sdf)  # an SDF log for the skipped stage to leave alone
    # an all-zero image: the ICP finds too few, the SDF stage is not run, the pose stays
    zeros = np.zeros_like(depth)
    d_zeros = HipBuffer(zeros.nbytes).from_host(zeros)
    try:
        host, hl, dev, dl, cell = _track_both(gv, zeros, d_zeros, start, icp, sdf, None)
    finally:
        d_zeros.free()
    assert host.stage == 0 and host.icp.status == capi.TF_ALIGN_TOO_FEW and host.sdf.status == -1
    assert dev == bytes(host) and dl == hl and len(hl[1]) > 0
    assert cell.valid == 0 and bytes(cell.pose) == np.asarray(start, np.float32).tobytes()
    # an ICP that holds, then an SDF stage whose depth range excludes the scene: stage 1, the ICP's pose
    far = capi.AlignParams(min_depth=0.01, max_depth=0.02, **SDF)
    host, hl, dev, dl, cell = _track_both(gv, depth, d_depth, start, icp, far, None)
    assert host.stage == 1 and host.icp.status <= capi.TF_ALIGN_MAX_ITERS and host.sdf.status == capi.TF_ALIGN_TOO_FEW
    assert dev == bytes(host) and dl == hl
    assert cell.valid == 1 and bytes(cell.pose) == bytes(host.icp.pose)  # accept == NULL: stage >= 1
    # a start cell that holds no pose: valid == 0, and a NaN entry
    nan = np.asarray(start, np.float32).copy()
    nan[1, 2] = np.nan
    before = _logs(gv)
    for pose, valid in ((start, 0), (nan, 1)):
        d_start, d_out, d_pose = _cell_buf(pose, valid), HipBuffer(256), HipBuffer(64)
        try:
            gv.track_frame_device(d_depth.ptr, d_start.ptr, icp, sdf, None, d_out.ptr, d_pose.ptr)
            gv.sync()
            assert bytes(d_out.to_host(TRK)) == bytes(_skipped(pose))
            cell = _read_cell(d_pose)
            assert cell.valid == 0 and bytes(cell.pose) == np.asarray(pose, np.float32).tobytes()
        finally:
            for b in (d_start, d_out, d_pose):
                b.free()
        icp_log, sdf_log = _logs(gv)
        assert icp_log == b"" and sdf_log == before[1]  # no records of this call; the SDF log is the last run's


# ---- 3. acceptance -----------------------------------------------------------------------------------------------------------
def _largest_fraction(nv, ns):
    """the largest f32 q with f32(q * f32(ns)) <= f32(nv): the acceptance expression's own edge"""
    F = np.float32
    ok = lambda q: F(F(q) * F(ns)) <= F(nv)
    q = F(F(nv) / F(ns))
    while not ok(q):
        q = np.nextafter(q, F(-1))
    while ok(np.nextafter(q, F(2))):
        q = np.nextafter(q, F(2))
    return q


def test_acceptance_flips_at_the_readings_and_agrees_with_relocalise():
    gv = capi.Volume(I.HAND_RES, I.CAM, max_chunks=1 << 10)
    ids, s, w, c = I.hand_corner()
    for k in range(len(ids)):
        gv.set_chunk(ids[k], s[k], w[k], c[k])
    true = I.hand_pose()
    depth = I.hand_depth(true)
    rgb = np.full(depth.shape + (3,), 128, np.uint8)
    d_depth = HipBuffer(depth.nbytes).from_host(depth)
    icp, sdf = capi.AlignIcpParams(), capi.AlignParams(**SDF)
    F = np.float32
    try:
        # one indexed keyframe at the start pose; the pose tf_relocalise starts from is the rigid inverse of the stored matrix
        gv.keyframe_cache(7, rgb, depth, QI.pose_inv16(II.ladder_start(*II.TRACK_START)))
        gv.reloc_configure()
        gv.reloc_index_add([7])

        def reloc(**kw):
            p = capi.RelocaliseParams(icp=icp, sdf=sdf, max_tries=1, **kw)
            res = capi.RelocaliseResult()
            f32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
            assert gv.L.tf_relocalise(gv.h, f32p(depth), rgb.ctypes.data_as(C.POINTER(C.c_uint8)), 3, C.byref(p), C.byref(res)) == capi.TF_OK
            assert res.n_tried == 1
            return res

        first = reloc(max_rms=0.0)  # nothing passes: NOT_FOUND reports the keyframe's pose, the try's start
        assert first.status == capi.TF_RELOC_NOT_FOUND
        start = np.array(first.pose, np.float32)
        t = first.tries[0].track
        assert t.stage == 2
        nv, ns, rms = t.sdf.n_valid_last, t.sdf.n_sampled, F(t.sdf.rms_last)
        q = _largest_fraction(nv, ns)
        print("readings: n_valid_last %d of %d (largest passing fraction %.9g), rms_last %.9g" % (nv, ns, q, rms))
        assert 0 < q < 1 and rms > 0
        cases = [(dict(min_stage=2, min_valid_fraction=q, max_rms=rms), True),
                 (dict(min_stage=2, min_valid_fraction=np.nextafter(q, F(2)), max_rms=rms), False),
                 (dict(min_stage=2, min_valid_fraction=q, max_rms=np.nextafter(rms, F(-1))), False),
                 (dict(min_stage=1, min_valid_fraction=np.nextafter(q, F(-1)), max_rms=np.nextafter(rms, F(2))), True)]
        for kw, want in cases:
            r = reloc(**kw)
            assert bytes(r.tries[0].track) == bytes(t)
            assert (r.status == capi.TF_RELOC_FOUND) == want, kw
            d_start, d_out, d_pose = _cell_buf(start), HipBuffer(256), HipBuffer(64)
            try:
                gv.track_frame_device(d_depth.ptr, d_start.ptr, icp, sdf, capi.TrackAccept(**kw), d_out.ptr, d_pose.ptr)
                gv.sync()
                assert bytes(d_out.to_host(TRK)) == bytes(t)
                cell = _read_cell(d_pose)
            finally:
                for b in (d_start, d_out, d_pose):
                    b.free()
            assert cell.valid == int(want), kw
            assert bytes(cell.pose) == (bytes(t.pose) if want else start.tobytes())
            assert _accepted(t, capi.TrackAccept(**kw)) == want
    finally:
        d_depth.free()
        gv.close()


# ---- 4 / 5. the posed integrate ------------------------------------------------------------------------------------------------
def _state(gv):
    ids = sorted_ids(gv.list_chunks())
    s, w, c = gv.get_chunks(ids)
    return dict(ids=ids.tobytes(), sdf=s.tobytes(), weight=w.tobytes(), color=c.tobytes(), dirty=sorted_ids(gv.dirty()).tobytes(),
                stats=bytes(gv.stats()))


def _same_state(a, b, what=""):
    for k in a:
        assert a[k] == b[k], (what, k)


def _upload(frames, color):
    return [(HipBuffer(d.nbytes).from_host(d), HipBuffer(c.nbytes).from_host(c) if color else None) for d, c, _ in frames]


@pytest.mark.parametrize("res", PR.RESOLUTIONS)
@pytest.mark.parametrize("color", [False, True])
def test_posed_integrate_equals_the_host_pose_integrate(gpu_required, res, color):
    frames = I.corner_frames()[:4]
    a = capi.Volume(res, I.CAM, max_chunks=1 << 14)
    b = capi.Volume(res, I.CAM, max_chunks=1 << 14)
    bufs = _upload(frames, color)
    cells = [_cell_buf(p) for _, _, p in frames]
    try:
        for k, (_, _, pose) in enumerate(frames):
            d, c = bufs[k]
            a.integrate_frames_device([d.ptr], [c.ptr] if color else None, [np.asarray(pose, np.float32).reshape(12)])
            b.integrate_frame_posed_device(d.ptr, c.ptr if color else 0, cells[k].ptr)
            if k == 1:  # states compared between frames too (the others go out back to back, no wait in between)
                _same_state(_state(a), _state(b), "after frame 1")
        sa, sb = _state(a), _state(b)
        _same_state(sa, sb)
        st = a.stats()
        assert st.n_chunks > 20 and st.n_dirty > 20 and st.n_selected > 0
        assert a.update_meshes() == b.update_meshes() > 0
        ids = sorted_ids(a.list_meshes())
        assert len(ids) > 20 and np.array_equal(ids, sorted_ids(b.list_meshes()))
        for x, y in zip(a.mesh_counts(ids), b.mesh_counts(ids)):
            assert np.array_equal(x, y)
        assert a.mesh_counts(ids)[0].sum() > 0
    finally:
        for d, c in bufs:
            d.free()
            if c:
                c.free()
        for x in cells:
            x.free()
        a.close()
        b.close()


def test_posed_integrate_discards_selections_made_ahead(gpu_required):
    """a stream that selected two frames ahead, then goes on from a device pose elsewhere"""
    frames = I.corner_frames()[:4]
    a = capi.Volume(RES5, I.CAM, max_chunks=1 << 14)
    b = capi.Volume(RES5, I.CAM, max_chunks=1 << 14)
    bufs = _upload(frames, False)
    poses = [np.asarray(p, np.float32).reshape(12) for _, _, p in frames]
    cell = _cell_buf(poses[3])
    try:
        for v in (a, b):
            v.stream_frames_device([d.ptr for d, _ in bufs[:3]], None, poses[:3], n_ahead=2)
        a.integrate_frames_device([bufs[3][0].ptr], None, [poses[3]])
        b.integrate_frame_posed_device(bufs[3][0].ptr, 0, cell.ptr)
        _same_state(_state(a), _state(b))
    finally:
        for d, _ in bufs:
            d.free()
        cell.free()
        a.close()
        b.close()


@pytest.mark.parametrize("color", [False, True])
def test_posed_integrate_with_the_gate_off_leaves_the_volume_alone(gpu_required, color):
    frames = I.corner_frames()[:3]
    gv = capi.Volume(RES5, I.CAM, max_chunks=1 << 14)
    bufs = _upload(frames, color)
    try:
        for k in range(2):
            gv.integrate_frames_device([bufs[k][0].ptr], [bufs[k][1].ptr] if color else None,
                                       [np.asarray(frames[k][2], np.float32).reshape(12)])
        before = _state(gv)
        st0 = gv.stats()
        nan = np.asarray(frames[2][2], np.float32).copy()
        nan[2, 3] = np.inf
        for pose, valid in ((frames[2][2], 0), (nan, 1)):
            cell = _cell_buf(pose, valid)
            try:
                gv.integrate_frame_posed_device(bufs[2][0].ptr, bufs[2][1].ptr if color else 0, cell.ptr)
                after = _state(gv)
            finally:
                cell.free()
            for k in ("ids", "sdf", "weight", "color", "dirty"):
                assert after[k] == before[k], k
            st = gv.stats()
            assert all(getattr(st, k) == getattr(st0, k) for k in VOLUME_STATS)
            assert all(getattr(st, k) == 0 for k in FRAME_STATS) and list(st.min_id) + list(st.max_id) == [0] * 6
        # the handle goes on as if nothing had happened: the third frame for real equals a volume that never saw the gate
        ref = capi.Volume(RES5, I.CAM, max_chunks=1 << 14)
        try:
            for k in range(3):
                ref.integrate_frames_device([bufs[k][0].ptr], [bufs[k][1].ptr] if color else None,
                                            [np.asarray(frames[k][2], np.float32).reshape(12)])
            cell = _cell_buf(frames[2][2])
            try:
                gv.integrate_frame_posed_device(bufs[2][0].ptr, bufs[2][1].ptr if color else 0, cell.ptr)
                _same_state(_state(gv), _state(ref), "after the gate")
            finally:
                cell.free()
        finally:
            ref.close()
    finally:
        for d, c in bufs:
            d.free()
            if c:
                c.free()
        gv.close()


# ---- 6. the loop -------------------------------------------------------------------------------------------------------------
def _loop_frames(n=8):
    """corner_frames' scene along a gentle path: 0.8 degrees of yaw, 0.5 of pitch and a centimetre per frame"""
    out = []
    for k in range(n):
        pose = I.corner_pose(45.0 + 0.8 * k, -28.0 - 0.5 * k, 0.3 * k, (0.01 * k, -0.005 * k, 0.004 * k))
        depth, rgba = I.render_box(pose, I.CAM, seed=100 + k)
        out.append((depth, rgba, np.asarray(pose, np.float32)))
    return out


ACCEPT = dict(min_stage=2, min_valid_fraction=0.3, max_rms=0.02)


@pytest.mark.parametrize("zero_at", [None, 4])
def test_the_loop_on_the_stream_equals_the_host_loop(gpu_required, zero_at):
    frames = _loop_frames()
    if zero_at is not None:
        frames[zero_at] = (np.zeros_like(frames[zero_at][0]),) + frames[zero_at][1:]
    icp, sdf, acc = capi.AlignIcpParams(), capi.AlignParams(**SDF), capi.TrackAccept(**ACCEPT)
    a = capi.Volume(RES5, I.CAM, max_chunks=1 << 14)  # the host loop
    b = capi.Volume(RES5, I.CAM, max_chunks=1 << 14)  # the loop on the stream
    bufs = _upload(frames, True)
    d_out = HipBuffer(256 * len(frames))
    first = frames[0][2].reshape(12)
    cell = _cell_buf(first)
    try:
        for v in (a, b):
            v.integrate_frames_device([bufs[0][0].ptr], [bufs[0][1].ptr], [first])
        # the device loop: one cell fed back, nothing waited for
        for k in range(1, len(frames)):
            b.track_integrate_device(bufs[k][0].ptr, bufs[k][1].ptr, cell.ptr, icp, sdf, acc, d_out.ptr + 256 * k, cell.ptr)
        b.sync()
        got = [bytes(d_out.to_host()[256 * k:256 * k + TRK]) for k in range(len(frames))]
        # the host loop: tf_track_frame, the same test, tf_integrate_frames_device where it passes; once a frame fails the
        # cell holds no pose and every later frame is skipped
        pose, alive, n_ok = first.copy(), True, 0
        for k in range(1, len(frames)):
            if not alive:
                assert got[k] == bytes(_skipped(pose)), k
                continue
            t = _track_host(a, frames[k][0], pose, icp, sdf)
            assert got[k] == bytes(t), k
            if _accepted(t, acc):
                pose = np.array(t.pose, np.float32)
                a.integrate_frames_device([bufs[k][0].ptr], [bufs[k][1].ptr], [pose])
                n_ok += 1
            else:
                alive = False
        end = _read_cell(cell)
        assert end.valid == int(alive) and bytes(end.pose) == pose.tobytes()
        print("loop: %d of %d frames accepted" % (n_ok, len(frames) - 1))
        assert n_ok == (len(frames) - 1 if zero_at is None else zero_at - 1)
        sa, sb = _state(a), _state(b)
        for k in ("ids", "sdf", "weight", "color", "dirty"):
            assert sa[k] == sb[k], k
        if zero_at is None:
            assert sa["stats"] == sb["stats"]
        else:  # the skipped frames selected nothing
            for k in VOLUME_STATS:
                assert getattr(a.stats(), k) == getattr(b.stats(), k), k
            assert all(getattr(b.stats(), k) == 0 for k in FRAME_STATS)
        assert a.update_meshes() == b.update_meshes() > 0
    finally:
        for d, c in bufs:
            d.free()
            c.free()
        d_out.free()
        cell.free()
        a.close()
        b.close()


# ---- 7. invalid arguments ------------------------------------------------------------------------------------------------------
def test_invalid_arguments_launch_nothing(hand):
    gv, true, depth, d_depth = hand
    L = gv.L
    start = II.ladder_start(0.040, 2.0)
    rgba = np.full(depth.shape + (4,), 200, np.uint8)
    pert = I.perturb(true, I.HAND_DELTA, np.zeros(3))
    gv.align_frame(depth, pert)
    gv.align_frame_color(depth, rgba, pert)
    gv.align_group([depth], [pert])
    gv.align_frame_icp(depth, start)

    def logs():
        n = C.c_int64(0)
        out = [_log_raw(gv, "tf_align_icp_log"), _log_raw(gv, "tf_align_log")]
        buf = (capi.AlignColorIter * capi.TF_ALIGN_MAX_EVALUATIONS)()
        assert L.tf_align_color_log(gv.h, buf, capi.TF_ALIGN_MAX_EVALUATIONS, C.byref(n)) == capi.TF_OK
        out.append(bytes(buf)[:n.value * C.sizeof(capi.AlignColorIter)])
        buf = (capi.AlignIter * capi.TF_ALIGN_MAX_EVALUATIONS)()
        assert L.tf_align_group_log(gv.h, 0, buf, capi.TF_ALIGN_MAX_EVALUATIONS, C.byref(n)) == capi.TF_OK
        out.append(bytes(buf)[:n.value * C.sizeof(capi.AlignIter)])
        assert all(len(x) > 0 for x in out)
        return out

    good = logs()
    before = _state(gv)
    pattern = np.full(256, 0x5A, np.uint8)
    d_start, d_out, d_pose = _cell_buf(start), HipBuffer(256).from_host(pattern), HipBuffer(80).from_host(pattern[:80])
    cell0 = bytes(d_start.to_host())
    icp, sdf, acc = capi.AlignIcpParams(), capi.AlignParams(), capi.TrackAccept()

    def track(depth_p=d_depth.ptr, start_p=d_start.ptr, icp_p=icp, sdf_p=sdf, acc_p=acc, out_p=d_out.ptr, pose_p=d_pose.ptr):
        ref = lambda x: None if x is None else C.byref(x)
        assert L.tf_track_frame_device(gv.h, depth_p, start_p, ref(icp_p), ref(sdf_p), ref(acc_p), out_p, pose_p) == INV
        assert L.tf_track_integrate_device(gv.h, depth_p, None, start_p, ref(icp_p), ref(sdf_p), ref(acc_p), out_p, pose_p) == INV

    try:
        # what tf_track_frame rejects from its parameters
        for kw in (dict(n_levels=0), dict(n_levels=5), dict(stride=[0, 1, 1, 1]), dict(min_depth=np.nan), dict(min_depth=2.0, max_depth=1.0),
                   dict(huber=-0.1), dict(damping=-1e-3), dict(eps_r=np.inf), dict(iters=[30, 30, 5, 0]), dict(max_distance=-0.01),
                   dict(max_distance=np.nan), dict(ray_near=-0.1), dict(ray_far=np.inf), dict(ray_max_steps=0)):
            track(icp_p=capi.AlignIcpParams(**kw))
        for kw in (dict(n_levels=0), dict(huber=-1.0), dict(iters=[60, 30, 0, 0])):
            track(sdf_p=capi.AlignParams(**kw))
        for kw in (dict(min_stage=0), dict(min_stage=3), dict(min_valid_fraction=-0.1), dict(min_valid_fraction=1.5),
                   dict(min_valid_fraction=np.nan), dict(max_rms=-1.0), dict(max_rms=np.inf), dict(max_rms=np.nan)):
            track(acc_p=capi.TrackAccept(**kw))
        # null pointers, cells that are not 16-byte aligned
        for kw in (dict(depth_p=None), dict(start_p=None), dict(icp_p=None), dict(sdf_p=None), dict(out_p=None), dict(pose_p=None),
                   dict(start_p=d_pose.ptr + 8), dict(pose_p=d_pose.ptr + 8)):
            track(**kw)
        assert L.tf_track_frame_device(None, d_depth.ptr, d_start.ptr, C.byref(icp), C.byref(sdf), None, d_out.ptr, d_pose.ptr) == INV
        assert L.tf_integrate_frame_posed_device(gv.h, None, None, d_start.ptr) == INV
        assert L.tf_integrate_frame_posed_device(gv.h, d_depth.ptr, None, None) == INV
        assert L.tf_integrate_frame_posed_device(gv.h, d_depth.ptr + 4, None, d_start.ptr) == INV
        assert L.tf_integrate_frame_posed_device(gv.h, d_depth.ptr, d_depth.ptr + 2, d_start.ptr) == INV
        assert L.tf_integrate_frame_posed_device(gv.h, d_depth.ptr, None, d_start.ptr + 8) == INV
        host = capi.PoseConsts()
        assert L.tf_pose_consts_download(gv.h, None, C.byref(host), C.sizeof(host)) == INV
        assert L.tf_pose_consts_download(gv.h, d_start.ptr, None, C.sizeof(host)) == INV
        assert L.tf_pose_consts_download(gv.h, d_start.ptr, C.byref(host), C.sizeof(host) + 1) == INV
        assert L.tf_track_accept_default(None) == INV
        # tf_relocalise's rule: a raycast camera of another size
        gv.raycast_camera(synth.Camera(80, 60, 65.0, 65.0, 39.5, 29.5))
        try:
            track()
        finally:
            gv.raycast_camera(None)
        # a handle with a partition
        gv.set_partition(0, 64)
        try:
            track()
            assert L.tf_integrate_frame_posed_device(gv.h, d_depth.ptr, None, d_start.ptr) == INV
        finally:
            gv.set_partition(-(2 ** 31), 2 ** 31 - 1)
        # nothing was written and nothing ran
        assert bytes(d_out.to_host()) == pattern.tobytes() and bytes(d_pose.to_host()) == pattern[:80].tobytes()
        assert bytes(d_start.to_host()) == cell0
        assert logs() == good
        _same_state(_state(gv), before)
        # ... and with the partition gone the same arguments are taken
        gv.track_frame_device(d_depth.ptr, d_start.ptr, icp, sdf, acc, d_out.ptr, d_pose.ptr)
        gv.sync()
        assert capi.TrackResult.from_buffer_copy(bytes(d_out.to_host(TRK))).stage == 2
    finally:
        for b in (d_start, d_out, d_pose):
            b.free()
