"""Texturing a frame whose pose is kept in device memory (tf_integrate_frame_textured_posed_device, tf_track_texture_device,
tf_pose_inverse_download), on the MI355X.  Every comparison is bit for bit: the inverse block against the restatement
(tests/pose_inverse_ref.py), the posed textured unit against tf_stream_frames_textured_device with the restated inverse --
volume, dirty set, meshes, patches, atlas texels, the atlas's next location -- the loop on the stream against the host loop,
and what a gated or refused call leaves behind.  160 x 120 frames throughout.  The only thresholds are test 2's floors,
which keep it from passing on empty state: more than 20 meshes, more than 20 patches with an atlas slot, non-zero texels.

What a skipped frame does to the figures: the host cannot know the gate, so the handle moves on as after any frame.
tf_get_stats' last-frame figures are 0 (tests/test_gpu_devpose.py), and so are tf_get_texture_stats' -- all of them describe
the last frame's dirty set -- except n_slots, the atlas slots handed out so far, which stays."""
import ctypes as C

import numpy as np
import pytest

from tests import align_inputs as I
from tests import pose_consts_ref as PR
from tests import pose_inverse_ref as IR
from tests.test_gpu_devpose import (ACCEPT, FRAME_STATS, SDF, TRK, VOLUME_STATS, _accepted, _cell, _cell_buf, _loop_frames,
                                    _read_cell, _skipped, _state, _track_host, _upload)
from tests.util import RES5, HipBuffer, sorted_ids
from texturefusion_amd import capi

pytestmark = pytest.mark.gpu
INV = capi.TF_ERR_INVALID
AW = 13824  # tf_config's default atlas
NO_TEXLOC = np.uint64((1 << 64) - 1)
TEX_FRAME_STATS = ("n_dirty", "n_meshes", "n_vertices", "n_triangles", "roi_pixels", "n_patches", "n_exact", "n_survivors",
                   "n_surface")


def _vol(res=RES5):
    return capi.Volume(res, I.CAM, max_chunks=1 << 14)


def _p12(pose):
    return np.ascontiguousarray(pose, np.float32).reshape(12)


def _host_textured(gv, buf, pose, frame_id):
    """the host-pose call the posed one is defined by: one frame, nothing ahead, the restated inverse"""
    p = _p12(pose)
    gv.stream_frames_textured_device([buf[0].ptr], [buf[1].ptr], [p], [IR.inverse16(p)], frame_id)


def _full(gv):
    """everything a textured frame leaves behind, as bytes"""
    s = _state(gv)
    mids = sorted_ids(gv.list_meshes())
    s["mesh_ids"] = mids.tobytes()
    s["meshes"] = b"".join(np.ascontiguousarray(x).tobytes() for x in gv.get_meshes(mids))
    g = gv.get_patches(mids)
    s["patches"] = b"".join(np.ascontiguousarray(g[k]).tobytes() for k in sorted(g))
    s["texture_stats"] = bytes(gv.texture_stats())
    s["atlas_loc_next"] = gv.atlas_loc_next()
    rows = min(AW, int(gv.atlas_loc_next() // AW) + gv.atlas_patch_size()[1])  # every row handed out
    s["atlas"] = gv.atlas_rows(0, rows, AW).tobytes()
    return s, (mids, g, rows)


def _same(a, b, what="", skip=()):
    for k in a:
        if k not in skip:
            assert a[k] == b[k], (what, k)


def _free(*bufs):
    for b in bufs:
        if isinstance(b, tuple):
            _free(*b)
        elif b is not None:
            b.free()


# ---- 1. the inverse block -----------------------------------------------------------------------------------------------------
def test_inverse_block_equals_the_restatement(gpu_required):
    gv = capi.Volume(RES5, I.CAM, max_chunks=1 << 8)
    try:
        for name, pose in PR.poses().items():
            buf = _cell_buf(pose)
            try:
                blk = gv.pose_inverse_download(buf.ptr)
                pc = gv.pose_consts_download(buf.ptr)  # the launch is shared: its first block is what it was
            finally:
                buf.free()
            got, want = np.array(blk.T, np.float32).view(np.uint32), IR.inverse16(pose).view(np.uint32)
            assert np.array_equal(got, want), (name, np.flatnonzero(got != want))
            assert blk.gate == 1 and list(blk.pad) == [0, 0, 0] and pc.gate == 1
            assert np.array_equal(np.array(pc.P, np.float32).view(np.uint32), np.asarray(pose, np.float32).view(np.uint32))
        bad = PR.poses()["generic"].copy()
        bad[6] = np.inf
        for cell in (_cell(PR.poses()["generic"], 0), _cell(bad, 1)):
            buf = HipBuffer(64).from_host(np.frombuffer(bytes(cell), np.uint8))
            try:
                assert gv.pose_inverse_download(buf.ptr).gate == 0
            finally:
                buf.free()
        # a prefix is copied, the rest of the caller's buffer is left alone
        buf = _cell_buf(PR.poses()["generic"])
        try:
            part = (C.c_uint8 * 80)(*([0x5A] * 80))
            assert gv.L.tf_pose_inverse_download(gv.h, buf.ptr, part, 16) == capi.TF_OK
            assert bytes(part)[:16] == IR.inverse16(PR.poses()["generic"]).tobytes()[:16] and bytes(part)[16:] == b"\x5a" * 64
            host = capi.PoseInverse()
            L = gv.L
            assert L.tf_pose_inverse_download(None, buf.ptr, C.byref(host), 80) == INV
            assert L.tf_pose_inverse_download(gv.h, None, C.byref(host), 80) == INV
            assert L.tf_pose_inverse_download(gv.h, buf.ptr, None, 80) == INV
            assert L.tf_pose_inverse_download(gv.h, buf.ptr, C.byref(host), 81) == INV
            assert L.tf_pose_inverse_download(gv.h, buf.ptr + 8, C.byref(host), 80) == INV
            assert bytes(host) == bytes(80)
        finally:
            buf.free()
    finally:
        gv.close()


# ---- 2. posed against host-pose -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", PR.RESOLUTIONS)
def test_posed_textured_equals_the_host_pose_textured(gpu_required, res):
    frames = I.corner_frames()[:4]
    a, b = _vol(res), _vol(res)
    bufs = _upload(frames, True)
    cells = [_cell_buf(p) for _, _, p in frames]
    try:
        for k, (_, _, pose) in enumerate(frames):
            _host_textured(a, bufs[k], pose, k)
            b.integrate_frame_textured_posed_device(bufs[k][0].ptr, bufs[k][1].ptr, cells[k].ptr, k)
            if k == 1:  # between frames too (the others go out back to back, no wait in between)
                _same(_full(a)[0], _full(b)[0], "after frame 1")
        (sa, (mids, g, rows)), (sb, _) = _full(a), _full(b)
        n_slot = int((g["texloc"] != NO_TEXLOC).sum())
        n_texel = int(np.count_nonzero(np.frombuffer(sa["atlas"], np.uint8)))
        print("res %g: %d meshes, %d patches with a slot, %d atlas rows, %d non-zero texel bytes, last frame ids %s"
              % (float(res), len(mids), n_slot, rows, n_texel, sorted(set(g["frameid"].tolist()))))
        assert len(mids) > 20 and n_slot > 20 and n_texel > 0  # volume a alone: the comparison is not of empty state
        assert set(g["frameid"].tolist()) <= {0, 1, 2, 3} and 3 in g["frameid"]
        _same(sa, sb)
    finally:
        _free(*bufs, *cells)
        a.close()
        b.close()


# ---- 3. mixed callers ---------------------------------------------------------------------------------------------------------
def test_posed_textured_after_a_stream_that_selected_ahead(gpu_required):
    """a textured stream that selected two frames ahead and left its patch stage pending, then a frame from a device pose
    elsewhere, then a host-pose frame again"""
    frames = I.corner_frames()[:4]
    a, b = _vol(), _vol()
    bufs = _upload(frames, True)
    poses = [_p12(p) for _, _, p in frames]
    inv = [IR.inverse16(p) for p in poses]
    cell = _cell_buf(poses[3])
    try:
        for v in (a, b):
            v.stream_frames_textured_device([d.ptr for d, _ in bufs[:3]], [c.ptr for _, c in bufs[:3]], poses[:3], inv[:3], 0,
                                            n_ahead=2)
        _host_textured(a, bufs[3], poses[3], 3)
        b.integrate_frame_textured_posed_device(bufs[3][0].ptr, bufs[3][1].ptr, cell.ptr, 3)
        for v in (a, b):
            _host_textured(v, bufs[2], poses[2], 2)
        (sa, (mids, g, _)), (sb, _) = _full(a), _full(b)
        assert len(mids) > 20 and {0, 2, 3} >= set(g["frameid"].tolist()) and 3 in g["frameid"]
        _same(sa, sb)
    finally:
        _free(*bufs, cell)
        a.close()
        b.close()


# ---- 4. gate off --------------------------------------------------------------------------------------------------------------
def _assert_skipped_frame(gv, before, st0, ts0, what):
    after, _ = _full(gv)
    _same(before, after, what, skip=("stats", "texture_stats"))
    st, ts = gv.stats(), gv.texture_stats()
    assert all(getattr(st, k) == getattr(st0, k) for k in VOLUME_STATS), what
    assert all(getattr(st, k) == 0 for k in FRAME_STATS) and list(st.min_id) + list(st.max_id) == [0] * 6, what
    assert ts.n_slots == ts0.n_slots and all(getattr(ts, k) == 0 for k in TEX_FRAME_STATS), what


def test_posed_textured_with_the_gate_off_leaves_everything_alone(gpu_required):
    frames = I.corner_frames()[:3]
    gv, ref = _vol(), _vol()
    bufs = _upload(frames, True)
    try:
        for k in range(2):
            _host_textured(gv, bufs[k], frames[k][2], k)
        before, (mids, _, _) = _full(gv)
        st0, ts0 = gv.stats(), gv.texture_stats()
        assert len(mids) > 20 and ts0.n_slots > 20 and ts0.n_patches > 0
        inf = np.asarray(frames[2][2], np.float32).copy()
        inf[2, 3] = np.inf
        for pose, valid in ((frames[2][2], 0), (inf, 1)):
            cell = _cell_buf(pose, valid)
            try:
                gv.integrate_frame_textured_posed_device(bufs[2][0].ptr, bufs[2][1].ptr, cell.ptr, 2)
                _assert_skipped_frame(gv, before, st0, ts0, "valid %d" % valid)
            finally:
                cell.free()
        # the handle goes on as if nothing had happened: the third frame for real equals a volume that never saw the gate
        for k in range(3):
            _host_textured(ref, bufs[k], frames[k][2], k)
        cell = _cell_buf(frames[2][2])
        try:
            gv.integrate_frame_textured_posed_device(bufs[2][0].ptr, bufs[2][1].ptr, cell.ptr, 2)
            _same(_full(gv)[0], _full(ref)[0], "after the gate")
        finally:
            cell.free()
    finally:
        _free(*bufs)
        gv.close()
        ref.close()


# ---- 5. the loop --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_at", [None, 4])
def test_the_textured_loop_on_the_stream_equals_the_host_loop(gpu_required, zero_at):
    frames = _loop_frames()
    if zero_at is not None:
        frames[zero_at] = (np.zeros_like(frames[zero_at][0]),) + frames[zero_at][1:]
    icp, sdf, acc = capi.AlignIcpParams(), capi.AlignParams(**SDF), capi.TrackAccept(**ACCEPT)
    a, b = _vol(), _vol()  # the host loop, the loop on the stream
    bufs = _upload(frames, True)
    d_out = HipBuffer(256 * len(frames))
    first = frames[0][2].reshape(12)
    cell = _cell_buf(first)
    try:
        for v in (a, b):
            _host_textured(v, bufs[0], first, 0)
        for k in range(1, len(frames)):  # one cell fed back, nothing waited for
            b.track_texture_device(bufs[k][0].ptr, bufs[k][1].ptr, cell.ptr, icp, sdf, acc, d_out.ptr + 256 * k, cell.ptr, k)
        b.sync()
        got = [bytes(d_out.to_host()[256 * k:256 * k + TRK]) for k in range(len(frames))]
        pose, alive, n_ok, at3 = first.copy(), True, 0, None
        for k in range(1, len(frames)):
            if not alive:
                assert got[k] == bytes(_skipped(pose)), k
                continue
            t = _track_host(a, frames[k][0], pose, icp, sdf)
            assert got[k] == bytes(t), k
            if _accepted(t, acc):
                pose = np.array(t.pose, np.float32)
                _host_textured(a, bufs[k], pose, k)
                n_ok += 1
            else:
                alive = False
        end = _read_cell(cell)
        assert end.valid == int(alive) and bytes(end.pose) == pose.tobytes()
        print("textured loop: %d of %d frames accepted" % (n_ok, len(frames) - 1))
        assert n_ok == (len(frames) - 1 if zero_at is None else zero_at - 1)
        (sa, (mids, g, _)), (sb, _) = _full(a), _full(b)
        assert len(mids) > 20 and int(g["frameid"].max()) == n_ok  # the last accepted frame's patches are there
        if zero_at is None:
            _same(sa, sb)
        else:
            # a did nothing after frame 3, b skipped four frames: untextured, the atlas as frame 3 left it
            _same(sa, sb, skip=("stats", "texture_stats"))
            _assert_skipped_frame(b, sa, a.stats(), a.texture_stats(), "skipped frames")
    finally:
        _free(*bufs, d_out, cell)
        a.close()
        b.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
def test_refused_calls_launch_nothing(gpu_required):
    frames = I.corner_frames()[:4]
    gv = _vol()
    L = gv.L
    bufs = _upload(frames, True)
    pattern = np.full(256, 0x5A, np.uint8)
    d_out, d_pose = HipBuffer(256).from_host(pattern), HipBuffer(80).from_host(pattern[:80])
    cell = _cell_buf(frames[2][2])
    cell0 = bytes(cell.to_host())
    icp, sdf, acc = capi.AlignIcpParams(), capi.AlignParams(**SDF), capi.TrackAccept(**ACCEPT)
    dd, dc = bufs[2][0].ptr, bufs[2][1].ptr
    ref = lambda x: None if x is None else C.byref(x)

    def integrate(depth_p=dd, rgba_p=dc, cell_p=cell.ptr):
        assert L.tf_integrate_frame_textured_posed_device(gv.h, depth_p, rgba_p, cell_p, 2) == INV
        return L.tf_last_error().decode()

    def track(depth_p=dd, rgba_p=dc, start_p=cell.ptr, acc_p=acc, out_p=d_out.ptr, pose_p=d_pose.ptr, icp_p=icp):
        assert L.tf_track_texture_device(gv.h, depth_p, rgba_p, start_p, ref(icp_p), ref(sdf), ref(acc_p), out_p, pose_p, 2) == INV
        return L.tf_last_error().decode()

    def untouched(state):
        assert bytes(d_out.to_host()) == pattern.tobytes() and bytes(d_pose.to_host()) == pattern[:80].tobytes()
        assert bytes(cell.to_host()) == cell0
        _same(_full(gv)[0], state)

    try:
        for k in range(2):
            _host_textured(gv, bufs[k], frames[k][2], k)
        before = _full(gv)[0]
        # a null colour image
        assert "colour image" in integrate(rgba_p=None) and "colour image" in track(rgba_p=None)
        # null and misaligned cells and images
        for kw in (dict(cell_p=None), dict(cell_p=d_pose.ptr + 8), dict(depth_p=None), dict(depth_p=dd + 4), dict(rgba_p=dc + 2)):
            integrate(**kw)
        for kw in (dict(start_p=None), dict(pose_p=None), dict(out_p=None), dict(start_p=d_pose.ptr + 8), dict(pose_p=d_pose.ptr + 8),
                   dict(depth_p=None), dict(rgba_p=dc + 2), dict(icp_p=None), dict(icp_p=capi.AlignIcpParams(max_distance=-0.01))):
            track(**kw)
        assert L.tf_integrate_frame_textured_posed_device(None, dd, dc, cell.ptr, 2) == INV
        # accept out of range
        for kw in (dict(min_stage=0), dict(min_stage=3), dict(min_valid_fraction=1.5), dict(max_rms=np.nan)):
            track(acc_p=capi.TrackAccept(**kw))
        # a handle with a partition
        gv.set_partition(0, 64)
        try:
            assert "partition" in integrate() and "partition" in track()
        finally:
            gv.set_partition(-(2 ** 31), 2 ** 31 - 1)
        untouched(before)
        # a backlog: one frame integrated without texturing ahead of the posed textured call
        p2 = _p12(frames[2][2])
        gv.integrate_frames_device([dd], [dc], [p2])
        backlog = _full(gv)[0]
        assert backlog["dirty"] != before["dirty"] and len(backlog["dirty"]) > 0
        assert "tf_texture_frame_device" in integrate(depth_p=bufs[3][0].ptr, rgba_p=bufs[3][1].ptr)
        assert "tf_texture_frame_device" in track(depth_p=bufs[3][0].ptr, rgba_p=bufs[3][1].ptr)
        untouched(backlog)
        # ... and once the backlog is textured the same call is taken
        gv.texture_frame_device(IR.inverse16(p2), 2)
        c3 = _cell_buf(frames[3][2])
        try:
            gv.integrate_frame_textured_posed_device(bufs[3][0].ptr, bufs[3][1].ptr, c3.ptr, 3)
            after, (_, g, _) = _full(gv)
            assert len(after["dirty"]) == 0 and 3 in g["frameid"] and after["atlas"] != backlog["atlas"]
        finally:
            c3.free()
    finally:
        _free(*bufs, d_out, d_pose, cell)
        gv.close()
