"""Buffers that follow the camera or the request: the frame images, the group staging, the host ring, the keyframe cache's
images and the snapshot buffer (fitted buffers, texturefusion_amd/csrc/tf_mem.h).  A handle that went through a size change
must compute what a fresh handle that only ever had the final size computes, bit for bit -- in both directions, since a
fitted buffer grows on the way up and is kept on the way down.  Small pools and a 1920 x 720 atlas keep every case short."""
import numpy as np
import pytest

from tests.util import RES5, sorted_ids
from texturefusion_amd import capi, synth

pytestmark = pytest.mark.gpu

SMALL = synth.Camera(64, 48, 52.5, 52.5, 31.5, 23.5, 0.01, 5.0)
LARGE = synth.Camera(128, 96, 105.0, 105.0, 63.5, 47.5, 0.01, 5.0)
AW, AH = 1920, 720  # 80 x 40 slots of 24 x 18 (as tests/test_gpu_patch_borders.py)
POSES = [synth.pose_identity(), synth.pose_euler(0.12, -0.05, 0.02, (0.04, -0.02, 0.0)), synth.pose_yaw(-0.08, (-0.03, 0.01, 0.0))]
_FRAMES = {}


def _volume(cam):
    return capi.Volume(RES5, cam, max_chunks=4096, atlas_w=AW, atlas_h=AH)


def _frames(cam):
    """six frames of a wall at 0.8 m with a position-dependent colour: (depth, rgba, quality, pose); computed once per camera"""
    if cam not in _FRAMES:
        uv = np.stack(np.meshgrid(np.arange(cam.width) * (6.4 / cam.width), np.arange(cam.height) * (4.8 / cam.height)), -1)
        out = []
        for k in range(6):
            d, _, q, pose = synth.wall_frame(0.8, cam, pose=POSES[k % 3], hole_stride=17, seed=k)
            out.append((d, synth._hash_colour(uv[..., [0, 1, 1]] + k, 5), q, pose))
        _FRAMES[cam] = out
    return _FRAMES[cam]


def _chunks(v):
    ids = sorted_ids(v.list_chunks())
    assert len(ids) > 100
    return (ids,) + tuple(v.get_chunks(ids))


def _assert_same_chunks(a, b, what):
    assert np.array_equal(a[0], b[0]), "%s: chunk lists differ" % what
    for x, y, name in zip(a[1:], b[1:], ("sdf", "weight", "colour")):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s: %s differs" % (what, name)


def _keyframe_round(v, cam, rgb_upload, with_group):
    fr = _frames(cam)
    d, rgba, q, pose = fr[0]
    if rgb_upload:
        v.frame_upload_rgb(d, np.ascontiguousarray(rgba[..., :3]), np.ascontiguousarray(rgba[..., 3]), q)
    else:
        v.frame_upload(d, rgba, q)
    ids, new = v.prepare(pose)
    needs = np.zeros(len(ids), np.uint8)
    v.integrate(pose, ids, needs, 1, True, True)
    v.finalize(ids, needs, new)
    if with_group:  # a second list, two local frames as host images
        ids, new = v.prepare(fr[1][3])
        needs = np.zeros(len(ids), np.uint8)
        v.integrate_depth_group_host([fr[1][0], fr[2][0]], np.stack([fr[1][3].reshape(12), fr[2][3].reshape(12)]), ids, needs, 1)
        v.finalize(ids, needs, new)


@pytest.mark.parametrize("first,last", [(SMALL, LARGE), (LARGE, SMALL)], ids=["grow", "shrink"])
def test_frame_images_and_group_staging_follow_the_camera(first, last, gpu_required):
    a, b = _volume(first), _volume(last)
    try:
        _keyframe_round(a, first, rgb_upload=False, with_group=False)
        a.reset()
        a.set_camera(last)
        _keyframe_round(a, last, rgb_upload=True, with_group=True)
        _keyframe_round(b, last, rgb_upload=True, with_group=True)
        _assert_same_chunks(_chunks(a), _chunks(b), "after %dx%d" % (first.width, first.height))
    finally:
        a.close()
        b.close()


def _host_frames(v, cam):
    for k, (d, rgba, _, pose) in enumerate(_frames(cam)):
        v.integrate_frame_host(d, rgba, pose.reshape(12), synth.pose_inverse16(pose), k)
    v.sync()


@pytest.mark.parametrize("defer", [True, False], ids=["deferred", "immediate"])
def test_host_ring_follows_the_camera(defer, gpu_required):
    a, b = _volume(SMALL), _volume(LARGE)
    try:
        a.host_frame_set_deferral(defer)
        b.host_frame_set_deferral(defer)
        _host_frames(a, SMALL)
        a.reset()
        a.set_camera(LARGE)
        _host_frames(a, LARGE)
        _host_frames(b, LARGE)
        _assert_same_chunks(_chunks(a), _chunks(b), "host ring")
        ma = sorted_ids(a.list_meshes())
        assert len(ma) > 100 and np.array_equal(ma, sorted_ids(b.list_meshes()))
        assert np.array_equal(a.atlas_rows(0, AH, AW), b.atlas_rows(0, AH, AW))
    finally:
        a.close()
        b.close()


def _patch_flow(v, cam):
    """the flow of tests/test_gpu_atlas.py::test_generate_patches_update_atlas, one round: -> (ids, patches, atlas rows)"""
    fr = _frames(cam)
    for d, rgba, _, pose in fr:
        v.frame_upload(d, rgba, None)
        v.integrate_frame(pose, True)
    v.update_meshes()
    ids = v.compress_meshes()
    assert len(ids) > 100
    labels = np.where(np.arange(len(ids)) % 3 == 0, 8, 3).astype(np.int32)
    rc, hot = v.generate_patches(ids, labels)
    assert rc == 0 and hot[1] // AW > hot[0] // AW
    v.update_atlas(ids)
    return ids, v.get_patches(ids), v.atlas_rows(hot[0] // AW, hot[1] // AW, AW)


def _cache(v, cam, ids=(3, 8)):
    fr = _frames(cam)
    for kf, f in zip(ids, (fr[4], fr[5])):
        v.keyframe_cache(kf, np.ascontiguousarray(f[1][..., :3]), f[0], synth.pose_inverse16(f[3]))


def test_keyframe_cache_follows_the_camera(gpu_required):
    """The same kf_id cached at 64 x 48 and again, after tf_set_camera, at 128 x 96: the handle's copies are as large as the
    camera's images at each call."""
    a, b = _volume(SMALL), _volume(LARGE)
    try:
        _cache(a, SMALL)
        a.set_camera(LARGE)
        _cache(a, LARGE)
        _cache(b, LARGE)
        ia, pa, ra = _patch_flow(a, LARGE)
        ib, pb, rb = _patch_flow(b, LARGE)
        assert np.array_equal(ia, ib)
        have = (pa["flags"] & 1) != 0
        assert have.sum() > 100 and np.array_equal(pa["voff"], pb["voff"])
        assert np.array_equal(pa["texloc"], pb["texloc"]) and np.array_equal(pa["frameid"], pb["frameid"])
        assert np.array_equal(pa["flags"] & 31, pb["flags"] & 31)
        assert np.array_equal(pa["bbox"][have], pb["bbox"][have])
        assert np.array_equal(pa["ratio"][have].view(np.uint32), pb["ratio"][have].view(np.uint32))
        vert = np.repeat(have, np.diff(pa["voff"]))
        for key in ("texcoord", "texcolor"):
            assert np.array_equal(pa[key][vert].view(np.uint32), pb[key][vert].view(np.uint32)), key
        assert ra.any() and np.array_equal(ra, rb)
    finally:
        a.close()
        b.close()


def test_snapshot_buffer_grows_by_doubling(gpu_required):
    """8 rows (the first allocation holds 64), 200 rows (two doublings), 8 rows again: each snapshot is the atlas."""
    v = _volume(LARGE)
    try:
        _cache(v, LARGE)
        _patch_flow(v, LARGE)
        whole = v.atlas_rows(0, AH, AW)
        assert whole[:8].any()
        for r0, n in ((0, 8), (10, 200), (4, 8)):
            rows, _, _ = v.atlas_snapshot_rows(r0, r0 + n, AW)
            assert np.array_equal(rows, whole[r0:r0 + n]), "snapshot of rows %d..%d" % (r0, r0 + n)
    finally:
        v.close()
