"""Reading the fused volume back on the MI355X: tf_query_points against the numpy restatement (bit for bit), tf_raycast
against the input depth and against the restated march, the read-only guarantee, edge cases, the device forms, and the
host mirror's ChunkManager::GetSDF / GetSDFAndGradient."""
import os
import subprocess

import numpy as np
import pytest

from texturefusion_amd import capi, synth
from tests.raycast_ref import RefVolume, wall_frames, wall_poses
from tests.util import RES5, HipBuffer, assert_chunks_equal, make_pair, sorted_ids

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = synth.Camera(160, 120, 131.25, 131.25, 79.5, 59.5)
# S-room: 13 frames of the orbit with a hand-held pitch / roll (synth.room_frame wobble); the view is frame 10, whose pitch
# lies mid-range of the set, so that the space just outside its top and bottom image rows was observed by other frames (a
# yaw-only orbit never observes it: rays near those rows then meet a surface with no observed voxels behind it)
ROOM_FRAMES, ROOM_VIEW = 13, 10


@pytest.fixture(scope="module")
def wall_pair(gpu_required):
    ov, gv, cam, _ = make_pair(max_chunks=1 << 15)
    for k, (depth, rgba, pose) in enumerate(wall_frames(cam)):
        ov.integrate_frame(depth, rgba, pose)
        gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, k)
    gv.sync()
    yield ov, gv, cam
    gv.close()
    ov.close()


@pytest.fixture(scope="module")
def room(gpu_required):
    cam = synth.Camera()
    gv = capi.Volume(RES5, cam, max_chunks=1 << 18)
    frames = [synth.room_frame(k, cam, with_quality=False, wobble=0.1) for k in range(ROOM_FRAMES)]
    for k, (depth, rgba, _, pose) in enumerate(frames):
        gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, k)
    gv.sync()
    yield gv, cam, frames
    gv.close()


def _ref(gv):
    ids = gv.list_chunks()
    return RefVolume.from_volume(gv, ids, gv.res), ids


def _border_points(ids, rng, res=RES5):
    """points exactly on voxel faces, chunk faces and corners, and in chunks next to the present ones (mostly absent)"""
    pick = ids[rng.choice(len(ids), min(len(ids), 300), replace=False)].astype(np.float64)
    e = 8 * float(res)
    out = [pick * e, (pick + 1) * e, pick * e + float(res) * 3, (pick + [0.5, 0.5, 0]) * e, (pick + [0, 0.5, 0.5]) * e,
           (pick + [0.5, 0, 0.5]) * e, (pick + [1.5, 0.5, 0.5]) * e, (pick - [0.5, 0.5, 0.5]) * e,
           pick * e + rng.integers(0, 8, pick.shape) * float(res)]
    return np.concatenate(out).astype(np.float32)


def _assert_query_equal(got, exp):
    assert np.array_equal(got["flags"], exp["flags"]), "flags differ at %d points" % (got["flags"] != exp["flags"]).sum()
    for k in ("sdf", "weight", "grad", "sdf_tri"):
        assert np.array_equal(got[k].view(np.uint32), exp[k].view(np.uint32)), "%s differs" % k
    assert np.array_equal(got["rgb"], exp["rgb"]), "rgb differs"


@pytest.mark.parametrize("scene", ["wall", "room"])
def test_query_points_bit_exact_against_the_restatement(scene, wall_pair, room):
    gv = wall_pair[1] if scene == "wall" else room[0]
    ref, ids = _ref(gv)
    rng = np.random.default_rng(11)
    lo, hi = ids.min(0) * 8 * float(RES5), (ids.max(0) + 1) * 8 * float(RES5)
    rnd = rng.uniform(lo - 0.05, hi + 0.05, (200000, 3)).astype(np.float32)
    near = (ids[rng.integers(0, len(ids), 100000)] * 8 + rng.uniform(0, 8, (100000, 3))) * float(RES5)
    pts = np.concatenate([rnd, near.astype(np.float32), _border_points(ids, rng)])
    got = gv.query(pts)
    exp = ref.query(pts)
    _assert_query_equal(got, exp)
    f = exp["flags"]
    assert (f & 1).sum() > 1000 and (f & 4).sum() > 1000 and (f & 8).sum() > 1000 and (f & 16).sum() > 1000
    assert (f == 0).sum() > 1000  # missing chunks too


def _angle_deg(n, ref_n):
    c = np.clip(np.einsum("i...,i->...", n, np.asarray(ref_n, np.float32)), -1, 1)
    return np.degrees(np.arccos(c))


def test_raycast_wall_from_its_integration_pose(wall_pair):
    _, gv, cam = wall_pair
    depth_in, _, pose = wall_frames(cam)[0]
    r = gv.raycast(pose, 0.1, 3.0, 1024)
    valid = depth_in > 0
    hit = r["depth"] > 0
    assert hit[valid].mean() >= 0.99, hit[valid].mean()
    close = np.abs(r["depth"] - depth_in) <= RES5 / 2
    assert (close & hit)[valid].mean() >= 0.99
    ang = _angle_deg(r["normal"][:, hit], (0, 0, -1))
    assert np.quantile(ang, 0.99) < 5.0, np.quantile(ang, 0.99)
    assert np.all(r["rgba"][hit, 3] == 255) and np.all(r["rgba"][~hit] == 0)
    c = r["rgba"][hit, :3]
    assert (np.all(c == [200, 100, 50], axis=1)).mean() >= 0.99
    # the vertex map is the world hit point: pose is a translation, camera-frame z = depth
    assert np.allclose(r["vertex"][2][hit], r["depth"][hit] + pose[2, 3], atol=1e-5)


def test_raycast_room_from_its_integration_pose(room):
    gv, cam, frames = room
    depth_in, _, _, pose = frames[ROOM_VIEW]
    r = gv.raycast(pose, 0.1, 5.0, 2048)
    valid = depth_in > 0
    hit = r["depth"] > 0
    assert hit[valid].mean() >= 0.99, hit[valid].mean()
    close = np.abs(r["depth"] - depth_in) <= RES5 / 2
    assert (close & hit)[valid].mean() >= 0.99, (close & hit)[valid].mean()
    nrm = np.linalg.norm(r["normal"][:, hit], axis=0)
    assert (np.abs(nrm - 1) < 1e-5).mean() >= 0.99


def test_raycast_matches_the_restated_march(wall_pair, room):
    for gv, pose, cover in ((wall_pair[1], wall_poses()[0], 0.9), (room[0], room[2][ROOM_VIEW][3], 0.9),
                            (room[0], synth.pose_yaw(0.7, (0.1, 0.05, -0.2)), 0.2)):  # (off the orbit: a partial view)
        ref, _ = _ref(gv)
        gv.raycast_camera(SMALL)
        try:
            r = gv.raycast(pose, 0.1, 5.0, 2048)
        finally:
            gv.raycast_camera(None)
        exp = ref.raycast_depth(pose, SMALL.fx, SMALL.fy, SMALL.cx, SMALL.cy, SMALL.width, SMALL.height, 0.1, 5.0, 2048)
        assert np.array_equal(r["depth"] > 0, exp > 0), "hit masks differ at %d pixels" % ((r["depth"] > 0) != (exp > 0)).sum()
        diff = r["depth"].view(np.uint32) != exp.view(np.uint32)
        assert not diff.any(), "depth differs at %d pixels, first (y, x) %s" % (diff.sum(), np.argwhere(diff)[:4].tolist())
        assert (exp > 0).mean() > cover


def _snapshot(gv):
    st = gv.stats()
    ids = sorted_ids(gv.list_chunks())  # (both lists come back in no fixed order)
    s, w, c = gv.get_chunks(ids)
    dirty = sorted_ids(gv.dirty())
    return (bytes(st), dirty.tobytes(), ids.tobytes(), s.tobytes(), w.tobytes(), c.tobytes())


def test_read_only_and_integration_stays_bit_exact(gpu_required):
    ov, gv, cam, _ = make_pair(max_chunks=1 << 15)
    frames = wall_frames(cam)
    for k, (depth, rgba, pose) in enumerate(frames[:4]):
        ov.integrate_frame(depth, rgba, pose)
        gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, k)
    gv.update_meshes()  # the neighbour table and the summaries filled in: the raycaster reads the table
    ov.update_meshes()
    gv.sync()
    before = _snapshot(gv)
    ids = gv.list_chunks()
    rng = np.random.default_rng(3)
    gv.query(_border_points(ids, rng))
    gv.raycast(frames[0][2], 0.1, 3.0, 1024)
    gv.raycast(synth.pose_yaw(0.3, (0.05, 0.0, 0.1)), 0.1, 3.0, 1024)
    assert _snapshot(gv) == before
    depth, rgba, pose = frames[4]
    ov.integrate_frame(depth, rgba, pose)
    gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, 4)
    gv.sync()
    assert_chunks_equal(ov, gv, ov.list_chunks(), "after a raycast and a query")
    gv.close()
    ov.close()


def test_empty_volume_looking_away_and_bad_arguments(wall_pair):
    _, gv, cam = wall_pair
    empty = capi.Volume(RES5, cam, max_chunks=1 << 10)
    try:
        r = empty.raycast(synth.pose_identity(), 0.1, 3.0, 256)
        assert not r["depth"].any() and not r["rgba"].any() and not r["normal"].any()
        q = empty.query(np.array([[0, 0, 1.0], [1e30, 0, 0], [np.nan, 0, 0]], np.float32))
        assert not q["flags"].any()
    finally:
        empty.close()
    r = gv.raycast(synth.pose_yaw(np.pi), 0.1, 3.0, 256)
    assert not r["depth"].any()
    for near, far, steps in ((1.0, 1.0, 64), (2.0, 1.0, 64), (-0.1, 1.0, 64), (0.1, 1.0, 0), (0.1, np.inf, 64)):
        with pytest.raises(capi.TFError) as e:
            gv.raycast(synth.pose_identity(), near, far, steps)
        assert e.value.code == capi.TF_ERR_INVALID
    bad = synth.pose_identity().copy()
    bad[0, 3] = np.nan
    with pytest.raises(capi.TFError) as e:
        gv.raycast(bad, 0.1, 1.0, 64)
    assert e.value.code == capi.TF_ERR_INVALID
    with pytest.raises(capi.TFError) as e:
        gv.query(np.zeros((1, 3), np.float32), want=64)
    assert e.value.code == capi.TF_ERR_INVALID
    gv.sync()  # the handle is still usable


def test_raycast_outputs_follow_the_raycast_camera(wall_pair):
    """Volume.raycast sizes its arrays from the camera raycast_camera set: a larger and a smaller camera, then back"""
    _, gv, cam = wall_pair
    big = synth.Camera(1280, 960, 1050.0, 1050.0, 639.5, 479.5)
    pose = wall_poses()[0]
    try:
        for c in (big, SMALL):
            gv.raycast_camera(c)
            r = gv.raycast(pose, 0.1, 3.0, 1024)
            assert r["depth"].shape == (c.height, c.width) and r["normal"].shape == (3, c.height, c.width)
            assert r["rgba"].shape == (c.height, c.width, 4) and r["vertex"].shape == (3, c.height, c.width)
            assert (r["depth"] > 0).mean() > 0.9
    finally:
        gv.raycast_camera(None)
    assert gv.raycast(pose, 0.1, 3.0, 1024)["depth"].shape == (cam.height, cam.width)


def test_raycast_camera_rejects_bad_arguments(wall_pair):
    _, gv, cam = wall_pair
    L = gv.L
    bad = ((np.nan, 525, 319.5, 239.5, 640, 480), (525, np.inf, 319.5, 239.5, 640, 480),
           (525, 525, np.nan, 239.5, 640, 480), (525, 525, 319.5, -np.inf, 640, 480),
           (525, 525, 3e9, 239.5, 640, 480), (3e9, 525, 319.5, 239.5, 640, 480), (0.5, 525, 319.5, 239.5, 640, 480),
           (525, 525, 319.5, 239.5, 640, 0), (525, 525, 319.5, 239.5, -8, 480), (525, 525, 319.5, 239.5, 40000, 480))
    for a in bad:
        assert L.tf_raycast_camera(gv.h, *a) == capi.TF_ERR_INVALID, a
    # nothing was set: the handle's camera is still the raycaster's
    assert (gv.raycast(wall_poses()[0], 0.1, 3.0, 1024)["depth"] > 0).mean() > 0.9


def test_device_forms_match_the_host_forms(wall_pair):
    _, gv, cam = wall_pair
    pose = wall_poses()[0]
    host = gv.raycast(pose, 0.1, 3.0, 1024)
    P = cam.width * cam.height
    bufs = [HipBuffer(4 * P), HipBuffer(12 * P), HipBuffer(4 * P), HipBuffer(12 * P)]
    try:
        gv.raycast_device(pose, 0.1, 3.0, 1024, *[b.ptr for b in bufs])
        gv.sync()
        assert np.array_equal(bufs[0].to_host().view(np.float32).reshape(cam.height, cam.width), host["depth"])
        assert np.array_equal(bufs[1].to_host().view(np.float32).reshape(3, cam.height, cam.width), host["normal"])
        assert np.array_equal(bufs[2].to_host().reshape(cam.height, cam.width, 4), host["rgba"])
        assert np.array_equal(bufs[3].to_host().view(np.float32).reshape(3, cam.height, cam.width), host["vertex"])
    finally:
        for b in bufs:
            b.free()
    rng = np.random.default_rng(5)
    pts = _border_points(gv.list_chunks(), rng)
    n = len(pts)
    hq = gv.query(pts)
    qb = [HipBuffer(12 * n).from_host(pts), HipBuffer(4 * n), HipBuffer(4 * n), HipBuffer(12 * n), HipBuffer(4 * n),
          HipBuffer(3 * n), HipBuffer(4 * n)]
    try:
        gv.query_device(qb[0].ptr, n, 31, *[b.ptr for b in qb[1:]])
        gv.sync()
        got = {"sdf": qb[1].to_host().view(np.float32), "weight": qb[2].to_host().view(np.float32),
               "grad": qb[3].to_host().view(np.float32).reshape(n, 3), "sdf_tri": qb[4].to_host().view(np.float32),
               "rgb": qb[5].to_host().reshape(n, 3), "flags": qb[6].to_host().view(np.uint32)}
        _assert_query_equal(got, hq)
    finally:
        for b in qb:
            b.free()


def test_host_mirror_point_queries(gpu_required, tmp_path):
    exe = str(tmp_path / "mirror_query")
    src = os.path.join(ROOT, "tests", "cpp_ray", "mirror_query.cpp")
    lib = os.path.join(ROOT, "texturefusion_amd")
    subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", src, "-o", exe, "-L" + lib, "-ltexfusion_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mirror ok" in r.stdout, r.stdout + r.stderr
