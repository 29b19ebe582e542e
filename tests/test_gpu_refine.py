"""Refining depth against the fused volume on the MI355X: tf_distance_from_surface and tf_refine_frame_in_voxel against
the numpy restatement (tests/refine_ref.py) bit for bit, the read-only guarantee, the device forms (and a device-resident
refine -> integrate), an empty volume, argument checks, and the host mirror's Chisel::GetDistanceFromSurface /
RefineFrameInVoxel."""
import os
import subprocess

import numpy as np
import pytest

from texturefusion_amd import capi, synth
from tests import refine_ref
from tests.raycast_ref import RefVolume, wall_frames
from tests.util import RES5, HipBuffer, make_pair, sorted_ids

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ROOM_FRAMES = 13
SENTINEL = F(-7.25)


@pytest.fixture(scope="module")
def wall_pair(gpu_required):
    ov, gv, cam, _ = make_pair(max_chunks=1 << 15)
    for k, (depth, rgba, pose) in enumerate(wall_frames(cam)):
        gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, k)
    gv.update_meshes()  # the neighbour table filled in (it names parked chunks too)
    gv.sync()
    ov.close()
    yield gv, cam
    gv.close()


@pytest.fixture(scope="module")
def room(gpu_required):
    cam = synth.Camera()
    gv = capi.Volume(RES5, cam, max_chunks=1 << 18)
    frames = [synth.room_frame(k, cam, with_quality=False, wobble=0.1) for k in range(ROOM_FRAMES)]
    for k, (depth, rgba, _, pose) in enumerate(frames):
        gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, k)
    gv.update_meshes()
    gv.sync()
    yield gv, cam, frames
    gv.close()


def _scene(name, wall_pair, room):
    if name == "wall":
        gv, cam = wall_pair
        return gv, cam, [(d, p) for d, _, p in wall_frames(cam)]
    gv, cam, frames = room
    return gv, cam, [(f[0], f[3]) for f in frames]


def _ref(gv):
    ids = gv.list_chunks()
    return RefVolume.from_volume(gv, ids, gv.res), ids


def _points(ids, rng, res=RES5):
    """random points over the chunks' box, points with integral rasterized coordinates (corners repeat), on chunk faces,
    negative coordinates, in the 26-neighbourhood of the chunks (absent and parked chunks), NaN / inf / huge"""
    r, e = float(res), 8 * float(res)
    lo, hi = ids.min(0) * e, (ids.max(0) + 1) * e
    rnd = rng.uniform(lo - 0.05, hi + 0.05, (100000, 3))
    pick = ids[rng.choice(len(ids), min(len(ids), 400), replace=False)].astype(np.float64)
    out = [rnd, pick * e + r / 2, (pick + 1) * e + r / 2, pick * e + r / 2 + r * rng.integers(0, 8, pick.shape),
           pick * e + r / 2 + r * rng.integers(-1, 9, pick.shape) + rng.uniform(0, r, pick.shape) * [1, 0, 0],
           (pick + [0.5, 0.5, 0.0]) * e, (pick + rng.uniform(-1.0, 2.0, pick.shape)) * e,
           (pick + rng.integers(-1, 2, pick.shape)) * e + rng.uniform(0, e, pick.shape),
           -np.abs(rng.uniform(0, 0.5, (2000, 3))),
           [[np.nan, 0, 1], [0, np.nan, 0], [1e30, 0, 0], [-1e30, 1, 1], [np.inf, 0, 0], [0, -np.inf, 0],
            [4.2e4, 0, 1], [-4.2e4, 0, 1], [4.19430e4, 1.0, 1.2]]]
    return np.concatenate([np.asarray(a, np.float64).reshape(-1, 3) for a in out]).astype(np.float32)


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("scene", ["wall", "room"])
def test_distance_from_surface_bit_exact(scene, wall_pair, room):
    gv, _, _ = _scene(scene, wall_pair, room)
    st = gv.stats()
    ref, ids = _ref(gv)
    assert st.n_slots > st.n_chunks  # parked chunks exist (GarbageCollect): the restatement counts them absent
    pts = _points(ids, np.random.default_rng(31))
    d, tw = gv.distance_from_surface(pts)
    ed, etw = refine_ref.surface_dist(ref, pts)
    assert _bits_equal(d, ed), "dist differs at %d points" % (d.view(np.uint32) != ed.view(np.uint32)).sum()
    assert _bits_equal(tw, etw), "tsdf_weight differs at %d points" % (tw.view(np.uint32) != etw.view(np.uint32)).sum()
    assert (etw > 0).sum() > 10000 and (etw == 0).sum() > 1000


def _special_depth(depth, rng):
    d = depth.copy().reshape(-1)
    d[::97] = 0.0
    d[5::211] = np.nan
    d[7::307] = 0.04
    d[9::401] = 3.5
    d[11::503] = 0.05
    d[13::601] = 3.0
    d[15::701] = -1.0
    d[17::809] = np.inf
    return d.reshape(depth.shape)


@pytest.mark.parametrize("scene", ["wall", "room"])
def test_refine_frame_bit_exact(scene, wall_pair, room):
    gv, cam, frames = _scene(scene, wall_pair, room)
    ref, _ = _ref(gv)
    rng = np.random.default_rng(32)
    depth, pose = frames[len(frames) // 2]
    noisy = np.where(depth > 0, depth + rng.uniform(-0.003, 0.003, depth.shape).astype(np.float32), depth).astype(F)
    for inp in (depth, noisy, _special_depth(noisy, rng)):
        sent = np.full(inp.shape, SENTINEL, F)
        got_d, got_w = gv.refine_frame(inp, pose, weight=sent)
        exp_d, exp_w = refine_ref.refine_frame(ref, inp, pose, cam, weight=sent)
        assert _bits_equal(got_d, exp_d), "depth differs at %d pixels" % (got_d.view(np.uint32) != exp_d.view(np.uint32)).sum()
        assert _bits_equal(got_w, exp_w), "weight differs at %d pixels" % (got_w.view(np.uint32) != exp_w.view(np.uint32)).sum()
        assert np.all(sent == SENTINEL)  # the caller's arrays were not touched
        with np.errstate(invalid="ignore"):
            skipped = (inp.astype(np.float64) < 0.05) | (inp.astype(np.float64) > 3.0)
        assert np.all(got_w[skipped] == SENTINEL) and _bits_equal(got_d[skipped], inp[skipped])
        assert (got_w[~skipped] > 0).mean() > 0.8
    nan = np.isnan(inp)
    assert nan.any() and np.all(np.isnan(got_d[nan])) and np.all(got_w[nan] == 0)


def _snapshot(gv):
    st = gv.stats()
    ids = sorted_ids(gv.list_chunks())
    s, w, c = gv.get_chunks(ids)
    dirty = sorted_ids(gv.dirty())
    mids = sorted_ids(gv.list_meshes())
    assert len(mids) > 0
    nv, ni, adj, simp = gv.mesh_counts(mids)
    return (bytes(st), dirty.tobytes(), ids.tobytes(), s.tobytes(), w.tobytes(), c.tobytes(), mids.tobytes(), nv.tobytes(),
            ni.tobytes(), adj.tobytes(), simp.tobytes(), gv.check_neighbours().tobytes())


def test_read_only(wall_pair):
    gv, cam = wall_pair
    before = _snapshot(gv)
    depth, _, pose = wall_frames(cam)[0]
    gv.refine_frame(depth, pose)
    gv.distance_from_surface(_points(gv.list_chunks(), np.random.default_rng(33)))
    assert _snapshot(gv) == before


def test_device_forms_and_refine_then_integrate_on_the_device(gpu_required):
    vols = []
    try:
        for _ in range(2):
            ov, gv, cam, _ = make_pair(max_chunks=1 << 15)
            ov.close()
            vols.append(gv)
            for k, (depth, rgba, pose) in enumerate(wall_frames(cam)[:4]):
                gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, k)
            gv.sync()
        a, b = vols
        depth, rgba, pose = wall_frames(cam)[4]
        rng = np.random.default_rng(34)
        noisy = np.where(depth > 0, depth + rng.uniform(-0.003, 0.003, depth.shape).astype(F), depth).astype(F)
        P = cam.width * cam.height
        # point form
        pts = _points(a.list_chunks(), rng)
        n = len(pts)
        hd, htw = a.distance_from_surface(pts)
        qb = [HipBuffer(12 * n).from_host(pts), HipBuffer(4 * n), HipBuffer(4 * n)]
        try:
            a.distance_from_surface_device(qb[0].ptr, n, qb[1].ptr, qb[2].ptr)
            a.sync()
            assert _bits_equal(qb[1].to_host().view(F), hd) and _bits_equal(qb[2].to_host().view(F), htw)
        finally:
            for x in qb:
                x.free()
        # a: host refine, then the refined depth integrated from a device buffer; b: refine in place on the device and
        # integrate that same buffer -- no host round trip
        hd_img, hw_img = a.refine_frame(noisy, pose)
        bufs = [HipBuffer(4 * P).from_host(hd_img), HipBuffer(4 * P).from_host(noisy), HipBuffer(4 * P),
                HipBuffer(4 * P).from_host(rgba), HipBuffer(4 * P).from_host(rgba)]
        try:
            a.integrate_frames_device([bufs[0].ptr], [bufs[3].ptr], pose.reshape(1, 12))
            bufs[2].from_host(np.zeros(P, F))
            b.refine_frame_device(bufs[1].ptr, bufs[2].ptr, pose)
            b.integrate_frames_device([bufs[1].ptr], [bufs[4].ptr], pose.reshape(1, 12))
            a.sync()
            b.sync()
            assert _bits_equal(bufs[1].to_host().view(F).reshape(depth.shape), hd_img)
            assert _bits_equal(bufs[2].to_host().view(F).reshape(depth.shape), hw_img)
        finally:
            for x in bufs:
                x.free()
        ids_a, ids_b = sorted_ids(a.list_chunks()), sorted_ids(b.list_chunks())
        assert np.array_equal(ids_a, ids_b)
        sa, wa, ca = a.get_chunks(ids_a)
        sb, wb, cb = b.get_chunks(ids_b)
        assert _bits_equal(sa, sb) and _bits_equal(wa, wb) and np.array_equal(ca, cb)
    finally:
        for gv in vols:
            gv.close()


def test_empty_volume_and_bad_arguments(wall_pair):
    cam = synth.Camera()
    empty = capi.Volume(RES5, cam, max_chunks=1 << 10)
    try:
        d, tw = empty.distance_from_surface(np.array([[0, 0, 1.0], [1e30, 0, 0], [np.nan, 0, 0]], F))
        assert not d.any() and not tw.any()
        depth = np.full((cam.height, cam.width), F(1.0))
        depth[0, :8] = [0.0, 0.04, 0.05, 3.0, 3.5, np.nan, 0.005, 4.0]
        depth[1, :2] = [0.006, 2.0]
        sent = np.full(depth.shape, SENTINEL, F)
        cam_far = synth.Camera(near=0.01, far=1.5)
        empty.set_camera(cam_far)
        depth[1, 1] = 2.0  # in [0.05, 3] but beyond far
        rd, rw = empty.refine_frame(depth, synth.pose_identity(), weight=sent)
        inr = ~((depth.astype(np.float64) < 0.05) | (depth.astype(np.float64) > 3.0)) & ~np.isnan(depth)
        inr_near_far = inr & (depth <= F(1.5)) & (depth >= F(0.01))
        assert _bits_equal(rd[inr_near_far], depth[inr_near_far]) and np.all(rw[inr] == 0)
        assert rd[1, 1] == 0 and rw[1, 1] == 0
        assert np.all(rw[~inr & ~np.isnan(depth)] == SENTINEL) and np.isnan(rd[0, 5]) and rw[0, 5] == 0
        assert rd[0, 1] == F(0.04) and rd[0, 4] == F(3.5)  # skipped
        assert rd[0, 2] == F(0.05) and rw[0, 2] == 0  # (double)0.05f >= 0.05: refined, kept
        assert rd[0, 3] == 0 and rw[0, 3] == 0  # 3.0 is not > 3: refined, then beyond far
    finally:
        empty.close()
    gv, cam = wall_pair
    L = gv.L
    depth = np.ones(cam.width * cam.height, F)
    w = np.zeros_like(depth)
    pose = synth.pose_identity().astype(F).reshape(12)
    dp, wp, pp = (capi._p(x, capi.C.c_float) for x in (depth, w, pose))
    xyz = np.zeros(3, F)
    assert L.tf_refine_frame_in_voxel(None, dp, wp, pp) == capi.TF_ERR_INVALID
    assert L.tf_refine_frame_in_voxel(gv.h, None, wp, pp) == capi.TF_ERR_INVALID
    assert L.tf_refine_frame_in_voxel(gv.h, dp, None, pp) == capi.TF_ERR_INVALID
    assert L.tf_refine_frame_in_voxel(gv.h, dp, wp, None) == capi.TF_ERR_INVALID
    assert L.tf_refine_frame_in_voxel_device(gv.h, None, None, pp) == capi.TF_ERR_INVALID
    bad = pose.copy()
    bad[7] = np.inf
    with pytest.raises(capi.TFError) as e:
        gv.refine_frame(depth.reshape(cam.height, cam.width), bad)
    assert e.value.code == capi.TF_ERR_INVALID and "finite" in str(e.value)
    xp = capi._p(xyz, capi.C.c_float)
    assert L.tf_distance_from_surface(gv.h, xp, -1, wp, wp) == capi.TF_ERR_INVALID
    assert L.tf_distance_from_surface(None, xp, 1, wp, wp) == capi.TF_ERR_INVALID
    assert L.tf_distance_from_surface(gv.h, None, 1, wp, wp) == capi.TF_ERR_INVALID
    assert L.tf_distance_from_surface(gv.h, xp, 1, None, wp) == capi.TF_ERR_INVALID
    assert L.tf_distance_from_surface(gv.h, None, 0, None, None) == capi.TF_OK  # n = 0: a no-op
    assert L.tf_distance_from_surface_device(gv.h, None, 0, None, None) == capi.TF_OK
    d, tw = gv.distance_from_surface(np.zeros((0, 3), F))
    assert d.shape == (0,) and tw.shape == (0,)
    gv.sync()  # the handle is still usable


def test_host_mirror_refine(gpu_required, tmp_path):
    exe = str(tmp_path / "mirror_refine")
    src = os.path.join(ROOT, "tests", "cpp_refine", "mirror_refine.cpp")
    lib = os.path.join(ROOT, "texturefusion_amd")
    subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", src, "-o", exe, "-L" + lib, "-ltexfusion_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mirror ok" in r.stdout, r.stdout + r.stderr
