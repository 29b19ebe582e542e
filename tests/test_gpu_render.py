"""The device rasteriser on the MI355X: every input set of tests/render_inputs.py in every mode against the numpy
restatement (triangle ids equal, depth bit-equal, colour equal), host form against device form, run against run, the error
returns, and the model level: the wall scene through the textured per-frame path, rendered from its integration pose --
held to what tests/test_render_cpu.py shows the reference pipeline to deliver -- with the read-only guarantee."""
import ctypes as C

import numpy as np
import pytest

from tests import render_inputs as RI
from tests import render_ref as R
from tests.test_render_cpu import SHARE, model_conditions, ref_cached, wall_scene
from tests.util import RES5, HipBuffer, sorted_ids
from texturefusion_amd import capi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gv(gpu_required):
    v = capi.Volume(RES5, RI.CAMERAS["small"], max_chunks=1 << 10)
    yield v
    v.close()


@pytest.fixture(scope="module")
def wall(gpu_required):
    cam = synth.Camera()
    v = capi.Volume(RES5, cam, max_chunks=1 << 15)
    frames = wall_scene(cam)
    for k, (depth, rgba, pose) in enumerate(frames):
        v.integrate_frame_host(depth, rgba, pose.reshape(12), synth.pose_inverse16(pose), k)
    v.sync()
    yield v, cam, frames
    v.close()


def _run(gv, s, mode):
    gv.raycast_camera(s["cam"])
    try:
        return gv.render_stream(s["V"], s["I"], s["pose"], s["near"], s["far"], mode, s["texture"])
    finally:
        gv.raycast_camera(None)


def _assert_equal(got, exp, what):
    assert np.array_equal(got["tri"], exp["tri"]), "%s: triangle ids differ at %d pixels" % (what, (got["tri"] != exp["tri"]).sum())
    assert np.array_equal(got["depth"].view(np.uint32), exp["depth"].view(np.uint32)), "%s: depth differs" % what
    bad = np.any(got["rgba"] != exp["rgba"], axis=-1)
    assert not bad.any(), "%s: rgba differs at %d pixels, first %s" % (what, bad.sum(), np.argwhere(bad)[:3].tolist())


@pytest.mark.parametrize("name", list(RI.all_sets()))
def test_every_input_set_matches_the_restatement(name, gv):
    s = RI.all_sets()[name]
    for mode in RI.MODES:
        _assert_equal(_run(gv, s, mode), ref_cached(name, mode), "%s mode %d" % (name, mode))


def test_out_of_range_index_and_vanishing_triangles(gv):
    s = RI.all_sets()["h_vanish"]
    assert int(s["I"].max()) == len(s["V"])  # dropped by the kernel's bounds test, never dereferenced
    r = _run(gv, s, 2)
    assert set(np.unique(r["tri"])) - {-1} == set(s["stay"]) | {s["crossing"]}
    empty = r["tri"] < 0
    assert not r["rgba"][empty].any() and not r["depth"][empty].any() and np.all(r["rgba"][~empty, 3] == 255)


def _device_render(gv, s, mode, outputs=(True, True, True)):
    H, W = s["cam"].height, s["cam"].width
    P = W * H
    bufs = [HipBuffer(max(s["V"].nbytes, 16)).from_host(s["V"]), HipBuffer(max(s["I"].nbytes, 16)).from_host(s["I"]),
            HipBuffer(s["texture"].nbytes).from_host(s["texture"]), HipBuffer(4 * P), HipBuffer(4 * P), HipBuffer(4 * P)]
    gv.raycast_camera(s["cam"])
    try:
        th, tw = s["texture"].shape[:2]
        gv.render_stream_device(bufs[0].ptr, len(s["V"]), bufs[1].ptr, len(s["I"]), s["pose"], s["near"], s["far"], mode,
                                bufs[2].ptr, tw, th, *[b.ptr if on else 0 for b, on in zip(bufs[3:], outputs)])
        gv.sync()
        return {"rgba": bufs[3].to_host().reshape(H, W, 4), "depth": bufs[4].to_host().view(np.float32).reshape(H, W),
                "tri": bufs[5].to_host().view(np.int32).reshape(H, W)}
    finally:
        gv.raycast_camera(None)
        for b in bufs:
            b.free()


@pytest.mark.parametrize("name", ["i_full_mixed", "g_modes", "j_count_257", "j_count_0"])
def test_host_and_device_forms_and_two_runs_agree(name, gv):
    s = RI.all_sets()[name]
    for mode in (2, 3):
        host = _run(gv, s, mode)
        _assert_equal(_device_render(gv, s, mode), host, "%s device form" % name)
        _assert_equal(_run(gv, s, mode), host, "%s second run" % name)
    # every output is optional: depth alone
    one = _device_render(gv, s, 4, outputs=(False, True, False))
    assert np.array_equal(one["depth"].view(np.uint32), ref_cached(name, 4)["depth"].view(np.uint32))


def test_error_returns(gv, gpu_required):
    s = RI.all_sets()["a_triangle_ccw"]
    V, I, tex, pose = s["V"], s["I"], s["texture"], np.ascontiguousarray(s["pose"], np.float32).reshape(12)
    H, W = gv.cam.height, gv.cam.width
    cap = max(H * W, 640 * 480)  # (room for a handle's default camera too: a call that should fail must not overrun if it does not)
    rgba, depth, tri = np.zeros((cap, 4), np.uint8), np.zeros(cap, np.float32), np.zeros(cap, np.int32)
    p = capi._p

    def call(h=None, ni=len(I), near=0.05, far=4.0, mode=2, outs=(rgba, depth, tri), texture=tex, pose=pose):
        return gv.L.tf_render_stream(h or gv.h, p(V, C.c_float), len(V), p(I, C.c_uint32), ni,
                                     None if texture is None else p(texture, C.c_uint8), 8, 8, p(pose, C.c_float), near,
                                     far, mode, None if outs[0] is None else p(outs[0], C.c_uint8),
                                     None if outs[1] is None else p(outs[1], C.c_float),
                                     None if outs[2] is None else p(outs[2], C.c_int32))

    assert call() == capi.TF_OK
    for mode in (0, 5, -1):
        assert call(mode=mode) == capi.TF_ERR_INVALID
    assert call(ni=2) == capi.TF_ERR_INVALID
    for near, far in ((1.0, 1.0), (2.0, 1.0), (-0.1, 1.0), (0.1, np.inf), (np.nan, 1.0)):
        assert call(near=near, far=far) == capi.TF_ERR_INVALID
    assert call(outs=(None, None, None)) == capi.TF_ERR_INVALID
    bad = pose.copy()
    bad[3] = np.nan
    assert call(pose=bad) == capi.TF_ERR_INVALID
    # no camera: a handle is created with one (640 x 480), so the only way to be without is a focal length that truncates to 0
    blind = capi.Volume(RES5, synth.Camera(W, H, 0.5, 0.5, 79.5, 59.5, 0.01, 5.0), max_chunks=1 << 10)
    try:
        assert call(h=blind.h) == capi.TF_ERR_INVALID
        assert blind.L.tf_render_model(blind.h, p(pose, C.c_float), 0.05, 4.0, 4, p(rgba, C.c_uint8), None, None) == capi.TF_ERR_INVALID
    finally:
        blind.close()
    assert call(mode=4, texture=None) == capi.TF_OK  # NULL texture = the atlas, which every handle owns
    assert call(mode=1, outs=(None, None, tri)) == capi.TF_OK
    gv.sync()  # the handle is still usable


def _snapshot(v, atlas_rows):
    st = v.stats()
    ids = sorted_ids(v.list_chunks())
    s, w, c = v.get_chunks(ids[len(ids) // 2:len(ids) // 2 + 1])
    V, I = v.draw_meshes()
    return (bytes(st), bytes(v.texture_stats()), ids.tobytes(), s.tobytes(), w.tobytes(), c.tobytes(),
            v.atlas_rows(0, atlas_rows, 13824).tobytes(), V.tobytes(), I.tobytes())


def test_model_from_its_integration_pose(wall):
    v, cam, frames = wall
    depth_in, _, pose = frames[0]
    rows = min(13824, int(v.atlas_loc_next() // 13824) + 36)
    before = _snapshot(v, rows)
    r4 = v.render_model(pose, 0.1, 3.0, 4)
    cover, close, colour = model_conditions(r4, depth_in)
    print("device, wall: covered %.4f, depth %.4f, colour %.4f" % (cover, close, colour))
    assert cover >= SHARE and close >= SHARE and colour >= SHARE
    # render_model == render_stream of draw_meshes_device's stream, bit for bit; and both == the restatement
    V, I = v.draw_meshes()
    assert len(I) > 300000  # (past the first capacity of the handle's stream buffers, 196 608 indices: tf_render_model grew them)
    bufs = [HipBuffer(V.nbytes), HipBuffer(I.nbytes)]
    try:
        nv, ni = C.c_int64(0), C.c_int64(0)
        v._ck(v.L.tf_draw_meshes_device(v.h, bufs[0].ptr, bufs[1].ptr, len(V), len(I), C.byref(nv), C.byref(ni)))
        assert (nv.value, ni.value) == (len(V), len(I))
        P = cam.width * cam.height
        out = [HipBuffer(4 * P), HipBuffer(4 * P), HipBuffer(4 * P)]
        bufs += out
        for mode in (4, 3, 2, 1):
            v.render_stream_device(bufs[0].ptr, len(V), bufs[1].ptr, len(I), pose, 0.1, 3.0, mode,
                                   d_rgba=out[0].ptr, d_depth=out[1].ptr, d_tri=out[2].ptr)
            v.sync()
            got = {"rgba": out[0].to_host().reshape(cam.height, cam.width, 4),
                   "depth": out[1].to_host().view(np.float32).reshape(cam.height, cam.width),
                   "tri": out[2].to_host().view(np.int32).reshape(cam.height, cam.width)}
            _assert_equal(v.render_model(pose, 0.1, 3.0, mode), got, "render_model mode %d" % mode)
            if mode in (4, 3):
                atlas = v.atlas_rows(0, rows, 13824)
                exp = R.render(V, I, cam, pose, 0.1, 3.0, mode, _AtlasRows(atlas))
                _assert_equal(got, exp, "model against the restatement, mode %d" % mode)
        v.render_model_device(pose, 0.1, 3.0, 4, d_rgba=out[0].ptr)
        v.sync()
        assert np.array_equal(out[0].to_host().reshape(cam.height, cam.width, 4), r4["rgba"])
    finally:
        for b in bufs:
            b.free()
    # from another pose too, then: nothing of the volume, the meshes, the patches or the atlas has changed
    v.render_model(synth.pose_yaw(0.3, (0.05, 0.0, 0.1)), 0.1, 3.0, 3)
    assert _snapshot(v, rows) == before


class _AtlasRows:
    """the atlas's hot rows as the restatement's texture: shaped like the whole atlas (the clamp is against its size),
    holding only the rows that were downloaded -- the model's texcoords lie inside them"""

    def __init__(self, rows):
        self.rows = rows
        self.shape = (13824, 13824, 3)

    def __array__(self, dtype=None, copy=None):
        raise TypeError("index it instead")

    def __getitem__(self, key):
        y, x, k = key
        assert int(np.max(y, initial=0)) < len(self.rows)
        return self.rows[y, x, k]


def test_model_without_patches_renders_empty(gpu_required):
    cam = RI.CAMERAS["small"]
    v = capi.Volume(RES5, cam, max_chunks=1 << 14)
    try:
        r = v.render_model(synth.pose_identity(), 0.1, 3.0, 4)
        assert not r["rgba"].any() and not r["depth"].any() and np.all(r["tri"] == -1)
        depth, rgba, _, _ = synth.wall_frame(1.0, cam)
        v.integrate_frame_host(depth, rgba, synth.pose_identity().reshape(12), None, 0)  # a volume, still no patch
        v.sync()
        r = v.render_model(synth.pose_identity(), 0.1, 3.0, 2)
        assert not r["rgba"].any() and np.all(r["tri"] == -1)
        v.reset()  # the stream buffers go with the reset; the next render allocates them again
        assert np.all(v.render_model(synth.pose_identity(), 0.1, 3.0, 2)["tri"] == -1)
    finally:
        v.close()
