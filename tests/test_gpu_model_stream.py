"""The model stream resident in the handle (tf_model_stream_*, texturefusion_amd/csrc/tf_model.hip) and tf_render_model on
top of it.  The yardstick for the stream's contents is tf_draw_meshes, which tests/test_gpu_atlas.py holds to the oracle:
counts, vertex words and index words are compared as uint32 -- equal bits, not equal floats.  The yardstick for a render is
tf_render_stream over that stream and the handle's atlas.  Nothing here is arranged to fault: every input is an ordinary
call of the ABI, and the capacity cases are the documented overflow (nothing is written)."""
import ctypes as C

import numpy as np
import pytest

from tests import cc_inputs as CI
from tests import texmap_inputs as TI
from tests.test_gpu_cc_edges import scenes  # noqa: F401  (the fixture that builds the hand-built scene)
from tests.test_render_cpu import wall_scene
from tests.util import RES5, HipBuffer, sorted_ids
from texturefusion_amd import capi, synth

pytestmark = pytest.mark.gpu
IMAGE = 8  # TF_PATCH_HAS_IMAGE


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _d2h(ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    if nbytes:
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0
    return out


def _fetch(gv, n_vertices=None):
    """the control block, and the stream up to the counts it states (or n_vertices vertices), by device copies; the caller
    has synchronised"""
    g = gv.model_stream_get()
    ctl = _d2h(g["counts"], 32).view(np.uint32)
    nv = int(ctl[0]) if n_vertices is None else n_vertices
    assert nv <= g["cap_vertices"] and ctl[1] <= g["cap_indices"]
    V = _d2h(g["vertices"], 48 * nv).view(np.float32).reshape(-1, 12)
    I = _d2h(g["indices"], 4 * int(ctl[1])).view(np.uint32)
    return ctl, V, I


def _assert_current_stream(gv, V, I, what):
    gv.sync()
    ctl, sV, sI = _fetch(gv)
    assert (int(ctl[0]), int(ctl[1])) == (len(V), len(I)), "%s: counts %s" % (what, ctl[:6].tolist())
    assert ctl[3] == 0 and (int(ctl[4]), int(ctl[5])) == (len(V), len(I)) and not ctl[6:].any(), what
    assert np.array_equal(_u32(sV), _u32(V)), "%s: vertex bits differ" % what
    assert np.array_equal(sI, I), "%s: index bits differ" % what
    return ctl


def _assert_update_equals_draw(gv, what):
    V, I = gv.draw_meshes()
    assert gv.model_stream_update() == (len(V), len(I)), what
    ctl = _assert_current_stream(gv, V, I, what)
    return V, I, int(ctl[2])


def _assert_render_equal(got, exp, what):
    assert np.array_equal(got["tri"], exp["tri"]), "%s: triangle ids differ" % what
    assert np.array_equal(_u32(got["depth"]), _u32(exp["depth"])), "%s: depth bits differ" % what
    assert np.array_equal(got["rgba"], exp["rgba"]), "%s: bytes differ" % what


def _fresh_render(gv, pose, near, far, mode):
    V, I = gv.draw_meshes()
    return gv.render_stream(V, I, pose, near, far, mode)  # (texture None = the handle's atlas)


def _render_device(gv, cam, pose, near, far, mode):
    P = cam.width * cam.height
    out = [HipBuffer(4 * P), HipBuffer(4 * P), HipBuffer(4 * P)]
    try:
        gv.render_model_device(pose, near, far, mode, d_rgba=out[0].ptr, d_depth=out[1].ptr, d_tri=out[2].ptr)
        gv.sync()
        return {"rgba": out[0].to_host().reshape(cam.height, cam.width, 4),
                "depth": out[1].to_host().view(np.float32).reshape(cam.height, cam.width),
                "tri": out[2].to_host().view(np.int32).reshape(cam.height, cam.width)}
    finally:
        for b in out:
            b.free()


# ---- 1 + 7: the hand-built clusters ----------------------------------------------------------------------------------
def test_hand_built_clusters(scenes):  # noqa: F811
    S = scenes()
    gv = S.gv
    nv_mesh = np.array([len(m["verts"]) for m in S.sc["meshes"]])
    assert len(nv_mesh) == 568 and {1, 2, 63, 64, 65, 127, 128, 129, 192, 300, 2240} <= set(nv_mesh.tolist()) and (nv_mesh == 0).any()
    V0, I0, np0 = _assert_update_equals_draw(gv, "behind GeneratePatches")
    assert 256 < np0 < 568, "two rank tiles, and the empty meshes are skipped (%d patches)" % np0
    assert (V0[:, 11] != 0).any() and not V0[:, 5].any()  # wrongly mapped patches; no labs yet
    assert gv.compensate_color_device() > 0
    V1, I1, np1 = _assert_update_equals_draw(gv, "behind CompensateColor")
    assert np1 == np0 and (V1[:, 5] != 0).any() and not np.array_equal(_u32(V1), _u32(V0))
    # cluster B's labs are NaN: its one vertex packs a zero delta, 255 per field
    p = gv.get_patches(S.ids)
    b = [i for i, m in enumerate(S.sc["meshes"]) if m["cluster"] == "B"]
    assert len(b) == 1 and np.isnan(p["labs"][p["voff"][b[0]]]).all()
    assert (V1[:, 5] == np.float32((255 << 18) + (255 << 9) + 255)).any()
    # a second run over the same model gives the same bits; release, then update packs again
    packs = gv.model_stream_stats()["packs"]
    assert gv.model_stream_update() == (len(V1), len(I1))
    _assert_current_stream(gv, V1, I1, "second run")
    gv.model_stream_release()
    st = gv.model_stream_stats()
    assert (st["cap_vertices"], st["cap_indices"]) == (0, 0)
    assert gv.L.tf_model_stream_get(gv.h, None, None, None, None, None) == capi.TF_ERR_INVALID
    assert gv.model_stream_update() == (len(V1), len(I1))
    _assert_current_stream(gv, V1, I1, "behind release")
    assert gv.model_stream_stats()["packs"] == packs + 2
    # the scene has no triangle (tf_meshes_upload gave it vertices only), so this half only shows that a stream without
    # indices renders the empty image in every mode, through the stream as through draw_meshes; the rasteriser over a
    # resident stream -- host counts and device counts -- is checked on the wall model and on the one-triangle meshes below
    for mode in (1, 2, 3, 4):
        r = gv.render_model(S.sc["pose"], 0.1, 3.0, mode)
        _assert_render_equal(r, _fresh_render(gv, S.sc["pose"], 0.1, 3.0, mode), "hand-built scene, mode %d" % mode)
        assert np.all(r["tri"] == -1)


# ---- 2 + 3: one-triangle meshes on chunk ids of both signs -----------------------------------------------------------
class Signed:
    """One wall frame seen from a yawed pose that puts the wall across the world's origin: the chunks it marks have ids
    of both signs on all three axes.  Meshes (one triangle on the wall each) go into allMeshes under such ids the way
    tests/test_gpu_patch_borders.py's _upload_hand_meshes puts them there -- tf_meshes_upload, then CompressMeshes marks
    them simplified -- but under ids picked by a fixed-seed shuffle and uploaded in that order."""
    YAW, Z, KF = 0.3, 1.2, 3

    def __init__(self, n_max, seed=11):
        self.cam = cam = synth.Camera()
        self.gv = capi.Volume(RES5, cam, max_chunks=1 << 14, atlas_w=1920, atlas_h=720)
        t = (-np.sin(self.YAW) * self.Z, 0.0, -np.cos(self.YAW) * self.Z)  # the wall's centre at the world's origin
        self.pose = synth.pose_yaw(self.YAW, t)
        self.depth, self.rgba, _, _ = synth.wall_frame(self.Z, cam, pose=self.pose, hole_stride=10 ** 7, seed=0)
        self._mark()
        self.gv.keyframe_cache(self.KF, np.ascontiguousarray(self.rgba[..., :3]), self.depth, synth.pose_inverse16(self.pose))
        have = {tuple(c) for c in self.gv.list_chunks().tolist()}
        marked = sorted_ids([c for c in self.gv.dirty().tolist() if tuple(c) in have])
        # the pixel the chunk's centre projects to, well inside the image
        R, tt = np.asarray(self.pose, np.float64)[:, :3], np.asarray(self.pose, np.float64)[:, 3]
        c = ((marked + 0.5) * (8 * RES5) - tt) @ R
        u, v = cam.fx * c[:, 0] / c[:, 2] + cam.cx, cam.fy * c[:, 1] / c[:, 2] + cam.cy
        ok = (u > 24) & (u < cam.width - 24) & (v > 24) & (v < cam.height - 24)
        cand, u, v = marked[ok], u[ok], v[ok]
        assert len(cand) >= n_max, "%d candidate chunks" % len(cand)
        for k in range(3):
            assert cand[:, k].min() < 0 < cand[:, k].max(), "axis %d: ids %d..%d" % (k, cand[:, k].min(), cand[:, k].max())
        rng = np.random.default_rng(seed)
        ends = [int(f(cand[:, k])) for k in range(3) for f in (np.argmin, np.argmax)]  # both signs on every axis, from 6 meshes on
        order = list(dict.fromkeys(ends + rng.permutation(len(cand)).tolist()))[:n_max]
        rng.shuffle(order)
        self.ids = cand[order]
        px = np.stack([np.stack([u[order] + du, v[order] + dv], -1) for du, dv in ((0, 0), (3, 0), (0, 3))], 1)  # [n, 3, 2]
        pc = np.stack([(px[..., 0] - cam.cx) / cam.fx * self.Z, (px[..., 1] - cam.cy) / cam.fy * self.Z, np.full(px.shape[:2], self.Z)], -1)
        self.verts = (pc @ R.T + tt).astype(np.float32)  # [n, 3, 3]
        self.colors = rng.random((n_max, 3, 3)).astype(np.float32)
        self.done = 0

    def _mark(self):
        self.gv.frame_upload(self.depth, self.rgba, None)
        self.gv.integrate_frame(self.pose, True)

    def add(self, n):
        """the next n meshes, in the shuffled order -> the number of complete() patches the model has now"""
        gv, a, b = self.gv, self.done, self.done + n
        if n:
            if a:
                self._mark()  # (CompressMeshes cleared the dirty set: the chunks are marked again)
            ids = self.ids[a:b]
            if n >= 6 and not a:
                for k in range(3):
                    assert ids[:, k].min() < 0 < ids[:, k].max()
            assert not np.array_equal(ids, sorted_ids(ids)) or n == 1
            N = np.zeros((n * 3, 3), np.float32)
            N[:, 2] = 1
            gv.meshes_upload(ids, 3 * np.arange(n + 1), 3 * np.arange(n + 1), self.verts[a:b].reshape(-1, 3), N,
                             self.colors[a:b].reshape(-1, 3), np.tile(np.arange(3, dtype=np.uint32), n))
            gv.compress_meshes()
            rc, hot = gv.generate_patches(sorted_ids(ids), np.full(n, self.KF, np.int32))
            assert rc == 0
            gv.update_atlas(sorted_ids(ids))
            self.done = b
        if not self.done:
            return 0
        every = sorted_ids(self.ids[:self.done])
        p = gv.get_patches(every)
        simp = gv.get_meshes(every)[7]
        return int((((p["flags"] & IMAGE) > 0) & (p["frameid"] >= 0) & (simp > 0)).sum())

    def close(self):
        self.gv.close()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1025])
def test_counts_and_order(n, gpu_required):
    S = Signed(max(n, 1))
    try:
        gv = S.gv
        complete = S.add(n)
        assert complete == n, "%d of %d patches are complete: the rank tiles the case is about are not all met" % (complete, n)
        V, I, n_patches = _assert_update_equals_draw(gv, "%d meshes" % n)
        print("n = %d: %d complete patches, %d vertices, %d indices" % (n, complete, len(V), len(I)))
        assert (n_patches, len(V), len(I)) == (complete, 3 * complete, 3 * complete)
        r = gv.render_model(S.pose, 0.1, 3.0, 2)
        _assert_render_equal(r, _fresh_render(gv, S.pose, 0.1, 3.0, 2), "%d meshes" % n)
        if n == 0:
            assert gv.model_stream_update() == (0, 0)
            assert not r["rgba"].any() and not r["depth"].any() and np.all(r["tri"] == -1)
        else:
            assert (r["tri"] >= 0).any()
    finally:
        S.close()


N_SMALL, N_BIG = 40, 100


@pytest.fixture(scope="module")
def big_model(gpu_required):
    """what the model of N_BIG meshes packs to, and the exact-capacity case on the way"""
    S = Signed(N_BIG)
    try:
        gv = S.gv
        assert gv.L.tf_model_stream_update_device(gv.h) == capi.TF_ERR_INVALID  # no capacity yet
        gv.sync()
        S.add(N_SMALL)
        S.add(N_BIG - N_SMALL)
        V, I = gv.draw_meshes()
        assert len(V) > 3 * N_SMALL
        gv.model_stream_reserve(len(V), len(I))
        st = gv.model_stream_stats()
        assert (st["cap_vertices"], st["cap_indices"]) == (len(V), len(I))
        gv.model_stream_update_device()
        gv.sync()  # TF_OK: it fits exactly
        _assert_current_stream(gv, V, I, "capacity exactly as needed")
        return V.copy(), I.copy()
    finally:
        S.close()


@pytest.mark.parametrize("short", ["vertex", "index"])
def test_capacity_one_short(short, big_model):
    V, I = big_model
    cap = (len(V) - 1, len(I)) if short == "vertex" else (len(V), len(I) - 1)
    S = Signed(N_BIG)
    try:
        gv = S.gv
        S.add(N_SMALL)
        gv.model_stream_reserve(*cap)
        Vs, Is = gv.draw_meshes()
        assert gv.model_stream_update() == (len(Vs), len(Is)) and 0 < len(Vs) < len(V)
        _assert_current_stream(gv, Vs, Is, "the smaller model")
        S.add(N_BIG - N_SMALL)
        gv.sync()
        assert gv.L.tf_model_stream_update_device(gv.h) == capi.TF_OK
        assert gv.L.tf_sync(gv.h) == capi.TF_ERR_CAPACITY
        ctl, sV, sI = _fetch(gv, n_vertices=len(Vs))
        assert ctl[:3].tolist() == [0, 0, 0] and ctl[3] != 0 and (int(ctl[4]), int(ctl[5])) == (len(V), len(I))
        st = gv.model_stream_stats()
        assert (st["cap_vertices"], st["cap_indices"]) == cap
        g = gv.model_stream_get()
        assert np.array_equal(_u32(sV), _u32(Vs)), "a refused pack wrote vertices"
        assert np.array_equal(_d2h(g["indices"], 4 * len(Is)).view(np.uint32), Is), "a refused pack wrote indices"
        gv.sync()  # the status was reported once
        # recovery: the synchronous form grows the buffers; the handle keeps working
        assert gv.model_stream_update() == (len(V), len(I))
        _assert_current_stream(gv, V, I, "behind the growth")
        st = gv.model_stream_stats()
        assert st["cap_vertices"] >= len(V) and st["cap_indices"] >= len(I)
        assert st["cap_vertices"] & (st["cap_vertices"] - 1) == 0
        r = gv.render_model(S.pose, 0.1, 3.0, 4)
        _assert_render_equal(r, _fresh_render(gv, S.pose, 0.1, 3.0, 4), "behind the growth")
        gv.sync()
    finally:
        S.close()


# ---- 4 + 5: render and cache on the wall model -----------------------------------------------------------------------
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


def test_render_model_equals_render_stream(wall):
    v, cam, frames = wall
    pose = frames[0][2]
    for mode in (1, 2, 3, 4):
        exp = _fresh_render(v, pose, 0.1, 3.0, mode)
        assert (exp["tri"] >= 0).mean() > 0.5
        host = v.render_model(pose, 0.1, 3.0, mode)  # a miss: draw_meshes is no whitelisted reader
        _assert_render_equal(host, exp, "wall, host form, mode %d" % mode)
        _assert_render_equal(_render_device(v, cam, pose, 0.1, 3.0, mode), exp, "wall, device form (a hit), mode %d" % mode)
    # a hit whose counts the host never read: the rasteriser takes them from the control block
    v.draw_meshes()
    v.model_stream_update_device()
    packs = v.model_stream_stats()
    _assert_render_equal(_render_device(v, cam, pose, 0.1, 3.0, 4), exp, "wall, counts on the device")
    after = v.model_stream_stats()
    assert (after["packs"], after["hits"]) == (packs["packs"], packs["hits"] + 1)
    other = synth.pose_yaw(0.3, (0.05, 0.0, 0.1))
    _assert_render_equal(v.render_model(other, 0.1, 3.0, 3), _fresh_render(v, other, 0.1, 3.0, 3), "wall, another pose")


def test_cache_hits_and_misses(wall):
    v, cam, frames = wall
    depth, rgba, pose = frames[0]
    near, far = 0.1, 3.0

    def stats():
        s = v.model_stream_stats()
        return s["packs"], s["hits"]

    def miss(what):
        """the next render packs once more and equals a fresh draw_meshes + render_stream"""
        p0, h0 = stats()
        r = v.render_model(pose, near, far, 4)
        assert stats() == (p0 + 1, h0), "%s: the stream was served stale" % what
        _assert_render_equal(r, _fresh_render(v, pose, near, far, 4), what)
        return r

    v.draw_meshes()
    p0, h0 = stats()
    first = v.render_model(pose, near, far, 4)
    second = v.render_model(pose, near, far, 4)
    assert stats() == (p0 + 1, h0 + 1)
    _assert_render_equal(second, first, "a hit")
    v.sync()
    v.raycast(pose, near, far)
    v.model_stream_get()
    v.model_stream_stats()
    _assert_render_equal(v.render_model(pose, near, far, 3), _fresh_render(v, pose, near, far, 3), "a hit behind readers")
    assert stats() == (p0 + 1, h0 + 2)

    ids = sorted_ids(v.list_meshes())
    # tf_update_atlas alone may hit or miss; the picture is the fresh one either way (texels are read live)
    v.update_atlas(ids[:64])
    _assert_render_equal(v.render_model(pose, near, far, 4), _fresh_render(v, pose, near, far, 4), "behind UpdateAtlas")
    # tf_update_meshes behind an integrate
    d2, c2, _, p2 = synth.wall_frame(1.0, cam, pose=synth.pose_yaw(0.1, (0.02, 0.0, 0.0)), seed=3)
    v.frame_upload(d2, c2, None)
    v.integrate_frame(p2, True)
    v.update_meshes()
    miss("behind UpdateMeshes")
    # tf_generate_patches with another label
    v.compress_meshes()
    v.keyframe_cache(900, np.ascontiguousarray(rgba[..., :3] // 2), depth, synth.pose_inverse16(pose))
    pick = ids[len(ids) // 3:len(ids) // 3 + 200]
    rc, hot = v.generate_patches(pick, np.full(len(pick), 900, np.int32))
    assert rc == 0
    v.update_atlas(pick)
    r = miss("behind GeneratePatches")
    assert not np.array_equal(r["rgba"], first["rgba"])
    # tf_compensate_color_device
    assert v.compensate_color_device() >= 1
    miss("behind CompensateColor")
    # tf_meshes_upload moving one vertex
    one = pick[np.flatnonzero(v.mesh_counts(pick)[0] > 0)[:1]]
    voff, ioff, V, N, Cc, I_, adj, simp = v.get_meshes(one)
    V = V.copy()
    V[0, 2] += 0.002
    v.meshes_upload(one, voff, ioff, V, N, Cc, I_)
    miss("behind tf_meshes_upload")
    # one frame of the textured stream
    bufs = [HipBuffer(depth.nbytes).from_host(depth), HipBuffer(rgba.nbytes).from_host(rgba)]
    try:
        v.stream_frames_textured_device([bufs[0].ptr], [bufs[1].ptr], pose.reshape(1, 12), synth.pose_inverse16(pose).reshape(1, 16), 50)
        miss("behind a textured stream frame")
        v.sync()
    finally:
        for b in bufs:
            b.free()
    # tf_volume_reset: the buffers go, the image is empty
    v.reset()
    st = v.model_stream_stats()
    assert (st["cap_vertices"], st["cap_indices"]) == (0, 0)
    r = miss("behind tf_volume_reset")
    assert not r["rgba"].any() and not r["depth"].any() and np.all(r["tri"] == -1)


# ---- 6: the keyframe flow, nothing waiting between the tail and the pack --------------------------------------------
def _tail_run(gv, behind_tail):
    plain = gv.texture_tail

    def tail(*a, **kw):
        plain(*a, compensate_color=True, **kw)
        behind_tail()  # (nothing between the tail's return and this)

    gv.texture_tail = tail
    return TI.Run(gv, unit=True, tail=True, extra=False)


def test_keyframe_flow_without_waits(gpu_required):
    gv = capi.Volume(TI.RES8, TI.CAM, max_chunks=1 << 15)
    gv.model_stream_reserve(1 << 20, 3 << 20)  # once, up front
    run = _tail_run(gv, gv.model_stream_update_device)
    pose = synth.pose_identity()
    try:
        for i in range(4):
            p0 = gv.model_stream_stats()["packs"]
            run.step(i)
            assert gv.model_stream_stats()["packs"] == p0 + 1
            gv.sync()
            ctl, sV, sI = _fetch(gv)
            V, I = gv.draw_meshes()
            assert len(V) > 0 and len(I) > 0, i
            assert (int(ctl[0]), int(ctl[1]), int(ctl[3])) == (len(V), len(I), 0), i
            assert np.array_equal(_u32(sV), _u32(V)) and np.array_equal(sI, I), "step %d" % i
            gv.model_stream_update_device()  # (draw_meshes was the yardstick, and is no reader)
            s0 = gv.model_stream_stats()
            got = _render_device(gv, TI.CAM, pose, 0.1, 4.0, 3)
            s1 = gv.model_stream_stats()
            assert (s1["packs"], s1["hits"]) == (s0["packs"], s0["hits"] + 1), "step %d: the render was no hit" % i
            _assert_render_equal(got, _fresh_render(gv, pose, 0.1, 4.0, 3), "step %d" % i)
    finally:
        run.close()
        gv.close()


def test_cache_miss_behind_unit_and_tail(gpu_required):
    gv = capi.Volume(TI.RES8, TI.CAM, max_chunks=1 << 15)
    gv.model_stream_reserve(1 << 20, 3 << 20)  # (room for both steps: a pack that has to grow the buffers runs twice)
    run = _tail_run(gv, lambda: None)
    pose = synth.pose_identity()
    try:
        run.step(0)
        gv.render_model(pose, 0.1, 4.0, 4)
        s0 = gv.model_stream_stats()
        gv.render_model(pose, 0.1, 4.0, 4)
        s1 = gv.model_stream_stats()
        assert (s1["packs"], s1["hits"]) == (s0["packs"], s0["hits"] + 1)
        run.step(1)  # tf_keyframe_unit_device + tf_texture_tail_device
        r = gv.render_model(pose, 0.1, 4.0, 4)
        s2 = gv.model_stream_stats()
        assert (s2["packs"], s2["hits"]) == (s1["packs"] + 1, s1["hits"])
        _assert_render_equal(r, _fresh_render(gv, pose, 0.1, 4.0, 4), "behind unit + tail")
    finally:
        run.close()
        gv.close()
