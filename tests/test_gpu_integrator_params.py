"""The device integrator under non-default truncation and weight (tf_set_truncation / tf_set_weight) against the oracle
built with the same integrator (MobileFusion.h:236-249: QuadraticTruncator(quad, linear, const, scale) and
ConstantWeighter(weight)), bit for bit: chunk lists, every voxel's sdf / weight / colour bits, meshes, patches and atlas
rows where the flow has them.  The parameter grid and the oracle flows are in tests/integrator_params.py; the CPU
companion (tests/test_integrator_params_cpu.py) checks that every case changes the voxels against the default and gives
no NaN, so that a plain bit comparison is the right one everywhere here.

Flows: the call-by-call flow (colour and depth only) with de-integration; the streamed entry point with and without
frames selected ahead (n_ahead); the textured per-frame unit; the keyframe-group kernel and the keyframe unit; the order
of setters against frames already handed over; the readers (point queries, distance from surface, refinement, the
raycaster) on volumes fused under such an integrator.

When a setter takes effect (the rule the device must follow, as the oracle does): a frame is integrated under the
integrator in effect when the call that hands it over is made, whatever the library has staged or selected ahead of
it.  In the call-by-call flow the selection (tf_prepare: tfo_select, the positive band) reads the truncation when
tf_prepare runs, and K-A (tf_integrate: tfo_voxel_update) reads truncation and weight when tf_integrate runs -- a setter
between the two changes the voxel update of that frame, not the list it was given."""
import numpy as np
import pytest

from oracle import api as O
from texturefusion_amd import capi, synth
from tests import integrator_params as P
from tests import refine_ref
from tests.raycast_ref import RefVolume
from tests.test_gpu_atlas import _compare_atlas, _compare_patches
from tests.test_gpu_raycast import SMALL, _assert_query_equal
from tests.test_gpu_unit import _oracle_group
from tests.util import RES5, HipBuffer, assert_chunks_equal, sorted_ids

pytestmark = pytest.mark.gpu
F = np.float32
CASE_ID = lambda c: "set%d-w%g" % c


def _device(case, max_chunks=1 << 16, **kw):
    gv = capi.Volume(RES5, P.CAM, max_chunks=max_chunks, **kw)
    set_integrator(gv, case)
    return gv


def set_integrator(gv, case):
    k, w = case
    gv.set_truncation(*[F(p) for p in P.SETS[k]])
    gv.set_weight(F(w))


def _assert_volumes_equal(ov, gv, what):
    ids = sorted_ids(ov.list_chunks())
    assert len(ids) > 1000, what
    assert np.array_equal(ids, sorted_ids(gv.list_chunks())), "%s: chunk lists differ" % what
    assert_chunks_equal(ov, gv, ids, what)
    return ids


def _assert_meshes_equal(ov, gv, what):
    mids = sorted_ids(ov.list_meshes())
    assert len(mids) > 100, what
    assert np.array_equal(mids, sorted_ids(gv.list_meshes())), "%s: mesh lists differ" % what
    voff, ioff, V, N, Cc, I, adj, simp = gv.get_meshes(mids)
    for i, cid in enumerate(mids):
        m = ov.get_mesh(cid)
        assert np.array_equal(V[voff[i]:voff[i + 1]].view(np.uint32), m["verts"].view(np.uint32)), (what, cid)
        assert np.array_equal(N[voff[i]:voff[i + 1]].view(np.uint32), m["normals"].view(np.uint32)), (what, cid)
        assert np.array_equal(I[ioff[i]:ioff[i + 1]], m["indices"]), (what, cid)
        assert bool(simp[i]) == m["simplified"] and np.array_equal(adj[i], m["adj"]), (what, cid)
    return mids


def _buffers(frames):
    return [(HipBuffer(f[0].nbytes).from_host(f[0]), HipBuffer(f[1].nbytes).from_host(f[1])) for f in frames]


def _free(bufs):
    for t in bufs:
        for b in t:
            if b is not None:
                b.free()


# ---- 1. the call-by-call flow --------------------------------------------------------------------------------------
def _frame_both(ov, gv, frame, color, kf_id):
    """prepare -> integrate -> finalize on both sides, compared after each call"""
    depth, rgba, quality, pose = frame
    oids, onew = ov.prepare(depth, pose)
    gv.frame_upload(depth, rgba if color else None, quality if color else None)
    gids, gnew = gv.prepare(pose)
    assert np.array_equal(oids, gids) and np.array_equal(onew, gnew), "visible-chunk list differs"
    on, gn = np.zeros(len(oids), np.uint8), np.zeros(len(oids), np.uint8)
    oq = ov.integrate(depth, rgba if color else None, quality if color else None, pose, oids, on, 1, kf_id)
    gq = gv.integrate(pose, gids, gn, 1, color, color)
    assert np.array_equal(on, gn), "needsUpdate differs"
    assert np.array_equal(oq.view(np.uint32), gq.view(np.uint32)), "chunkObservationQuality differs"
    assert_chunks_equal(ov, gv, oids, "after integrate")
    ovalid, gvalid = ov.finalize(oids, on, onew), gv.finalize(gids, gn, gnew)
    assert np.array_equal(ovalid, gvalid), "validChunks differs"
    return ovalid


@pytest.mark.parametrize("color", [True, False], ids=["colour", "depth_only"])
@pytest.mark.parametrize("case", P.CALL_BY_CALL, ids=CASE_ID)
def test_call_by_call_and_deintegration(gpu_required, case, color):
    """tf_prepare + tf_integrate + tf_finalize over the room frames, then the first two frames de-integrated over their
    validChunks (integrateFlag 0: K-A negates weight / (2 truncation)); the residual weights must be the oracle's bits"""
    ov, gv = P.oracle_volume(case), _device(case)
    frames = [P.room(k) for k in P.ROOM_FRAMES]
    valids = [_frame_both(ov, gv, f, color, k) for k, f in enumerate(frames)]
    for k in (0, 1):
        depth, rgba, quality, pose = frames[k]
        on = P.deintegrate(ov, frames[k], valids[k], color, k)
        gn = np.ones(len(valids[k]), np.uint8)
        gv.frame_upload(depth, rgba if color else None, quality if color else None)
        gv.integrate(pose, valids[k], gn, 0, color, color)
        assert np.array_equal(on, gn), "needsUpdate of the de-integration differs"
        assert_chunks_equal(ov, gv, valids[k], "de-integrated frame %d" % k)
    ids = _assert_volumes_equal(ov, gv, "call by call %s" % (case,))
    assert np.array_equal(sorted_ids(ov.dirty()), sorted_ids(gv.dirty()))
    if case[1] in P.DEINTEGRATE_WEIGHTS:
        _, w, _ = gv.get_chunks(ids)
        assert ((w > 0) & (w != np.round(w))).sum() > 1000  # residual weights that are not round numbers
    P.assert_differs(ov, P.oracle_call_by_call(P.DEFAULT, color), "call by call %s" % (case,))
    gv.close()


# ---- 2. the streamed entry point -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ahead", [0, 2])
@pytest.mark.parametrize("case", P.STREAMED, ids=CASE_ID)
def test_streamed_frames(gpu_required, case, n_ahead):
    """tf_stream_frames_device in two calls, the first leaving n_ahead frames selected ahead (K-C records hold
    weight / (2 truncation)) for the second"""
    ov, gv = P.oracle_stream(case), _device(case)
    frames = [P.room(k, quality=False) for k in P.STREAM_FRAMES]
    bufs = _buffers(frames)
    poses = np.stack([f[3].reshape(12) for f in frames])
    dd, dc = [b[0].ptr for b in bufs], [b[1].ptr for b in bufs]
    gv.stream_frames_device(dd[0:3 + n_ahead], dc[0:3 + n_ahead], poses[0:3 + n_ahead], n_ahead=n_ahead)
    gv.stream_frames_device(dd[3:], dc[3:], poses[3:])
    gv.sync()
    _assert_volumes_equal(ov, gv, "streamed %s" % (case,))
    assert np.array_equal(sorted_ids(ov.dirty()), sorted_ids(gv.dirty()))
    P.assert_differs(ov, P.oracle_stream(P.DEFAULT), "streamed %s" % (case,))
    _free(bufs)
    gv.close()


# ---- 3. the textured per-frame unit --------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["host", "stream"])
@pytest.mark.parametrize("case", P.TEXTURED, ids=CASE_ID)
def test_textured_unit(gpu_required, case, entry):
    """integrate -> UpdateMeshes -> CompressMeshes -> GeneratePatches -> UpdateAtlas per frame; with weight 3 the w > 50
    class (K-A's ballots, the mesher's cell test) is reached from the second frame on"""
    ov, oa = P.oracle_textured(case)
    gv = _device(case, max_chunks=1 << 17, max_list=1 << 17)
    frames = [P.room(k, quality=False) for k in P.TEXTURED_FRAMES]
    pinv = [synth.pose_inverse16(f[3]) for f in frames]
    bufs = []
    if entry == "host":
        for i, f in enumerate(frames):
            gv.integrate_frame_host(f[0], f[1], f[3].reshape(12), pinv[i], 10 + i)
    else:
        bufs = _buffers(frames)
        gv.stream_frames_textured_device([b[0].ptr for b in bufs], [b[1].ptr for b in bufs],
                                         np.stack([f[3].reshape(12) for f in frames]), np.stack(pinv), 10)
    gv.sync()
    ids = _assert_volumes_equal(ov, gv, "textured %s" % (case,))
    mids = _assert_meshes_equal(ov, gv, "textured %s" % (case,))
    assert gv.atlas_loc_next() == oa.loc_next()
    _compare_patches(ov, gv, mids, "textured %s" % (case,))
    g = gv.get_patches(mids)
    used = g["texloc"][g["texloc"] != np.uint64((1 << 64) - 1)]
    assert len(used) > 0
    _compare_atlas(oa, gv, oa.hot_range(used))
    if case[1] == 3.0:
        _, w, _ = gv.get_chunks(ids)
        assert (w > 50).sum() > 100000
    _free(bufs)
    gv.close()


# ---- 4. the keyframe-group kernel and the keyframe unit ------------------------------------------------------------
def test_keyframe_group_kernel(gpu_required):
    """tf_integrate_depth_group_host (local frames in one visit per chunk, records from the group kernel's own chunk_pre)
    against the oracle's frame-after-frame IntegrateDepthScanColor, then the group de-integrated again"""
    case = P.KEYFRAME
    ov, gv = P.oracle_volume(case), _device(case)
    kf = P.room(10)
    local = [P.room(k, quality=False, wobble=0.03) for k in (11, 12, 13)]
    depth, rgba, quality, pose = kf
    oids, onew = ov.prepare(depth, pose)
    gv.frame_upload(depth, rgba, quality)
    gids, gnew = gv.prepare(pose)
    assert np.array_equal(oids, gids) and np.array_equal(onew, gnew)
    on, gn = np.zeros(len(oids), np.uint8), np.zeros(len(oids), np.uint8)
    ov.integrate(depth, rgba, quality, pose, oids, on, 1, 40)
    gv.integrate(pose, gids, gn, 1, True, True)
    for f in local:
        ov.integrate(f[0], None, None, f[3], oids, on, 1, -1)
    poses = np.stack([f[3].reshape(12) for f in local])
    gv.integrate_depth_group_host([f[0] for f in local], poses, gids, gn, 1)
    assert np.array_equal(on, gn), "needsUpdate flags after the group"
    ovalid, gvalid = ov.finalize(oids, on, onew), gv.finalize(gids, gn, gnew)
    assert np.array_equal(ovalid, gvalid)
    ids = _assert_volumes_equal(ov, gv, "keyframe group")
    dn_o, dn_g = np.ones(len(ovalid), np.uint8), np.ones(len(ovalid), np.uint8)
    for f in local:
        ov.integrate(f[0], None, None, f[3], ovalid, dn_o, 0, -1)
    gv.integrate_depth_group_host([f[0] for f in local], poses, gvalid, dn_g, 0)
    assert np.array_equal(dn_o, dn_g)
    assert_chunks_equal(ov, gv, ids, "keyframe group de-integrated")
    od = P.oracle_volume(P.DEFAULT)
    dvalid = _oracle_group(od, 40, kf, [(f[0], f[3]) for f in local], 1)
    for f in local:
        od.integrate(f[0], None, None, f[3], dvalid, np.ones(len(dvalid), np.uint8), 0, -1)
    P.assert_differs(ov, od, "keyframe group")
    gv.close()


def test_keyframe_unit(gpu_required):
    """tf_keyframe_unit_device: a keyframe group, then a second one with the first MOVED (de-integrated at its old poses,
    integrated at new ones), textured -- against the oracle's call-by-call sequence (tests/test_gpu_unit.py)"""
    case = P.KEYFRAME
    ov, gv = P.oracle_volume(case), _device(case)
    oa = O.Atlas(RES5)
    fr = [P.room(k) for k in range(11)]
    bufs = [(HipBuffer(f[0].nbytes).from_host(f[0]), HipBuffer(f[1].nbytes).from_host(f[1]),
             HipBuffer(f[2].nbytes).from_host(f[2])) for f in fr]
    key = lambda k, pose: (bufs[k][0].ptr, bufs[k][1].ptr, bufs[k][2].ptr, pose)
    A_loc, B_loc = [1, 2, 3], [7, 8, 9, 10]

    def oracle_side(ov, oa):
        validA = _oracle_group(ov, 5, fr[0], [(fr[k][0], fr[k][3]) for k in A_loc], 1)
        ov.update_meshes()
        ids = ov.compress_meshes()
        kfs = {5: (np.ascontiguousarray(fr[0][1][..., :3]), fr[0][0], synth.pose_inverse16(fr[0][3]))}
        ov.generate_patches(oa, ids, np.full(len(ids), 5, np.int32), kfs)
        ov.update_atlas(oa, ids)
        ov.retract_observations(5, validA)
        _oracle_group(ov, 5, fr[0], [(fr[k][0], fr[k][3]) for k in A_loc], 0, ids=validA)
        movedA = (fr[0][0], fr[0][1], fr[0][2], newA[0])
        _oracle_group(ov, 5, movedA, [(fr[k][0], newA[1 + i]) for i, k in enumerate(A_loc)], 1)
        _oracle_group(ov, 9, fr[6], [(fr[k][0], fr[k][3]) for k in B_loc], 1)
        ov.update_meshes()
        ids = ov.compress_meshes()
        kfs[9] = (np.ascontiguousarray(fr[6][1][..., :3]), fr[6][0], synth.pose_inverse16(fr[6][3]))
        ov.generate_patches(oa, ids, np.full(len(ids), 9, np.int32), kfs)
        ov.update_atlas(oa, ids)

    newA = [fr[k + 1][3] for k in [0] + A_loc]
    gA = capi.Volume.unit_group(5, key(0, fr[0][3]), [(bufs[k][0].ptr, fr[k][3]) for k in A_loc])
    gv.keyframe_unit(fresh=gA, texture=True, pose_inv16=synth.pose_inverse16(fr[0][3]))
    gB = capi.Volume.unit_group(9, key(6, fr[6][3]), [(bufs[k][0].ptr, fr[k][3]) for k in B_loc])
    gA2 = capi.Volume.unit_group(5, key(0, newA[0]), [(bufs[k][0].ptr, newA[1 + i]) for i, k in enumerate(A_loc)],
                                 old_keyframe_pose=fr[0][3], old_local_poses=[fr[k][3] for k in A_loc])
    gv.keyframe_unit(fresh=gB, moved=[gA2], texture=True, pose_inv16=synth.pose_inverse16(fr[6][3]))
    oracle_side(ov, oa)
    gv.sync()
    oids = _assert_volumes_equal(ov, gv, "keyframe unit")
    want = np.zeros((len(oids), 2), np.float32)
    for i, cid in enumerate(oids):
        obs = ov.observations(cid)
        want[i] = [obs.get(9, 0.0), obs.get(5, 0.0)]
    got = gv.export_datacost(oids, 9, [5])
    assert np.array_equal(want.view(np.uint32), got.view(np.uint32))
    mids = _assert_meshes_equal(ov, gv, "keyframe unit")
    assert gv.atlas_loc_next() == oa.loc_next()
    _compare_patches(ov, gv, mids, "keyframe unit")
    g = gv.get_patches(mids)
    used = g["texloc"][g["texloc"] != np.uint64((1 << 64) - 1)]
    assert len(used) > 0
    _compare_atlas(oa, gv, oa.hot_range(used))
    assert len(gv.dirty()) == 0 and len(ov.dirty()) == 0
    od = P.oracle_volume(P.DEFAULT)
    oracle_side(od, O.Atlas(RES5))
    P.assert_differs(ov, od, "keyframe unit")
    _free(bufs)
    gv.close()


# ---- 5. setters against frames already handed over -----------------------------------------------------------------
def _switch(setter):
    """(the integrator after the setter, a function applying the setter to the device)"""
    if setter == "weight":
        return (0, P.SETTER_WEIGHT), lambda gv: gv.set_weight(F(P.SETTER_WEIGHT))
    return (P.SETTER_TRUNCATION, 1.0), lambda gv: gv.set_truncation(*[F(p) for p in P.SETS[P.SETTER_TRUNCATION]])


@pytest.mark.parametrize("setter", ["weight", "truncation"])
def test_setter_after_frames_selected_ahead(gpu_required, setter):
    """Frames 0..2 streamed with frames 3 and 4 selected ahead (n_ahead = 2), the setter, then frames 3..6 streamed: the
    oracle integrates frames 3.. under the new integrator, and so must the device -- frame 3's list records, made ahead
    under the old one, must not be used"""
    after, apply = _switch(setter)
    ov = P.oracle_volume(P.DEFAULT)
    frames = [P.room(k, quality=False) for k in P.STREAM_FRAMES]
    for k, f in enumerate(frames):
        if k == 3:
            ov.set_integrator(P.integrator(after))
        ov.integrate_frame(f[0], f[1], f[3])
    gv = _device(P.DEFAULT)
    bufs = _buffers(frames)
    poses = np.stack([f[3].reshape(12) for f in frames])
    dd, dc = [b[0].ptr for b in bufs], [b[1].ptr for b in bufs]
    gv.stream_frames_device(dd[0:5], dc[0:5], poses[0:5], n_ahead=2)
    apply(gv)
    gv.stream_frames_device(dd[3:], dc[3:], poses[3:])
    gv.sync()
    _assert_volumes_equal(ov, gv, "%s set after frames selected ahead" % setter)
    P.assert_differs(ov, P.oracle_stream(P.DEFAULT), "setter %s" % setter)
    _free(bufs)
    gv.close()


@pytest.mark.parametrize("setter", ["weight", "truncation"])
def test_setter_between_deferred_host_frames(gpu_required, setter):
    """tf_integrate_frame_host defers its frames (they go to the device calls later); a setter between two frames still
    splits the stream where the caller made the call"""
    after, apply = _switch(setter)
    ov = P.oracle_volume(P.DEFAULT)
    gv = _device(P.DEFAULT)
    for k in P.STREAM_FRAMES:
        f = P.room(k, quality=False)
        if k == 4:
            ov.set_integrator(P.integrator(after))
            apply(gv)
        ov.integrate_frame(f[0], f[1], f[3])
        gv.integrate_frame_host(f[0], f[1], f[3].reshape(12), None, k)
    gv.sync()
    _assert_volumes_equal(ov, gv, "%s set between host frames" % setter)
    gv.close()


@pytest.mark.parametrize("setter", ["weight", "truncation"])
def test_setter_between_prepare_and_integrate(gpu_required, setter):
    """tf_prepare selects under the old truncation, tf_integrate updates the voxels under the new integrator"""
    after, apply = _switch(setter)
    ov = P.oracle_volume(P.DEFAULT)
    gv = _device(P.DEFAULT)
    _frame_both(ov, gv, P.room(0), True, 0)
    depth, rgba, quality, pose = P.room(1)
    oids, onew = ov.prepare(depth, pose)
    gv.frame_upload(depth, rgba, quality)
    gids, gnew = gv.prepare(pose)
    assert np.array_equal(oids, gids) and np.array_equal(onew, gnew)
    ov.set_integrator(P.integrator(after))
    apply(gv)
    on, gn = np.zeros(len(oids), np.uint8), np.zeros(len(oids), np.uint8)
    oq = ov.integrate(depth, rgba, quality, pose, oids, on, 1, 1)
    gq = gv.integrate(pose, gids, gn, 1, True, True)
    assert np.array_equal(on, gn) and np.array_equal(oq.view(np.uint32), gq.view(np.uint32))
    assert np.array_equal(ov.finalize(oids, on, onew), gv.finalize(gids, gn, gnew))
    _frame_both(ov, gv, P.room(2), True, 2)
    _assert_volumes_equal(ov, gv, "%s set between prepare and integrate" % setter)
    gv.close()


# ---- 6. the readers on a volume fused under such an integrator -----------------------------------------------------
@pytest.mark.parametrize("case", P.READERS, ids=CASE_ID)
def test_readers(gpu_required, case):
    """tf_query_points (the weight output: w > 0), tf_distance_from_surface (weight-averaged corners), tf_refine_frame
    (w > 1e-12) and the raycaster against their numpy restatements, on the hand-held room fused under the case"""
    ov, gv = P.oracle_volume(case), _device(case, max_chunks=1 << 17)
    frames = [P.room(k, quality=False, wobble=0.1) for k in P.READER_FRAMES]
    for k, (depth, rgba, _, pose) in enumerate(frames):
        ov.integrate_frame(depth, rgba, pose)
        gv.integrate_frame_host(depth, rgba, pose.reshape(12), None, k)
    gv.sync()
    _assert_volumes_equal(ov, gv, "readers %s" % (case,))
    ids = gv.list_chunks()
    ref = RefVolume.from_volume(gv, ids, gv.res)
    rng = np.random.default_rng(17)
    e = 8 * float(RES5)
    near = (ids[rng.integers(0, len(ids), 60000)] + rng.uniform(0, 1, (60000, 3))) * e
    rnd = rng.uniform(ids.min(0) * e - 0.05, (ids.max(0) + 1) * e + 0.05, (40000, 3))
    pts = np.concatenate([near, rnd]).astype(np.float32)
    got, exp = gv.query(pts), ref.query(pts)
    _assert_query_equal(got, exp)
    assert (exp["flags"] & 2).sum() > 10000  # weights read
    d, tw = gv.distance_from_surface(pts)
    ed, etw = refine_ref.surface_dist(ref, pts)
    assert np.array_equal(d.view(np.uint32), ed.view(np.uint32)) and np.array_equal(tw.view(np.uint32), etw.view(np.uint32))
    assert (etw > 0).sum() > 10000
    depth, _, _, pose = frames[len(frames) // 2]
    noisy = np.where(depth > 0, depth + rng.uniform(-0.003, 0.003, depth.shape).astype(F), depth).astype(F)
    gd, gw = gv.refine_frame(noisy, pose)
    xd, xw = refine_ref.refine_frame(ref, noisy, pose, P.CAM)
    assert np.array_equal(gd.view(np.uint32), xd.view(np.uint32)) and np.array_equal(gw.view(np.uint32), xw.view(np.uint32))
    assert (xw > 0).mean() > 0.1
    gv.raycast_camera(SMALL)
    try:
        r = gv.raycast(pose, 0.1, 5.0, 2048)
    finally:
        gv.raycast_camera(None)
    xr = ref.raycast_depth(pose, SMALL.fx, SMALL.fy, SMALL.cx, SMALL.cy, SMALL.width, SMALL.height, 0.1, 5.0, 2048)
    assert np.array_equal(r["depth"] > 0, xr > 0), "hit masks differ at %d pixels" % ((r["depth"] > 0) != (xr > 0)).sum()
    assert np.abs(r["depth"] - xr).max() <= 1e-4 and (xr > 0).mean() > 0.1
    od = P.oracle_volume(P.DEFAULT)
    for depth, rgba, _, pose in frames:
        od.integrate_frame(depth, rgba, pose)
    P.assert_differs(ov, od, "readers %s" % (case,))
    gv.close()
