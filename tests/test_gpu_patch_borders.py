"""The patch stage -- patch_body<PROJECT, BLIT, FUSED>, texturefusion_amd/csrc/tf_patch_body.h: Patch::CalculateTexCoords /
bilinear / bilinear_depth / SetImage and Atlas::UpdateBuffer (Structure/Patch.cpp:40-175, Structure/Atlas.cpp:71-91) --
at and beyond the keyframe image's borders, in the three kernels that carry it, bit for bit against the oracle:

  (a) k_patch behind tf_generate_patches / tf_update_atlas, on hand-made meshes (tf_meshes_upload) whose vertices are
      back-projected from chosen image positions: on, around and beyond every edge and corner, behind the camera, in the
      plane z == 0; 0 .. 2240 vertices per mesh; three cameras, both slot sizes, keyframes cached from the host and
      borrowed on the device (strides 3 and 4);
  (b) k_frame's patch range and k_patch<true, true, true> behind the fused per-frame entry points, with a pose_inv16
      that is not the integration pose's (turned, pitched, shifted, looking away, centre inside the surface);
  (c) k_mesh_filter's patch range behind tf_keyframe_unit_device(texture = 1) with a turned pose_inv16;
  (d) after each: an honest call through the same handle, compared the same way -- nothing was left behind;
  and the projections that are not a number.

The inputs come from tests/patch_inputs.py; tests/test_patch_cpu.py holds the census conditions that say which
branches they take.  Device images sit inside larger buffers between guard bands of a row and a pixel (0xA5 bytes, 1e9
for the depth): the oracle reads 0 outside the image, so a device read outside it shows as a different texcolor or a
flipped depth compare instead of going unnoticed; the bands are read back after every case.  Nothing here is arranged
to fault."""
import itertools

import numpy as np
import pytest

from oracle import api as O
from tests import patch_inputs as PI
from tests import patch_ref as PR
from tests.test_gpu_atlas import _compare_atlas, _compare_patches
from tests.util import HipBuffer, assert_chunks_equal, sorted_ids
from texturefusion_amd import capi, synth

pytestmark = pytest.mark.gpu
NO_SLOT = (1 << 64) - 1
AW, AH = 1920, 720  # atlas of the call-by-call cases: 80 x 40 slots of 24 x 18, 40 x 20 of 48 x 36


class Guarded:
    """A device image in the middle of a larger buffer, between two guard bands of at least one image row plus one
    pixel, filled with 0xA5 bytes (colour) or 1e9 (depth)."""

    def __init__(self, image):
        image = np.ascontiguousarray(image)
        row = image.strides[0] + image.strides[1]  # one row and one pixel, in bytes
        self.guard = (row + 255) // 256 * 256
        host = np.empty(2 * self.guard + image.nbytes, np.uint8)
        if image.dtype == np.float32:
            host.view(np.float32)[:] = np.float32(1e9)
        else:
            host[:] = 0xA5
        host[self.guard:self.guard + image.nbytes] = image.reshape(-1).view(np.uint8)
        self.host = host
        self.buf = HipBuffer(host.nbytes).from_host(host)
        self.ptr = self.buf.ptr + self.guard

    def check_and_free(self, what):
        back = self.buf.to_host()
        self.buf.free()
        assert np.array_equal(back, self.host), "%s: a guard band or the image was written" % what


# ---------------------------------------------------------------------------------------------------------------------
# (a) call by call, hand-made meshes
# ---------------------------------------------------------------------------------------------------------------------
class AtlasModel:
    """Chisel::GeneratePatches / UpdateAtlas (Structure/Chisel.cpp:149-196) on meshes the oracle's volume does not hold:
    Atlas::AddPatch on first sight, Patch::clear + CalculateTexCoords + SetFrameid + SetImage, UpdateBuffer for complete
    patches -- from the oracle's own pieces (O.Atlas.alloc / blit, O.patch_project)."""

    def __init__(self, case):
        self.case = case
        self.atlas = O.Atlas(case["res"], AW, AH)
        self.cam = O.camera_from(case["cam"])
        self.p = {}

    def generate(self, order, labels):
        for i, lab in zip(order, labels):
            m = self.case["meshes"][i]
            if i not in self.p:
                rc, tl = self.atlas.alloc()
                assert rc == 0
                self.p[i] = dict(texloc=tl)
            rgb, depth, alpha, pose = self.case["keyframes"][int(lab)]
            r = O.patch_project(m["verts"], m["colors"], synth.pose_inverse16(pose), rgb, depth, self.cam)
            self.p[i].update(frameid=int(lab), bbox=r["bbox"], texcoord=r["texcoord"], texcolor=r["texcolor"],
                             flags=1 | 8 | (2 if r["flag"] < 0 else 0) | (4 if r["wrong_mapping"] else 0),
                             ratio=np.ones(2, np.float32))

    def update(self, order):
        for i in order:
            p = self.p[i]
            if len(self.case["meshes"][i]["verts"]) == 0:
                continue  # Patch::complete (Patch.cpp:191-196)
            rc, p["ratio"] = self.atlas.blit(p["texloc"], self.case["keyframes"][p["frameid"]][0], p["bbox"], p["ratio"])
            assert rc == 0

    def compare(self, gv, ids, what):
        g = gv.get_patches(ids)
        for i in range(len(ids)):
            tag = "%s: mesh %d (%s, %d vertices)" % (what, i, self.case["meshes"][i]["theme"],
                                                     len(self.case["meshes"][i]["verts"]))
            o = self.p.get(i)
            if o is None:
                assert int(g["texloc"][i]) == NO_SLOT and not (g["flags"][i] & 1), tag
                continue
            a, b = g["voff"][i], g["voff"][i + 1]
            assert int(g["texloc"][i]) == o["texloc"], tag
            assert g["frameid"][i] == o["frameid"], tag
            assert (int(g["flags"][i]) & 31) == o["flags"], "%s: flags %d vs %d" % (tag, g["flags"][i], o["flags"])
            assert np.array_equal(g["bbox"][i], o["bbox"]), "%s: bbox %s vs %s" % (tag, g["bbox"][i], o["bbox"])
            assert np.array_equal(g["ratio"][i].view(np.uint32), o["ratio"].view(np.uint32)), tag
            assert b - a == len(o["texcoord"]), tag
            assert np.array_equal(g["texcoord"][a:b].view(np.uint32), o["texcoord"].view(np.uint32)), tag + ": texcoord"
            assert np.array_equal(g["texcolor"][a:b].view(np.uint32), o["texcolor"].view(np.uint32)), tag + ": texcolor"
        return g

    def compare_atlas(self, gv):
        used = np.array([p["texloc"] for p in self.p.values()], np.uint64)
        hot = self.atlas.hot_range(used)
        r0, r1 = hot[0] // AW, hot[1] // AW
        assert r1 > r0
        assert np.array_equal(gv.atlas_rows(r0, r1, AW), self.atlas.buffer()[r0:r1]), "atlas rows %d..%d differ" % (r0, r1)
        return r0, r1


def _upload_hand_meshes(gv, cam, meshes):
    """Puts the meshes into allMeshes under the ids of chunks one integrated wall frame has just marked, and has
    CompressMeshes mark them simplified (Patch::complete asks for it) -> their chunk ids, ascending."""
    d, rgba, q, pose = synth.wall_frame(1.2, cam, seed=0)
    gv.frame_upload(d, rgba, None)
    gv.integrate_frame(pose, True)
    have = {tuple(c) for c in gv.list_chunks().tolist()}
    marked = sorted_ids([c for c in gv.dirty().tolist() if tuple(c) in have])
    assert len(marked) >= len(meshes), "the wall marks %d chunks, %d meshes to place" % (len(marked), len(meshes))
    ids = marked[:len(meshes)]
    nv = [len(m["verts"]) for m in meshes]
    voff = np.concatenate([[0], np.cumsum(nv)]).astype(np.int64)
    ioff = np.zeros(len(meshes) + 1, np.int64)
    V = np.concatenate([m["verts"] for m in meshes]).astype(np.float32)
    Cc = np.concatenate([m["colors"] for m in meshes]).astype(np.float32)
    N = np.zeros_like(V)
    N[:, 2] = 1
    gv.meshes_upload(ids, voff, ioff, V, N, Cc, np.zeros(1, np.uint32)[:0])
    listed = gv.compress_meshes()
    assert np.array_equal(sorted_ids(listed), ids), "CompressMeshes lists every uploaded mesh"
    v2, i2, V2, N2, C2, I2, adj, simp = gv.get_meshes(ids)
    assert np.array_equal(v2, voff) and np.array_equal(V2.view(np.uint32), V.view(np.uint32)) and simp.all()
    return ids


def _cache_keyframes(gv, case, source):
    """-> the guarded device buffers (none when the keyframes are cached from the host)"""
    guards = []
    for kid, (rgb, depth, alpha, pose) in case["keyframes"].items():
        T = synth.pose_inverse16(pose)
        if source == "host":
            gv.keyframe_cache(kid, rgb, depth, T)
            continue
        img = rgb if source == "device3" else np.concatenate([rgb, alpha], -1)
        gc, gd = Guarded(img), Guarded(depth)
        guards += [gc, gd]
        gv.keyframe_cache_device(kid, gc.ptr, gd.ptr, stride=3 if source == "device3" else 4, pose_inv16=T)
    return guards


def _run_hand_case(case, source, meshes=None):
    """generate + update over every mesh, compared; then the honest round -> (model, patches, atlas rows)"""
    cam = case["cam"]
    if meshes is not None:
        case = dict(case, meshes=meshes)
    gv = capi.Volume(case["res"], cam, max_chunks=1 << 14, atlas_w=AW, atlas_h=AH)
    assert gv.atlas_patch_size() == case["slot"]
    model = AtlasModel(case)
    ids = _upload_hand_meshes(gv, cam, case["meshes"])
    guards = _cache_keyframes(gv, case, source)
    order = list(range(len(ids)))
    labels = np.array([m["kf"] for m in case["meshes"]], np.int32)
    model.generate(order, labels)
    grc, ghot = gv.generate_patches(ids, labels)
    assert grc == 0 and gv.atlas_loc_next() == model.atlas.loc_next()
    model.compare(gv, ids, "GeneratePatches")
    model.update(order)
    gv.update_atlas(ids)
    g = model.compare(gv, ids, "UpdateAtlas")  # (the ratio is written by UpdateBuffer)
    r0, r1 = model.compare_atlas(gv)
    rows = gv.atlas_rows(r0, r1, AW)
    # (d) an honest round through the same handle: the meshes an ordinary keyframe sees whole, in another order
    whole = {id(m) for m in PI.honest_meshes(case)}
    honest = [i for i in order if id(case["meshes"][i]) in whole][::-1]
    if honest:
        lab2 = np.full(len(honest), PI.KF_HONEST, np.int32)
        model.generate(honest, lab2)
        grc, _ = gv.generate_patches(ids[honest], lab2)
        assert grc == 0 and gv.atlas_loc_next() == model.atlas.loc_next()
        model.update(honest)
        gv.update_atlas(ids[honest])
        model.compare(gv, ids, "the honest round")
        model.compare_atlas(gv)
    gv.sync()
    gv.close()
    for k, gb in enumerate(guards):
        gb.check_and_free("keyframe buffer %d" % k)
    return model, g, rows


@pytest.mark.parametrize("source", ["host", "device3", "device4"])
@pytest.mark.parametrize("key", PI.hand_case_keys(), ids=lambda k: "%s-%d" % k)
def test_hand_made_meshes_call_by_call(gpu_required, key, source):
    case = PI.hand_case(*key)
    model, g, rows = _run_hand_case(case, source)
    assert (g["ratio"][:, 0] < 1).sum() >= 5 and (g["ratio"][:, 1] < 1).sum() >= 5  # the resize branch ran, both ways
    assert (g["flags"] & 2).sum() >= 5 and (g["flags"] & 4).sum() >= 5
    assert rows.any()


# ---------------------------------------------------------------------------------------------------------------------
# not a number
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "device4"])
def test_projection_that_is_not_a_number(gpu_required, source):
    """a NaN coordinate counts as outside the image (caution, clamped to 0).  The call returns; the
    NaN patches equal the oracle under that definition and are the same in two runs; every other patch and every
    atlas texel outside the NaN patches' slots are what a run without the NaN vertices gives."""
    case, bad = PI.nan_case()
    m1, g1, rows1 = _run_hand_case(case, source)
    m2, g2, rows2 = _run_hand_case(case, source)
    for k in ("texloc", "frameid", "bbox", "flags"):
        assert np.array_equal(g1[k], g2[k]), k
    for k in ("ratio", "texcoord", "texcolor"):
        assert np.array_equal(g1[k].view(np.uint32), g2[k].view(np.uint32)), k
    assert np.array_equal(rows1, rows2)
    assert all(g1["flags"][i] & 2 for i in bad)
    # the same meshes with the NaN vertex replaced by its neighbour in the list
    clean = []
    for i, m in enumerate(case["meshes"]):
        if i in bad:
            V = m["verts"].copy()
            rows_bad = np.where(~np.isfinite(V).all(axis=1) | (V[:, 2] == 0))[0]
            assert len(rows_bad) == 1
            V[rows_bad[0]] = V[rows_bad[0] - 1] if len(V) > 1 else (0.0, 0.0, 1.1)
            m = dict(m, verts=V)
        clean.append(m)
    m3, g3, rows3 = _run_hand_case(case, source, meshes=clean)
    assert np.array_equal(g1["texloc"], g3["texloc"])
    pw, ph = case["slot"]
    mask = np.ones(rows1.shape[:2], bool)
    r0 = int(g1["texloc"].min()) // AW
    for i in range(len(case["meshes"])):
        a, b = g1["voff"][i], g1["voff"][i + 1]
        if i in bad:
            x, y = int(g1["texloc"][i]) % AW, int(g1["texloc"][i]) // AW - r0
            mask[y:y + ph, x:x + pw] = False
            continue
        for k in ("bbox", "flags", "frameid"):
            assert np.array_equal(g1[k][i], g3[k][i]), (i, k)
        assert np.array_equal(g1["texcoord"][a:b].view(np.uint32), g3["texcoord"][a:b].view(np.uint32)), i
        assert np.array_equal(g1["texcolor"][a:b].view(np.uint32), g3["texcolor"][a:b].view(np.uint32)), i
    assert np.array_equal(rows1[mask], rows3[mask])


# ---------------------------------------------------------------------------------------------------------------------
# (b) the fused per-frame kernels with a keyframe pose that is not the integration pose
# ---------------------------------------------------------------------------------------------------------------------
def _check_textured_state(ov, oa, gv, tag, min_meshes):
    mids = sorted_ids(ov.list_meshes())
    assert np.array_equal(mids, sorted_ids(gv.list_meshes())), tag
    assert len(mids) >= min_meshes, tag
    g = _compare_patches(ov, gv, mids, tag)
    used = g["texloc"][g["texloc"] != np.uint64(NO_SLOT)]
    assert len(used) >= min_meshes, tag
    _compare_atlas(oa, gv, oa.hot_range(used))
    assert gv.atlas_loc_next() == oa.loc_next(), tag
    return mids, g


def _compare_meshes(ov, gv, mids):
    voff, ioff, V, N, Cc, I, adj, simp = gv.get_meshes(mids)
    for i, cid in enumerate(mids):
        m = ov.get_mesh(cid)
        assert np.array_equal(V[voff[i]:voff[i + 1]].view(np.uint32), m["verts"].view(np.uint32)), cid
        assert np.array_equal(I[ioff[i]:ioff[i + 1]], m["indices"]), cid
        assert bool(simp[i]) == m["simplified"] and np.array_equal(adj[i], m["adj"]), cid
    return np.diff(voff)


def test_fused_frames_with_foreign_keyframe_poses(gpu_required):
    """tests/patch_inputs.py FUSED_PLAN: tf_stream_frames_textured_device with n_ahead 0 and 2, tf_integrate_frame_host,
    a TSDF-only frame in between (the pending stage goes out through k_patch<true, true, true> on its own),
    tf_stream_frames_device + tf_texture_frame_device, and an honest last frame -- against the oracle's per-frame unit
    after every entry point.  The census over this very run is test_patch_cpu's."""
    case = PI.fused_case()
    cam, res, frames = case["cam"], case["res"], case["frames"]
    ov = O.Volume(res, O.camera_from(cam), O.default_integrator())
    gv = capi.Volume(res, cam, max_chunks=1 << 15)
    oa = O.Atlas(res)
    gd = [Guarded(f["depth"]) for f in frames]
    gr = [Guarded(f["rgba"]) for f in frames]
    poses = np.stack([f["pose"].reshape(12) for f in frames])
    ident = synth.pose_inverse16(synth.pose_identity())
    pinv = np.stack([f["pose_inv16"] if f["pose_inv16"] is not None else ident for f in frames])

    def oracle_step(f):
        if f["pose_inv16"] is None:
            ov.integrate_frame(f["depth"], f["rgba"], f["pose"])
        else:
            ov.frame_textured(oa, f["depth"], f["rgba"], f["pose"], f["pose_inv16"], f["frame_id"])

    seen = set()
    for how, grp in itertools.groupby(range(len(frames)), key=lambda k: frames[k]["how"]):
        idx = list(grp)
        seen.add(how)
        for k in idx:
            oracle_step(frames[k])
        a, b = idx[0], idx[-1] + 1
        if how in ("stream0", "stream2"):
            ahead = 0 if how == "stream0" else 2  # (selected ahead: the two frames that follow, which then arrive as host frames)
            dd, dr = [g.ptr for g in gd[a:b + ahead]], [g.ptr for g in gr[a:b + ahead]]
            gv.stream_frames_textured_device(dd, dr, poses[a:b + ahead], pinv[a:b + ahead], frames[a]["frame_id"],
                                             n_ahead=ahead)
        elif how == "host":
            for k in idx:
                f = frames[k]
                gv.integrate_frame_host(f["depth"], f["rgba"], f["pose"], f["pose_inv16"], f["frame_id"])
        elif how == "host_tsdf":
            for k in idx:
                gv.integrate_frame_host(frames[k]["depth"], frames[k]["rgba"], frames[k]["pose"], None, 0)
        elif how == "texture_frame":
            for k in idx:
                gv.stream_frames_device([gd[k].ptr], [gr[k].ptr], poses[k:k + 1])
                gv.texture_frame_device(frames[k]["pose_inv16"], frames[k]["frame_id"])
        else:
            raise KeyError(how)
        if how != "host_tsdf" and b > 5:  # (the first frames only build up weight)
            _check_textured_state(ov, oa, gv, "behind %s, frames %d..%d" % (how, a, b - 1), 300)
    assert seen == {"stream0", "stream2", "host", "host_tsdf", "texture_frame"}
    gv.sync()
    oids = sorted_ids(ov.list_chunks())
    assert np.array_equal(oids, sorted_ids(gv.list_chunks()))
    assert_chunks_equal(ov, gv, oids[::11], "foreign keyframe poses")
    mids, g = _check_textured_state(ov, oa, gv, "at the end", 300)
    nv = _compare_meshes(ov, gv, mids)
    assert (nv > 128).sum() >= 5, "the second sweep of the fused kernels"
    assert frames[-1]["variant"] == "honest" and (g["frameid"] == frames[-1]["frame_id"]).sum() >= 300
    gv.close()
    for k, gb in enumerate(gd + gr):
        gb.check_and_free("frame buffer %d" % k)


# ---------------------------------------------------------------------------------------------------------------------
# (c) the keyframe unit with its texture stage
# ---------------------------------------------------------------------------------------------------------------------
def test_keyframe_unit_with_a_turned_keyframe_pose(gpu_required):
    """tf_keyframe_unit_device(texture = 1, pose_inv16): groups of 1 + 2 frames, the second and third textured with a
    pose_inv16 that is not the keyframe's (turned towards the right-hand clamp; centre inside the surface) -- the stage
    of one unit rides on the mesh filter's launch of the next (k_mesh_filter<.., PATCH>); then an honest unit."""
    case = PI.fused_case()
    cam, res, frames = case["cam"], case["res"], case["frames"]
    ov = O.Volume(res, O.camera_from(cam), O.default_integrator())
    gv = capi.Volume(res, cam, max_chunks=1 << 15)
    oa = O.Atlas(res)
    gd = [Guarded(f["depth"]) for f in frames[:12]]
    gr = [Guarded(f["rgba"]) for f in frames[:12]]
    kfs = {}
    classes = []
    for u, variant in enumerate(("honest", "turn-", "inside", "honest")):
        key, loc = frames[3 * u], [frames[3 * u + 1], frames[3 * u + 2]]
        kid = 70 + u
        T = synth.pose_inverse16(PI.variant_pose(key["pose"], variant, key["centre"]))
        grp = capi.Volume.unit_group(kid, (gd[3 * u].ptr, gr[3 * u].ptr, None, key["pose"]),
                                     [(gd[3 * u + 1 + j].ptr, f["pose"]) for j, f in enumerate(loc)])
        gv.keyframe_unit(fresh=grp, texture=True, pose_inv16=T)
        # the oracle, call by call in the reference's order (tests/test_gpu_unit.py)
        ids, new = ov.prepare(key["depth"], key["pose"])
        needs = np.zeros(len(ids), np.uint8)
        ov.integrate(key["depth"], key["rgba"], None, key["pose"], ids, needs, 1, kid)
        for f in loc:
            ov.integrate(f["depth"], None, None, f["pose"], ids, needs, 1, -1)
        ov.finalize(ids, needs, new)
        ov.update_meshes()
        cids = ov.compress_meshes()
        kfs[kid] = (np.ascontiguousarray(key["rgba"][..., :3]), key["depth"], T)
        ov.generate_patches(oa, cids, np.full(len(cids), kid, np.int32), kfs)
        ov.update_atlas(oa, cids)
        if u >= 1:
            mids, g = _check_textured_state(ov, oa, gv, "behind unit %d (%s)" % (u, variant), 200)
            mine = [PR.project(ov.get_mesh(c)["verts"], ov.get_mesh(c)["colors"], T, kfs[kid][0], kfs[kid][1], cam)
                    for i, c in enumerate(mids) if g["frameid"][i] == kid]
            classes.append(PR.census(mine, oa.pw, oa.ph))
    gv.sync()
    # the inputs were hostile where they were meant to be, and honest at the end
    assert classes[0]["clamp_r"] >= 20 and classes[0]["kind2"] >= 20 and classes[0]["next_row"] >= 20
    assert classes[1]["read_past"] >= 20 and classes[1]["kind3"] >= 20 and classes[1]["roi_1_2_wide"] >= 5
    assert classes[2]["patches"] >= 200 and classes[2]["clamp_r"] == 0
    oids = sorted_ids(ov.list_chunks())
    assert np.array_equal(oids, sorted_ids(gv.list_chunks()))
    assert_chunks_equal(ov, gv, oids[::11], "keyframe units")
    _compare_meshes(ov, gv, sorted_ids(ov.list_meshes()))
    gv.close()
    for k, gb in enumerate(gd + gr):
        gb.check_and_free("frame buffer %d" % k)
