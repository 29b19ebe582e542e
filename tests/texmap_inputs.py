"""The keyframe sequence of the resident-TexMap tests, driven in MobileFusion::tsdfFusion's order
(GCFusion/MobileFusion.cpp:274-406) through the oracle + tests/texmap_ref.py and -- when a device volume is given -- call
by call through tf_texmap_*: S-room at 320x240 / 8 mm, six keyframes with quality images, one keyframe MOVED (retract,
de-integrate at the old pose, re-integrate at a new one) and one de-integrated FOR GOOD, so that meshes vanish and
check_graph has work.  tests/test_texmap_cpu.py checks on the CPU that the sequence is not vacuous."""
import numpy as np

from oracle import api as O
from texturefusion_amd import synth
from tests import texmap_ref as T

RES8 = np.float32(0.008)
CAM = synth.Camera(320, 240, 262.5, 262.5, 159.5, 119.5, 0.01, 5.0)
# kflist row 0 is a keyframe fused before the sequence starts (tsdfFusion returns early for the first keyframe,
# :282): it owns no observation here and is the "keyframe before the newest" of the label-0 rule at the first step
SEED_KF = 1
# (keyframe frame index, room frame, moved = [(keyframe, new room frame or None = de-integrated for good)])
STEPS = [(4, 0, []), (7, 12, []), (9, 60, []), (12, 24, [(4, 2)]), (15, 36, [(9, None)]), (18, 18, [])]
WRONG = 4  # TF_PATCH_WRONG_MAPPING
# check_graph needs nodes whose mesh is not in allMeshes.  The reference never takes a mesh out of allMeshes through
# integration or de-integration: RecomputeMeshes only inserts (ChunkManager.cpp:232-264) and RemoveChunk only reaches
# chunks created in the same call (Chisel.h:472-477) -- the keyframe de-integrated for good leaves every mesh in place.
# (The library clears kMsInMap in the same place only -- finalize's garbage collection -- and tf_update_meshes never does.)
# So at this step the update is handed, besides chunksToUpdate, some dirty chunks that own no mesh (the entry point makes
# every listed chunk a node): their neighbours' adj flags give them edges, their observations a column, and check_graph
# -- which the step runs because it has a moved keyframe -- takes both away again.
EXTRA_STEP = 3


def frame(room_k):
    return synth.room_frame(room_k, CAM, with_quality=True, wobble=0.02)


N_LOCAL = 5  # local frames of a keyframe group: the room frames behind the keyframe's (with fewer, no voxel passes the mesher's weight test at 8 mm)


def group_frames(room_k):
    """(keyframe, [(depth, pose)] of its local frames) of the group whose keyframe is room frame room_k"""
    return frame(room_k), [(f[0], f[3]) for f in (frame(room_k + 1 + j) for j in range(N_LOCAL))]


def group_poses(room_k):
    return [frame(room_k + j)[3] for j in range(1 + N_LOCAL)]


def _keyframe(ov, gv, grp, poses, kf_id, flag, ids=None):
    """ReIntegrateKeyframe (MobileFusion.cpp:114-221) on both sides: the keyframe's depth + colour + quality, then its
    local frames depth-only over the same list; poses = [keyframe pose, local poses...]"""
    (depth, rgba, quality, _), local = grp
    pose = poses[0]
    if gv is not None:
        gv.frame_upload(depth, rgba, quality)
    if flag == 1:
        ids, new = ov.prepare(depth, pose)
        if gv is not None:
            gids, gnew = gv.prepare(pose)
            assert np.array_equal(ids, gids) and np.array_equal(new, gnew)
        needs = np.zeros(len(ids), np.uint8)
    else:
        new = np.zeros(len(ids), np.uint8)
        needs = np.ones(len(ids), np.uint8)
    needs_g = needs.copy()
    ov.integrate(depth, rgba, quality, pose, ids, needs, flag, kf_id)
    for (d, _), p in zip(local, poses[1:]):
        ov.integrate(d, None, None, p, ids, needs, flag, -1)
    valid = ov.finalize(ids, needs, new)
    if gv is not None:
        gv.integrate(pose, ids, needs_g, flag, True, True)
        gv.observations_record(kf_id)
        for (d, _), p in zip(local, poses[1:]):
            gv.frame_upload(d)
            gv.integrate(p, ids, needs_g, flag, False, False)
        assert np.array_equal(needs, needs_g)
        assert np.array_equal(valid, gv.finalize(ids, needs_g, new))
    return valid


class Run:
    """state of both sides while the sequence runs"""

    def __init__(self, gv=None, unit=False, tail=False, extra=True):
        """unit: the device side integrates through tf_keyframe_unit_device(texture = 0) -- which retracts the moved
        keyframes' observations AND their data-cost entries by itself and ends behind UpdateMeshes -- instead of call by
        call (steps with a keyframe de-integrated for good cannot run that way: the unit always re-integrates)"""
        self.gv = gv
        self.unit = unit or tail
        self.tail = tail    # ... and everything behind the unit is ONE call, tf_texture_tail_device
        self.extra = extra and not tail  # (the tail makes its own list: no mesh-less chunks can be slipped into its update)
        self.bufs = {}      # kf -> device images of its group
        self.ov = O.Volume(RES8, O.camera_from(CAM), O.default_integrator())
        self.oa = O.Atlas(RES8)
        self.tm = T.TexMap()
        self.kflist = [SEED_KF]
        self.kfs = {}       # kf -> (rgb, depth, T16): the oracle's keyframe images
        self.valid = {}     # kf -> validChunks
        self.pose = {}      # kf -> poses of its last integration (keyframe, local frames)
        self.frames = {}    # kf -> its group (group_frames)
        self.stats = dict(check_removed=0, wrong_removed=0, improved=0)
        self.hot = None
        f0 = frame(0)
        self._cache(SEED_KF, f0, f0[3])

    def close(self):
        self.ov.close()
        self.oa.close()
        for t in self.bufs.values():
            for b in t:
                b.free()

    def _dev_group(self, kf, poses, old=None):
        from texturefusion_amd import capi
        from tests.util import HipBuffer
        (depth, rgba, quality, _), local = self.frames[kf]
        if kf not in self.bufs:
            self.bufs[kf] = [HipBuffer(a.nbytes).from_host(np.ascontiguousarray(a)) for a in [depth, rgba, quality] + [d for d, _ in local]]
        b = self.bufs[kf]
        kw = {} if old is None else dict(old_keyframe_pose=old[0], old_local_poses=old[1:])
        return capi.Volume.unit_group(kf, (b[0].ptr, b[1].ptr, b[2].ptr, poses[0]),
                                      [(b[3 + j].ptr, poses[1 + j]) for j in range(len(local))], **kw)

    def lookup(self):
        return {f: r for r, f in enumerate(self.kflist)}

    def _cache(self, kf, fr, pose):
        T16 = synth.pose_inverse16(pose)
        rgb = np.ascontiguousarray(fr[1][..., :3])
        self.kfs[kf] = (rgb, fr[0], T16)
        if self.gv is not None:
            self.gv.keyframe_cache(kf, rgb, fr[0], T16)

    def wrong_patches(self):
        out = []
        for cid in self.ov.list_meshes():
            p = self.ov.get_patch(cid)
            if p is not None and (p["flags"] & 1) and (p["flags"] & WRONG):
                out.append((tuple(int(x) for x in cid), int(p["frameid"])))
        return out

    def step(self, i, select="full"):
        """one tsdfFusion; returns dict(ids = chunksToUpdate, solution, labels of the restatement for ids, ...)"""
        kf, room_k, moved = STEPS[i]
        ov, gv, tm = self.ov, self.gv, self.tm
        cbc = None if self.unit else gv  # the device side of the call-by-call integration
        dev_moved = []
        self.kflist.append(kf)
        look = self.lookup()
        if gv is not None:
            gv.texmap_set_keyframes(self.kflist)
        for m, new_k in moved:  # :301-315
            tm.retract(m, self.valid[m], look, lambda c: ov.has_chunk(c))
            ov.retract_observations(m, self.valid[m])
            if cbc is not None:
                gv.observations_retract(m, self.valid[m])
                gv.texmap_retract(m, self.valid[m])
            _keyframe(ov, cbc, self.frames[m], self.pose[m], m, 0, ids=self.valid[m])
            old = self.pose[m]
            if new_k is not None:
                self.pose[m] = group_poses(new_k)
                self.valid[m] = _keyframe(ov, cbc, self.frames[m], self.pose[m], m, 1)
                self._cache(m, self.frames[m][0], self.pose[m][0])
            if self.unit:
                assert new_k is not None, "the unit re-integrates every moved keyframe"
                dev_moved.append(self._dev_group(m, self.pose[m], old))
        grp = group_frames(room_k)
        self.frames[kf], self.pose[kf] = grp, group_poses(room_k)
        self.valid[kf] = _keyframe(ov, cbc, grp, self.pose[kf], kf, 1)
        self._cache(kf, grp[0], self.pose[kf][0])
        if self.unit and gv is not None:
            gv.keyframe_unit(fresh=self._dev_group(kf, self.pose[kf]), moved=dev_moved, texture=False)
        ov.update_meshes()  # :327
        wrong = self.wrong_patches()  # :330-342 (every keyframe index of the sequence is > 3)
        n_wrong = tm.remove_wrong_mapping(wrong, look)
        extra = np.zeros((0, 3), np.int32)
        if i == EXTRA_STEP and self.extra:
            have = {tuple(int(x) for x in c) for c in ov.list_meshes()}
            bare = [tuple(int(x) for x in c) for c in ov.dirty()
                    if tuple(int(x) for x in c) not in have and ov.has_chunk(c)]
            extra = np.array(sorted(bare)[::max(1, len(bare) // 48)], np.int32).reshape(-1, 3)
        ids = ov.compress_meshes()  # :345-355
        upd = np.concatenate([ids, extra]) if len(extra) else ids
        out = dict(kf=kf, ids=ids, upd=upd, n_wrong=n_wrong, n_check=None)
        frames_to_update = [m for m, _ in moved]
        if gv is not None and self.tail:
            gv.texture_tail(kf, frames_to_update, wrong_mapping=True, check_graph=bool(moved), sub_problem=select == "sub")
            assert np.array_equal(ids, gv.texture_tail_list())
        elif gv is not None:
            if not self.unit:
                gv.update_meshes()
            out["g_wrong"] = gv.texmap_remove_wrong_mapping()
            gids = gv.compress_meshes()
            assert np.array_equal(ids, gids)
        has_mesh = {tuple(int(x) for x in c) for c in ov.list_meshes()}

        def adj_of(cid):
            m = ov.get_mesh(cid)
            return None if m is None else m["adj"]

        tm.update_chunkgraph(upd, adj_of)  # :356
        tm.update_datacost(upd, lambda c: ov.observations(c), look, kf, frames_to_update)  # :357-359
        if gv is not None and not self.tail:
            gv.texmap_update(upd, kf, frames_to_update)
        if moved:  # :360-361
            out["n_check"] = tm.check_graph(lambda c: c in has_mesh)
            if gv is not None and not self.tail:
                out["g_check"] = gv.texmap_check_graph()
        if select == "full":  # :362-369
            out["solution"] = tm.view_selection(self.kflist)
            if gv is not None and not self.tail:
                out["g_solution"] = gv.texmap_view_selection()
        elif select == "sub":
            out["solution"] = tm.view_selection_sub(ids, self.kflist)
            if gv is not None and not self.tail:
                out["g_solution"] = gv.texmap_view_selection(ids)
        self.stats["wrong_removed"] += n_wrong
        self.stats["check_removed"] += out["n_check"] or 0
        if out.get("solution") is not None and out["solution"][2][-1] < out["solution"][2][0]:
            self.stats["improved"] += 1
        return out

    def patches(self, ids):
        """GeneratePatches(labels of the graph) + UpdateAtlas (:374-382) on both sides"""
        labels = np.array([tm_label for tm_label in (self.tm.chunkGraph.labels[self.tm.chunkGraph.chunks[tuple(int(x) for x in c)]]
                                                     for c in ids)], np.int32)
        rc, hot = self.ov.generate_patches(self.oa, ids, labels, self.kfs)
        assert rc == 0
        self.ov.update_atlas(self.oa, ids)
        if self.gv is not None and not self.tail:
            grc, ghot = self.gv.generate_patches_selected(ids)
            assert grc == 0 and ghot == hot, (grc, ghot, hot)
            self.gv.update_atlas(ids)
        return labels, hot
