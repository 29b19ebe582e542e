"""The hand-built keyframe sequence of the resident TexMap's edge tests (a helper, no tests): one wall, one cheap integration
per keyframe, a keyframe table that grows past two blocks of 64 rows, and quality images that are zero outside a pixel
rectangle chosen per keyframe -- so that which rows a chunk's column holds is decided here, row by row.

Scene: tests/align_inputs.CAM (160x120) with near 0.01 / far 5.0, 8 mm voxels, synth.wall_frame(0.6) head-on.  A chunk is
14 pixels wide; its column holds keyframe k where k's rectangle gives it a positive sum, and chunks with a voxel projecting
outside the image carry the reference's negative sentinel: no observation, an empty column.  Row 0 is a seed keyframe (six
depth-only integrations, so that the meshes -- the nodes -- exist before the first keyframe) that owns no observation; row k
is frame index 10 + 3 k, so a row is never mistaken for a frame index.

Rows (quality_of below):  1..60 the left half, value by k % 5 (ties inside block 0) | 61..70 a central band with a per-tile
factor (neighbours disagree: the solve has work); row 63 reaches further left (columns whose LAST entry is row 63), row 64
further right (columns whose FIRST entry is row 64) | 71..135 the right half, value by 7 k % 11 (ties inside block 1 and
between blocks 1 and 2); row 131 higher in the upper part (labels > 128 are chosen) | rows 30, 94 and 100 are TWINS: the
same frame, pose and quality image under three ids, the highest quality of every chunk their rectangle covers -- three
costs of exactly 0.0 in rows of block 0 and block 1, 30 and 94 on the same lane of the row walk, 100 on another.

Run.play() replays the sequence on the oracle + tests/texmap_ref.TexMap and, given a device volume, call by call through
tf_texmap_*; it yields one checkpoint after every step at which map and problem are to be compared:

  rows N          table of N = 1, 2, 63, 64, 65, 127, 128, 129, 136 rows: set_keyframes, ONE update naming every keyframe
                  since the last checkpoint, a full solve (cold at 1 row, warm after)
  c1 / c2         keyframe 70 integrated again with another quality image; update(ids, 70, []) keeps the old entry
                  (add_value), update(ids, newest, [70]) overwrites it (set_value); full solve
  d1 / d2         the two most-chosen keyframes of rows >= 64 retracted, warm full solve (stored label gone: offset 0);
                  both integrated again and brought back through keys whose quality was 0 -- one by add_value, one by
                  set_value; full solve
  e               texmap_retract over every third node, a chunk that is no node and an id the volume never held
  b               texmap_clear, then ONE update naming all 135 earlier keyframes rebuilds every column
  g               the sub-problem (always cold) over a subset: a chunk listed twice, neighbours left out, a listed node
                  with an empty column, the twins' tie
  f / f2          the first full solve after the clear (cold, the twins' tie), and a second one straight after (warm,
                  every start at the offset the first one chose)
  h full / h sub  two more keyframes; behind each the rest of tsdfFusion's tail call by call (CompressMeshes, update,
                  solve, GeneratePatches with the resident labels, UpdateAtlas) or -- tail=True -- as ONE
                  tf_texture_tail_device call.  (Without the wrong-mapping pass on either form: the oracle side of this
                  sequence cuts no patches, so the restatement would not know what the pass removes;
                  tests/test_gpu_texmap_resident.py holds that pass.)
"""
from types import SimpleNamespace

import numpy as np

from oracle import api as O
from texturefusion_amd import synth
from tests import align_inputs as A
from tests import texmap_ref as T

RES8 = np.float32(0.008)
CAM = synth.Camera(A.CAM.width, A.CAM.height, A.CAM.fx, A.CAM.fy, A.CAM.cx, A.CAM.cy, 0.01, 5.0)
MAX_CHUNKS = 1 << 10
MAX_KEYFRAMES = 256   # tf_config.max_keyframes: the tail's GeneratePatches wants every chosen keyframe cached
SEED_KF = 5
SEED_FRAMES = 6       # depth-only integrations before the first keyframe (the mesher's weight test at 8 mm)
N_MAIN = 135          # keyframes of the main table: rows 1 .. 135
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, N_MAIN + 1)  # table sizes with a checkpoint
TWINS = (30, 94, 100)  # rows; 30 and 94 share lane 30 of the row walk
KC_ROW = 20           # the keyframe integrated twice (steps c1 / c2)
E_ROW = 5             # the keyframe step e retracts
NO_CHUNK = (9999, 9999, 9999)


def frame_of(row):
    return SEED_KF if row == 0 else 10 + 3 * row


def _tiles(k):
    yy, xx = np.mgrid[0:CAM.height, 0:CAM.width]
    return (1.0 + 0.8 * ((((xx // 14) + (yy // 14) + k) % 3) == 0)).astype(np.float32)


def quality_of(row, again=False):
    """the quality image of the keyframe in `row`; again: the image of its second integration (step c)"""
    q = np.zeros((CAM.height, CAM.width), np.float32)
    k = row
    if again:
        q[0:60, 10:70] = 0.3
    elif k in TWINS:
        q[44:90, 50:110] = 0.5
    elif k <= 60:
        q[:, 10:70] = 0.1 + 0.01 * (k % 5)
    elif k <= 70:
        x0, x1 = (12 if k == 63 else 40), (150 if k == 64 else 120)
        q[20:100, x0:x1] = 0.1
        q *= _tiles(k)
    elif k <= N_MAIN:
        q[:, 90:150] = 0.1 + 0.01 * ((k * 7) % 11)
        if k == 131:
            q[0:60, 90:150] = 1.0
    else:  # the two keyframes of step h: everything, weakly
        q[:, :] = 0.05 + 0.01 * (k % 2)
    return q


def tup(c):
    return tuple(int(x) for x in c)


class Run:
    """both sides while the sequence runs"""

    def __init__(self, gv=None, tail=False):
        self.gv, self.tail = gv, tail
        self.ov = O.Volume(RES8, O.camera_from(CAM), O.default_integrator())
        self.tm = T.TexMap()
        self.kflist = []
        self.valid = {}      # frame -> validChunks of its last integration
        self.depth, self.rgba, _, self.pose = synth.wall_frame(0.6, CAM)
        self.T16 = synth.pose_inverse16(self.pose)
        self.rgb = np.ascontiguousarray(self.rgba[..., :3])
        self.improved = 0    # solves of >= 2 rounds that end strictly below their start
        self.facts = {}      # what test_texmap_edges_cpu.py asks about single steps

    def close(self):
        self.ov.close()

    def lookup(self):
        return {f: r for r, f in enumerate(self.kflist)}

    def node_ids(self):
        return np.array(sorted(self.tm.chunkGraph.chunks), np.int32).reshape(-1, 3)

    # ---- one integration on both sides (ReIntegrateKeyframe without local frames; kf < 0: depth only, no observation)
    def _integrate(self, kf, quality):
        ov, gv = self.ov, self.gv
        rgba = self.rgba if kf >= 0 else None
        ids, new = ov.prepare(self.depth, self.pose)
        needs = np.zeros(len(ids), np.uint8)
        ov.integrate(self.depth, rgba, quality, self.pose, ids, needs, 1, kf)
        valid = ov.finalize(ids, needs, new)
        if gv is not None:
            gv.frame_upload(self.depth, rgba, quality)
            gids, gnew = gv.prepare(self.pose)
            assert np.array_equal(ids, gids) and np.array_equal(new, gnew), "prepare, keyframe %d" % kf
            needs_g = np.zeros(len(ids), np.uint8)
            gv.integrate(self.pose, ids, needs_g, 1, kf >= 0, kf >= 0)
            if kf >= 0:
                gv.observations_record(kf)
            assert np.array_equal(needs, needs_g), "integrate, keyframe %d" % kf
            assert np.array_equal(valid, gv.finalize(ids, needs_g, new)), "finalize, keyframe %d" % kf
        if kf >= 0:
            self.valid[kf] = valid
        return valid

    def _keyframe(self, row, again=False, cache=True):
        kf = frame_of(row)
        self._integrate(kf, quality_of(row, again))
        if self.gv is not None and cache and not again:
            self.gv.keyframe_cache(kf, self.rgb, self.depth, self.T16)

    def _meshes(self):
        """UpdateMeshes + CompressMeshes on both sides -> chunksToUpdate"""
        self.ov.update_meshes()
        ids = self.ov.compress_meshes()
        if self.gv is not None:
            self.gv.update_meshes()
            assert np.array_equal(ids, self.gv.compress_meshes()), "chunksToUpdate"
        return ids

    def _adj_of(self, cid):
        m = self.ov.get_mesh(cid)
        return None if m is None else m["adj"]

    def _update(self, ids, kf, frames=()):
        frames = [int(f) for f in frames]
        self.tm.update_chunkgraph(ids, self._adj_of)
        self.tm.update_datacost(ids, lambda c: self.ov.observations(c), self.lookup(), kf, frames)
        if self.gv is not None:
            self.gv.texmap_update(ids, kf, frames)

    def _retract(self, kf, ids):
        self.tm.retract(kf, ids, self.lookup(), lambda c: self.ov.has_chunk(c))
        if self.gv is not None:
            self.gv.texmap_retract(kf, ids)

    def _solve(self, sub=None):
        """-> (restatement's (offsets, rounds, trace), device's (n_nodes, rounds, trace) or None)"""
        if sub is None:
            sol = self.tm.view_selection(self.kflist)
            g = None if self.gv is None else self.gv.texmap_view_selection()
        else:
            sol = self.tm.view_selection_sub(sub, self.kflist)
            g = None if self.gv is None else self.gv.texmap_view_selection(sub)
        if sol[1] >= 2 and sol[2][-1] < sol[2][0]:
            self.improved += 1
        return sol, g

    def _cp(self, name, sol=None, g=None, **kw):
        return SimpleNamespace(name=name, kflist=list(self.kflist), solution=sol, g_solution=g, solved=sol is not None, **kw)

    def _exports(self, ids, kf, frames):
        """(oracle's table, device's table, oracle's edge set, device's edge set) of the exports an update consumes"""
        frames = [int(f) for f in frames]
        want = np.zeros((len(ids), 1 + len(frames)), np.float32)
        have = {tup(c) for c in self.ov.list_meshes()}
        edges = set()
        for i, cid in enumerate(ids):
            obs = self.ov.observations(cid)
            for j, f in enumerate([kf] + frames):
                want[i, j] = obs.get(f, 0.0)
            adj = self._adj_of(cid)
            for k, d in enumerate(T.NEIGHBOURHOOD):
                q = (int(cid[0]) + d[0], int(cid[1]) + d[1], int(cid[2]) + d[2])
                if adj is not None and adj[k] and q in have:
                    edges.add((i,) + q)
        got = self.gv.export_datacost(ids, kf, frames)
        got_e = {tup(e) for e in self.gv.export_adjacency(ids)}
        return want, got, edges, got_e

    def chosen_labels(self):
        """label (row + 1, 0 = none) the last solve left every node of its problem with"""
        p, off = self.tm.problem, self.tm.solution[0]
        return p["labels"][p["col_off"][:-1] + off]

    def play(self):
        ov, gv, tm = self.ov, self.gv, self.tm
        # ---- the seed keyframe: row 0, meshes, no observation
        for _ in range(SEED_FRAMES):
            self._integrate(-1, None)
        if gv is not None:
            gv.keyframe_cache(SEED_KF, self.rgb, self.depth, self.T16)
        self.kflist.append(SEED_KF)
        pending = []
        # ---- a. the table sizes (and b.: one update names every keyframe since the last checkpoint)
        for row in range(0, N_MAIN + 1):
            if row:
                self._keyframe(row)
                self.kflist.append(frame_of(row))
                pending.append(frame_of(row))
            if len(self.kflist) not in SIZES:
                continue
            if gv is not None:
                gv.texmap_set_keyframes(self.kflist)
            ids = self._meshes()
            newest, frames = self.kflist[-1], pending[:-1]
            exports = None if gv is None else self._exports(ids, newest, frames)
            self._update(ids, newest, frames)
            sol, g = self._solve()
            yield self._cp("rows %d" % len(self.kflist), sol, g, exports=exports, n_rows=len(self.kflist), ids=ids)
            pending = []
        newest = self.kflist[-1]
        nodes = self.node_ids()
        # ---- c. add_value keeps the existing entry, set_value overwrites it
        kc = frame_of(KC_ROW)
        col = lambda c: dict(tm._column(tm.chunkGraph.chunks[c]))
        watch = [tup(c) for c in nodes if ov.observations(c).get(kc, 0.0) > 0.0]
        obs0 = {c: ov.observations(c)[kc] for c in watch}
        self._keyframe(KC_ROW, again=True)
        obs1 = {c: ov.observations(c).get(kc, 0.0) for c in watch}
        col0 = {c: col(c).get(KC_ROW) for c in watch}
        self._update(nodes, kc)
        col1 = {c: col(c).get(KC_ROW) for c in watch}
        yield self._cp("c1")
        self._update(nodes, newest, [kc])
        col2 = {c: col(c).get(KC_ROW) for c in watch}
        self.facts["c"] = dict(watch=watch, obs0=obs0, obs1=obs1, col0=col0, col1=col1, col2=col2)
        sol, g = self._solve()
        yield self._cp("c2", sol, g)
        # ---- d. remove and re-add: the two most-chosen keyframes of rows >= 64
        chosen = self.chosen_labels()
        late, cnt = np.unique(chosen[chosen > 64], return_counts=True)
        picked = [int(late[i]) - 1 for i in np.argsort(-cnt, kind="stable")[:2]]  # rows
        assert len(picked) == 2, "step d needs two chosen keyframes in rows >= 64"
        zeroed = tm.warm_zeroed
        for r in picked:
            kf = frame_of(r)
            ov.retract_observations(kf, self.valid[kf])
            if gv is not None:
                gv.observations_retract(kf, self.valid[kf])
            self._retract(kf, self.valid[kf])
        sol, g = self._solve()
        self.facts["d"] = dict(rows=picked, warm_zeroed=tm.warm_zeroed - zeroed)
        yield self._cp("d1", sol, g)
        for r in picked:
            self._keyframe(r, cache=False)
        self._update(nodes, frame_of(picked[0]))              # add_value into a key whose quality is 0
        self._update(nodes, newest, [frame_of(picked[1])])    # set_value into one
        sol, g = self._solve()
        yield self._cp("d2", sol, g)
        # ---- e. retract over ids outside the graph
        bare = [tup(c) for c in ov.list_chunks() if tup(c) not in tm.chunkGraph.chunks]
        self.facts["e"] = dict(bare=len(bare))
        ids_e = np.array([tup(c) for c in nodes[::3]] + bare[:1] + [NO_CHUNK], np.int32)
        self._retract(frame_of(E_ROW), ids_e)
        yield self._cp("e")
        # ---- b. clear, then one update fills every column from every earlier keyframe
        tm.clear()
        if gv is not None:
            gv.texmap_clear()
        meshed = np.array(sorted(tup(c) for c in ov.list_meshes()), np.int32)
        self._update(meshed, newest, self.kflist[:-1])
        yield self._cp("b")
        # ---- g. the sub-problem: a chunk twice, neighbours left out, an empty column among the listed
        nodes = self.node_ids()
        empty = [tup(c) for c in nodes if not tm._column(tm.chunkGraph.chunks[tup(c)])]
        keep = [tup(c) for i, c in enumerate(nodes) if i % 4 != 1 or tup(c) in empty]
        sub = np.array(keep + keep[3:5], np.int32)
        sol, g = self._solve(sub)
        yield self._cp("g", sol, g, sub=sub)
        # ---- f. the first full solve after the clear is cold; the second starts where the first ended
        sol, g = self._solve()
        yield self._cp("f", sol, g)
        sol, g = self._solve()
        yield self._cp("f2", sol, g)
        # ---- h. two more keyframes, the tail behind each: full, then the sub-problem over chunksToUpdate
        for j, select in enumerate(("full", "sub")):
            row = N_MAIN + 1 + j
            self._keyframe(row)
            kf = frame_of(row)
            self.kflist.append(kf)
            frames = [frame_of(KC_ROW + j)]
            ov.update_meshes()
            ids = ov.compress_meshes()
            tm.update_chunkgraph(ids, self._adj_of)
            tm.update_datacost(ids, lambda c: ov.observations(c), self.lookup(), kf, frames)
            sol = tm.view_selection(self.kflist) if select == "full" else tm.view_selection_sub(ids, self.kflist)
            g = hot = None
            if gv is not None:
                gv.texmap_set_keyframes(self.kflist)
                gv.update_meshes()
                if self.tail:
                    gv.texture_tail(kf, frames, wrong_mapping=False, check_graph=False, sub_problem=select == "sub")
                    assert np.array_equal(ids, gv.texture_tail_list()), "chunksToUpdate of the tail"
                else:
                    assert np.array_equal(ids, gv.compress_meshes()), "chunksToUpdate"
                    gv.texmap_update(ids, kf, frames)
                    g = gv.texmap_view_selection(None if select == "full" else ids)
                    rc, hot = gv.generate_patches_selected(ids)
                    assert rc == 0
                    gv.update_atlas(ids)
            yield self._cp("h " + select, sol, g, ids=ids, hot=hot)
