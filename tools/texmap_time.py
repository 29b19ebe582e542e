"""Wall time per keyframe of tsdfFusion's tail (GCFusion/MobileFusion.cpp:345-382 without CompensateColor) behind
tf_keyframe_unit_device(texture = 0), three ways, on the room of DESIGN.md s.7d (16 keyframes x 7 frames, 640x480 @ 5 mm):

  a  host-built   tf_compress_meshes, tf_export_adjacency + tf_export_datacost, graph / cost table / problem / warm start
                  built on the host (numpy: `build_ms` is reported on its own, a C++ caller's is smaller), tf_view_select,
                  labels back to keyframe indices on the host, tf_generate_patches with them, tf_update_atlas
  b  resident     tf_compress_meshes, tf_texmap_update, tf_texmap_view_selection, tf_generate_patches_selected,
                  tf_update_atlas
  c  tail         tf_texture_tail_device

The room has no moved keyframe, so none of the three runs the wrong-mapping removal or check_graph.  Every pass runs
the whole room on a fresh volume; the unit call of a keyframe is not timed, the stream is drained before and after the
timed part.  Per keyframe the best of --reps passes after one warm-up pass.  The patches' keyframes after the last
keyframe must agree between the three.  --profile b|c runs one pass of that path in a child process of its own under
`rocprofv3 --kernel-trace --stats` and reports the share of the solve's kernels (k_mrf_*) and of the map's (k_tm_*) in the
kernel time.  One JSON line per path (append them to profiles/r7/texmap_time.jsonl).  Needs the GPU; run it under a time
limit:

    timeout -k 10 900 python tools/texmap_time.py [--keyframes 16] [--reps 5] [--paths abc] [--profile bc]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from texturefusion_amd import capi, synth  # noqa: E402
from tests.util import HipBuffer  # noqa: E402

STEP = np.array(((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)), np.int32)
SEED_KF = 1000  # kflist row 0: a keyframe fused before the room starts (the label-0 rule's "keyframe before the newest")


class HostTexMap:
    """the parent commit's host side: UniGraph + SparseMat as dense numpy tables, TexMap::solve's problem, the warm start"""

    def __init__(self, n_rows):
        self.index = {}
        self.ids = np.zeros((0, 3), np.int32)
        self.nbr = np.zeros((0, 6), np.int32)
        self.table = np.zeros((0, n_rows), np.float32)
        self.label = np.zeros(0, np.int32)
        self.stored = np.zeros(0, np.int32)
        self.solved = False

    def update(self, ids, edges, q, row):
        new = [tuple(c) for c in ids.tolist() if tuple(c) not in self.index]
        for c in new:
            self.index[c] = len(self.index)
        if new:
            k = len(new)
            self.ids = np.concatenate([self.ids, np.array(new, np.int32)])
            self.nbr = np.concatenate([self.nbr, np.full((k, 6), -1, np.int32)])
            self.table = np.concatenate([self.table, np.zeros((k, self.table.shape[1]), np.float32)])
            self.label = np.concatenate([self.label, np.zeros(k, np.int32)])
        at = np.array([self.index[tuple(c)] for c in ids.tolist()], np.int64)
        for i, x, y, z in edges.tolist():
            j = self.index.get((x, y, z))
            if j is None:
                continue
            a = at[i]
            k = int(np.nonzero((STEP == np.array((x, y, z)) - self.ids[a]).all(axis=1))[0][0])
            self.nbr[a, k] = j
            self.nbr[j, k ^ 1] = a
        col = self.table[at, row]
        self.table[at, row] = np.where((col == 0) & (q > 0), q, col)  # add_value keeps an existing entry
        return at

    def problem(self):
        seen = self.table > 0
        empty = ~seen.any(axis=1)
        nbr = self.nbr.copy()
        nbr[empty] = -1
        nbr[(nbr >= 0) & empty[np.maximum(nbr, 0)]] = -1
        qmax = np.where(empty, np.float32(1), self.table.max(axis=1)).astype(np.float32)
        unary = (np.float32(1) - self.table / qmax[:, None]).astype(np.float32)
        counts = np.where(empty, 1, seen.sum(axis=1))
        col_off = np.zeros(len(self.ids) + 1, np.int64)
        col_off[1:] = np.cumsum(counts)
        rows, cols = np.nonzero(seen)
        labels = np.zeros(col_off[-1], np.int32)
        costs = np.ones(col_off[-1], np.float32)
        before = np.cumsum(seen, axis=1)
        labels[col_off[rows] + before[rows, cols] - 1] = cols + 1
        costs[col_off[rows] + before[rows, cols] - 1] = unary[rows, cols]
        init = None
        if self.solved:  # TexMap.cpp:208-217
            init = np.zeros(len(self.ids), np.int32)
            m = len(self.stored)
            st = self.stored - 1
            ok = (st >= 0) & seen[np.arange(m), np.maximum(st, 0)]
            init[:m][ok] = before[np.arange(m), np.maximum(st, 0)][ok] - 1
        return (self.ids, nbr, col_off, labels, costs), init

    def assign(self, p, off, kflist):
        ids, nbr, col_off, labels, costs = p
        lab = labels[col_off[:-1] + off]
        kf = np.array(kflist, np.int32)
        self.label = np.where(lab == 0, np.where(self.label == 0, kf[-2], self.label), kf[np.maximum(lab, 1) - 1]).astype(np.int32)
        self.stored = lab.copy()
        self.solved = True


def one_pass(path, frames, bufs, cam, n_key):
    vol = capi.Volume(np.float32(0.005), cam, max_chunks=1 << 18, max_list=1 << 18, mesh_blocks=1 << 16)
    times, parts = [], []
    try:
        kflist = [SEED_KF]
        vol.keyframe_cache_device(SEED_KF, bufs[0][1].ptr, bufs[0][0].ptr, stride=4, pose_inv16=synth.pose_inverse16(frames[0][0][3]))
        host = HostTexMap(n_key + 1)
        ids = np.zeros((0, 3), np.int32)
        for g in range(n_key):
            fr, b, kf = frames[g], bufs[g], g + 1
            grp = capi.Volume.unit_group(kf, (b[0].ptr, b[1].ptr, b[2].ptr, fr[0][3]), [(b[3 + j].ptr, fr[1 + j][3]) for j in range(6)])
            vol.keyframe_unit(fresh=grp, texture=False)
            vol.keyframe_cache_device(kf, b[1].ptr, b[0].ptr, stride=4, pose_inv16=synth.pose_inverse16(fr[0][3]))
            kflist.append(kf)
            if path != "a":
                vol.texmap_set_keyframes(kflist)
            vol.sync()
            t0 = time.perf_counter()
            if path == "c":
                vol.texture_tail(kf, wrong_mapping=False)
                vol.sync()
                t1 = time.perf_counter()
                ids = vol.texture_tail_list()
            elif path == "b":
                ids = vol.compress_meshes()
                vol.texmap_update(ids, kf)
                vol.texmap_view_selection(wait=False)
                vol.generate_patches_selected(ids)
                vol.update_atlas(ids)
                vol.sync()
                t1 = time.perf_counter()
            else:
                ids = vol.compress_meshes()
                ta = time.perf_counter()
                edges = vol.export_adjacency(ids)
                q = vol.export_datacost(ids, kf)[:, 0]
                tb = time.perf_counter()
                at = host.update(ids, edges, q, len(kflist) - 1)
                p, init = host.problem()
                tc = time.perf_counter()
                off, rounds, trace = vol.view_select(*p, 0.5, init=init)
                td = time.perf_counter()
                host.assign(p, off, kflist)
                labels = host.label[at]
                te = time.perf_counter()
                vol.generate_patches(ids, labels)
                vol.update_atlas(ids)
                vol.sync()
                t1 = time.perf_counter()
                parts.append([1e3 * x for x in (ta - t0, tb - ta, tc - tb + te - td, td - tc, t1 - te)])
            times.append(1e3 * (t1 - t0))
        frameid = vol.get_patches(ids)["frameid"].copy() if len(ids) else np.zeros(0, np.int32)
        return times, parts, (ids.tobytes(), frameid.tobytes()), len(ids)
    finally:
        vol.close()


def profile_share(path, n_key):
    """one pass of `path` under rocprofv3 --kernel-trace --stats in a child process: share of k_mrf_* / k_tm_* in the kernel time"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--paths", path, "--reps", "0", "--keyframes", str(n_key)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=840)
        if r.returncode != 0:
            return {"error": (r.stdout + r.stderr)[-400:]}
        tot = {"all": 0.0, "k_mrf_": 0.0, "k_tm_": 0.0}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                name = row.get("Name") or row.get("KernelName") or ""
                ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
                tot["all"] += ns
                for k in ("k_mrf_", "k_tm_"):
                    if k in name:
                        tot[k] += ns
        if not tot["all"]:
            return {"error": "no kernel statistics found"}
        return {"kernel_ms": round(tot["all"] / 1e6, 3), "solve_share": round(tot["k_mrf_"] / tot["all"], 4),
                "texmap_share": round(tot["k_tm_"] / tot["all"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--paths", default="abc")
    ap.add_argument("--profile", default="")
    args = ap.parse_args()
    cam = synth.Camera()
    frames, bufs = [], []
    for g in range(args.keyframes):
        fr = [synth.room_frame(7 * g + j, cam, with_quality=j == 0) for j in range(7)]
        frames.append(fr)
        bufs.append([HipBuffer(x.nbytes).from_host(x) for x in (fr[0][0], fr[0][1], fr[0][2])] +
                    [HipBuffer(f[0].nbytes).from_host(f[0]) for f in fr[1:]])
    names = {"a": "host-built", "b": "resident", "c": "tail"}
    final = {}
    for path in args.paths:
        best, best_parts, n_list = None, None, 0
        for rep in range(args.reps + 1):  # (the first pass warms up: scratch pools, code objects)
            times, parts, state, n_list = one_pass(path, frames, bufs, cam, args.keyframes)
            final[path] = state
            if rep == 0 and args.reps:
                continue
            best = times if best is None else [min(a, b) for a, b in zip(best, times)]
            if parts:
                best_parts = parts if best_parts is None else [[min(a, b) for a, b in zip(x, y)] for x, y in zip(best_parts, parts)]
        out = {"path": names[path], "keyframes": args.keyframes, "reps": args.reps, "last_list": n_list,
               "per_keyframe_ms": [round(t, 3) for t in best], "sum_ms": round(sum(best), 3), "last_keyframe_ms": round(best[-1], 3)}
        if best_parts:
            s = np.array(best_parts).sum(axis=0)
            out.update(dict(zip(("compress_ms", "exports_ms", "build_ms", "solve_ms", "patches_ms"), [round(float(x), 3) for x in s])))
        if path in args.profile:
            out["rocprofv3"] = profile_share(path, args.keyframes)
        print(json.dumps(out))
        sys.stdout.flush()
    states = list(final.values())
    assert all(s == states[0] for s in states), "the paths disagree on chunksToUpdate or on the patches' keyframes"
    for b in bufs:
        for x in b:
            x.free()


if __name__ == "__main__":
    main()
