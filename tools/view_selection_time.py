"""Wall time of the view-selection solve (tf_view_select / tf_view_select_device) with both ways of walking a line.

Two problems: the chunk graph of the S-room (640x480 @ 5 mm) as a keyframe-unit stream leaves it -- K keyframes along the
orbit (seven consecutive frames each: the keyframe and six local frames) through tf_keyframe_unit_device without its
texture stage, nodes = the chunks that own a mesh, edges from
tf_export_adjacency, label sets and qualities from tf_export_datacost, unaries 1 - q / qmax -- and a synthetic sheet of
2 * 10^5 nodes (447 x 447 x 1, 90 % of the edges, 2-6 labels out of 12 per node).  Each is solved with the line arrays
(the default) and with TF_MRF_WALK=pointers; per variant: the host form's wall time (staging and read-back included; it
stops enqueueing when the solve has ended), the device form's with the default round cap (the launches behind the end
all return at once, but they are launched) and with the cap set to the rounds the solve takes.  Best of --reps.  The
two variants must give the same bytes.  One JSON line per problem.  Needs the GPU; run it under a time limit:

    timeout -k 10 600 python tools/view_selection_time.py [--keyframes 16] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from texturefusion_amd import capi, synth  # noqa: E402
from tests.util import HipBuffer  # noqa: E402

STEP = np.array(((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)), np.int32)


def problem_from_table(ids, nbr, table):
    """table [n, K] of qualities (0 = not observed) -> the problem TexMap::view_selection builds: a node without an
    observation gets the label 0 at cost 1 and loses its edges"""
    seen = table > 0
    empty = ~seen.any(axis=1)
    nbr = nbr.copy()
    nbr[empty] = -1
    nbr[(nbr >= 0) & empty[np.maximum(nbr, 0)]] = -1
    qmax = np.where(empty, np.float32(1), table.max(axis=1)).astype(np.float32)
    unary = (np.float32(1) - table / qmax[:, None]).astype(np.float32)
    counts = np.where(empty, 1, seen.sum(axis=1))
    col_off = np.zeros(len(ids) + 1, np.int64)
    col_off[1:] = np.cumsum(counts)
    rows, cols = np.nonzero(seen)
    labels = np.zeros(col_off[-1], np.int32)
    costs = np.ones(col_off[-1], np.float32)
    at = col_off[rows] + (np.cumsum(seen, axis=1)[rows, cols] - 1)
    labels[at] = cols + 1
    costs[at] = unary[rows, cols]
    return ids, nbr, col_off, labels, costs


def room_problem(vol, cam, n_key):
    bufs = []
    for g in range(n_key):  # keyframe g: seven consecutive frames of the orbit, the first one the keyframe
        fr = [synth.room_frame(7 * g + j, cam, with_quality=j == 0) for j in range(7)]
        b = [HipBuffer(x.nbytes).from_host(x) for x in (fr[0][0], fr[0][1], fr[0][2])] + [HipBuffer(f[0].nbytes).from_host(f[0]) for f in fr[1:]]
        bufs.append(b)
        grp = capi.Volume.unit_group(g + 1, (b[0].ptr, b[1].ptr, b[2].ptr, fr[0][3]), [(b[3 + j].ptr, fr[1 + j][3]) for j in range(6)])
        vol.keyframe_unit(fresh=grp, texture=False)
        vol.compress_meshes()
    vol.sync()
    ids = vol.list_meshes()
    assert len(ids) > 100, "the keyframe stream left only %d meshes" % len(ids)
    ids = ids[np.lexsort((ids[:, 2], ids[:, 1], ids[:, 0]))]
    index = {tuple(p): i for i, p in enumerate(ids.tolist())}
    nbr = np.full((len(ids), 6), -1, np.int32)
    for i, x, y, z in vol.export_adjacency(ids).tolist():
        j = index.get((x, y, z))
        if j is None:
            continue
        k = int(np.nonzero((STEP == np.array((x, y, z)) - ids[i]).all(axis=1))[0][0])
        nbr[i, k] = j
        nbr[j, k ^ 1] = i
    keys = list(range(1, n_key + 1))
    table = vol.export_datacost(ids, keys[0], keys[1:])
    for b in bufs:
        for x in b:
            x.free()
    return problem_from_table(ids, nbr, table)


def sheet_problem(side=447, seed=1):
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(side, dtype=np.int32), np.arange(side, dtype=np.int32), indexing="ij")
    ids = np.stack([x.ravel() - side // 2, y.ravel(), np.zeros(side * side, np.int32)], axis=1)
    node = np.arange(side * side, dtype=np.int32).reshape(side, side)
    nbr = np.full((side * side, 6), -1, np.int32)
    for k, (a, b) in ((1, (node[:-1, :], node[1:, :])), (3, (node[:, :-1], node[:, 1:]))):
        keep = rng.random(a.shape) < 0.9
        nbr[a[keep], k] = b[keep]
        nbr[b[keep], k ^ 1] = a[keep]
    n_lab = rng.integers(2, 7, side * side)
    rank = np.argsort(np.argsort(rng.random((side * side, 12)), axis=1), axis=1)
    table = np.where(rank < n_lab[:, None], rng.uniform(0.05, 1.0, (side * side, 12)), 0.0).astype(np.float32)
    return problem_from_table(ids, nbr, table)


def measure(vol, p, reps):
    ids, nbr, col_off, labels, costs = p
    n = len(ids)
    arrs = [ids, nbr, col_off, labels, costs]
    dev = [HipBuffer(a.nbytes).from_host(a) for a in arrs]
    d_off, d_en, d_r = HipBuffer(4 * n), HipBuffer(8 * 33), HipBuffer(16)
    out = {"nodes": n, "edges": int((nbr >= 0).sum() // 2), "labels": int(col_off[-1])}
    results = {}
    for walk in ("lines", "pointers"):
        os.environ["TF_MRF_WALK"] = walk
        best = {"host_ms": 1e30, "device_ms": 1e30, "device_exact_ms": 1e30}
        for _ in range(reps + 1):  # (the first pass grows the scratch pool)
            t0 = time.perf_counter()
            off, rounds, trace = vol.view_select(ids, nbr, col_off, labels, costs, 0.5)
            best["host_ms"] = min(best["host_ms"], 1e3 * (time.perf_counter() - t0))
            for key, cap in (("device_ms", 0), ("device_exact_ms", rounds)):
                vol.sync()
                t0 = time.perf_counter()
                vol.view_select_device(n, dev[0].ptr, dev[1].ptr, dev[2].ptr, int(col_off[-1]), dev[3].ptr, dev[4].ptr, 0.5, 0, cap,
                                       d_off.ptr, d_en.ptr, d_r.ptr)
                vol.sync()
                best[key] = min(best[key], 1e3 * (time.perf_counter() - t0))
            assert np.array_equal(d_off.to_host().view(np.int32), off)
        results[walk] = (off.tobytes(), rounds, trace.tobytes())
        out[walk] = {k: round(v, 3) for k, v in best.items()}
        out.update(rounds=rounds, energy_initial=float(trace[0]), energy_final=float(trace[-1]))
    os.environ.pop("TF_MRF_WALK", None)
    assert results["lines"] == results["pointers"], "the walking variants disagree"
    for b in dev + [d_off, d_en, d_r]:
        b.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    cam = synth.Camera()
    vol = capi.Volume(np.float32(0.005), cam, max_chunks=1 << 18, max_list=1 << 18, mesh_blocks=1 << 16)
    try:
        print(json.dumps({"problem": "room", "keyframes": args.keyframes, **measure(vol, room_problem(vol, cam, args.keyframes), args.reps)}))
        sys.stdout.flush()
        print(json.dumps({"problem": "sheet", **measure(vol, sheet_problem(), args.reps)}))
    finally:
        vol.close()


if __name__ == "__main__":
    main()
