"""TexMap resident on the device (tf_texmap_*, tf_generate_patches_selected) against the oracle + tests/texmap_ref.py,
call by call in MobileFusion::tsdfFusion's order over the keyframe sequence of tests/texmap_inputs.py.  Every comparison
is by chunk id, at tolerance 0.

What the sequence is and why one update is handed chunks without a mesh (the only way check_graph gets work: the
reference never takes a mesh out of allMeshes) is said in tests/texmap_inputs.py; tests/test_texmap_cpu.py checks on the
CPU that the sequence is not vacuous.  The wrong-mapping removal finds entries in the synthetic room by itself (188 over
the sequence), so no mesh is uploaded for it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from texturefusion_amd import capi
from tests import mrf_ref as R
from tests import texmap_inputs as I
from tests import texmap_ref as T
from tests.util import sorted_ids

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_TEXLOC = (1 << 64) - 1


def _volume():
    return capi.Volume(I.RES8, I.CAM, max_chunks=1 << 15)


def _check_map(run, gv, what):
    """node set, edge masks, labels, stored labels and columns (frame, quality bits) of every node and of some chunks
    that are none"""
    views = run.tm.all_node_views(run.kflist)
    others = [tuple(int(x) for x in c) for c in sorted_ids(run.ov.list_chunks())[::23]]
    ids = sorted(views) + [c for c in others if c not in views] + [(9999, 9999, 9999)]
    d = gv.texmap_download(np.array(ids, np.int32))
    for i, cid in enumerate(ids):
        a, b = int(d["col_off"][i]), int(d["col_off"][i + 1])
        if cid not in views:
            assert d["is_node"][i] == 0 and d["edges"][i] == 0 and a == b, (what, cid)
            continue
        mask, label, stored, col = views[cid]
        got = list(zip(d["col_frame"][a:b].tolist(), d["col_q"][a:b].view(np.uint32).tolist()))
        assert d["is_node"][i] == 1 and int(d["edges"][i]) == mask, (what, cid, int(d["edges"][i]), mask)
        assert int(d["label"][i]) == label and int(d["stored"][i]) == stored, (what, cid, d["label"][i], label, d["stored"][i], stored)
        assert got == col, (what, cid, got, col)
    return len(views)


def _check_problem(run, gv, g_solution, what):
    """the assembled problem (labels, cost bits, neighbour ids, start offsets), rounds, f64 trace, solved labels; and the
    same problem handed to the host form tf_view_select"""
    off, rounds, trace = run.tm.solution
    p = run.tm.problem
    gn, gr, gt = g_solution
    print(what, "nodes", gn, "rounds", gr, "trace", gt.tolist())
    assert gn == len(p["ids"]) and gr == rounds, (what, gn, len(p["ids"]), gr, rounds)
    assert gt.tobytes() == trace.tobytes(), (what, gt, trace)
    P = gv.texmap_problem()
    assert T.problem_view_of(P["ids"], P["nbr"], P["col_off"], P["labels"], P["costs"], P["init"]) == run.tm.problem_view(), what
    want = {tuple(int(x) for x in p["ids"][i]): int(p["labels"][p["col_off"][i] + off[i]]) for i in range(len(off))}
    got = {tuple(int(x) for x in P["ids"][i]): int(P["labels"][P["col_off"][i] + P["offsets"][i]]) for i in range(gn)}
    assert got == want, what
    warm = bool((P["init"] >= 0).all())
    assert warm or bool((P["init"] == -1).all())
    h_off, h_r, h_tr = gv.view_select(P["ids"], P["nbr"], P["col_off"], P["labels"], P["costs"], np.float32(0.5),
                                      init=P["init"] if warm else None)
    assert h_r == gr and np.array_equal(h_off, P["offsets"]) and h_tr.tobytes() == gt.tobytes(), what
    return warm


def _check_patches(run, gv, ids, hot, what):
    ov, oa = run.ov, run.oa
    g = gv.get_patches(ids)
    for i, cid in enumerate(ids):
        o = ov.get_patch(cid)
        tl = o["texloc"] if o["flags"] & 1 else NO_TEXLOC
        assert int(g["texloc"][i]) == tl and g["frameid"][i] == o["frameid"], (what, cid, g["frameid"][i], o["frameid"])
        if o["flags"] & 1:
            a, b = g["voff"][i], g["voff"][i + 1]
            assert np.array_equal(g["bbox"][i], o["bbox"]), (what, cid)
            assert np.array_equal(g["texcoord"][a:b].view(np.uint32), o["texcoord"].view(np.uint32)), (what, cid)
            assert np.array_equal(g["texcolor"][a:b].view(np.uint32), o["texcolor"].view(np.uint32)), (what, cid)
    assert gv.atlas_loc_next() == oa.loc_next()
    buf = oa.buffer()
    w = buf.shape[1]
    r0, r1 = hot[0] // w, min(hot[1] // w, buf.shape[0])
    assert r1 > r0 and np.array_equal(gv.atlas_rows(r0, r1, w), buf[r0:r1]), what


def test_keyframe_sequence_call_by_call(gpu_required):
    """tests 1 and 2 of the issue: after every keyframe the node set, edge masks and columns; the assembled problem;
    rounds and trace; chunk labels and stored labels; patches and hot atlas rows behind tf_generate_patches_selected +
    tf_update_atlas; and the downloaded problem through the host form of the solve."""
    gv = _volume()
    run = I.Run(gv)
    try:
        warm_seen = 0
        for i in range(len(I.STEPS)):
            what = "keyframe %d" % I.STEPS[i][0]
            o = run.step(i)
            assert o["g_wrong"] == o["n_wrong"], (what, o["g_wrong"], o["n_wrong"])
            if o["n_check"] is not None:
                assert o["g_check"] == o["n_check"], (what, o["g_check"], o["n_check"])
            n_nodes = _check_map(run, gv, what)
            assert n_nodes == run.tm.chunkGraph.num_nodes()
            warm_seen += _check_problem(run, gv, o["g_solution"], what)
            labels, hot = run.patches(o["ids"])
            _check_patches(run, gv, o["ids"], hot, what)
        tm = run.tm
        multi = sum(1 for k in range(tm.chunkGraph.num_nodes()) if len(tm._column(k)) >= 2)
        print("guards", multi, run.stats, tm.warm_zeroed, warm_seen)
        assert multi >= 50 and run.stats["improved"] >= 1 and tm.warm_zeroed >= 1
        assert run.stats["check_removed"] >= 1 and run.stats["wrong_removed"] >= 1
        assert warm_seen == len(I.STEPS) - 1  # every solve but the first starts from the stored labels
    finally:
        run.close()
        gv.close()


def test_behind_the_keyframe_unit(gpu_required):
    """The map behind tf_keyframe_unit_device(texture = 0) over a plan with a moved keyframe: the unit's own
    RetractObservations removes the moved keyframe's data-cost entries too (k_kf_load, guarded by the map's existence),
    and the rest of the tail runs on what the unit left in HBM.  (The tail as ONE call: test_tail_equals_the_call_by_call_sequence.)"""
    gv = _volume()
    run = I.Run(gv, unit=True)
    try:
        n_moved = 0
        for i in range(4):  # keyframes 4, 7, 9, and 12 with keyframe 4 moved
            what = "unit, keyframe %d" % I.STEPS[i][0]
            o = run.step(i)
            n_moved += len(I.STEPS[i][2])
            assert o["g_wrong"] == o["n_wrong"] and (o["n_check"] is None or o["g_check"] == o["n_check"]), what
            _check_map(run, gv, what)
            _check_problem(run, gv, o["g_solution"], what)
            labels, hot = run.patches(o["ids"])
            _check_patches(run, gv, o["ids"], hot, what)
        assert n_moved == 1 and run.stats["check_removed"] >= 1
    finally:
        run.close()
        gv.close()


def _state_bytes(run, gv, ids, hot):
    """everything the tail leaves behind, by chunk id, as bytes: the map of every node, the assembled problem with its
    start and solved offsets, the patches of chunksToUpdate, the hot atlas rows"""
    nodes = np.array(sorted(run.tm.chunkGraph.chunks), np.int32)
    d = gv.texmap_download(nodes)
    P = gv.texmap_problem()
    view = T.problem_view_of(P["ids"], P["nbr"], P["col_off"], P["labels"], P["costs"], P["init"])
    solved = {tuple(int(x) for x in P["ids"][i]): int(P["offsets"][i]) for i in range(len(P["ids"]))}
    g = gv.get_patches(ids)
    w = run.oa.buffer().shape[1]
    rows = gv.atlas_rows(hot[0] // w, hot[1] // w, w)
    parts = [d[k].tobytes() for k in ("is_node", "edges", "label", "stored", "col_off", "col_frame", "col_q")]
    parts += [repr(sorted(view.items())).encode(), repr(sorted(solved.items())).encode()]
    parts += [g[k].tobytes() for k in ("texloc", "frameid", "bbox", "flags", "ratio", "texcoord", "texcolor")]
    return parts + [rows.tobytes(), str(gv.atlas_loc_next()).encode()]


def _run_tail_plan(tail, select):
    gv = _volume()
    run = I.Run(gv, unit=True, tail=tail, extra=False)
    out = []
    try:
        for i in range(4):  # keyframes 4, 7, 9, and 12 with keyframe 4 moved
            what = "%s, keyframe %d" % ("tail" if tail else "call by call", I.STEPS[i][0])
            o = run.step(i, select=select if i == 3 else "full")
            labels, hot = run.patches(o["ids"])
            _check_map(run, gv, what)                       # against the oracle + restatement ...
            _check_patches(run, gv, o["ids"], hot, what)
            out.append(_state_bytes(run, gv, o["ids"], hot))  # ... and run against run
        return out
    finally:
        run.close()
        gv.close()


@pytest.mark.parametrize("select", ["full", "sub"])
def test_tail_equals_the_call_by_call_sequence(gpu_required, select):
    """test 4: tf_texture_tail_device behind tf_keyframe_unit_device(texture = 0) over a plan with a moved keyframe equals
    the call-by-call sequence bit for bit, through to atlas rows; three runs of the tail give identical bytes (the
    problem's node numbering comes from an atomic counter and differs from run to run: nothing may depend on it).
    select = sub: the last keyframe's solve is the chunksToUpdate overload (TF_TAIL_SUB_PROBLEM)."""
    ref = _run_tail_plan(False, select)
    for k in range(3):
        got = _run_tail_plan(True, select)
        assert len(got) == len(ref)
        for step, (a, b) in enumerate(zip(ref, got)):
            for j, (x, y) in enumerate(zip(a, b)):
                assert x == y, "run %d, keyframe step %d, part %d differs" % (k, step, j)


def test_sub_problem_overload(gpu_required):
    """test 3: the chunksToUpdate overload on a subset -- stored labels unchanged, no edge out of the subset"""
    gv = _volume()
    run = I.Run(gv)
    try:
        for i in range(2):
            o = run.step(i)
            run.patches(o["ids"])
        sub = o["ids"][::2]
        before = gv.texmap_download(o["ids"])
        sol = run.tm.view_selection_sub(sub, run.kflist)
        gn, gr, gt = gv.texmap_view_selection(sub)
        assert gn == len(run.tm.problem["ids"]) == len(sub) and gr == sol[1] and gt.tobytes() == sol[2].tobytes()
        P = gv.texmap_problem()
        assert (P["init"] == -1).all()  # cold
        assert T.problem_view_of(P["ids"], P["nbr"], P["col_off"], P["labels"], P["costs"], P["init"]) == run.tm.problem_view()
        inside = {tuple(int(x) for x in c) for c in sub}
        full_edges = run.tm.all_node_views(run.kflist)
        dropped = 0
        for i, cid in enumerate(P["ids"]):
            for k in range(6):
                j = P["nbr"][i, k]
                if j >= 0:
                    assert tuple(int(x) for x in P["ids"][j]) in inside
                elif full_edges[tuple(int(x) for x in cid)][0] >> k & 1:
                    dropped += 1
        assert dropped > 0
        after = gv.texmap_download(o["ids"])
        assert np.array_equal(after["stored"], before["stored"])
        _check_map(run, gv, "sub-problem")
        # a chunk listed twice is one node; chunks that are no nodes do not count
        gn2, _, _ = gv.texmap_view_selection(np.concatenate([sub, sub[:5], [[9999, 9999, 9999]]]))
        assert gn2 == len(sub)
    finally:
        run.close()
        gv.close()


def test_problem_arrays_and_keyframe_table_grow(gpu_required):
    """The two growth paths of the map's own buffers, each crossed once with the map compared against the host model
    behind it (as _check_map / _check_problem do, tolerance 0).

    Problem arrays: their capacity follows the length of the list handed to the sub-problem overload (a power of two of at
    least 1024), so with no solve before, 600 ids give room for 1024 nodes and 1 500 ids make it grow to 2048.  No
    chunksToUpdate of the sequence is that long (589, 468, 200, 1429, 1283, 1394 ids), so the list is every node of the
    graph after the first step that leaves at least 1 500 of them (keyframe 12: 1 678).

    Keyframe table: 2 rows, then 200 rows -- past the first table of 256 words, which keeps 64 behind its rows -- then an
    update that names keyframes to update and a full solve whose column walk covers four blocks of 64 rows."""
    gv = _volume()
    run = I.Run(gv)
    try:
        for i in range(len(I.STEPS)):
            o = run.step(i, select="none")
            nodes = np.array(sorted(run.tm.chunkGraph.chunks), np.int32)
            if len(nodes) >= 1500:
                break
        assert len(nodes) >= 1500, len(nodes)
        for m in (600, 1500):
            what = "sub-problem over %d ids" % m
            run.tm.view_selection_sub(nodes[:m], run.kflist)
            g = gv.texmap_view_selection(nodes[:m])
            assert g[0] == m, (what, g[0])  # (all distinct nodes: the second problem does not fit the first capacity)
            _check_problem(run, gv, g, what)
            _check_map(run, gv, what)
        gv.texmap_set_keyframes(run.kflist[:2])
        run.kflist += list(range(1000, 1000 + 200 - len(run.kflist)))
        assert len(run.kflist) == 200
        gv.texmap_set_keyframes(run.kflist)
        to_update = [k for k, _, _ in I.STEPS[:i]][:2]
        assert len(to_update) == 2
        run.tm.update_chunkgraph(o["ids"], lambda c: run.ov.get_mesh(c)["adj"])
        run.tm.update_datacost(o["ids"], lambda c: run.ov.observations(c), run.lookup(), o["kf"], to_update)
        gv.texmap_update(o["ids"], o["kf"], to_update)
        run.tm.view_selection(run.kflist)
        g = gv.texmap_view_selection()
        _check_problem(run, gv, g, "200 rows")
        assert _check_map(run, gv, "200 rows") == len(nodes)
    finally:
        run.close()
        gv.close()


def _snapshot(v):
    st = v.stats()
    ids = sorted_ids(v.list_chunks())
    s, w, c = v.get_chunks(ids)
    dirty = sorted_ids(v.dirty())
    mids = sorted_ids(v.list_meshes())
    voff, ioff, V, N, Cc, Ix, adj, simp = v.get_meshes(mids)
    obs = v.export_datacost(ids, 4, [7, 1])
    return (bytes(st), dirty.tobytes(), ids.tobytes(), s.tobytes(), w.tobytes(), c.tobytes(), mids.tobytes(), V.tobytes(),
            Ix.tobytes(), adj.tobytes(), obs.tobytes())


def test_volume_untouched_and_clear_and_reset(gpu_required):
    """tests 5 and 6: the map's calls leave voxels, meshes' geometry, observations and the dirty set alone;
    tf_texmap_clear and tf_volume_reset empty the map"""
    gv = _volume()
    run = I.Run(gv)
    try:
        for i in range(2):
            o = run.step(i, select="none")
        # (step() ran CompressMeshes: mark something again so that the dirty set is not trivially empty)
        grp = I.group_frames(30)
        gv.frame_upload(*grp[0][:3])
        ids, new = gv.prepare(grp[0][3])
        needs = np.zeros(len(ids), np.uint8)
        gv.integrate(grp[0][3], ids, needs, 1, True, True)
        gv.finalize(ids, needs, new)
        assert len(gv.dirty()) > 0
        before = _snapshot(gv)
        gv.texmap_set_keyframes(run.kflist)
        gv.texmap_update(o["ids"], o["kf"], [4])
        gv.texmap_retract(4, o["ids"][::3])
        gv.texmap_remove_wrong_mapping()
        gv.texmap_check_graph()
        n, r, tr = gv.texmap_view_selection()
        assert n > 0 and r >= 1
        gv.texmap_view_selection(o["ids"][::2])
        gv.texmap_download(o["ids"])
        gv.texmap_problem()
        assert _snapshot(gv) == before
        d = gv.texmap_download(o["ids"])
        assert d["is_node"].all() and d["col_off"][-1] > 0
        gv.texmap_clear()
        d = gv.texmap_download(o["ids"])
        assert not d["is_node"].any() and d["col_off"][-1] == 0 and not d["label"].any()
        assert gv.texmap_view_selection()[0] == 0
        assert _snapshot(gv) == before
        gv.texmap_update(o["ids"], o["kf"])
        assert gv.texmap_view_selection()[0] == len(o["ids"])
        assert (gv.texmap_problem()["init"] == -1).all()  # the first solve after a clear starts cold
        gv.reset()
        d = gv.texmap_download(o["ids"])
        assert not d["is_node"].any() and d["col_off"][-1] == 0
        with pytest.raises(capi.TFError):  # the keyframe table went with the map
            gv.texmap_update(o["ids"][:1], o["kf"])
    finally:
        run.close()
        gv.close()


_PROBE = r"""
import ctypes as C, sys
sys.path.insert(0, %r)
import numpy as np
from texturefusion_amd import capi, synth
capi.lib()
hip = C.CDLL("libamdhip64.so")
def free():
    a, b = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(a), C.byref(b)) == 0
    return a.value
hip.hipFree(None)
f0 = free()
v = capi.Volume(np.float32(0.008), synth.Camera(), max_chunks=1 << 15)
v.sync()
f1 = free()
if sys.argv[1] == "map":
    v.texmap_set_keyframes([1, 2])
    v.sync()
print("USED", f0 - f1, f1 - free())
v.close()
"""


def test_a_handle_without_a_map_allocates_nothing_for_it(gpu_required, tmp_path):
    """test 7: device memory taken by tf_volume_create (hipMemGetInfo around it, fresh child process) does not depend on
    this change: the map's first use, and only it, takes more"""
    script = tmp_path / "probe.py"
    script.write_text(_PROBE % ROOT)
    out = {}
    for mode in ("plain", "map"):
        r = subprocess.run([sys.executable, str(script), mode], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out[mode] = [int(x) for x in r.stdout.split("USED")[1].split()]
    print(out)
    assert out["plain"][0] == out["map"][0] and out["plain"][1] == 0
    # node, label, stored, idx words per pool slot + the cost table (as large as the observation table)
    assert out["map"][1] >= 4 * 4 * (1 << 15) + 12 * 4 * (1 << 15)


def test_invalid_arguments(gpu_required):
    """test 8: a label naming an uncached keyframe, n_rows of 0, a frame index outside the keyframe table; the handle
    keeps working"""
    gv = _volume()
    run = I.Run(gv)
    try:
        o = run.step(0)
        for bad in ([], [3, 3], [-1, 2]):
            with pytest.raises(capi.TFError) as e:
                gv.texmap_set_keyframes(bad)
            assert e.value.code == capi.TF_ERR_INVALID
        for kw in (dict(frame_index=99), dict(frame_index=4, frames_to_update=[5])):
            with pytest.raises(capi.TFError) as e:
                gv.texmap_update(o["ids"], **kw)
            assert e.value.code == capi.TF_ERR_INVALID and "keyframe table" in str(e.value)
        _check_map(run, gv, "after refused updates")
        # keyframe 4 leaves the cache: every chunk of the list is labelled 4 or 1 (the seed keyframe, still cached)
        labels = np.array([run.tm.chunkGraph.labels[run.tm.chunkGraph.chunks[tuple(int(x) for x in c)]] for c in o["ids"]])
        first = int(np.argmax(labels == 4))
        assert labels[first] == 4
        gv.keyframe_release(4)
        before = gv.get_patches(o["ids"])
        with pytest.raises(capi.TFError) as e:
            gv.generate_patches_selected(o["ids"])
        assert e.value.code == capi.TF_ERR_INVALID
        after = gv.get_patches(o["ids"])
        assert np.array_equal(after["texloc"][first:], before["texloc"][first:])  # it and everything behind it: unprocessed
        assert (after["texloc"][first:] == np.uint64(NO_TEXLOC)).all()
        # ... and the handle goes on: with the keyframe back the whole sequence step compares as usual
        rgb, depth, T16 = run.kfs[4]
        gv.keyframe_cache(4, rgb, depth, T16)
        labels, hot = run.patches(o["ids"])
        _check_patches(run, gv, o["ids"], hot, "after the refused call")
        o = run.step(1)
        _check_map(run, gv, "next keyframe")
        _check_problem(run, gv, o["g_solution"], "next keyframe")
    finally:
        run.close()
        gv.close()


def test_resident_path_equals_the_host_built_path(gpu_required, tmp_path):
    """test 9: tests/cpp_texmap/resident_vs_host.cpp -- one room sequence through the host mirror twice, host-built
    problem (update_*_device + view_selection) against the *_resident methods: equal chunk labels and traces after
    every keyframe.  Built and run like test_host_mirror_view_selection."""
    from texturefusion_amd import synth
    frames = [synth.room_frame(k, I.CAM, with_quality=True, wobble=0.02) for k in range(17)]
    path = str(tmp_path / "frames.bin")
    with open(path, "wb") as f:
        np.array([len(frames), I.CAM.width, I.CAM.height], np.int32).tofile(f)
        np.array([I.CAM.fx, I.CAM.fy, I.CAM.cx, I.CAM.cy, I.CAM.near, I.CAM.far, 0.008], np.float32).tofile(f)
        for depth, rgba, quality, pose in frames:
            np.ascontiguousarray(pose, np.float32).reshape(12).tofile(f)
            np.ascontiguousarray(synth.pose_inverse16(pose), np.float32).reshape(16).tofile(f)
            np.ascontiguousarray(depth, np.float32).tofile(f)
            np.ascontiguousarray(rgba, np.uint8).tofile(f)
            np.ascontiguousarray(quality, np.float32).tofile(f)
    exe = str(tmp_path / "resident_vs_host")
    src = os.path.join(ROOT, "tests", "cpp_texmap", "resident_vs_host.cpp")
    lib = os.path.join(ROOT, "texturefusion_amd")
    subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", src, "-o", exe, "-L" + lib, "-ltexfusion_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True, timeout=300)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "resident ok" in r.stdout, r.stdout + r.stderr
