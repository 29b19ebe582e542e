"""The resident TexMap (tf_texmap.hip: tm_for_rows, k_tm_update, k_tm_count, k_tm_fill, k_tm_assign, k_tm_download) on the
hand-built keyframe sequence of tests/texmap_edge_inputs.py, whose keyframe table grows past two blocks of 64 rows:
columns that straddle rows 64 and 128, that start at row 64, that end at row 63; warm starts found in a later block; ties
for the cheapest label that cross a block; tables of 1, 2, 63, 64, 65, 127, 128 and 129 rows; add_value / set_value /
remove and the re-use of a cost-table key whose quality is 0.  tests/test_texmap_edges_cpu.py proves on the CPU that the
sequence reaches each of these.

The sequence runs once per form (call by call; the last two keyframes through tf_texture_tail_device) on a module-scoped
volume; at every checkpoint the device's downloads are recorded beside the restatement's views, and the tests compare
the records.  No tolerance anywhere: integers and raw bits, by chunk id."""
import numpy as np
import pytest

from tests import texmap_edge_inputs as E
from tests import texmap_ref as T
from texturefusion_amd import capi

pytestmark = pytest.mark.gpu
MAP_KEYS = ("is_node", "edges", "label", "stored", "col_off", "col_frame", "col_q")
PATCH_KEYS = ("texloc", "frameid", "bbox", "flags", "ratio", "texcoord", "texcolor")


def _view(P):
    return T.problem_view_of(P["ids"], P["nbr"], P["col_off"], P["labels"], P["costs"], P["init"])


def _solved(P):
    """chunk id -> (solved offset, solved label)"""
    return {E.tup(P["ids"][i]): (int(P["offsets"][i]), int(P["labels"][P["col_off"][i] + P["offsets"][i]])) for i in range(len(P["ids"]))}


def _record(tail, hot_of=None, compare=True):
    """the sequence on a fresh volume -> its checkpoints, each with the device's downloads (and the restatement's views)"""
    gv = capi.Volume(E.RES8, E.CAM, max_chunks=E.MAX_CHUNKS, max_keyframes=E.MAX_KEYFRAMES)
    run = E.Run(gv, tail=tail)
    out = {}
    try:
        for cp in run.play():
            views = run.tm.all_node_views(run.kflist)
            bare = [E.tup(c) for c in run.ov.list_chunks() if E.tup(c) not in views]
            cp.map_ids = sorted(views) + bare[::7] + [E.NO_CHUNK]
            cp.map = gv.texmap_download(np.array(cp.map_ids, np.int32))
            if compare:
                cp.want_map = views
            if cp.solved:
                cp.P = P = gv.texmap_problem()
                if compare:
                    p, off = run.tm.problem, run.tm.solution[0]
                    cp.want_problem = run.tm.problem_view()
                    cp.want_solved = {E.tup(p["ids"][i]): (int(off[i]), int(p["labels"][p["col_off"][i] + off[i]])) for i in range(len(off))}
                    warm = bool((P["init"] >= 0).all())
                    cp.host = gv.view_select(P["ids"], P["nbr"], P["col_off"], P["labels"], P["costs"], np.float32(0.5),
                                             init=P["init"] if warm else None)
            if cp.name.startswith("h "):
                hot = cp.hot if hot_of is None else hot_of[cp.name]
                w = 13824  # Atlas::MAX_PATCH_WIDTH, the default tf_config.atlas_w
                cp.hot = hot
                cp.patches = gv.get_patches(cp.ids)
                cp.atlas = (gv.atlas_loc_next(), gv.atlas_rows(hot[0] // w, hot[1] // w + 1, w))
            out[cp.name] = cp
        return out
    finally:
        run.close()
        gv.close()


@pytest.fixture(scope="module")
def by_call(gpu_required):
    return _record(False)


@pytest.fixture(scope="module")
def by_tail(gpu_required, by_call):
    return _record(True, hot_of={n: cp.hot for n, cp in by_call.items() if n.startswith("h ")})


def test_exports_equal_the_oracle(by_call):
    """what every update of step a consumes, before the map is looked at: a failure here is the observations' or the
    mesher's, not the map's"""
    for n in E.SIZES:
        want, got, want_e, got_e = by_call["rows %d" % n].exports
        assert np.array_equal(want.view(np.uint32), got.view(np.uint32)), n
        assert got_e == want_e and (n == 1 or (want > 0).any()), n
    assert by_call["rows 127"].exports[0].shape[1] == 127 - 65  # the newest keyframe and the 61 since the last checkpoint


def _check_map(cp):
    d = cp.map
    for i, cid in enumerate(cp.map_ids):
        a, b = int(d["col_off"][i]), int(d["col_off"][i + 1])
        if cid not in cp.want_map:
            assert d["is_node"][i] == 0 and d["edges"][i] == 0 and a == b, (cp.name, cid)
            continue
        mask, label, stored, col = cp.want_map[cid]
        got = list(zip(d["col_frame"][a:b].tolist(), d["col_q"][a:b].view(np.uint32).tolist()))
        assert d["is_node"][i] == 1 and int(d["edges"][i]) == mask, (cp.name, cid, int(d["edges"][i]), mask)
        assert int(d["label"][i]) == label and int(d["stored"][i]) == stored, (cp.name, cid, d["label"][i], label, d["stored"][i], stored)
        assert got == col, (cp.name, cid, got, col)


@pytest.mark.parametrize("form", ["by_call", "by_tail"])
def test_map_at_every_checkpoint(form, request):
    """node set, edge masks, chunk labels, stored labels and columns (frame, quality bits) of every node, of some chunks
    that are none and of an id the volume never held"""
    cps = request.getfixturevalue(form)
    assert len(cps) == len(E.SIZES) + 11
    for cp in cps.values():
        _check_map(cp)


@pytest.mark.parametrize("form", ["by_call", "by_tail"])
def test_problem_at_every_solve(form, request):
    """the downloaded problem (ids, neighbours by chunk id, labels, cost bits, start), the solved offsets and labels,
    rounds and the f64 trace byte for byte; the same problem through the host form tf_view_select"""
    cps = request.getfixturevalue(form)
    n_solved = 0
    for cp in cps.values():
        if not cp.solved:
            continue
        n_solved += 1
        P = cp.P
        off, rounds, trace = cp.solution
        assert len(P["ids"]) == len(off), (cp.name, len(P["ids"]), len(off))
        assert _view(P) == cp.want_problem, cp.name
        assert _solved(P) == cp.want_solved, cp.name
        h_off, h_r, h_tr = cp.host
        assert h_r == rounds and h_tr.tobytes() == trace.tobytes() and np.array_equal(h_off, P["offsets"]), cp.name
        if cp.g_solution is not None:  # (the tail hands no trace back)
            gn, gr, gt = cp.g_solution
            print(cp.name, "nodes", gn, "rounds", gr, "trace", gt.tolist())
            assert gn == len(off) and gr == rounds, (cp.name, gn, len(off), gr, rounds)
            assert gt.tobytes() == trace.tobytes(), (cp.name, gt, trace)
    assert n_solved == len(E.SIZES) + 8


def test_cold_and_warm_starts_are_where_the_sequence_puts_them(by_call):
    cold = [n for n, cp in by_call.items() if cp.solved and (cp.P["init"] == -1).all()]
    warm = [n for n, cp in by_call.items() if cp.solved and (cp.P["init"] >= 0).all()]
    assert cold == ["rows 1", "g", "f", "h sub"] and len(cold) + len(warm) == len(E.SIZES) + 8


@pytest.mark.parametrize("form", ["by_call", "by_tail"])
def test_properties_of_the_devices_own_downloads(form, request):
    """nothing here is shared with tests/texmap_ref.py: the labels of a column ascend strictly and each is 1 + the row of
    its frame in the table that was set; a filled column holds a cost of exactly 0.0 and all its costs lie in [0, 1), an
    empty one is the single label 0 at cost 1.0; col_off is the running sum of max(len, 1); the trace never rises"""
    cps = request.getfixturevalue(form)
    longest = 0
    for cp in cps.values():
        if not cp.solved:
            continue
        row_of = {f: r for r, f in enumerate(cp.kflist)}
        d, P = cp.map, cp.P
        at = {cid: i for i, cid in enumerate(cp.map_ids)}
        assert P["col_off"][0] == 0
        for i in range(len(P["ids"])):
            cid = E.tup(P["ids"][i])
            m = at[cid]
            frames = d["col_frame"][int(d["col_off"][m]):int(d["col_off"][m + 1])].tolist()
            a, b = int(P["col_off"][i]), int(P["col_off"][i + 1])
            L, c = P["labels"][a:b], P["costs"][a:b]
            assert b - a == max(len(frames), 1), (cp.name, cid)
            if not frames:
                assert L.tolist() == [0] and c.tolist() == [1.0], (cp.name, cid)
                continue
            assert L.tolist() == [1 + row_of[f] for f in frames], (cp.name, cid)
            assert (np.diff(L) > 0).all() and (c == 0.0).any() and (c >= 0.0).all() and (c < 1.0).all(), (cp.name, cid)
            longest = max(longest, b - a)
        if cp.g_solution is not None:
            assert (np.diff(cp.g_solution[2]) <= 0).all(), cp.name
    assert longest > 64


def test_tables_of_one_and_two_rows(by_call):
    """step a, literally: at 1 row every node solves to label 0 and its chunk label stays 0 (n_rows >= 2 is false); at 2
    rows a node with an empty column takes kflist[-2], every other node the one keyframe it has"""
    one, two = by_call["rows 1"], by_call["rows 2"]
    nodes = one.map["is_node"] == 1
    assert nodes.sum() >= 64 and one.map["col_off"][-1] == 0
    assert not one.P["labels"].any() and not one.map["label"][nodes].any() and not one.map["stored"][nodes].any()
    d = two.map
    nodes = np.nonzero(d["is_node"] == 1)[0]
    lens = np.diff(d["col_off"])[nodes]
    assert (lens == 0).any() and (lens == 1).any() and lens.max() == 1
    assert (d["label"][nodes][lens == 0] == two.kflist[-2]).all() and (d["label"][nodes][lens == 1] == two.kflist[-1]).all()
    assert (d["stored"][nodes][lens == 0] == 0).all() and (d["stored"][nodes][lens == 1] == 2).all()


def test_tail_equals_the_call_by_call_sequence(by_call, by_tail):
    """step h: the last two keyframes' tails as ONE call each (full, then TF_TAIL_SUB_PROBLEM) leave what the call-by-call
    sequence leaves: map, problem with its start and solved offsets, patches of chunksToUpdate, hot atlas rows"""
    for name in ("h full", "h sub"):
        a, b = by_call[name], by_tail[name]
        for k in MAP_KEYS:
            assert a.map[k].tobytes() == b.map[k].tobytes(), (name, k)
        assert _view(a.P) == _view(b.P) and _solved(a.P) == _solved(b.P), name
        for k in PATCH_KEYS:
            assert a.patches[k].tobytes() == b.patches[k].tobytes(), (name, k)
        assert a.atlas[0] == b.atlas[0] and a.atlas[1].tobytes() == b.atlas[1].tobytes(), name
        assert (a.patches["texloc"] != np.uint64((1 << 64) - 1)).any() and a.atlas[1].any(), name


def test_a_repeat_on_a_fresh_volume_gives_the_same_bytes(by_call):
    again = _record(False, compare=False)
    assert list(again) == list(by_call)
    for name, a in by_call.items():
        b = again[name]
        assert a.map_ids == b.map_ids
        for k in MAP_KEYS:
            assert a.map[k].tobytes() == b.map[k].tobytes(), (name, k)
        if a.solved:
            assert _view(a.P) == _view(b.P) and _solved(a.P) == _solved(b.P), name
            assert a.g_solution[1] == b.g_solution[1] and a.g_solution[2].tobytes() == b.g_solution[2].tobytes(), name
