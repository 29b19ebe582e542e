"""The census of tests/texmap_edge_inputs.py, on the CPU: the hand-built keyframe sequence, replayed on the oracle and the
restatement (tests/texmap_ref.py) alone, reaches every edge of the resident TexMap's row walk that
tests/test_gpu_texmap_edges.py relies on.  These are conditions on the inputs, not measurements of the device: where one
fails, the GPU file's comparison no longer means what it says.  Every assert names the step of the sequence it guards.

No GPU."""
import time

import numpy as np
import pytest

from tests import mrf_ref as R
from tests import texmap_edge_inputs as E


def _rows(tm):
    """rows of every node's column"""
    return [[r for r, _ in tm._column(k)] for k in range(tm.chunkGraph.num_nodes())]


def _ties(p):
    """nodes of problem p whose cheapest cost stands at least twice, in rows of different blocks of 64:
    -> [(node, lowest tied offset, highest tied offset)]"""
    out = []
    for i in range(len(p["ids"])):
        a, b = int(p["col_off"][i]), int(p["col_off"][i + 1])
        c = p["costs"][a:b].view(np.uint32)
        tied = np.nonzero(c == c[np.argmin(p["costs"][a:b])])[0]
        blocks = {(int(p["labels"][a + j]) - 1) // 64 for j in tied}
        if len(tied) >= 2 and len(blocks) >= 2 and p["labels"][a] != 0:
            out.append((i, int(tied[0]), int(tied[-1])))
    return out


@pytest.fixture(scope="module")
def census():
    t0 = time.perf_counter()
    run = E.Run()
    cps = {}
    try:
        for cp in run.play():
            tm = run.tm
            cp.rows = _rows(tm)
            cp.chunk_labels = list(tm.chunkGraph.labels)
            if cp.solved:
                p = tm.problem
                cp.problem = {k: (None if v is None else np.array(v).copy()) for k, v in p.items() if k != "nodes"}
                cp.chosen = run.chosen_labels().copy()
                cp.warm = p["init"] is not None
                cp.late_hits = 0 if not cp.warm else sum(
                    1 for i in range(len(p["init"])) if p["init"][i] > 0 and p["labels"][p["col_off"][i] + p["init"][i]] > 64)
            if cp.name == "g":
                cp.graph = ({c: k for c, k in tm.chunkGraph.chunks.items()}, [list(a) for a in tm.chunkGraph.adj_lists])
            cps[cp.name] = cp
        yield SimpleCensus(cps, run.facts, run.improved, time.perf_counter() - t0)
    finally:
        run.close()


class SimpleCensus:
    def __init__(self, cps, facts, improved, seconds):
        self.cps, self.facts, self.improved, self.seconds = cps, facts, improved, seconds


def test_the_sequence_has_every_checkpoint(census):
    names = ["rows %d" % n for n in E.SIZES] + ["c1", "c2", "d1", "d2", "e", "b", "g", "f", "f2", "h full", "h sub"]
    assert list(census.cps) == names
    assert E.SIZES[:8] == (1, 2, 63, 64, 65, 127, 128, 129) and E.SIZES[8] >= 130           # step a
    assert all(len(census.cps["rows %d" % n].kflist) == n for n in E.SIZES)                 # step a
    assert len(set(E.frame_of(r) for r in range(E.N_MAIN + 3))) == E.N_MAIN + 3
    assert all(E.frame_of(r) != r and E.frame_of(r) != r + 1 for r in range(E.N_MAIN + 3))  # a row is no frame index


@pytest.mark.parametrize("name", ["rows %d" % E.SIZES[-1], "f"])
def test_columns_reach_the_block_boundaries(census, name):
    """the full table, as it grew (step a) and as one update rebuilt it (step b)"""
    cols = census.cps[name].rows
    assert any(c and c[0] < 64 <= c[-1] for c in cols), "a column on both sides of row 64"
    assert any(c and c[0] < 128 <= c[-1] for c in cols), "a column on both sides of row 128"
    assert any(c and c[0] >= 64 for c in cols), "a column with entries only in rows >= 64"
    assert any(c and c[-1] == 63 for c in cols), "a column whose last entry is row 63"
    assert any(c and c[0] == 64 for c in cols), "a column whose first entry is row 64"
    assert any(63 in c and 64 in c for c in cols), "a column with rows 63 and 64"
    assert any(127 in c and 128 in c for c in cols), "a column with rows 127 and 128"
    assert any(not c for c in cols), "an empty column"
    n = len(cols) * max(len(c) for c in cols)
    assert len(cols) >= 64 and max(len(c) for c in cols) > 64 and n < 16384, "far below the cost table's 64 k entries"


def test_the_intermediate_tables_end_at_their_newest_row(census):
    """step a: at 63, 64, 65, 127, 128 and 129 rows the newest keyframe -- the last lane in use of the last block -- is in
    some column, and the update that put it there named every keyframe since the checkpoint before"""
    for n in E.SIZES[2:8]:
        cols = census.cps["rows %d" % n].rows
        assert any(c and c[-1] == n - 1 for c in cols), n
    assert any(len(c) >= 60 for c in census.cps["rows 63"].rows), "step b: one update fills 60 rows of a column"


def test_sizes_one_and_two(census):
    """step a: at 1 row every node solves to label 0 and keeps chunk label 0; at 2 rows a node with an empty column takes
    kflist[-2], the seed keyframe"""
    one, two = census.cps["rows 1"], census.cps["rows 2"]
    assert len(one.chosen) >= 64 and not one.chosen.any() and not any(one.chunk_labels)
    assert not one.warm and two.warm
    empty = [k for k, c in enumerate(two.rows) if not c]
    full = [k for k, c in enumerate(two.rows) if c]
    assert empty and full
    assert all(two.chunk_labels[k] == E.SEED_KF for k in empty) and all(two.chunk_labels[k] == E.frame_of(1) for k in full)


@pytest.mark.parametrize("name", ["g", "f"])
def test_a_tie_for_the_cheapest_label_crosses_a_block(census, name):
    """step f: the twins' costs are bit-equal (0.0) with one entry per block; the cold start -- the sub-problem's and the
    first full solve's -- sits on the lower offset, and the higher one would be seen: another first trace value or
    another solved label"""
    cp = census.cps[name]
    p = cp.problem
    assert not cp.warm
    ties = _ties(p)
    assert len(ties) >= 4, name
    start = R.argmin_init(p["col_off"], p["costs"])
    rows = set()
    for i, lo, hi in ties:
        a = int(p["col_off"][i])
        assert start[i] == lo and p["costs"][a + lo] == 0.0 and p["costs"][a + hi] == 0.0
        rows |= {int(p["labels"][a + lo]) - 1, int(p["labels"][a + hi]) - 1}
    assert {E.TWINS[0], E.TWINS[2]} <= rows, "the twins' rows are the tied ones"
    # (rows 30 and 94 meet on one lane of the walk, 94 and 100 in one block: both ways of breaking the tie are asked)
    assert E.TWINS[0] % 64 == E.TWINS[1] % 64 != E.TWINS[2] % 64 and E.TWINS[0] // 64 != E.TWINS[1] // 64 == E.TWINS[2] // 64
    off, rounds, trace = cp.solution
    for pick in (1, 2):  # the highest tied offset; the next to lowest
        alt = start.copy()
        for i, lo, hi in ties:
            a, b = int(p["col_off"][i]), int(p["col_off"][i + 1])
            tied = np.nonzero(p["costs"][a:b].view(np.uint32) == p["costs"][a + lo].view(np.uint32))[0]
            alt[i] = tied[-1] if pick == 1 else tied[1]
        off2, rounds2, trace2 = R.solve(p["ids"], p["nbr"], p["col_off"], p["labels"], p["costs"], np.float32(0.5), init=alt)
        seen = trace2[0] != trace[0] or not np.array_equal(p["labels"][p["col_off"][:-1] + off2], cp.chosen)
        assert seen, "a start on another tied offset would go unseen (%s, pick %d)" % (name, pick)


def test_warm_starts_land_inside_later_blocks(census):
    """step a / f2: a stored label > 64 found at a non-zero offset; a second full solve straight after the first starts
    from every offset the first one chose"""
    assert census.cps["rows 128"].late_hits >= 1 and census.cps["f2"].late_hits >= 1
    f, f2 = census.cps["f"], census.cps["f2"]
    assert f2.warm and np.array_equal(f2.problem["init"], f.solution[0])
    # ... among them a start in a column whose first entry is row 64: offset > 0 with nothing in block 0 before it
    p = f2.problem
    first = [int(p["labels"][p["col_off"][i]]) for i in range(len(p["init"]))]
    assert any(first[i] == 65 and p["init"][i] > 0 for i in range(len(first)))


def test_retraction_zeroes_warm_starts(census):
    """step d: the retracted keyframes stand in rows >= 64, nodes had chosen them, and the warm solve behind the
    retraction finds their stored labels gone; the re-integration brings both back"""
    d = census.facts["d"]
    assert len(d["rows"]) == 2 and all(r >= 64 for r in d["rows"]) and d["warm_zeroed"] >= 1
    before, gone, back = census.cps["c2"], census.cps["d1"], census.cps["d2"]
    for r in d["rows"]:
        assert (before.chosen == r + 1).any()
        assert any(r in c for c in before.rows) and not any(r in c for c in gone.rows) and any(r in c for c in back.rows)
    assert gone.warm and back.warm


def test_solves_have_work_and_choose_late_rows(census):
    assert census.improved >= 1, "a solve of >= 2 rounds that ends strictly below its start"
    chosen = np.concatenate([cp.chosen for cp in census.cps.values() if cp.solved])
    assert (chosen > 64).any() and (chosen > 128).any()
    for cp in census.cps.values():
        if cp.solved:
            assert (np.diff(cp.solution[2]) <= 0).all(), cp.name


def test_add_value_keeps_and_set_value_overwrites(census):
    """step c: the second integration changes the oracle's observation; update(ids, kf, []) leaves the restatement's
    column as it was; naming the keyframe in frames_to_update changes it"""
    c = census.facts["c"]
    changed = [x for x in c["watch"] if c["obs0"][x] != c["obs1"][x] and c["obs1"][x] > 0.0]
    assert changed and c["col1"] == c["col0"]
    assert all(c["col0"][x] == np.float32(c["obs0"][x]) for x in c["watch"])
    assert all(c["col2"][x] == np.float32(c["obs1"][x]) != c["col0"][x] for x in changed)


def test_retract_ids_outside_the_graph(census):
    """step e: the volume holds chunks that are no nodes; the retraction changes some columns and leaves others"""
    assert census.facts["e"]["bare"] >= 1
    before, after = census.cps["d2"].rows, census.cps["e"].rows
    lost = [k for k in range(len(before)) if E.E_ROW in before[k] and E.E_ROW not in after[k]]
    kept = [k for k in range(len(before)) if E.E_ROW in before[k] and E.E_ROW in after[k]]
    assert lost and kept


def test_the_subset_of_the_sub_problem(census):
    """step g: a chunk listed twice is one node; listed nodes have graph neighbours that are left out; a listed node with
    an empty column has a listed neighbour with a filled one, which gets no edge to it"""
    cp = census.cps["g"]
    chunks, adj = cp.graph
    listed = [E.tup(c) for c in cp.sub]
    assert len(listed) > len(set(listed)) == len(cp.problem["ids"])
    inside = {chunks[c] for c in listed}
    assert any(j not in inside for k in inside for j in adj[k]), "a neighbour left out"
    hollow = [(k, j) for k in inside if not cp.rows[k] for j in adj[k] if j in inside and cp.rows[j]]
    assert hollow, "a listed node with an empty column beside a listed node with a filled one"
    local = {E.tup(c): i for i, c in enumerate(cp.problem["ids"])}
    id_of = {k: c for c, k in chunks.items()}
    for k, j in hollow:
        assert local[id_of[k]] not in cp.problem["nbr"][local[id_of[j]]].tolist()


def test_the_replay_is_quick(census):
    assert census.seconds < 5.0, census.seconds
