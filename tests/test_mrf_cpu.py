"""The numpy restatement of the view-selection solve (tests/mrf_ref.py) against what can be proved from the energy
    E(x) = sum_i u_i(x_i) + w * sum_(i,j) [label_i != label_j]
itself: exact optima on instances made of straight lines, a monotone trace, line-wise fixed points, and the edge cases of
the interface.  No GPU: the device tests (tests/test_gpu_view_selection.py) then compare the kernels with this file's
subject bit for bit."""
import numpy as np
import pytest

from tests import mrf_inputs as I
from tests import mrf_ref as R

W = np.float32(0.5)


def _solve(p, **kw):
    ids, nbr, col_off, labels, costs = p
    off, rounds, trace = R.solve(ids, nbr, col_off, labels, costs, W, **kw)
    assert len(trace) == rounds + 1
    assert trace[-1] == R.energy(nbr, col_off, labels, costs, W, off)
    return off, rounds, trace


def _lines(nbr, a):
    for h in range(len(nbr)):
        if nbr[h, 2 * a] == -1:
            yield R._line_nodes(nbr, h, a)


def _assert_line_fixed_point(p, off, max_len=6):
    """no line of any axis has a strictly better labelling with the rest fixed (brute force, lines of <= max_len nodes)"""
    ids, nbr, col_off, labels, costs = p
    e = R.energy(nbr, col_off, labels, costs, W, off)
    for a in range(3):
        for nodes in _lines(nbr, a):
            if len(nodes) > max_len or np.prod([col_off[t + 1] - col_off[t] for t in nodes], dtype=np.int64) > 1 << 16:
                continue
            best, _ = R.brute_force(nbr, col_off, labels, costs, W, free=nodes, offsets=off)
            assert best >= e, (a, nodes, best, e)


@pytest.mark.parametrize("block", range(6))
def test_straight_lines_reach_the_optimum(block):
    for seed in range(block * 10, block * 10 + 10):
        p = I.line_instance(seed)
        off, rounds, trace = _solve(p)
        best, _ = _line_optimum(p)
        assert trace[-1] == best, (seed, trace, best)
        assert rounds < R.DEFAULT_ROUNDS
        assert np.all(np.diff(trace) <= 0)
        _assert_line_fixed_point(p, off)


def _line_optimum(p):
    """the lines are disjoint: the optimum is the sum of each line's own (sums of multiples of 2^-6: exact)"""
    ids, nbr, col_off, labels, costs = p
    total, seen = 0.0, 0
    zero = np.zeros(len(ids), np.int32)
    base = R.energy(nbr, col_off, labels, costs, W, zero)
    for a in range(3):
        for nodes in _lines(nbr, a):
            if len(nodes) == 1 and any(nbr[nodes[0], k] >= 0 for k in range(6)):
                continue  # a node of a line of another axis
            best, _ = R.brute_force(nbr, col_off, labels, costs, W, free=nodes, offsets=zero)
            total += best - base
            seen += len(nodes)
    assert seen == len(ids)
    return base + total, None


@pytest.mark.parametrize("block", range(8))
def test_small_loopy_grids(block):
    for seed in range(block * 25, block * 25 + 25):
        p = I.small_grid(seed)
        ids, nbr, col_off, labels, costs = p
        off, rounds, trace = _solve(p)
        assert np.all(np.diff(trace) <= 0), (seed, trace)
        assert trace[0] == R.energy(nbr, col_off, labels, costs, W, R.argmin_init(col_off, costs))
        assert trace[-1] <= trace[0]
        assert rounds < R.DEFAULT_ROUNDS, seed
        best, _ = R.brute_force(nbr, col_off, labels, costs, W)
        assert trace[-1] >= best  # (no optimality bar: the gap's distribution is in DESIGN.md s.7d)
        _assert_line_fixed_point(p, off)


def test_sheet_is_monotone_and_converges():
    p = I.sheet()
    off, rounds, trace = _solve(p)
    assert np.all(np.diff(trace) <= 0), trace
    assert trace[-1] < trace[0] and rounds < R.DEFAULT_ROUNDS
    _assert_line_fixed_point(p, off, max_len=2)


def test_many_labels_and_large_label_values():
    p = I.many_labels()
    ids, nbr, col_off, labels, costs = p
    assert (np.diff(col_off) == 150).any() and labels.max() == 20000
    off, rounds, trace = _solve(p)
    assert np.all(np.diff(trace) <= 0) and rounds < R.DEFAULT_ROUNDS
    assert np.all((off >= 0) & (off < np.diff(col_off)))


def test_unlabelled_and_isolated_nodes():
    p = I.with_unlabelled()
    ids, nbr, col_off, labels, costs = p
    off, rounds, trace = _solve(p)
    lab = R.node_labels(col_off, labels, off)
    zero = labels[col_off[:-1]] == 0
    assert zero.any() and np.all(lab[zero] == 0) and np.all(nbr[zero] == -1)
    alone = np.all(nbr == -1, axis=1) & ~zero
    assert alone.any() and np.array_equal(off[alone], R.argmin_init(col_off, costs)[alone])
    _assert_line_fixed_point(p, off)


def test_warm_start_at_the_solution_changes_nothing():
    for p in (I.sheet(12, 9, 2, seed=2), I.small_grid(3), I.line_instance(4)):
        off, rounds, trace = _solve(p)
        off2, rounds2, trace2 = _solve(p, init=off)
        assert rounds2 == 1 and np.array_equal(off2, off)
        assert trace2[0] == trace2[1] == trace[-1]


def test_max_rounds_one():
    p = I.sheet(12, 9, 2, seed=2)
    off, rounds, trace = _solve(p)
    assert rounds > 2
    off1, rounds1, trace1 = _solve(p, max_rounds=1)
    assert rounds1 == 1 and len(trace1) == 2 and np.array_equal(trace1, trace[:2])


def test_single_node():
    col_off, labels, costs = I.columns([[3, 7, 9]], [[0.5, 0.25, 0.25]])
    ids, nbr = I.lattice([(4, -2, 0)], lambda i, j: True)
    off, rounds, trace = _solve((ids, nbr, col_off, labels, costs))
    assert off.tolist() == [1] and rounds == 1 and trace.tolist() == [0.25, 0.25]
    off, rounds, trace = _solve((ids, nbr, col_off, labels, costs), init=[0])
    assert off.tolist() == [1] and rounds == 2 and trace.tolist() == [0.5, 0.25, 0.25]
