"""Problem instances of the view-selection tests (tests/mrf_ref.py has the layout): the same generators feed the CPU tests of
the restatement and the device tests, so both judge the same cases."""
from __future__ import annotations

import numpy as np

STEP = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))  # chisel::neighbourhood


def lattice(ids, keep_edge):
    """nbr [n, 6] of the nodes at integer points `ids`: an edge joins face neighbours for which keep_edge(i, j) (called
    once per pair, i the -a end)."""
    ids = np.asarray(ids, np.int32).reshape(-1, 3)
    at = {tuple(int(c) for c in p): i for i, p in enumerate(ids)}
    nbr = np.full((len(ids), 6), -1, np.int32)
    for i, p in enumerate(ids):
        for k in (1, 3, 5):
            j = at.get((int(p[0]) + STEP[k][0], int(p[1]) + STEP[k][1], int(p[2]) + STEP[k][2]))
            if j is not None and keep_edge(i, j):
                nbr[i, k] = j
                nbr[j, k ^ 1] = i
    return ids, nbr


def columns(label_sets, cost_sets):
    col_off = np.zeros(len(label_sets) + 1, np.int64)
    col_off[1:] = np.cumsum([len(s) for s in label_sets])
    labels = np.concatenate([np.asarray(s, np.int32) for s in label_sets])
    costs = np.concatenate([np.asarray(c, np.float32) for c in cost_sets])
    return col_off, labels, costs


def quality_costs(rng, k):
    """1 - q / qmax in f32, the reference's unary (Structure/TexMap.cpp:168-175)"""
    q = rng.uniform(0.05, 1.0, k).astype(np.float32)
    return (np.float32(1.0) - q / q.max()).astype(np.float32)


def grid_costs(rng, k):
    """multiples of 2^-6 in [0, 1]: every f32 sum of a line is exact"""
    return (rng.integers(0, 65, k) / 64.0).astype(np.float32)


def random_columns(rng, n, pool, kmin, kmax, cost_fn):
    ls, cs = [], []
    for _ in range(n):
        k = int(rng.integers(kmin, kmax + 1))
        ls.append(np.sort(rng.choice(pool, k, replace=False)))
        cs.append(cost_fn(rng, k))
    return columns(ls, cs)


def line_instance(seed):
    """disjoint straight lines, one or two along each axis, 2-8 nodes each, 1-3 labels out of a pool of 4"""
    rng = np.random.default_rng(1000 + seed)
    ids = []
    for a in range(3):
        for rep in range(int(rng.integers(1, 3))):
            base = [20 * a + 5 * rep + int(rng.integers(-3, 3)), 100 * (rep + 1) + 10 * a, -50 * a + 7 * rep]
            for t in range(int(rng.integers(2, 9))):
                p = list(base)
                p[a] += t
                ids.append(p)
    ids, nbr = lattice(ids, lambda i, j: True)
    return (ids, nbr) + random_columns(rng, len(ids), np.arange(1, 5), 1, 3, grid_costs)


def small_grid(seed):
    """3 x 2 x 2, 85 % of the edges, 1-3 labels out of a pool of 4, quality costs"""
    rng = np.random.default_rng(5000 + seed)
    ids = [(x - 1, y + 3, z - 7) for x in range(3) for y in range(2) for z in range(2)]
    ids, nbr = lattice(ids, lambda i, j: rng.random() < 0.85)
    return (ids, nbr) + random_columns(rng, len(ids), np.arange(1, 5), 1, 3, quality_costs)


def sheet(nx=40, ny=30, nz=2, seed=7, pool=12, kmin=2, kmax=6, p_edge=0.9):
    rng = np.random.default_rng(seed)
    ids = [(x - nx // 2, y - 3, z) for x in range(nx) for y in range(ny) for z in range(nz)]
    ids, nbr = lattice(ids, lambda i, j: rng.random() < p_edge)
    return (ids, nbr) + random_columns(rng, len(ids), np.arange(1, pool + 1), kmin, kmax, quality_costs)


def many_labels(seed=3):
    """an L of 9 nodes whose corner has 150 labels, with label values up to 20 000"""
    rng = np.random.default_rng(seed)
    ids = [(t, 0, 0) for t in range(5)] + [(2, t, 0) for t in range(1, 5)]
    ids, nbr = lattice(ids, lambda i, j: True)
    pool = np.concatenate([np.arange(1, 200), [5000, 19999, 20000]])
    ls, cs = [], []
    for i in range(len(ids)):
        k = 150 if i == 2 else int(rng.integers(2, 70))
        ls.append(np.sort(rng.choice(pool, k, replace=False)))
        cs.append(quality_costs(rng, k))
    return (ids, nbr) + columns(ls, cs)


def with_unlabelled(seed=11):
    """a 6 x 5 x 1 sheet in which some nodes have the single label 0 at cost 1 and no edges (empty cost columns as
    TexMap::view_selection hands them over) and some labelled nodes are isolated"""
    rng = np.random.default_rng(seed)
    ids = [(x, y, 4) for x in range(6) for y in range(5)]
    empty = rng.random(len(ids)) < 0.2
    alone = rng.random(len(ids)) < 0.15
    ids, nbr = lattice(ids, lambda i, j: not (empty[i] or empty[j] or alone[i] or alone[j]))
    ls, cs = [], []
    for i in range(len(ids)):
        if empty[i]:
            ls.append([0]); cs.append([1.0])
        else:
            k = int(rng.integers(1, 5))
            ls.append(np.sort(rng.choice(np.arange(1, 8), k, replace=False)))
            cs.append(quality_costs(rng, k))
    return (ids, nbr) + columns(ls, cs)


N_LINES = 60
N_GRIDS = 200
