"""numpy restatement of the view-selection solve (texturefusion_amd/csrc/tf_mrf.hip, tf_view_select): the same
schedule, the same recurrence in f32 and the same tie rules, so that offsets, rounds and energy trace can be compared
bit for bit.  Its own f64 energy() and a brute-force optimum for tiny instances are the yardsticks that do not depend
on the schedule.

    E(x) = sum_i u_i(x_i) + w * sum_(i,j) [label_i != label_j]

A problem is (ids [n, 3] i32, nbr [n, 6] i32 in chisel::neighbourhood order -x +x -y +y -z +z with -1 = no edge,
col_off [n + 1] i64, labels [nnz] i32 ascending within a node, costs [nnz] f32)."""
from __future__ import annotations

import numpy as np

DEFAULT_ROUNDS = 32
F32 = np.float32


def node_labels(col_off, labels, offsets):
    return np.asarray(labels)[np.asarray(col_off)[:-1] + np.asarray(offsets)]


def energy(nbr, col_off, labels, costs, w, offsets):
    """f64 energy of a labelling given as offsets; every edge counted once (from its -a end)."""
    nbr = np.asarray(nbr).reshape(-1, 6)
    col_off = np.asarray(col_off, np.int64)
    lab = node_labels(col_off, labels, offsets)
    e = np.asarray(costs, np.float32)[col_off[:-1] + np.asarray(offsets)].astype(np.float64).sum()
    cut = 0
    for k in (1, 3, 5):
        nb = nbr[:, k]
        has = nb >= 0
        cut += int(np.count_nonzero(lab[has] != lab[nb[has]]))
    return float(e + np.float64(F32(w)) * cut)


def argmin_init(col_off, costs):
    """the cheapest label of every node, lowest offset"""
    costs = np.asarray(costs, np.float32)
    return np.array([int(np.argmin(costs[col_off[i]:col_off[i + 1]])) for i in range(len(col_off) - 1)], np.int32)


def line_heads(ids, nbr):
    """heads[axis][cls]: nodes without a -axis neighbour whose other two coordinates sum to parity cls"""
    heads = [[[], []] for _ in range(3)]
    for i in range(len(nbr)):
        for a in range(3):
            if nbr[i, 2 * a] == -1:
                heads[a][int(ids[i, (a + 1) % 3] + ids[i, (a + 2) % 3]) & 1].append(i)
    return heads


def _line_nodes(nbr, head, a):
    out = []
    t = head
    while t >= 0:
        out.append(t)
        t = int(nbr[t, 2 * a + 1])
    return out


def _solve_line(nodes, a, nbr, col_off, labels, costs, w, off, cur):
    """One line with everything else fixed; rewrites off / cur in place when strictly better.  True if it did."""
    others = [k for k in range(6) if k >> 1 != a]
    choices = []
    m_prev = l_prev = None
    M_prev = F32(0)
    arg_prev = 0
    e = F32(0)
    lab_prev = -1
    for pos, t in enumerate(nodes):
        c0, c1 = int(col_off[t]), int(col_off[t + 1])
        L = labels[c0:c1]
        cnt = np.zeros(c1 - c0, np.float32)
        for k in others:
            nb = int(nbr[t, k])
            if nb >= 0:
                cnt += (L != cur[nb]).astype(np.float32)
        c = costs[c0:c1] + w * cnt                      # f32 + f32 * f32, each rounded
        if pos == 0:
            m = c
            ch = np.zeros(c1 - c0, np.int32)
        else:
            sw = F32(M_prev + w)
            idx = np.searchsorted(l_prev, L)
            idc = np.minimum(idx, len(l_prev) - 1)
            found = (idx < len(l_prev)) & (l_prev[idc] == L)
            stay = found & (m_prev[idc] <= sw)          # ties go to the same label
            best = np.where(stay, m_prev[idc], sw).astype(np.float32)
            ch = np.where(stay, idc, arg_prev).astype(np.int32)
            m = c + best
        choices.append(ch)
        cc = c[off[t]]
        if pos == 0:
            e = cc
        else:
            e = F32(cc + (e if cur[t] == lab_prev else F32(e + w)))
        lab_prev = cur[t]
        m_prev, l_prev = m, L
        arg_prev = int(np.argmin(m))                    # the lowest offset among equals
        M_prev = m[arg_prev]
    if not (M_prev < e):
        return False
    j = arg_prev
    for pos in range(len(nodes) - 1, -1, -1):
        t = nodes[pos]
        off[t] = j
        cur[t] = labels[col_off[t] + j]
        j = int(choices[pos][j])
    return True


def solve(ids, nbr, col_off, labels, costs, w=0.5, init=None, max_rounds=0):
    """-> (offsets i32[n], rounds, trace f64[rounds + 1]); trace[0] = the start labelling, trace[r] after round r."""
    ids = np.asarray(ids, np.int32).reshape(-1, 3)
    nbr = np.asarray(nbr, np.int32).reshape(-1, 6)
    col_off = np.asarray(col_off, np.int64)
    labels = np.asarray(labels, np.int32)
    costs = np.asarray(costs, np.float32)
    w = F32(w)
    R = max_rounds if max_rounds > 0 else DEFAULT_ROUNDS
    off = argmin_init(col_off, costs) if init is None else np.array(init, np.int32)
    cur = node_labels(col_off, labels, off).copy()
    heads = line_heads(ids, nbr)
    lines = [[[_line_nodes(nbr, h, a) for h in heads[a][c]] for c in range(2)] for a in range(3)]
    trace = [energy(nbr, col_off, labels, costs, w, off)]
    rounds = 0
    for r in range(1, R + 1):
        changed = False
        for a in range(3):
            for c in range(2):
                for nodes in lines[a][c]:
                    if _solve_line(nodes, a, nbr, col_off, labels, costs, w, off, cur):
                        changed = True
        trace.append(energy(nbr, col_off, labels, costs, w, off))
        rounds = r
        if not changed:
            break
    return off, rounds, np.array(trace, np.float64)


def brute_force(nbr, col_off, labels, costs, w=0.5, free=None, offsets=None):
    """(minimum f64 energy, one minimiser) over every labelling of the nodes in `free` (default: all), the others held
    at `offsets`.  Enumerates all labellings at once, in slabs of 2^18."""
    nbr = np.asarray(nbr).reshape(-1, 6)
    col_off = np.asarray(col_off, np.int64)
    labels = np.asarray(labels)
    costs64 = np.asarray(costs, np.float32).astype(np.float64)
    n = len(col_off) - 1
    free = list(range(n)) if free is None else list(free)
    base = np.zeros(n, np.int32) if offsets is None else np.array(offsets, np.int32)
    sizes = [int(col_off[i + 1] - col_off[i]) for i in free]
    total = int(np.prod(sizes, dtype=np.int64)) if sizes else 1
    w64 = np.float64(F32(w))
    edges = [(i, int(nbr[i, k])) for i in range(n) for k in (1, 3, 5) if nbr[i, k] >= 0]
    best, arg = None, None
    for lo in range(0, total, 1 << 18):
        hi = min(total, lo + (1 << 18))
        X = np.tile(base, (hi - lo, 1))
        if sizes:
            for i, col in zip(free, np.unravel_index(np.arange(lo, hi), sizes)):
                X[:, i] = col
        lab = labels[col_off[:-1][None, :] + X]
        e = costs64[col_off[:-1][None, :] + X].sum(axis=1)
        cut = np.zeros(hi - lo, np.int64)
        for i, j in edges:
            cut += lab[:, i] != lab[:, j]
        e = e + w64 * cut
        k = int(np.argmin(e))
        if best is None or e[k] < best:
            best, arg = float(e[k]), X[k].astype(np.int32)
    return best, arg
