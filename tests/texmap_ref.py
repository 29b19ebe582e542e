"""Python restatement of TexMap's bookkeeping (Structure/TexMap.cpp, uni_graph.cpp, sparse_matrix.cpp) -- the chunk graph,
the data-cost columns with their add_value / set_value / remove_* semantics, the problem the reference hands to mapMAP and
the assignment of the solved labels -- written from those files, fed from the oracle's observations() and
get_mesh()["adj"], solved with tests/mrf_ref.py.  It is the yardstick of the device-resident TexMap (tf_texmap_*)."""
from __future__ import annotations

import numpy as np

from tests import mrf_ref as R

NEIGHBOURHOOD = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))  # chisel::neighbourhood
F32 = np.float32


class SparseMat:
    """sparse_matrix.{h,cpp}: a vector of std::map<row, float> columns"""

    def __init__(self):
        self.column_wise = []
        self.nnz = 0
        self.row_len = 0

    def cols(self):
        return len(self.column_wise)

    def rows(self):
        return self.row_len

    def col(self, c):
        """ordered (row, value) pairs, as iterating the std::map gives them"""
        return sorted(self.column_wise[c].items())

    def resize(self, cols):
        if cols < len(self.column_wise):
            del self.column_wise[cols:]
        while len(self.column_wise) < cols:
            self.column_wise.append({})

    def add_value(self, col, row, value):  # :27-36: emplace keeps an existing entry
        if col >= len(self.column_wise):
            self.resize(col + 1)
        if row >= self.row_len:
            self.row_len = row + 1
        self.nnz += 1
        column = self.column_wise[col]
        if row in column:
            return False
        column[row] = F32(value)
        return True

    def set_value(self, col, row, value):  # :38-43
        if col >= len(self.column_wise):
            self.resize(col + 1)
        if row >= self.row_len:
            self.row_len = row + 1
        self.column_wise[col][row] = F32(value)

    def remove_observation(self, col, row):  # :45-50
        if col >= len(self.column_wise):
            return
        self.column_wise[col].pop(row, None)

    def remove_node(self, col):  # sparse_matrix.h:67-70
        if col >= len(self.column_wise):
            return
        self.column_wise[col].clear()

    def clear(self):
        self.column_wise = []
        self.nnz = 0
        self.row_len = 0


class UniGraph:
    """uni_graph.{h,cpp}"""

    def __init__(self):
        self.chunks = {}     # id -> node index
        self.adj_lists = []
        self.labels = []

    def num_nodes(self):
        return len(self.adj_lists)

    def add_node(self, cid):  # :22-28
        cid = tuple(int(x) for x in cid)
        if cid in self.chunks:
            return False
        self.chunks[cid] = len(self.adj_lists)
        self.adj_lists.append([])
        self.labels.append(0)
        return True

    def add_edge(self, a, b):  # "If the edge exists nothing happens"
        if b not in self.adj_lists[a]:
            self.adj_lists[a].append(b)
        if a not in self.adj_lists[b]:
            self.adj_lists[b].append(a)

    def add_edge_by_node(self, cid, flags):  # :41-49
        cid = tuple(int(x) for x in cid)
        if cid not in self.chunks:
            return
        n1 = self.chunks[cid]
        for k, d in enumerate(NEIGHBOURHOOD):
            other = (cid[0] + d[0], cid[1] + d[1], cid[2] + d[2])
            if flags[k] and other in self.chunks:
                self.add_edge(n1, self.chunks[other])

    def remove_node(self, cid):  # :89-107: the edges go, the index stays
        cid = tuple(int(x) for x in cid)
        if cid not in self.chunks:
            return
        n = self.chunks[cid]
        for hot in list(self.adj_lists[n]):
            self.adj_lists[hot] = [x for x in self.adj_lists[hot] if x != n]
        self.adj_lists[n] = []


class TexMap:
    """TexMap.cpp.  kflist = list of keyframe frame indices (KeyFrameDatabase::keyFrameIndex); lookup = frame -> row."""
    adjacent_cost = F32(0.5)
    pairwise_cost = F32(1.0)

    def __init__(self):
        self.chunkGraph = UniGraph()
        self.dataCost = SparseMat()
        self.labelstorage = []
        self.problem = None     # of the last solve: dict(nodes, ids, nbr, col_off, labels, costs, init)
        self.solution = None    # (offsets, rounds, trace)
        self.warm_zeroed = 0    # warm starts that put a node at offset 0 because its stored label had left the column

    # :50-61.  adj_of(cid) -> six flags, or None when the chunk owns no mesh
    def update_chunkgraph(self, chunks_to_update, adj_of):
        for cid in chunks_to_update:
            self.chunkGraph.add_node(cid)
        for cid in chunks_to_update:
            adj = adj_of(cid)
            if adj is not None:
                self.chunkGraph.add_edge_by_node(cid, adj)

    # :63-105.  obs_of(cid) -> dict frame -> quality (Chunk::observations)
    def update_datacost(self, chunks_to_update, obs_of, lookup, frameindex, frames_to_update):
        for cid in chunks_to_update:
            obs = obs_of(cid)
            node = self.chunkGraph.chunks[tuple(int(x) for x in cid)]
            quality = obs.get(frameindex, 0.0)
            if quality > 0.0:
                self.dataCost.add_value(node, lookup[frameindex], quality)
            if self.dataCost.cols() <= node:
                self.dataCost.resize(node + 1)
            for f in frames_to_update:
                if f not in obs:
                    self.dataCost.remove_observation(node, lookup[f])
                elif obs[f] > 0.0:
                    self.dataCost.set_value(node, lookup[f], obs[f])

    # MobileFusion::RetractObservations' data-cost half (MobileFusion.cpp:261-267); has_chunk(cid) -> bool
    def retract(self, frame_id, ids, lookup, has_chunk):
        for cid in ids:
            cid = tuple(int(x) for x in cid)
            if not has_chunk(cid) or cid not in self.chunkGraph.chunks:
                continue
            self.dataCost.remove_observation(self.chunkGraph.chunks[cid], lookup[frame_id])

    # MobileFusion.cpp:330-342.  wrong = iterable of (cid, patch frame id) of the meshes whose patch has wrong_mapping;
    # a chunk that is no node is skipped.  Returns the entries that were there.
    def remove_wrong_mapping(self, wrong, lookup):
        removed = 0
        for cid, frameid in wrong:
            cid = tuple(int(x) for x in cid)
            if cid not in self.chunkGraph.chunks or frameid not in lookup:
                continue
            node = self.chunkGraph.chunks[cid]
            if node < self.dataCost.cols() and lookup[frameid] in self.dataCost.column_wise[node]:
                removed += 1
            self.dataCost.remove_observation(node, lookup[frameid])
        return removed

    # :107-118.  has_mesh(cid) -> bool; returns the nodes found without a mesh
    def check_graph(self, has_mesh):
        cnt = 0
        for cid, node in self.chunkGraph.chunks.items():
            if not has_mesh(cid):
                self.chunkGraph.remove_node(cid)
                self.dataCost.remove_node(node)
                cnt += 1
        return cnt

    def _column(self, k):
        return self.dataCost.col(k) if k < self.dataCost.cols() else []

    def _build(self, nodes, warm):
        """the problem over graph nodes `nodes` as :123-180 (:271-335) build it"""
        id_of = {v: k for k, v in self.chunkGraph.chunks.items()}
        local = {k: i for i, k in enumerate(nodes)}
        n = len(nodes)
        ids = np.zeros((n, 3), np.int32)
        nbr = np.full((n, 6), -1, np.int32)
        col_off = np.zeros(n + 1, np.int64)
        labels, costs = [], []
        for i, k in enumerate(nodes):
            ids[i] = id_of[k]
            col = self._column(k)
            if not col:
                labels.append(0)
                costs.append(F32(1.0))
            else:
                column_max = max(F32(v) for _, v in col)
                for r, v in col:
                    labels.append(int(np.uint16(r + 1)))
                    costs.append(F32(1.0) - F32(v) / column_max)
                for adj in self.chunkGraph.adj_lists[k]:
                    if adj not in local or not self._column(adj):
                        continue
                    d = tuple(int(a - b) for a, b in zip(id_of[adj], id_of[k]))
                    nbr[i, NEIGHBOURHOOD.index(d)] = local[adj]
            col_off[i + 1] = len(labels)
        labels = np.array(labels, np.int32)
        costs = np.array(costs, np.float32)
        init = None
        if warm is not None:  # :208-217
            init = np.zeros(n, np.int32)
            for i in range(min(n, len(warm))):
                L = labels[col_off[i]:col_off[i + 1]]
                hit = np.nonzero(L == warm[i])[0]
                if len(hit):
                    init[i] = hit[0]
                elif warm[i] != 0:
                    self.warm_zeroed += 1
        self.problem = dict(nodes=list(nodes), ids=ids, nbr=nbr, col_off=col_off, labels=labels, costs=costs, init=init)
        return self.problem

    def _solve(self, p, max_rounds=0):
        w = F32(self.adjacent_cost * self.pairwise_cost)
        self.solution = R.solve(p["ids"], p["nbr"], p["col_off"], p["labels"], p["costs"], w, init=p["init"], max_rounds=max_rounds)
        return p["labels"][p["col_off"][:-1] + self.solution[0]]

    def _assign(self, nodes, solved, kflist):  # :227-246
        for i, k in enumerate(nodes):
            label = int(solved[i])
            if label == 0:
                if self.chunkGraph.labels[k] == 0 and len(kflist) >= 2:
                    self.chunkGraph.labels[k] = kflist[-2]
            else:
                self.chunkGraph.labels[k] = kflist[label - 1]

    def view_selection(self, kflist, max_rounds=0):  # :120-255
        nodes = list(range(self.chunkGraph.num_nodes()))
        if not nodes:
            return None
        p = self._build(nodes, self.labelstorage if self.labelstorage else None)
        solved = self._solve(p, max_rounds)
        self._assign(nodes, solved, kflist)
        self.labelstorage = [int(x) for x in solved]
        return self.solution

    def view_selection_sub(self, chunks_to_update, kflist, max_rounds=0):  # :257-406
        nodes = []
        for cid in chunks_to_update:
            cid = tuple(int(x) for x in cid)
            if cid in self.chunkGraph.chunks and self.chunkGraph.chunks[cid] not in nodes:
                nodes.append(self.chunkGraph.chunks[cid])
        if not nodes:
            return None
        p = self._build(nodes, None)
        solved = self._solve(p, max_rounds)
        self._assign(nodes, solved, kflist)
        return self.solution

    def clear(self):
        self.chunkGraph = UniGraph()
        self.dataCost = SparseMat()
        self.labelstorage = []

    # ---- views keyed by chunk id, for comparisons --------------------------------------------------------------
    def node_view(self, cid, kflist):
        """(edge mask, chunk label, stored label or -1, [(frame, quality bits)]) of a node, None if cid is no node"""
        cid = tuple(int(x) for x in cid)
        if cid not in self.chunkGraph.chunks:
            return None
        k = self.chunkGraph.chunks[cid]
        id_of = {v: c for c, v in self.chunkGraph.chunks.items()}
        mask = 0
        for adj in self.chunkGraph.adj_lists[k]:
            d = tuple(int(a - b) for a, b in zip(id_of[adj], cid))
            mask |= 1 << NEIGHBOURHOOD.index(d)
        stored = self.labelstorage[k] if k < len(self.labelstorage) else -1
        col = [(int(kflist[r]), int(np.float32(v).view(np.uint32))) for r, v in self._column(k)]
        return mask, int(self.chunkGraph.labels[k]), int(stored), col

    def all_node_views(self, kflist):
        """node_view of every node, keyed by chunk id (one pass)"""
        id_of = {v: c for c, v in self.chunkGraph.chunks.items()}
        out = {}
        for cid, k in self.chunkGraph.chunks.items():
            mask = 0
            for adj in self.chunkGraph.adj_lists[k]:
                d = tuple(int(a - b) for a, b in zip(id_of[adj], cid))
                mask |= 1 << NEIGHBOURHOOD.index(d)
            stored = self.labelstorage[k] if k < len(self.labelstorage) else -1
            col = [(int(kflist[r]), int(np.float32(v).view(np.uint32))) for r, v in self._column(k)]
            out[cid] = (mask, int(self.chunkGraph.labels[k]), int(stored), col)
        return out

    def problem_view(self):
        """the last problem keyed by chunk id: id -> (labels, cost bits, neighbour ids per face (None = no edge), init)"""
        p = self.problem
        out = {}
        for i in range(len(p["ids"])):
            a, b = int(p["col_off"][i]), int(p["col_off"][i + 1])
            nb = tuple(None if j < 0 else tuple(int(x) for x in p["ids"][j]) for j in p["nbr"][i])
            out[tuple(int(x) for x in p["ids"][i])] = (p["labels"][a:b].tolist(), p["costs"][a:b].view(np.uint32).tolist(), nb,
                                                       -1 if p["init"] is None else int(p["init"][i]))
        return out


def problem_view_of(ids, nbr, col_off, labels, costs, init):
    """the same view of a problem given as arrays (what tf_texmap_download_problem returns)"""
    out = {}
    for i in range(len(ids)):
        a, b = int(col_off[i]), int(col_off[i + 1])
        nb = tuple(None if j < 0 else tuple(int(x) for x in ids[j]) for j in nbr[i])
        out[tuple(int(x) for x in ids[i])] = (labels[a:b].tolist(), np.asarray(costs[a:b], np.float32).view(np.uint32).tolist(), nb,
                                              int(init[i]))
    return out
