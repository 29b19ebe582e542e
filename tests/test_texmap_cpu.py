"""The yardstick of the resident TexMap without a GPU: tests/texmap_ref.py against the compiled SparseMat, its quirks in
scripted sequences, the keyframe sequence of tests/texmap_inputs.py checked for the cases the GPU test relies on, and
the new entry points in header, binding and library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from texturefusion_amd import capi
from tests import texmap_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libtf_ref.so")       # Structure/sparse_matrix.cpp, compiled unmodified
MIR_SO = os.path.join(ROOT, "tests", "cpp", "libmirror_shim.so")    # the host mirror's SparseMat (pinned to the former)
NEW = ("tf_texmap_set_keyframes", "tf_texmap_update", "tf_texmap_retract", "tf_texmap_remove_wrong_mapping",
       "tf_texmap_check_graph", "tf_texmap_view_selection", "tf_texmap_download", "tf_texmap_download_problem",
       "tf_texmap_clear", "tf_generate_patches_selected")
fp = C.POINTER(C.c_float)
u64p = C.POINTER(C.c_uint64)


def _bind(path, pre):
    L = C.CDLL(path)
    g = lambda n: getattr(L, pre + n)
    g("sm_new").restype = C.c_void_p
    g("sm_free").argtypes = [C.c_void_p]
    for n in ("sm_cols", "sm_rows", "sm_nnz"):
        g(n).restype = C.c_uint64
        g(n).argtypes = [C.c_void_p]
    g("sm_add_value").argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_float]
    g("sm_set_value").argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_float]
    g("sm_resize").argtypes = [C.c_void_p, C.c_uint64]
    g("sm_clear").argtypes = [C.c_void_p]
    g("sm_remove_node").argtypes = [C.c_void_p, C.c_uint64]
    g("sm_remove_observation").argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    g("sm_col").restype = C.c_uint64
    g("sm_col").argtypes = [C.c_void_p, C.c_uint64, u64p, fp, C.c_uint64]
    return g


def _dump_c(g, h):
    cols = g("sm_cols")(h)
    out = [int(cols), int(g("sm_rows")(h)), int(g("sm_nnz")(h))]
    rows = np.empty(4096, np.uint64)
    vals = np.empty(4096, np.float32)
    for c in range(cols):
        k = g("sm_col")(h, c, rows.ctypes.data_as(u64p), vals.ctypes.data_as(fp), 4096)
        out.append((c, rows[:k].tolist(), vals[:k].view(np.uint32).tolist()))
    return out


def _dump_py(m):
    out = [m.cols(), m.rows(), m.nnz]
    for c in range(m.cols()):
        col = m.col(c)
        out.append((c, [int(r) for r, _ in col], [int(np.float32(v).view(np.uint32)) for _, v in col]))
    return out


@pytest.mark.parametrize("which", ["reference", "mirror"])
def test_column_container_agrees_with_the_compiled_sparse_mat(which):
    """one random stream of 2e4 operations (the stream of tests/test_ref_pin.py): every return value of add_value, and
    cols / rows / nnz and every column's ordered content at every 500th operation"""
    path, pre = (REF_SO, "tfref_") if which == "reference" else (MIR_SO, "tfmir_")
    if not os.path.exists(path):
        pytest.skip("%s not built" % os.path.relpath(path, ROOT))
    g = _bind(path, pre)
    rng = np.random.default_rng(11)
    h = g("sm_new")()
    m = T.SparseMat()
    n_ops = 20000
    for k in range(n_ops):
        op = int(rng.integers(0, 100))
        c, r = int(rng.integers(0, 40)), int(rng.integers(0, 24))
        v = np.float32(rng.random())
        if op < 40:
            assert bool(g("sm_add_value")(h, c, r, v)) == m.add_value(c, r, v), k
        elif op < 70:
            g("sm_set_value")(h, c, r, v)
            m.set_value(c, r, v)
        elif op < 85:
            g("sm_remove_observation")(h, c + 5, r)
            m.remove_observation(c + 5, r)
        elif op < 93:
            g("sm_remove_node")(h, c + 5)
            m.remove_node(c + 5)
        elif op < 98:
            g("sm_resize")(h, max(int(g("sm_cols")(h)), c))
            m.resize(max(m.cols(), c))
        elif op == 98 and k % 7 == 0:
            g("sm_clear")(h)
            m.clear()
        if k % 500 == 0 or k == n_ops - 1:
            assert _dump_c(g, h) == _dump_py(m), k
    g("sm_free")(h)


A, B, Cc = (0, 0, 0), (1, 0, 0), (1, 1, 0)
KF = [3, 5, 8]
LOOK = {3: 0, 5: 1, 8: 2}


def _two_nodes(obs):
    tm = T.TexMap()
    adj = {A: [0, 1, 0, 0, 0, 0], B: [1, 0, 0, 0, 0, 0]}
    tm.update_chunkgraph([A, B], lambda c: adj.get(c))
    tm.update_datacost([A, B], lambda c: obs[c], LOOK, 3, [])
    return tm, adj


def test_add_value_keeps_and_set_value_overwrites():
    obs = {A: {3: 0.5}, B: {3: 0.25}}
    tm, adj = _two_nodes(obs)
    obs[A][3] = 0.75
    tm.update_datacost([A], lambda c: obs[c], LOOK, 3, [])          # frameindex: add_value keeps 0.5
    assert tm.dataCost.col(0) == [(0, np.float32(0.5))]
    tm.update_datacost([A], lambda c: obs[c], LOOK, 5, [3])         # framesToUpdate: set_value overwrites
    assert tm.dataCost.col(0) == [(0, np.float32(0.75))]
    del obs[A][3]
    tm.update_datacost([A], lambda c: obs[c], LOOK, 5, [3])         # an absent observation removes
    assert tm.dataCost.col(0) == []
    obs[A][5] = 0.0
    tm.update_datacost([A], lambda c: obs[c], LOOK, 5, [5])         # quality 0: neither added nor set
    assert tm.dataCost.col(0) == []


def test_an_edge_survives_a_cleared_adj_flag_and_remove_node_keeps_the_index():
    obs = {A: {3: 0.5}, B: {3: 0.25}}
    tm, adj = _two_nodes(obs)
    assert tm.chunkGraph.adj_lists == [[1], [0]]
    adj[A] = [0] * 6
    adj[B] = [0] * 6
    tm.update_chunkgraph([A, B], lambda c: adj.get(c))
    assert tm.chunkGraph.adj_lists == [[1], [0]]
    # the order of the list does not matter: all nodes are added before any edge
    t2 = T.TexMap()
    t2.update_chunkgraph([B, A], lambda c: {A: [0, 1, 0, 0, 0, 0], B: [0] * 6}.get(c))
    assert t2.all_node_views(KF)[A][0] == 2 and t2.all_node_views(KF)[B][0] == 1
    # a neighbour without a mesh still gets the edge (it is a node); a flag towards a chunk that is no node gives none
    t3 = T.TexMap()
    t3.update_chunkgraph([A, B], lambda c: {A: [1, 1, 0, 0, 0, 0]}.get(c))
    assert t3.all_node_views(KF)[A][0] == 2 and t3.all_node_views(KF)[B][0] == 1
    assert tm.check_graph(lambda c: c != B) == 1
    assert tm.chunkGraph.chunks == {A: 0, B: 1} and tm.chunkGraph.adj_lists == [[], []]
    assert tm.dataCost.col(1) == [] and tm.dataCost.col(0) == [(0, np.float32(0.5))]
    assert tm.check_graph(lambda c: c != B) == 1  # it stays a node: counted again


def test_warm_start_rules():
    obs = {A: {3: 0.5, 5: 1.0}, B: {3: 0.25}}
    tm, adj = _two_nodes(obs)
    tm.update_datacost([A, B], lambda c: obs[c], LOOK, 5, [])
    tm.view_selection(KF[:2])
    assert tm.problem["init"] is None                       # no warm start on the first solve
    assert tm.labelstorage == [2, 1]
    tm.chunkGraph.add_node(Cc)                               # a node without a stored label starts at offset 0
    tm.dataCost.set_value(2, 0, 0.5)
    tm.dataCost.set_value(2, 2, 1.0)
    tm.dataCost.remove_observation(0, 1)                     # A's stored label 2 leaves its column: offset 0
    tm.dataCost.set_value(1, 2, 0.125)                       # B keeps label 1 at offset 0 of (1, 3)
    tm.dataCost.set_value(0, 2, 0.125)
    tm.view_selection(KF)
    assert tm.problem["init"].tolist() == [0, 0, 0] and tm.warm_zeroed == 1
    assert tm.problem["labels"].tolist() == [1, 3, 1, 3, 1, 3]
    tm.labelstorage = [3, 3, 3]
    tm._build([0, 1, 2], tm.labelstorage)
    assert tm.problem["init"].tolist() == [1, 1, 1]
    # the sub-problem starts cold and leaves the stored labels alone
    tm.view_selection_sub([B, (7, 7, 7), A], KF)
    assert tm.problem["init"] is None and tm.labelstorage == [3, 3, 3] and tm.problem["nodes"] == [1, 0]
    assert tm.problem["nbr"].tolist() == [[1, -1, -1, -1, -1, -1], [-1, 0, -1, -1, -1, -1]]  # B sees A across -x, A sees B across +x


@pytest.mark.parametrize("n_rows", [1, 2])
def test_label_zero_rule(n_rows):
    tm = T.TexMap()
    tm.update_chunkgraph([A, B], lambda c: None)
    tm.update_datacost([A, B], lambda c: {}, LOOK, 3, [])
    tm.chunkGraph.labels[1] = 5
    tm.view_selection(KF[:n_rows])
    p = tm.problem
    assert p["labels"].tolist() == [0, 0] and p["costs"].tolist() == [1.0, 1.0] and (p["nbr"] == -1).all()
    # label 0 keeps a label; a chunk without one takes the keyframe before the newest, if there is one
    assert tm.chunkGraph.labels == [KF[n_rows - 2] if n_rows >= 2 else 0, 5]
    assert tm.labelstorage == [0, 0]


def test_costs_are_one_minus_q_over_the_column_maximum_in_f32():
    tm = T.TexMap()
    tm.update_chunkgraph([A], lambda c: None)
    q = {3: 0.3, 5: 0.7, 8: 0.1}
    tm.update_datacost([A], lambda c: q, LOOK, 3, [5, 8])
    tm.view_selection(KF)
    mx = np.float32(0.7)
    want = [np.float32(1.0) - np.float32(v) / mx for v in (0.3, 0.7, 0.1)]
    assert tm.problem["costs"].view(np.uint32).tolist() == np.array(want, np.float32).view(np.uint32).tolist()
    assert tm.problem["labels"].tolist() == [1, 2, 3] and tm.chunkGraph.labels == [5]


def test_the_keyframe_sequence_is_not_vacuous():
    """the guards of the GPU test, on the oracle + restatement alone: >= 50 nodes with >= 2 labels at the last keyframe, a
    solve that ends strictly below its start energy, a warm start that zeroes a node whose stored label left its column,
    check_graph and the wrong-mapping removal with work"""
    from tests import texmap_inputs as I
    run = I.Run()
    try:
        for i in range(len(I.STEPS)):
            o = run.step(i)
            run.patches(o["ids"])
        tm = run.tm
        multi = sum(1 for k in range(tm.chunkGraph.num_nodes()) if len(tm._column(k)) >= 2)
        print(multi, run.stats, tm.warm_zeroed)
        assert multi >= 50 and run.stats["improved"] >= 1 and tm.warm_zeroed >= 1
        assert run.stats["check_removed"] >= 1 and run.stats["wrong_removed"] >= 1
        assert any(m for _, _, m in I.STEPS if any(n is not None for _, n in m))   # a moved keyframe
        assert any(m for _, _, m in I.STEPS if any(n is None for _, n in m))       # one de-integrated for good
    finally:
        run.close()


def test_header_binding_and_library_have_the_new_entry_points():
    """fails without the feature"""
    text = open(os.path.join(ROOT, "include", "tf_fusion.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"TF_API\s+[\w\s\*]+?\b(tf_\w+)\s*\(", text))
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
    for method in ("texmap_set_keyframes", "texmap_update", "texmap_retract", "texmap_remove_wrong_mapping", "texmap_check_graph",
                   "texmap_view_selection", "texmap_download", "texmap_problem", "texmap_clear", "generate_patches_selected"):
        assert callable(getattr(capi.Volume, method)), method
