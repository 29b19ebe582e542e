"""oracle/_ref -- the part of the reference that compiles here, unmodified and without stand-ins
(oracle/ref_shim.cpp: QuadraticTruncator / ConstantWeighter, chisel::parallel_for, SparseMat) -- against the oracle's
restatements and the host mirror's classes.  This ties SURVEY.md s.8 row a8, the thread policy of rows a6 / f-1 and
the data-cost container of row f-4 to compiled reference code.  It pins NOTHING else: K-A, the selection, the mesher
and the atlas need Eigen / OpenCV / Sophus and stay unpinned.

What the compiled reference returns on the fixed inputs below is stored in tests/golden/ref_pin.json (digests of the
exact bits; tests/golden/make_ref_pin.py writes it), together with the marching-cubes tables as the reference's source
holds them: the oracle and the mirror are checked against that file everywhere.  Where `build()` has made
oracle/_ref/libtf_ref.so, the library itself is checked against the same file as well."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import api as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libtf_ref.so")
MIR_SO = os.path.join(ROOT, "tests", "cpp", "libmirror_shim.so")
GOLD_JSON = os.path.join(ROOT, "tests", "golden", "ref_pin.json")

fp = C.POINTER(C.c_float)
u64p = C.POINTER(C.c_uint64)


def _bind_sm(L, pre):
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
    g("truncation_n").argtypes = [C.c_float] * 4 + [fp, fp, C.c_int64]
    g("weight_n").argtypes = [C.c_float, fp, fp, C.c_int64]


def bind_ref(L):
    _bind_sm(L, "tfref_")
    L.tfref_truncation.restype = C.c_float
    L.tfref_truncation.argtypes = [C.c_float] * 5
    L.tfref_parallel_for_groups.argtypes = [C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int)]
    return L


@pytest.fixture(scope="module")
def gold():
    with open(GOLD_JSON) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ref():
    """the compiled reference pieces when build() has made them, else None (the golden file stands in for them)"""
    if not os.path.exists(REF_SO):
        return None
    return bind_ref(C.CDLL(REF_SO))


@pytest.fixture(scope="module")
def mirror():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "libmirror_shim.so"], check=True, capture_output=True)
    L = C.CDLL(MIR_SO)
    _bind_sm(L, "tfmir_")
    return L


def _trunc_inputs(n, seed):
    rng = np.random.default_rng(seed)
    z = np.concatenate([
        rng.uniform(-6.0, 6.0, n).astype(np.float32),           # the depth range of the path (and behind the camera)
        np.float32(10.0) ** rng.uniform(-30, 30, n // 4).astype(np.float32),
        rng.integers(0, 2 ** 32, n // 4, dtype=np.uint64).astype(np.uint32).view(np.float32),  # any bit pattern
        np.array([0.0, -0.0, 1.5, 3.0, 0.4, 5.0, np.inf, -np.inf, np.nan, 1e-45, 3.4e38], np.float32)])
    return np.ascontiguousarray(z)


def truncation_inputs():
    return _trunc_inputs(20000, 1)


def weight_inputs():
    return np.abs(_trunc_inputs(20000, 2))


def _call_n(fn, params, x):
    out = np.empty_like(x)
    fn(*[C.c_float(p) for p in params], x.ctypes.data_as(fp), out.ctypes.data_as(fp), len(x))
    return out


def bits_digest(x):
    """SHA-256 of where a float32 result is NaN and of the exact bits of every other element (NaN payloads are free)"""
    x = np.ascontiguousarray(x, np.float32)
    nan = np.isnan(x)
    return hashlib.sha256(nan.tobytes() + x[~nan].view(np.uint32).tobytes()).hexdigest()


PARAM_SETS = [(0.0019, 0.00152, 0.001504, 6.0),      # MobileFusion.h:245-247
              (0.0019, 0.00152, 0.001504, 1.0), (0.0, 0.0, 0.03, 1.0), (-0.01, 0.02, -0.005, 8.0),
              (1e-3, -4e-3, 1e-3, 3.0)]
WEIGHTS = (1.0, 0.5, 3.0, 1e-3)


def test_truncation_equals_compiled_reference(gold, ref, mirror):
    """tfo_truncation and the mirror's QuadraticTruncator vs chisel::QuadraticTruncator::GetTruncationDistance called
    through the base-class pointer (ProjectionIntegrator.cpp:91), bit for bit, 3e4 inputs per parameter set."""
    L = O.lib()
    z = truncation_inputs()
    assert len(gold["truncation"]) == len(PARAM_SETS)
    for ps, want in zip(PARAM_SETS, gold["truncation"]):
        ps32 = [np.float32(p) for p in ps]
        if ref is not None:
            assert bits_digest(_call_n(ref.tfref_truncation_n, ps32, z)) == want, ps
        ig = O.Integrator(*ps32, np.float32(1.0))
        got = np.array([L.tfo_truncation(C.byref(ig), C.c_float(v)) for v in z], np.float32)
        assert bits_digest(got) == want, ps
        assert bits_digest(_call_n(mirror.tfmir_truncation_n, ps32, z)) == want, ps
    if ref is not None:
        assert ref.tfref_truncation(*[C.c_float(np.float32(p)) for p in PARAM_SETS[0]], C.c_float(1.5)) > 0


def test_weight_equals_compiled_reference(gold, ref, mirror):
    """tfo_weight / the mirror's ConstantWeighter vs chisel::ConstantWeighter::GetWeight (ProjectionIntegrator.cpp:92)."""
    L = O.lib()
    L.tfo_weight.restype = C.c_float
    L.tfo_weight.argtypes = [C.POINTER(O.Integrator), C.c_float]
    tr = weight_inputs()
    assert len(gold["weight"]) == len(WEIGHTS)
    for w, want in zip(WEIGHTS, gold["weight"]):
        w32 = np.float32(w)
        if ref is not None:
            assert bits_digest(_call_n(ref.tfref_weight_n, [w32], tr)) == want, w
        ig = O.Integrator(*[np.float32(p) for p in PARAM_SETS[0]], w32)
        got = np.array([L.tfo_weight(C.byref(ig), C.c_float(v)) for v in tr], np.float32)
        assert bits_digest(got) == want, w
        assert bits_digest(_call_n(mirror.tfmir_weight_n, [w32], tr)) == want, w


def _chunk_cases():
    """200 (pose, chunk) cases -> the oracle's (originInCamera, truncation, weight) for each"""
    ig = O.default_integrator()
    rng = np.random.default_rng(5)
    for _ in range(200):
        pose = np.eye(4, dtype=np.float32)[:3].copy()
        pose[:, 3] = rng.uniform(-1, 1, 3).astype(np.float32)
        cid = rng.integers(-40, 40, 3).astype(np.int32)
        yield ig, O.chunk_scalars(ig, pose, cid, np.float32(0.005))


def _u32(x):
    return int(np.float32(x).view(np.uint32))


def ref_chunk_scalars(ref):
    """[z, truncation, weight] bits: the reference functions applied to the oracle's originInCamera.z of every case"""
    rows = []
    for ig, (oc, _, _) in _chunk_cases():
        tr = ref.tfref_truncation(*[C.c_float(x) for x in (ig.quad, ig.lin, ig.cons, ig.scale)], C.c_float(oc[2]))
        w = _call_n(ref.tfref_weight_n, [np.float32(ig.weight)], np.array([tr], np.float32))[0]
        rows.append([_u32(oc[2]), _u32(tr), _u32(w)])
    return rows


def test_chunk_scalars_use_the_pinned_pieces(gold, ref):
    """The per-chunk truncation / weight K-A works with (tfo_chunk_scalars, ProjectionIntegrator.cpp:88-92) are the
    reference functions applied to the oracle's originInCamera.z -- the z itself depends on Eigen's dot order (unpinned;
    the golden file holds the z it was made from, so that a changed z is reported as such)."""
    want = gold["chunk_scalars"]
    if ref is not None:
        assert ref_chunk_scalars(ref) == want
    got = [[_u32(oc[2]), _u32(tr), _u32(w)] for _, (oc, tr, w) in _chunk_cases()]
    assert len(got) == len(want) == 200
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], ("originInCamera.z differs from the one the golden file was made from", k)
        assert g[1:] == w[1:], k


PF_SIZES = [1, 2, 999, 1000, 1001, 1999, 2000, 2001, 4606, 4999, 5000, 5001, 11000, 31449, 78000, 100000, 100003]


def _partition_digest(worker):
    """the stretches of a worker array, independent of the thread ids: workers renumbered by first appearance"""
    _, first, inv = np.unique(worker, return_index=True, return_inverse=True)
    canon = np.argsort(np.argsort(first))[inv].astype(np.int32)
    return hashlib.sha256(canon.tobytes()).hexdigest()


def ref_parallel_for(ref):
    """chisel::parallel_for run on index vectors of PF_SIZES: its thread count, and per size the threads that ran items
    and the partition of the items among them"""
    rows, nts = [], set()
    for n in PF_SIZES:
        worker = np.zeros(n, np.int32)
        nt = C.c_int(0)
        used = ref.tfref_parallel_for_groups(n, worker.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nt))
        nts.add(nt.value)
        rows.append([n, int(used), _partition_digest(worker)])
    assert len(nts) == 1
    return {"threads": nts.pop(), "sizes": rows}


def test_parallel_for_plan_equals_compiled_reference(gold, ref):
    """tfo_parallel_for_plan (the thread cut the oracle's chunk and mesh loops use for the CPU baseline) vs
    chisel::parallel_for itself, run with an index vector as Chisel.h:234 does: number of threads that ran items and
    the exact stretch every item fell into.  (n = 0 is not asked: the reference's loop bound `last - group` on an empty
    vector is a wrapped pointer -- it spawns threads until the process dies -- and Chisel.h:228 returns before it.)
    The reference takes its thread count from the host (hardware_concurrency() - 2): the golden file holds its answer for
    the thread count of the host that made it; the compiled library, where present, is asked with this host's count."""
    L = O.lib()
    L.tfo_parallel_for_plan.restype = C.c_int
    L.tfo_parallel_for_plan.argtypes = [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64)]

    def check(nt, rows):
        for n, used, part in rows:
            group = C.c_int64(0)
            T = L.tfo_parallel_for_plan(n, nt, 1000, C.byref(group))
            g = group.value
            assert g == max(1000, n // nt)
            assert used == T, (n, nt, used, T)
            # item i ran in stretch i // group: the same thread for a whole stretch, another one for the next
            assert part == _partition_digest(np.arange(n) // g), (n, nt)
        assert sum(r[0] for r in rows) >= 10 ** 4

    pf = gold["parallel_for"]
    assert [r[0] for r in pf["sizes"]] == PF_SIZES
    check(pf["threads"], pf["sizes"])
    if ref is not None:
        live = ref_parallel_for(ref)
        if live["threads"] >= 1:  # (hardware_concurrency() - 2 < 1: the reference itself divides by zero)
            check(live["threads"], live["sizes"])


def _dump(L, pre, h):
    g = lambda n: getattr(L, pre + n)
    cols = g("sm_cols")(h)
    out = [cols, g("sm_rows")(h), g("sm_nnz")(h)]
    rows = np.empty(4096, np.uint64)
    vals = np.empty(4096, np.float32)
    for c in range(cols):
        k = g("sm_col")(h, c, rows.ctypes.data_as(u64p), vals.ctypes.data_as(fp), 4096)
        out.append((c, rows[:k].tolist(), vals[:k].view(np.uint32).tolist()))
    return out


def _digest(obj):
    return hashlib.sha256(json.dumps(obj).encode()).hexdigest()


def sparse_mat_digests(L, pre):
    """one random stream of 2e4 operations on a SparseMat of library L: a digest of every return value of AddValue, and
    at every 500th operation (and the last) a digest of cols / rows / nnz and every column's ordered content"""
    g = lambda n: getattr(L, pre + n)
    rng = np.random.default_rng(11)
    h = g("sm_new")()
    n_ops = 20000
    added, dumps = [], []
    for k in range(n_ops):
        op = rng.integers(0, 100)
        c = int(rng.integers(0, 60))
        r = int(rng.integers(0, 40))
        v = np.float32(rng.uniform(-5, 5))
        if op < 45:
            added.append(int(g("sm_add_value")(h, c, r, v)))
        elif op < 70:
            g("sm_set_value")(h, c, r, v)
        elif op < 85:
            g("sm_remove_observation")(h, c + 5, r)
        elif op < 93:
            g("sm_remove_node")(h, c + 5)
        elif op < 98:
            g("sm_resize")(h, max(int(g("sm_cols")(h)), c))      # TexMap only ever grows the matrix (TexMap.cpp:66)
        elif op == 98 and k % 7 == 0:
            g("sm_clear")(h)
        if k % 500 == 0 or k == n_ops - 1:
            dumps.append(_digest(_dump(L, pre, h)))
    g("sm_free")(h)
    return {"add_value": _digest(added), "states": dumps}


def test_sparse_mat_mirror_equals_compiled_reference(gold, ref, mirror):
    """The mirror's SparseMat (the DataCosts of TexMap, row f-4) vs Structure/sparse_matrix.cpp under one random
    stream of 2e4 operations: every return value, cols / rows / nnz, and every column's ordered content."""
    want = gold["sparse_mat"]
    streams = [("mirror", mirror, "tfmir_")] + ([("reference", ref, "tfref_")] if ref is not None else [])
    for name, L, pre in streams:
        got = sparse_mat_digests(L, pre)
        assert len(got["states"]) == len(want["states"])
        for i, (a, b) in enumerate(zip(got["states"], want["states"])):
            assert a == b, (name, "state after operation", min(500 * i, 19999))
        assert got["add_value"] == want["add_value"], name


def test_mc_tables_equal_the_reference_source(gold):
    """The nibble-packed marching-cubes triangle table of the oracle and of the product (tools/gen_mc_table.py)
    against the table where the reference keeps it (marching_cubes/MarchingCubes.cpp:28-), and the edge -> corner
    pairs (:288-), as tests/golden/ref_pin.json holds them."""
    import re
    mc = gold["marching_cubes"]
    want = []
    for v in mc["triangle_table"]:
        assert len(v) == 16
        want.append(sum(((0xF if e < 0 else e) << (4 * j)) for j, e in enumerate(v)))
    assert len(want) == 256
    for path in ("oracle/mc_table.inc", "texturefusion_amd/csrc/tf_mc_table.h"):
        got = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{16})ull", open(os.path.join(ROOT, path)).read())]
        assert got == want, path
    pairs = [tuple(p) for p in mc["edge_index_pairs"]]
    assert pairs == [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
    assert [tuple(p) for p in mc["chunk_manager_edge_index_pairs"]] == pairs   # the copy the mesher uses (:68-75)
    offs = mc["cube_index_offsets"]                                            # column k = corner k (:65-66)
    oc = open(os.path.join(ROOT, "oracle", "tf_oracle.c")).read()
    mk = re.search(r"kCorner\[8\]\[3\]\s*=\s*\{(.*?)\};", oc, re.S)
    assert [[int(x) for x in p.split(",")] for p in re.findall(r"\{([^{}]*)\}", mk.group(1))] == offs
    m = re.search(r"kEdgePair\[12\]\[2\]\s*=\s*\{(.*?)\};", oc, re.S)
    assert m
    assert [tuple(int(x) for x in p.split(",")) for p in re.findall(r"\{(\s*\d+\s*,\s*\d+\s*)\}", m.group(1))] == pairs
