"""tf_view_select / tf_view_select_device on the MI355X: bit parity with the numpy restatement (tests/mrf_ref.py) in both
forms, properties checked on the device's own output with this file's f64 energy, the convergence cap, determinism,
the volume left untouched, the invalid-argument cases, both ways of walking a line, and the host mirror's
TexMap::view_selection inside the reference's tail of tsdfFusion (tests/cpp_mrf/mirror_view_selection.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from texturefusion_amd import capi, synth
from tests import mrf_inputs as I
from tests import mrf_ref as R
from tests.raycast_ref import wall_frames
from tests.util import RES5, HipBuffer, make_pair, sorted_ids

pytestmark = pytest.mark.gpu
W = np.float32(0.5)
SENTINEL = -77
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gv(gpu_required):
    v = capi.Volume(RES5, synth.Camera(), max_chunks=1 << 10)
    yield v
    v.close()


def _own_energy(p, off):
    """this file's f64 energy: plain loops over nodes and +a edges, nothing shared with mrf_ref"""
    ids, nbr, col_off, labels, costs = p
    e, cut = 0.0, 0
    for i in range(len(ids)):
        e += float(costs[col_off[i] + off[i]])
        for k in (1, 3, 5):
            j = nbr[i, k]
            if j >= 0 and labels[col_off[j] + off[j]] != labels[col_off[i] + off[i]]:
                cut += 1
    return e + 0.5 * cut


def _host(gv, p, **kw):
    ids, nbr, col_off, labels, costs = p
    return gv.view_select(ids, nbr, col_off, labels, costs, W, **kw)


def _device(gv, p, init=None, max_rounds=0):
    """the device form: every array in device memory, outputs preset so that unwritten entries show"""
    ids, nbr, col_off, labels, costs = p
    n, cap = len(ids), (max_rounds or 32) + 1
    arrs = [np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(nbr, np.int32), np.ascontiguousarray(col_off, np.int64),
            np.ascontiguousarray(labels, np.int32), np.ascontiguousarray(costs, np.float32)]
    bufs = [HipBuffer(max(a.nbytes, 16)).from_host(a) for a in arrs]
    b_init = HipBuffer(4 * n).from_host(np.ascontiguousarray(init, np.int32)) if init is not None else None
    b_off = HipBuffer(4 * n).from_host(np.full(n, SENTINEL, np.int32))
    b_en = HipBuffer(8 * cap).from_host(np.full(cap, -1.0, np.float64))
    b_r = HipBuffer(16).from_host(np.full(4, SENTINEL, np.int32))
    try:
        gv.view_select_device(n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, int(col_off[-1]), bufs[3].ptr, bufs[4].ptr, W,
                              b_init.ptr if b_init else 0, max_rounds, b_off.ptr, b_en.ptr, b_r.ptr)
        gv.sync()
        off = b_off.to_host().view(np.int32).copy()
        en = b_en.to_host().view(np.float64).copy()
        r = int(b_r.to_host().view(np.int32)[0])
    finally:
        for b in bufs + [b_off, b_en, b_r] + ([b_init] if b_init else []):
            b.free()
    if r == SENTINEL:
        return off, r, en
    assert np.all(en[r + 1:] == -1.0), "energies behind the last round were written"
    return off, r, en[:r + 1]


def _check(gv, p, what, **kw):
    """both forms bit-equal to the restatement; the properties of the device output; convergence before the cap"""
    ids, nbr, col_off, labels, costs = p
    exp_off, exp_r, exp_tr = R.solve(ids, nbr, col_off, labels, costs, W, **kw)
    for form, (off, r, tr) in (("host", _host(gv, p, **kw)), ("device", _device(gv, p, **kw))):
        tag = "%s, %s form" % (what, form)
        print(tag, "rounds", r, "trace", tr.tolist())
        assert r == exp_r, tag
        assert np.array_equal(off, exp_off), tag
        assert tr.tobytes() == exp_tr.tobytes(), (tag, tr, exp_tr)
        assert tr[-1] == _own_energy(p, off), tag
        assert np.all(np.diff(tr) <= 0), tag
        if not kw.get("max_rounds"):
            assert r < R.DEFAULT_ROUNDS, tag
    return exp_off, exp_r, exp_tr


def _line_optimum(p):
    """the lines are disjoint and their costs multiples of 2^-6: the optimum is the exact sum of each line's own"""
    ids, nbr, col_off, labels, costs = p
    zero = np.zeros(len(ids), np.int32)
    base = R.energy(nbr, col_off, labels, costs, W, zero)
    total = base
    for a in range(3):
        for h in range(len(ids)):
            if nbr[h, 2 * a] == -1 and nbr[h, 2 * a + 1] >= 0:
                nodes = R._line_nodes(nbr, h, a)
                total += R.brute_force(nbr, col_off, labels, costs, W, free=nodes, offsets=zero)[0] - base
    return total


@pytest.mark.parametrize("block", range(6))
def test_lines_match_the_restatement_and_reach_the_optimum(gv, block):
    for seed in range(block * 10, block * 10 + 10):
        p = I.line_instance(seed)
        off, r, tr = _check(gv, p, "lines %d" % seed)  # (off: what both forms returned)
        assert _own_energy(p, off) == _line_optimum(p), seed


@pytest.mark.parametrize("block", range(8))
def test_small_grids_match_the_restatement(gv, block):
    for seed in range(block * 25, block * 25 + 25):
        _check(gv, I.small_grid(seed), "grid %d" % seed)


def test_sheet_matches_the_restatement_cold_and_warm(gv):
    p = I.sheet()
    assert len(p[0]) == 2400
    off, r, tr = _check(gv, p, "sheet")
    assert tr[-1] < tr[0]
    # a warm start at the solution: one round, nothing changes
    off2, r2, tr2 = _check(gv, p, "sheet, warm", init=off)
    assert r2 == 1 and np.array_equal(off2, off) and tr2[0] == tr2[1] == tr[-1]
    # ... and one from a perturbed labelling
    rng = np.random.default_rng(5)
    init = off.copy()
    pick = rng.random(len(init)) < 0.3
    init[pick] = (rng.integers(0, 1 << 20, len(init)) % np.diff(p[2]))[pick]
    _check(gv, p, "sheet, perturbed", init=init)
    _check(gv, p, "sheet, one round", max_rounds=1)


def test_many_labels_and_unlabelled_nodes(gv):
    p = I.many_labels()
    assert (np.diff(p[2]) == 150).any() and p[3].max() == 20000
    _check(gv, p, "150 labels")
    q = I.with_unlabelled()
    off, r, tr = _check(gv, q, "label-0 and isolated nodes")
    zero = q[3][q[2][:-1]] == 0
    assert zero.any() and np.all(off[zero] == 0)
    col_off, labels, costs = I.columns([[3, 7, 9]], [[0.5, 0.25, 0.25]])
    ids, nbr = I.lattice([(4, -2, 0)], lambda i, j: True)
    _check(gv, (ids, nbr, col_off, labels, costs), "one node")
    # no nodes: TF_OK, nothing written
    z = np.zeros(0, np.int32)
    off, r, tr = gv.view_select(z.reshape(0, 3), z.reshape(0, 6), np.zeros(1, np.int64), z, np.zeros(0, np.float32), W)
    assert len(off) == 0 and r == 0 and len(tr) == 0


def test_three_runs_give_identical_bytes(gv):
    p = I.sheet(seed=21)
    runs = [_host(gv, p) for _ in range(3)] + [_device(gv, p) for _ in range(3)]
    for off, r, tr in runs[1:]:
        assert r == runs[0][1] and off.tobytes() == runs[0][0].tobytes() and tr.tobytes() == runs[0][2].tobytes()


def _snapshot(v):
    st = v.stats()
    ids = sorted_ids(v.list_chunks())  # (both lists come back in no fixed order)
    s, w, c = v.get_chunks(ids)
    dirty = sorted_ids(v.dirty())
    return (bytes(st), dirty.tobytes(), ids.tobytes(), s.tobytes(), w.tobytes(), c.tobytes())


def test_volume_untouched(gpu_required):
    ov, v, cam, _ = make_pair(max_chunks=1 << 15)
    try:
        for k, (depth, rgba, pose) in enumerate(wall_frames(cam)[:4]):
            v.integrate_frame_host(depth, rgba, pose.reshape(12), None, k)
        v.update_meshes()
        v.sync()
        before = _snapshot(v)
        p = I.sheet(12, 9, 2, seed=2)
        exp = R.solve(*p, W)
        for off, r, tr in (_host(v, p), _device(v, p)):
            assert np.array_equal(off, exp[0]) and r == exp[1] and tr.tobytes() == exp[2].tobytes()
        assert _snapshot(v) == before
    finally:
        v.close()
        ov.close()


def _broken(name):
    ids, nbr, col_off, labels, costs = [a.copy() for a in I.sheet(8, 6, 2, seed=4)]
    init = R.argmin_init(col_off, costs)
    n = len(ids)
    i = next(i for i in range(n) if nbr[i, 1] >= 0 and col_off[i + 1] - col_off[i] >= 2)
    if name == "empty column":
        col_off[i + 1:] -= col_off[i + 1] - col_off[i]  # node i keeps no label; the arrays stay long enough
    elif name == "unsorted labels":
        labels[col_off[i]], labels[col_off[i] + 1] = labels[col_off[i] + 1], labels[col_off[i]]
    elif name == "repeated label":
        labels[col_off[i] + 1] = labels[col_off[i]]
    elif name == "negative label":
        labels[col_off[i]] = -1
    elif name == "init too large":
        init[i] = col_off[i + 1] - col_off[i]
    elif name == "init negative":
        init[i] = -1
    elif name == "nbr not symmetric":
        nbr[nbr[i, 1], 0] = -1
    elif name == "nbr points elsewhere":
        nbr[i, 1] = next(j for j in range(n) if j != nbr[i, 1] and nbr[j, 0] >= 0 and nbr[j, 0] != i)
    elif name == "nbr out of range":
        nbr[i, 1] = n
    elif name == "ids do not match":
        ids[nbr[i, 1], 1] += 1
    else:
        raise KeyError(name)
    return (ids, nbr, col_off, labels, costs), init


@pytest.mark.parametrize("name", ["empty column", "unsorted labels", "repeated label", "negative label", "init too large",
                                  "init negative", "nbr not symmetric", "nbr points elsewhere", "nbr out of range",
                                  "ids do not match"])
def test_invalid_arguments(gv, name):
    p, init = _broken(name)
    n = len(p[0])
    out = (np.full(n, SENTINEL, np.int32), np.full(33, -1.0), np.full(1, SENTINEL, np.int32))
    with pytest.raises(capi.TFError) as e:
        _host(gv, p, init=init, out=out)
    assert e.value.code == capi.TF_ERR_INVALID and "node" in str(e.value), str(e.value)
    assert np.all(out[0] == SENTINEL) and np.all(out[1] == -1.0) and out[2][0] == SENTINEL
    # the device form cannot return what only the device finds out: it leaves every output unwritten
    off, r, en = _device(gv, p, init=init)
    assert r == SENTINEL and np.all(off == SENTINEL) and np.all(en == -1.0)
    # ... and the handle goes on working
    q = I.small_grid(0)
    assert np.array_equal(_host(gv, q)[0], R.solve(*q, W)[0])


def test_invalid_scalars(gv):
    p = I.small_grid(1)
    for kw in ({"max_rounds": -1}, {"edge_cost": -0.5}, {"edge_cost": float("nan")}):
        with pytest.raises(capi.TFError) as e:
            gv.view_select(*p, **({"edge_cost": W} | kw))
        assert e.value.code == capi.TF_ERR_INVALID


def test_host_mirror_view_selection(gpu_required, tmp_path):
    """TexMap::view_selection of the host mirror inside the reference's tail of tsdfFusion, on a synthetic room
    (tests/cpp_mrf/mirror_view_selection.cpp lists what it asserts)"""
    cam = synth.Camera(320, 240, 262.5, 262.5, 159.5, 119.5, 0.01, 5.0)
    frames = [synth.room_frame(k, cam, with_quality=True, wobble=0.02) for k in range(17)]
    path = str(tmp_path / "frames.bin")
    with open(path, "wb") as f:
        np.array([len(frames), cam.width, cam.height], np.int32).tofile(f)
        np.array([cam.fx, cam.fy, cam.cx, cam.cy, cam.near, cam.far, 0.008], np.float32).tofile(f)
        for depth, rgba, quality, pose in frames:
            np.ascontiguousarray(pose, np.float32).reshape(12).tofile(f)
            np.ascontiguousarray(synth.pose_inverse16(pose), np.float32).reshape(16).tofile(f)
            np.ascontiguousarray(depth, np.float32).tofile(f)
            np.ascontiguousarray(rgba, np.uint8).tofile(f)
            np.ascontiguousarray(quality, np.float32).tofile(f)
    exe = str(tmp_path / "mirror_view_selection")
    src = os.path.join(ROOT, "tests", "cpp_mrf", "mirror_view_selection.cpp")
    lib = os.path.join(ROOT, "texturefusion_amd")
    subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", src, "-o", exe, "-L" + lib, "-ltexfusion_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True, timeout=300)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "mirror ok" in r.stdout, r.stdout + r.stderr


def test_both_walking_variants_give_the_same_bytes(gv, monkeypatch):
    """the line arrays (the default) and the walk through the +a pointers (TF_MRF_WALK=pointers, kept for measurement)"""
    for p, kw in ((I.sheet(), {}), (I.many_labels(), {}), (I.with_unlabelled(), {}), (I.line_instance(7), {}),
                  (I.sheet(70, 3, 1, seed=9), {}), (I.sheet(300, 2, 2, seed=10, pool=40, kmin=30, kmax=40), {"max_rounds": 3})):
        exp = R.solve(*p, W, **kw)
        for walk in ("pointers", "lines"):
            monkeypatch.setenv("TF_MRF_WALK", walk)
            for off, r, tr in (_host(gv, p, **kw), _device(gv, p, **kw)):
                assert r == exp[1] and np.array_equal(off, exp[0]) and tr.tobytes() == exp[2].tobytes(), walk
