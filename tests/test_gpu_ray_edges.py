"""The raycaster (k_raycast: raycast_body, and tri_sample under it) on the hand-built volumes of tests/ray_inputs.py, at the
decision edges of the march, the normal, the colour and the tile grid (tests/test_raycast_cpu.py proves on the CPU that
every case reaches the branch it names and that every rule is told from its neighbour), device against the restatement
RefVolume.raycast_maps of tests/raycast_ref.py:

  host form      tf_raycast after tf_raycast_camera: hit mask, depth, vertex, normal as raw bits, rgba as bytes
  device form    tf_raycast_device into buffers with a sentinel margin behind every output (the lanes of a partial tile
                 beyond W or H must write nothing), all four outputs at once and each alone
  both states    of the neighbour table: as set_chunk left the volume (every corner through the hash) and after
                 finalize + update_meshes (through the table, tf_check_neighbours holding it against the hash)
  point queries  tf_query_points at the hits, their six taps and the faces, edges and corners of the chunks, in both states
  parked         a chunk the table still names after GarbageCollect parked it: as if absent

No tolerance anywhere: raw bits and bytes.  One handle per resolution, reset between cases."""
import functools

import numpy as np
import pytest

from tests import ray_inputs as RI
from tests.test_gpu_raycast import _assert_query_equal
from tests.util import HipBuffer, sorted_ids
from texturefusion_amd import capi

pytestmark = pytest.mark.gpu

MARGIN = 256   # elements behind each output: seven rows of the widest camera and seven pixels more
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def handles(gpu_required):
    """resolution -> device volume, made on first use"""
    made = {}

    def get(res):
        if float(res) not in made:
            made[float(res)] = capi.Volume(res, RI._cam(24, 17), max_chunks=RI.MAX_CHUNKS, max_list=RI.MAX_CHUNKS, max_coarse=1 << 14,
                                           atlas_w=1920, atlas_h=720)
        gv = made[float(res)]
        gv.reset()
        return gv

    yield get
    for gv in made.values():
        gv.close()


@functools.lru_cache(maxsize=None)
def _expected(name):
    return RI.ref_maps(RI.cases()[name])


def _load(handles, c):
    """the case's chunks on a reset handle, every corner resolved through the hash: the table holds nothing yet"""
    gv = handles(c["res"])
    for k in range(len(c["ids"])):
        gv.set_chunk(c["ids"][k], c["sdf"][k], c["weight"][k], c["colour"][k])
    gv.raycast_camera(c["cam"])
    gv.sync()
    assert gv.check_neighbours()[1] == 0
    return gv


def _adjacent(ids):
    d = np.abs(ids[:, None, :].astype(np.int64) - ids[None, :, :]).max(-1)
    return bool((d == 1).any())


def _fill_table(gv, ids):
    """the chunks made dirty and meshed: the filter writes their rows of the neighbour table"""
    ids = np.ascontiguousarray(ids, np.int32)
    gv.finalize(ids, np.ones(len(ids), np.uint8), np.zeros(len(ids), np.uint8))
    gv.update_meshes()
    gv.sync()
    n = gv.check_neighbours()
    assert n[2] == 0 and n[4] == 0, n.tolist()
    assert (n[1] > 0) == _adjacent(ids), n.tolist()
    return n


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_maps_equal(got, exp, what):
    assert np.array_equal(got["depth"] > 0, exp["depth"] > 0), "%s: hit masks differ at %d pixels" % (what, ((got["depth"] > 0) != (exp["depth"] > 0)).sum())
    for k in ("depth", "vertex", "normal"):
        diff = _bits(got[k]) != _bits(exp[k])
        assert not diff.any(), "%s: %s differs at %d values, first %s" % (what, k, diff.sum(), np.argwhere(diff)[0].tolist())
    assert np.array_equal(got["rgba"], exp["rgba"]), "%s: rgba differs" % what


def _host(gv, c):
    return gv.raycast(c["pose"], c["near"], c["far"], c["max_steps"])


def _device(gv, c, want=(True, True, True, True)):
    """raycast_device into sentinel-filled buffers -> the outputs asked for (None for the others), margins checked"""
    W, H = c["cam"].width, c["cam"].height
    P = W * H
    sizes = (4 * (P + MARGIN), 4 * (3 * P + MARGIN), 4 * P + MARGIN, 4 * (3 * P + MARGIN))
    used = (4 * P, 12 * P, 4 * P, 12 * P)
    bufs = [HipBuffer(n).from_host(np.full(n, SENTINEL, np.uint8)) if w else None for n, w in zip(sizes, want)]
    try:
        gv.raycast_device(c["pose"], c["near"], c["far"], c["max_steps"], *[b.ptr if b else 0 for b in bufs])
        gv.sync()
        raw = [b.to_host() if b else None for b in bufs]
    finally:
        for b in bufs:
            if b:
                b.free()
    for k, r in enumerate(raw):
        assert r is None or (r[used[k]:] == SENTINEL).all(), "output %d: written behind its %d x %d image" % (k, W, H)
    f = lambda r, n, shape: None if r is None else r[:n].view(np.float32).reshape(shape)
    return {"depth": f(raw[0], used[0], (H, W)), "normal": f(raw[1], used[1], (3, H, W)),
            "rgba": None if raw[2] is None else raw[2][:used[2]].reshape(H, W, 4), "vertex": f(raw[3], used[3], (3, H, W))}


def _check_device(gv, c, host, what):
    dev = _device(gv, c)
    _assert_maps_equal(dev, host, what + ", device form")
    for k, key in enumerate(("depth", "normal", "rgba", "vertex")):
        one = _device(gv, c, tuple(j == k for j in range(4)))
        assert all((one[o] is None) == (o != key) for o in one)
        assert np.array_equal(one[key].view(np.uint8), dev[key].view(np.uint8)), "%s: %s alone differs" % (what, key)


def _points(c, exp, rng):
    """about 200 world points: hits, their six taps, and the corners, edge and face midpoints of the chunks"""
    res = float(c["res"])
    hits = exp["vertex"][:, exp["depth"] > 0].T
    if len(hits) > 20:
        hits = hits[rng.choice(len(hits), 20, replace=False)]
    taps = [hits] + [hits + np.float32(s * res) * np.eye(3, dtype=np.float32)[a] for a in range(3) for s in (-1, 1)]
    ids = c["ids"][rng.choice(len(c["ids"]), min(len(c["ids"]), 3), replace=False)].astype(np.float64)
    offs = np.array([(x, y, z) for x in (0, 0.5, 1) for y in (0, 0.5, 1) for z in (0, 0.5, 1) if (x, y, z) != (0.5, 0.5, 0.5)])
    border = (ids[:, None, :] + offs[None]).reshape(-1, 3) * 8 * res
    return np.concatenate(taps + [border.astype(np.float32)]).astype(np.float32)


def _check_queries(gv, c, exp, rng, what):
    pts = _points(c, exp, rng)
    want = RI.ref_volume(c).query(pts)
    _assert_query_equal(gv.query(pts), want)
    return want["flags"]


@pytest.mark.parametrize("name", RI.NAMES)
def test_maps_equal_the_restatement_in_both_table_states(handles, name):
    c, exp = RI.cases()[name], _expected(name)
    gv = _load(handles, c)
    first = _host(gv, c)
    _assert_maps_equal(first, exp, name + ", through the hash")
    _assert_maps_equal(_host(gv, c), first, name + ", a second run")
    _fill_table(gv, c["ids"])
    _assert_maps_equal(_host(gv, c), exp, name + ", through the table")
    assert c["reach"](exp).sum() >= min(4, exp["depth"].size)


@pytest.mark.parametrize("name", RI.NAMES)
def test_device_form_writes_its_image_and_nothing_else(handles, name):
    c, exp = RI.cases()[name], _expected(name)
    gv = _load(handles, c)
    for state in ("hash", "table"):
        if state == "table":
            _fill_table(gv, c["ids"])
        host = _host(gv, c)
        _assert_maps_equal(host, exp, "%s, %s" % (name, state))
        _check_device(gv, c, host, "%s, %s" % (name, state))


@pytest.mark.parametrize("name", RI.NAMES)
def test_point_queries_at_the_hits_their_taps_and_the_chunk_borders(handles, name):
    c, exp = RI.cases()[name], _expected(name)
    gv = _load(handles, c)
    flags = _check_queries(gv, c, exp, np.random.default_rng(7), name + ", through the hash")
    _fill_table(gv, c["ids"])
    _check_queries(gv, c, exp, np.random.default_rng(7), name + ", through the table")
    assert (flags == 0).any()  # (a corner of a chunk with no chunk beyond it)


def _snapshot(gv):
    ids = sorted_ids(gv.list_chunks())
    s, w, col = gv.get_chunks(ids)
    return (bytes(gv.stats()), sorted_ids(gv.dirty()).tobytes(), ids.tobytes(), s.tobytes(), w.tobytes(), col.tobytes(),
            gv.check_summaries(), gv.check_neighbours().tobytes())


@pytest.mark.parametrize("name", ["front", "normal_thin_back", "neg_z"])
def test_read_only(handles, name):
    c, exp = RI.cases()[name], _expected(name)
    gv = _load(handles, c)
    for state in ("hash", "table"):
        if state == "table":
            _fill_table(gv, c["ids"])
        before = _snapshot(gv)
        host = _host(gv, c)
        _check_device(gv, c, host, name)
        _check_queries(gv, c, exp, np.random.default_rng(9), name)
        assert _snapshot(gv) == before, "%s, %s: the volume changed" % (name, state)
    ids = sorted_ids(c["ids"])
    order = np.lexsort((c["ids"][:, 2], c["ids"][:, 1], c["ids"][:, 0]))
    s, w, col = gv.get_chunks(ids)
    assert np.array_equal(_bits(s), _bits(c["sdf"][order])) and np.array_equal(_bits(w), _bits(c["weight"][order]))
    assert np.array_equal(col, c["colour"][order])


def test_a_parked_neighbour_the_table_still_names(handles):
    """front's four chunks are meshed (their rows name each other), then the call-by-call flow parks one of them the way
    GarbageCollect does (finalize with needs 0, new 1): its hash entry is dead, its storage fresh, the other chunks' voxels
    untouched, and their rows still hold its pool slot.  Samples whose corners reach into it come back invalid: every map
    and every query equals the restatement of the three chunks that are left"""
    c = RI.cases()["front"]
    parked = np.array([[0, 0, 3]], np.int32)
    keep = ~(c["ids"] == parked).all(1)
    assert keep.sum() == len(c["ids"]) - 1
    left = dict(c, ids=c["ids"][keep], sdf=c["sdf"][keep], weight=c["weight"][keep], colour=c["colour"][keep])
    full, exp = _expected("front"), RI.ref_maps(left)
    # pixels that hit with four chunks, whose cell starts in a chunk that stays and reaches into the parked one
    g = np.floor(full["vertex"].astype(np.float64) / float(c["res"]) - 0.5).astype(np.int64)
    starts_outside = ((g >> 3) != parked[0][:, None, None]).any(0)
    reaches_in = (((g + 1) >> 3) == parked[0][:, None, None]).all(0)
    through_table = (full["depth"] > 0) & starts_outside & reaches_in
    assert through_table.sum() >= 4 and not exp["depth"][through_table].any() and (exp["depth"] > 0).sum() >= 4
    gv = _load(handles, c)
    n_before = _fill_table(gv, c["ids"])
    _assert_maps_equal(_host(gv, c), full, "before parking")
    gv.finalize(parked, np.zeros(1, np.uint8), np.ones(1, np.uint8))
    gv.sync()
    assert not gv.has_chunk(parked[0]) and np.array_equal(sorted_ids(gv.list_chunks()), sorted_ids(left["ids"]))
    s, w, col = gv.get_chunks(sorted_ids(left["ids"]))
    order = np.lexsort((left["ids"][:, 2], left["ids"][:, 1], left["ids"][:, 0]))
    assert np.array_equal(_bits(s), _bits(left["sdf"][order])) and np.array_equal(_bits(w), _bits(left["weight"][order]))
    n = gv.check_neighbours()
    assert n[2] == 0 and n[4] == 0 and 0 < n[1], (n_before.tolist(), n.tolist())
    host = _host(gv, c)
    _assert_maps_equal(host, exp, "with the chunk parked")
    _check_device(gv, c, host, "with the chunk parked")
    _check_queries(gv, left, full, np.random.default_rng(11), "with the chunk parked")
