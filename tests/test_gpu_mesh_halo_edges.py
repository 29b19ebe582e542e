"""The mesher's halo staging and the filter's corner-voxel test at the edges of their neighbourhoods.

Both issue their scattered loads as one unconditional batch: a thread whose neighbour chunk does not exist (or that has no
table entry) reads a dummy voxel of the chunk itself and takes the fresh state afterwards.  What can go wrong is the
select -- a dummy that leaks into the staged region, a neighbour index clamped to the wrong chunk, a dummy address
outside the pool -- so the cases are hand-built neighbourhoods (none / every / exactly one of the 26 neighbours), the first
and the last pool slot, and for the filter a chunk whose only negative voxel lies in one of the seven +x / +y / +z
neighbours.  Chunk contents are uploaded on both sides (set_chunk), made dirty through finalize, meshed, and compared bit
for bit with the oracle (tests/test_gpu_mesh.py::_compare_meshes).

The volumes have 2^8 pool slots, and a volume's dirty list holds as many entries as its pool: finalize marks a chunk
and its six face neighbours (Chisel.h:197-203), seven ids per listed chunk, so the cases with many chunks list only the
chunks under test -- the centres -- and leave the rest to be meshed as their face neighbours or not at all."""
import numpy as np
import pytest

from texturefusion_amd import synth
from tests.test_gpu_mesh import _compare_meshes
from tests.util import RES5, make_pair

pytestmark = pytest.mark.gpu

MAX_CHUNKS = 1 << 8
NEIGHBOURS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
PLUS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]


def _field(rng):
    """sdf around 0 with some voxels at 1.0 (observed, the limit), 999 (fresh) and 0.0; weights around the threshold of 50
    (the halo's corner flags decide which vertices exist); colour counts 0, 1, 2 (0: the vertex is white)"""
    sdf = (rng.standard_normal(512) * 0.01).astype(np.float32)
    sdf[rng.random(512) < 0.04] = 1.0
    sdf[rng.random(512) < 0.04] = 999.0
    sdf[rng.random(512) < 0.04] = 0.0
    w = rng.choice(np.float32([49.0, 50.0, 51.0, 80.0]), 512).astype(np.float32)
    col = rng.integers(0, 600, 2048).astype(np.uint16)
    col[3::4] = rng.integers(0, 3, 512)
    return sdf, w, col


def _pair():
    ov, gv, _, _ = make_pair(RES5, synth.Camera(), max_chunks=MAX_CHUNKS)
    return ov, gv


def _put(ov, gv, cid, field):
    cid = np.array(cid, np.int32)
    for v in (ov, gv):
        v.set_chunk(cid, *field)
    return cid


def _mesh_and_compare(ov, gv, ids, what):
    ids = np.array(ids, np.int32).reshape(-1, 3)
    assert 7 * len(ids) <= MAX_CHUNKS  # (the dirty list's capacity, see above)
    needs, new = np.ones(len(ids), np.uint8), np.zeros(len(ids), np.uint8)
    ov.finalize(ids, needs, new)
    gv.finalize(ids, needs, new)
    ov.update_meshes()
    gv.update_meshes()
    _compare_meshes(ov, gv, what)
    gv.close()
    return {tuple(int(c) for c in cid) for cid in ov.list_meshes()}  # the chunks that have a mesh, on both sides


def _cluster(ov, gv, rng, centre, present, centre_first=True):
    """the chunk at `centre` and the listed ones of its 26 neighbours, random fields; -> their ids"""
    cells = [(0, 0, 0)] + list(present) if centre_first else list(present) + [(0, 0, 0)]
    return [_put(ov, gv, np.add(centre, d), _field(rng)) for d in cells]


def test_chunk_without_any_neighbour(gpu_required):
    ov, gv = _pair()
    ids = _cluster(ov, gv, np.random.default_rng(21), (3, -2, 5), [])
    assert _mesh_and_compare(ov, gv, ids, "no neighbour") == {(3, -2, 5)}


def test_chunk_with_all_26_neighbours(gpu_required):
    ov, gv = _pair()
    ids = _cluster(ov, gv, np.random.default_rng(22), (-4, 7, 1), NEIGHBOURS)
    assert (-4, 7, 1) in _mesh_and_compare(ov, gv, ids, "26 neighbours")


def test_chunk_with_exactly_one_neighbour_each_of_the_26(gpu_required):
    """26 clusters of two chunks, far enough apart to share nothing: neighbour k of cluster k is the only one there is"""
    ov, gv = _pair()
    rng = np.random.default_rng(23)
    ids = []
    for k, d in enumerate(NEIGHBOURS):
        ids += _cluster(ov, gv, rng, (5 * k - 60, 9, -3), [d])[:1]
    have = _mesh_and_compare(ov, gv, ids, "one neighbour")
    assert all((5 * k - 60, 9, -3) in have for k in range(26))


def _stripe(cid):
    """The pool's slots are dealt in 64 stripes of max_chunks / 64, by a hash of the packed chunk id, in order of arrival
    within a stripe (chunk_acquire, tf_devfn.h) -- restated here to place a chunk in a chosen slot.  (If this went out of
    step with the library, the full pool below would overflow a stripe and the upload would raise.)"""
    key = sum(((int(c) + (1 << 20)) & 0x1FFFFF) << sh for c, sh in zip(cid, (42, 21, 0)))
    h = (key * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)
    return ((((h >> 32) ^ h) & 0xFFFFFFFF) >> 7) & 63


PER_STRIPE = MAX_CHUNKS // 64


def _centre_in_stripe(stripe, present):
    """a chunk id of that stripe whose listed neighbours leave the stripe alone and fit their own stripes"""
    for c in np.ndindex(16, 16, 16):
        others = [_stripe(np.add(c, d)) for d in present]
        if _stripe(c) == stripe and stripe not in others and max(others.count(o) for o in others) <= PER_STRIPE:
            return tuple(int(x) for x in c)
    raise AssertionError("no such chunk id")


def test_meshed_chunk_in_the_first_pool_slot(gpu_required):
    """the centre chunk is the first arrival of stripe 0: pool slot 0 -- the slot a lane without a neighbour reads its
    dummy from is then also the lowest address of the pool"""
    ov, gv = _pair()
    present = NEIGHBOURS[::2]
    centre = _centre_in_stripe(0, present)
    ids = _cluster(ov, gv, np.random.default_rng(24), centre, present, centre_first=True)
    assert centre in _mesh_and_compare(ov, gv, ids, "slot 0")


def test_meshed_chunk_in_the_last_pool_slot(gpu_required):
    """every stripe of the pool filled, the centre chunk the last arrival of the last stripe: pool slot max_chunks - 1 --
    its dummy reads and its own voxels end where the pool ends"""
    ov, gv = _pair()
    rng = np.random.default_rng(25)
    present = NEIGHBOURS[1::2]
    centre = _centre_in_stripe(63, present)
    room = [PER_STRIPE] * 64
    for c in [centre] + [tuple(np.add(centre, d)) for d in present]:
        room[_stripe(c)] -= 1
    for c in np.ndindex(40, 40, 40):  # chunks far from the cluster, taken where their stripe still has room
        c = (int(c[0]) + 100, int(c[1]), int(c[2]))
        if not any(room):
            break
        if room[_stripe(c)]:
            room[_stripe(c)] -= 1
            _put(ov, gv, c, _field(rng))
    ids = _cluster(ov, gv, rng, centre, present, centre_first=False)
    assert gv.stats().n_chunks == MAX_CHUNKS
    assert centre in _mesh_and_compare(ov, gv, ids, "last slot")


def _flat(value, weight=80.0):
    return (np.full(512, value, np.float32), np.full(512, weight, np.float32), np.full(2048, 1, np.uint16))


@pytest.mark.parametrize("mode", ["present", "absent", "all_seven"])
def test_filter_finds_the_only_negative_voxel_in_a_plus_neighbour(gpu_required, mode):
    """The chunk's own voxels are all observed and positive: whether it can have a vertex is decided by the 217 corner
    voxels its +x / +y / +z neighbours contribute.  The only negative, heavy voxel of the neighbourhood lies in the
    x = 0 face of +x, the y = 0 face of +y, the z = 0 face of +z, on the matching edge of +x+y / +x+z / +y+z or in the
    corner of +x+y+z; `present`: only that neighbour exists, `absent`: not even that one (the voxel is nowhere: the chunk
    must end in the filter as the oracle's ends without a mesh), `all_seven`: all seven neighbours exist, so that the
    edge and corner voxels complete a cell.  A mesh must exist exactly where the oracle has one."""
    ov, gv = _pair()
    ids = []
    for k, d in enumerate(PLUS):
        centre = np.array((6 * k - 20, 2, 2), np.int32)
        ids.append(_put(ov, gv, centre, _flat(0.01)))
        for e in PLUS:
            if mode == "absent" or (mode == "present" and e != d):
                continue
            sdf, w, col = _flat(0.01)
            if e == d:  # coordinate 0 along the axes the neighbour is displaced on, mid-face / mid-edge along the others
                x, y, z = (0 if d[0] else 3), (0 if d[1] else 4), (0 if d[2] else 5)
                sdf[x + 8 * y + 64 * z] = -0.004
            _put(ov, gv, centre + np.array(e, np.int32), (sdf, w, col))
    have = _mesh_and_compare(ov, gv, ids, "filter, %s" % mode)
    centres = [(6 * k - 20, 2, 2) for k in range(7)]
    if mode == "absent":
        assert not have
    elif mode == "present":  # (an edge or corner voxel alone completes no cell: its cells need the face neighbours too)
        assert [c in have for c in centres] == [True] * 3 + [False] * 4
    else:
        assert all(c in have for c in centres)
