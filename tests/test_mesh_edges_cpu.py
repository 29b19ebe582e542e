"""The hand-built mesher cases of tests/mesh_inputs.py on the oracle: every case's known answer holds there, and the
conditions that make a case sit on its decision are true -- the cube cases used cover all 256, the four cells around a
chosen edge round its vertex differently, the capacity cases have exactly the counts they are named after.  The same
cases run on the device in tests/test_gpu_mesh_edges.py."""
import numpy as np
import pytest

from oracle import api as O
from texturefusion_amd import synth
from tests import mesh_inputs as M


SCENE_NAMES = M.SCENE_NAMES


def oracle_meshes(ov):
    return {tuple(int(c) for c in cid): ov.get_mesh(cid) for cid in ov.list_meshes()}


def run_on_oracle(scene):
    ov = O.Volume(scene.res, O.camera_from(synth.Camera()), O.default_integrator())
    cache = {}
    for step in scene.steps:
        M.apply_step(step, [ov], cache)
        ov.update_meshes()
        if step.compress:
            ov.compress_meshes()
            assert len(ov.dirty()) == 0
        M.check_step(step, oracle_meshes(ov), "oracle")
    return ov


def test_scene_names_are_complete():
    assert sorted(SCENE_NAMES) == sorted(M.scenes())


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_known_answers_hold_on_the_oracle(name):
    scene = M.scene(name)
    assert M.fits(scene.steps, scene.max_chunks), "the scene does not fit a volume of %d slots" % scene.max_chunks
    run_on_oracle(scene)


def test_a_the_cube_cases_cover_all_256_and_the_counts_follow_from_the_signs():
    seen = set()
    for seed in M.A_SEEDS:
        hood, exp = M.case_a(seed)
        nt, nv, cases = M.a_counts(hood)
        assert (exp.nv, exp.nt) == (nv, nt)  # the table walk against the closed formulas
        seen |= cases
        # every vertex on an edge midpoint: in units of half a voxel, relative to the chunk's origin, two coordinates odd
        # (a lattice point) and one even (halfway between two)
        u = np.round(exp.verts.astype(np.float64) / (float(M.RES5) / 2)).astype(int)
        assert np.all(np.abs(exp.verts.astype(np.float64) / (float(M.RES5) / 2) - u) < 1e-3)
        assert np.all((u % 2 == 0).sum(axis=1) == 1)
        # vertex order = ascending slot, the index array = ranks of slots
        assert exp.indices.max() == nv - 1 and len(exp.indices) == 3 * nt
    assert seen == set(range(256))


B_CHOSEN = [(4, 4)] + [o for o in M.B_BORDERS if len(M.slot_cells(M.slot_of(0, M.b_base(0, o)))) == 2]


@pytest.mark.parametrize("others", B_CHOSEN)
@pytest.mark.parametrize("axis", range(3))
def test_b_the_cells_around_a_chosen_edge_round_its_vertex_differently(axis, others):
    """the interior edge (four cells) and the four border edges with two cells, per axis: any two candidates differ"""
    cand = M.b_candidates(axis, others)
    assert len(cand) == (4 if others == (4, 4) else 2)
    for i in range(len(cand)):
        for j in range(i):
            assert np.any(cand[i].view(np.uint32) != cand[j].view(np.uint32)), (axis, others, i, j)
    # the answers of the subsets differ accordingly: the owner is the last emitting cell, and every cell owns in some subset
    m, cells, subs = M.b_subsets(axis, others)
    owners = set()
    for keep, step in subs:
        exp = step.expect[M.B_CENTRE]
        i = [k for k, (cell, e) in enumerate(exp.owners) if M.edge_slot(*cell, e) == m]
        assert len(i) == 1
        last = max((c for c, e in keep), key=lambda c: c[0] + 8 * c[1] + 64 * c[2])  # (cells are walked z, y, x)
        assert exp.owners[i[0]][0] == last
        owners.add(last)
    assert owners == {c for c, e in cells}


def test_f_the_capacity_cases_have_exactly_their_counts():
    for kind, add in M.F_ADDS.items():
        counts = [0, 0, 0, 0]
        counts[kind] = 1
        hood, exp = M.f_case(tuple(counts), (0, 0, 0))
        assert (exp.nv, exp.nt) == add
        ov = O.Volume(M.RES5, O.camera_from(synth.Camera()), O.default_integrator())
        for key, f in hood.chunks().items():
            ov.set_chunk(np.array(key, np.int32), *f)
        V, N, Cc, I = ov.mesh_chunk(np.zeros(3, np.int32))
        assert (len(V), len(I) // 3) == add
    for want, mix in M.F_MIXES.items():
        hood, exp = M.f_case(mix, M.f_centre(want))
        assert (exp.nv, exp.nt) == want
        assert M.F_FIT[want] == (want[0] <= 64 and want[1] <= 64)
    hood, exp = M.case_checkerboard()
    assert exp.nv == 3 * 8 * 81 == 1944 == M.a_counts(hood)[1] and exp.nt == M.a_counts(hood)[0]


def test_e_the_half_cell_crossings_are_decided_by_rounding():
    """t = 0.5 in the first / last cell: the flag follows from one rounding, and over the chosen chunk ids it falls both
    ways -- the ids sit on the decision"""
    scene = M.scene("E half")
    ov = run_on_oracle(scene)
    got = {k: set() for k in range(6)}
    for k in range(6):
        for j in range(8):
            m = ov.get_mesh(np.array(M.e_id(k, j), np.int32))
            assert m["simplified"]
            got[k].add(int(m["adj"][k]))
            assert [int(a) for i, a in enumerate(m["adj"]) if i != k] == [0] * 5
    assert any(v == {0, 1} for v in got.values()), got


def test_g_large_scenes_fit_their_volumes_and_the_clusters_hold_their_answers():
    step = M.g_forms_scene()
    assert len(step.ids) == 1536 and 7 * len(step.ids) == 10752 <= 1 << 14
    assert M.fits([step], 1 << 14)
    assert len(step.expect) == 69 and sum(e.key for e in step.expect.values()) == 48  # (21 beyond the layer that is read)
    ov = O.Volume(M.RES5, O.camera_from(synth.Camera()), O.default_integrator())
    M.apply_step(step, [ov], {})
    assert len(ov.dirty()) == 10752
    ov.update_meshes()
    M.check_step(step, oracle_meshes(ov), "oracle")
    chunks, ids = M.g_block_scene()
    assert len(ids) == 16 * 16 * 13
    assert M.fits([M.Step("block", chunks, ids, {})], 1 << 15)
