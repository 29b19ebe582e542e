"""The mesher (k_mesh_filter + k_mesh, tf_mesh.hip) on the hand-built cases of tests/mesh_inputs.py, one decision per case:
who owns a vertex, the edge validity thresholds, the adjacency flags and their exchange, the mesh store at its capacities,
the filter's classes and its two forms.  Every case goes onto both sides -- chunk contents uploaded (set_chunk), made
dirty through finalize, meshed -- and the device's meshes must equal the oracle's bit for bit (tests/test_gpu_mesh.py::
_compare_meshes) AND hold the case's known answer, which tests/test_mesh_edges_cpu.py proves on the oracle: a case does
not pass because both sides are wrong together."""
import numpy as np
import pytest

from texturefusion_amd import capi, synth
from tests import mesh_inputs as M
from tests.test_gpu_mesh import _compare_meshes
from tests.util import make_pair

pytestmark = pytest.mark.gpu


def device_meshes(gv):
    ids = gv.list_meshes()
    if len(ids) == 0:
        return {}
    voff, ioff, V, N, Cc, I, adj, simp = gv.get_meshes(ids)
    return {tuple(int(c) for c in cid): dict(verts=V[voff[i]:voff[i + 1]], normals=N[voff[i]:voff[i + 1]],
                                             colors=Cc[voff[i]:voff[i + 1]], indices=I[ioff[i]:ioff[i + 1]], adj=adj[i],
                                             simplified=bool(simp[i])) for i, cid in enumerate(ids)}


def run_on_both(scene):
    ov, gv, _, _ = make_pair(scene.res, synth.Camera(), max_chunks=scene.max_chunks, **scene.volume)
    cache = {}
    for step in scene.steps:
        M.apply_step(step, [ov, gv], cache)
        no, ng = ov.update_meshes(), gv.update_meshes()
        assert ng == len(ov.dirty()) and no <= ng
        if step.compress:
            assert np.array_equal(ov.compress_meshes(), gv.compress_meshes()), step.what
            assert len(gv.dirty()) == 0
        _compare_meshes(ov, gv, step.what)
        M.check_step(step, device_meshes(gv), "device")
    gv.close()


@pytest.mark.parametrize("name", M.SCENE_NAMES)
def test_known_answers_hold_on_the_device(gpu_required, name):
    run_on_both(M.scene(name))


def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("verts", "normals", "colors")) and \
        np.array_equal(a["indices"], b["indices"])


def test_f_without_an_overflow_pool(gpu_required):
    """blocks of 64 vertices / 64 triangles and no large pool: the meshes of exactly 64 / 64 and of 48 / 64 are stored and
    equal the oracle's, the ones a vertex or a triangle past are reported and stored empty"""
    scene = M.scene("F capacities")
    ov, gv, _, _ = make_pair(scene.res, synth.Camera(), max_chunks=scene.max_chunks, mesh_max_vertices=64,
                             mesh_max_triangles=64, mesh_overflow_blocks=-1)
    step = scene.steps[0]
    M.apply_step(step, [ov, gv], {})
    ov.update_meshes()
    with pytest.raises(capi.TFError) as e:
        gv.update_meshes()
    assert e.value.code == capi.TF_ERR_CAPACITY and "mesh" in str(e.value)
    dev = device_meshes(gv)
    past = {M.f_centre(want) for want, fit in M.F_FIT.items() if not fit}
    assert len(past) == 2
    for want in M.F_MIXES:
        c = M.f_centre(want)
        if c in past:
            assert c not in dev, "%s is past the block: nothing stored, and a chunk that never had a mesh gets no key" % (want,)
        else:
            M.check(step.expect[c], dev.get(c), "device, F without a large pool, %s" % (want,))
    for cid in ov.list_meshes():  # everything else, the small meshes of the face neighbours included
        key = tuple(int(c) for c in cid)
        if key not in past:
            assert key in dev and _same(ov.get_mesh(cid), dev[key]), key
    assert set(dev) - past == {tuple(int(c) for c in cid) for cid in ov.list_meshes()} - past
    gv.close()


def _upload(chunks, ids, vols):
    for key, f in chunks.items():
        for v in vols:
            v.set_chunk(np.array(key, np.int32), *f)
    ids = np.array(ids, np.int32)
    for v in vols:
        v.finalize(ids, np.ones(len(ids), np.uint8), np.zeros(len(ids), np.uint8))


def test_g_both_filter_forms(gpu_required):
    """10752 dirty ids in a volume of 2^14 slots: the first update_meshes picks the filter's wave form (it has not heard of
    a list yet) over a list longer than that form's grid of 10240 waves; the call leaves the list's length behind and the
    dirty set as it was, so the second call filters the same set in the workgroup-batch form.  Same meshes both times, and
    the clusters among the chunks -- the class's only voxel in a + neighbour that exists -- hold their known answers in
    both forms."""
    step = M.g_forms_scene()
    ov, gv, _, _ = make_pair(M.RES5, synth.Camera(), max_chunks=1 << 14, mesh_max_vertices=2240, mesh_max_triangles=2560,
                             mesh_blocks=2048)
    M.apply_step(step, [ov, gv], {})
    assert len(ov.dirty()) == 10752
    for call in ("first", "second"):
        ov.update_meshes()
        assert gv.update_meshes() == 10752
        assert _compare_meshes(ov, gv, "filter forms, %s call" % call) > 900
        step.what = "G forms, %s call" % call
        M.check_step(step, device_meshes(gv), "device")
        assert len(gv.dirty()) == 10752
    gv.close()


def test_g_more_survivors_than_the_meshers_grid(gpu_required):
    """16 x 16 x 13 = 3328 chunks with a surface through every one: more survivors than the mesher has workgroups (12 per
    CU), so some workgroups walk a second row of the survivor lists"""
    chunks, ids = M.g_block_scene()
    ov, gv, _, _ = make_pair(M.RES5, synth.Camera(), max_chunks=1 << 15)
    _upload(chunks, ids, [ov, gv])
    ov.update_meshes()
    gv.update_meshes()
    assert _compare_meshes(ov, gv, "block of chunks") == 3328
    gv.close()
