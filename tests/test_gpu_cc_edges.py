"""Chisel::CompensateColor -- the device-resident tf_compensate_color_device (k_ccd_*, tf_cc.hip) and the host-solved
tf_compensate_color (k_cc_reduce / k_cc_apply, tf_atlas.hip) -- on the hand-built scene of tests/cc_inputs.py: patches of
1, 2, 63, 64, 65, 127, 128, 129 and 2240 vertices; clusters of one and of two vertices; a constant, a grey, a
low-contrast and an identity keyframe; a cluster that mixes good, wrongly mapped and empty patches; clusters that learn
nothing; 64 frame ids on one probe chain of the frame-id table; 400 clusters of one patch each.

Reference: tests/cc_ref.py's exact-sum restatement with transfer_f64 (numpy.linalg.eigh: none of the Jacobi text the
device runs), fed the device's own patches -- which are first held, bit for bit, to tests/patch_ref.py's prediction, so
that the census of tests/test_cc_inputs_cpu.py (what every cluster is; the references agree on it within TOL) speaks
for this very run.  TOL is the stage's 2e-5 (tests/test_color_compensate.py); flags, frame ids, counts, the labs nobody
may write, the closed form of the constant keyframe and the vertex stream of DrawMeshes are exact.  Nothing here is
arranged to fault: every input is an ordinary call of the ABI."""
import numpy as np
import pytest

from oracle import api as O
from tests import cc_inputs as CI
from tests.cc_ref import labs_exact_sums, transfer_f64
from tests.test_color_compensate import TOL
from tests.test_gpu_patch_borders import _upload_hand_meshes
from tests.util import HipBuffer
from texturefusion_amd import capi

pytestmark = pytest.mark.gpu
HAS, WRONG, IMAGE, ADJ = CI.HAS, CI.WRONG, CI.IMAGE, CI.ADJ


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Scene:
    """the scene on one device volume, behind GeneratePatches"""

    def __init__(self):
        self.sc = CI.scene()
        self.gv = capi.Volume(CI.RES, CI.CAM, max_chunks=1 << 14, atlas_w=CI.AW, atlas_h=CI.AH,
                              max_keyframes=CI.MAX_KEYFRAMES)
        self.bufs = []

    def build(self):
        sc, gv = self.sc, self.gv
        assert gv.atlas_patch_size() == CI.SLOT
        self.ids = _upload_hand_meshes(gv, CI.CAM, sc["meshes"])
        shared = {}  # K's and L's ids borrow ONE device image each; the ten others are cached from the host
        for kid, (rgb, depth) in sc["keyframes"].items():
            if kid in CI.KF.values():
                gv.keyframe_cache(kid, rgb, depth, sc["T16"])
                continue
            if id(rgb) not in shared:
                shared[id(rgb)] = (HipBuffer(rgb.nbytes).from_host(rgb), HipBuffer(depth.nbytes).from_host(depth))
                self.bufs += shared[id(rgb)]
            c, d = shared[id(rgb)]
            gv.keyframe_cache_device(kid, c.ptr, d.ptr, stride=3, pose_inv16=sc["T16"])
        assert len(shared) == 2
        labels = np.array([m["kf"] for m in sc["meshes"]], np.int32)
        rc, hot = gv.generate_patches(self.ids, labels)
        assert rc == 0
        return self.ids

    def patches(self):
        return self.gv.get_patches(self.ids)

    def mesh_colours(self):
        voff, ioff, V, N, Cc, I_, adj, simp = self.gv.get_meshes(self.ids)
        return voff, Cc

    def close(self):
        if self.gv is not None:
            self.gv.sync()
            self.gv.close()
            self.gv = None
        for b in self.bufs:
            b.free()
        self.bufs = []


@pytest.fixture
def scenes(gpu_required):
    """-> a factory of built Scenes; whatever it made -- the volume of 1 << 14 chunks, its atlas, the cached keyframes,
    the two shared images -- is released when the test ends, passed or failed"""
    made = []

    def make():
        made.append(Scene())
        made[-1].build()
        return made[-1]

    yield make
    for S in made:
        S.close()


def _masks(sc, p):
    """vertex masks by cluster letter, and of the compared set: every vertex of every learnt, correctly mapped patch
    except B's"""
    wrong = (p["flags"] & WRONG) > 0
    by = {}
    for name in "ABCDEFGHIJKL":
        by[name] = CI.vertex_mask(p["voff"], [i for i, m in enumerate(sc["meshes"]) if m["cluster"] == name])
    compared = CI.vertex_mask(p["voff"], [i for i, m in enumerate(sc["meshes"])
                                          if m["cluster"] in CI.LEARNT and m["cluster"] != "B" and not wrong[i]])
    return by, compared, CI.vertex_mask(p["voff"], np.flatnonzero(wrong))


def _check_generated(S):
    """step 2: the device's patches are tests/patch_ref.py's prediction, texcolor bit for bit"""
    pred = CI.predicted()
    before = S.patches()
    assert np.array_equal(before["voff"], pred["voff"])
    assert np.array_equal(_bits(before["texcolor"]), _bits(pred["texcolor"])), "texcolor: the census no longer speaks for this run"
    assert np.array_equal(before["flags"] & 31, pred["flags"]) and np.array_equal(before["frameid"], pred["frameid"])
    voff, Cc = S.mesh_colours()
    assert np.array_equal(voff, pred["voff"]) and np.array_equal(_bits(Cc), _bits(pred["meshcolor"]))
    return pred, before, Cc


def _reference(before, Cc):
    has = (before["flags"] & HAS) > 0
    return labs_exact_sums(before["frameid"], (before["flags"] & WRONG) > 0, ((before["flags"] & ADJ) > 0) | ~has,
                           before["voff"], before["texcolor"], Cc, solve=transfer_f64)


def _closed_form_d(Cc, d):
    """D: Cs = 0, T = 0, labs = the mean of the mesh colours (tests/test_cc_inputs_cpu.py)"""
    return (Cc[d].astype(np.float64).sum(0) / d.sum()).astype(np.float32)


def _check_first_call(S, compensate, what, d_bit_for_bit):
    """steps 2-4 and 6 -> (before, after)"""
    sc = S.sc
    pred, before, Cc = _check_generated(S)
    by, compared, wrong_v = _masks(sc, pred)
    # step 3: count, flags, frame ids
    n1, flags1 = CI.compensate_model(pred["frameid"], pred["flags"], pred["nv"])
    assert n1 == CI.N_FRAMES == 474
    assert compensate() == n1, what
    after = S.patches()
    assert np.array_equal(after["flags"] & 31, flags1), what
    assert np.array_equal(after["frameid"], pred["frameid"]), what
    learnt = np.array([m["cluster"] in CI.LEARNT for m in sc["meshes"]])
    assert np.array_equal((after["flags"] & ADJ) > 0, learnt)  # H's wrong patches, H's empty mesh and B included
    assert ((after["flags"][~learnt] & ADJ) == 0).all() and (~learnt).sum() == 4  # I and J
    for k in ("texcolor", "texcoord"):
        assert np.array_equal(_bits(after[k]), _bits(before[k])), k
    # step 4: labs
    want, adj = _reference(before, Cc)
    wrote = ~np.isnan(want).any(1)
    assert np.array_equal(wrote, compared), "the compared set is every vertex of every learnt, correctly mapped patch but B's"
    assert np.array_equal(adj, learnt)
    err = np.abs(after["labs"] - want).max(1)
    assert np.isfinite(after["labs"][compared]).all(), what
    print("%s against exact sums + eigh: max |labs| difference %.3g over %d vertices; per cluster %s"
          % (what, err[compared].max(), compared.sum(),
             " ".join("%s %.2g" % (k, err[by[k] & compared].max()) for k in "ACDEFGHKL")))
    assert err[compared].max() <= TOL, what
    closed = _closed_form_d(Cc, by["D"])
    d_err = np.abs(after["labs"][by["D"]] - closed).max()
    d_same = np.array_equal(_bits(after["labs"][by["D"]]), _bits(np.broadcast_to(closed, (int(by["D"].sum()), 3))))
    print("%s: D against its closed form: max %.3g, bit for bit: %s" % (what, d_err, d_same))
    assert d_err <= TOL
    if d_bit_for_bit:
        assert d_same, what
    assert np.isnan(after["labs"][by["B"]]).all(), "B: labs of a one-vertex cluster are NaN (the census)"
    untouched = by["I"] | by["J"] | wrong_v
    assert untouched.sum() == 389
    assert np.array_equal(_bits(after["labs"][untouched]), _bits(before["labs"][untouched])), what
    return pred, before, after, Cc


def _check_second_call(S, compensate, after, what):
    """step 6: only I and J are left, and nothing moves"""
    assert compensate() == 2, what
    again = S.patches()
    assert np.array_equal(again["flags"], after["flags"]), what
    assert np.array_equal(_bits(again["labs"]), _bits(after["labs"])), what
    return again


def test_device_path_on_hand_built_clusters(scenes):
    S = scenes()
    sc, gv, ids = S.sc, S.gv, S.ids
    pred, before, after, Cc = _check_first_call(S, gv.compensate_color_device, "device path", d_bit_for_bit=True)
    # step 5: DrawMeshes over the whole scene, B's NaN labs included (a delta that is not a number packs as 255)
    gV, gI = gv.draw_meshes()
    voff, ioff, V, N, Cc2, I_, madj, simp = gv.get_meshes(ids)
    complete = ((np.diff(voff) > 0) & (simp > 0) & ((after["flags"] & IMAGE) > 0) & (after["frameid"] >= 0)).astype(np.uint8)
    wrong = ((after["flags"] & WRONG) > 0).astype(np.uint8)
    labs_valid = (((after["flags"] & ADJ) > 0) & (wrong == 0)).astype(np.uint8)
    assert complete.sum() == (np.diff(voff) > 0).sum() == CI.N_MESHES - 3
    rV, rI = O.pack_vertices(complete, wrong, labs_valid, after["texloc"], after["ratio"], CI.AW, CI.AH, voff, V, Cc2, N,
                             after["texcoord"], after["texcolor"], after["labs"], ioff, I_)
    assert len(gV) == voff[-1] and np.array_equal(_bits(rV), _bits(gV)) and np.array_equal(rI, gI)
    (b,) = [i for i, m in enumerate(sc["meshes"]) if m["cluster"] == "B"]
    assert gV[voff[b], 5] == np.float32((255 << 18) + (255 << 9) + 255)
    assert (gV[:, 5] != 0).sum() == np.repeat(labs_valid, np.diff(voff)).sum()
    # step 6
    again = _check_second_call(S, gv.compensate_color_device, after, "device path, second call")
    # step 7: every third mesh of A, E, H and K regenerated under A's keyframe; the rest keeps has_adjusted
    sub = CI.regen_subset(sc)
    labels = pred["frameid"].copy()
    labels[sub] = CI.KF["A"]
    q = CI.predict(dict(sc, meshes=[sc["meshes"][i] for i in sub]), labels[sub])
    rc, hot = gv.generate_patches(ids[sub], labels[sub])
    assert rc == 0
    g3 = S.patches()
    flags3 = again["flags"] & 31
    flags3[sub] = q["flags"]
    assert np.array_equal(g3["flags"] & 31, flags3) and np.array_equal(g3["frameid"], labels)
    in_sub = CI.vertex_mask(voff, sub)
    assert np.array_equal(_bits(g3["texcolor"][in_sub]), _bits(q["texcolor"]))
    assert np.array_equal(_bits(g3["texcolor"][~in_sub]), _bits(before["texcolor"][~in_sub]))
    n3, f3 = CI.compensate_model(labels, flags3, pred["nv"])
    assert n3 == 3  # A's id with the regenerated patches alone, and I and J once more
    assert gv.compensate_color_device() == n3
    g4 = S.patches()
    assert np.array_equal(g4["flags"] & 31, f3) and ((f3[sub] & ADJ) > 0).all()
    want, adj = _reference(g3, Cc)
    good = CI.vertex_mask(voff, [i for i in sub if not (flags3[i] & WRONG)])
    assert np.array_equal(~np.isnan(want).any(1), good) and good.sum() >= 100
    # the statistics are the subset's alone: with A's adjusted patches taken in as well, labs would be elsewhere
    mixed = g3["flags"].copy()
    mixed[g3["frameid"] == CI.KF["A"]] &= ~ADJ
    other, _ = _reference(dict(g3, flags=mixed), Cc)
    assert np.abs(other[good] - want[good]).max() > 100 * TOL
    err = np.abs(g4["labs"][good] - want[good]).max()
    print("device path, regenerated subset: max |labs| difference %.3g over %d vertices" % (err, good.sum()))
    assert err <= TOL
    assert np.array_equal(_bits(g4["labs"][~in_sub]), _bits(again["labs"][~in_sub]))


def test_host_path_on_hand_built_clusters(scenes):
    """k_cc_reduce / k_cc_apply (256 threads striding the vertices, f32 trees) at the same vertex-count and degeneracy
    edges, against the same reference and TOL.  D is held to TOL and, as the run shows it, to its closed form bit for
    bit: its f32 sums of multiples of 1 / 256 are exact and the one division rounds as the reference's does."""
    S = scenes()
    pred, before, after, Cc = _check_first_call(S, S.gv.compensate_color, "host path", d_bit_for_bit=True)
    _check_second_call(S, S.gv.compensate_color, after, "host path, second call")


def _written(g):
    """the labs the stage defines: those of the patches it has adjusted and that are not wrongly mapped (the reference
    leaves the labs of every other patch EMPTY; the device's planes there hold whatever they held -- a fresh pool's
    bytes, or an earlier scene's labs after tf_volume_reset -- and nothing reads them)"""
    ok = ((g["flags"] & ADJ) > 0) & ((g["flags"] & WRONG) == 0)
    return _bits(g["labs"][np.repeat(ok, np.diff(g["voff"]))]).copy()


def _one_run(scenes):
    S = scenes()
    assert S.gv.compensate_color_device() == CI.N_FRAMES
    g = S.patches()
    out = (S.ids.copy(), g["flags"].copy(), _written(g))
    S.close()  # before the second volume is made
    return out


def test_two_runs_give_the_same_bits_with_collisions(scenes):
    """K (64 ids on one probe chain, two patches racing for every entry) and L (400 ids) are where the slot a frame id
    lands in depends on timing: it may decide where a value is stored, never a bit of it."""
    a, b = _one_run(scenes), _one_run(scenes)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert ((a[1] & ADJ) > 0).sum() == CI.N_MESHES - 4
    assert len(a[2]) == CI.predicted()["voff"][-1] - 389 and np.array_equal(a[2], b[2])


def test_after_reset(scenes):
    """tf_volume_reset frees the path's block; the same handle then builds the scene again and gives the same bits"""
    S = scenes()
    ids = S.ids.copy()
    assert S.gv.compensate_color_device() == CI.N_FRAMES
    first = S.patches()
    S.gv.reset()
    assert S.gv.compensate_color_device() == 0  # nothing left to compensate, and the block is allocated anew
    S.build()
    assert np.array_equal(S.ids, ids)
    fresh = S.patches()
    assert ((fresh["flags"] & ADJ) == 0).all()
    assert S.gv.compensate_color_device() == CI.N_FRAMES
    second = S.patches()
    assert np.array_equal(second["flags"], first["flags"]) and ((second["flags"] & ADJ) > 0).sum() == CI.N_MESHES - 4
    assert len(_written(first)) == first["voff"][-1] - 389 and np.array_equal(_written(second), _written(first))
