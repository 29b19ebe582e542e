"""The hand-built scene of the CompensateColor edge tests, shared by tests/test_cc_inputs_cpu.py (which says, with the
references alone, what every cluster of it is) and tests/test_gpu_cc_edges.py (which runs it through both device paths):
the GPU tests cannot drift to inputs the census never saw.

numpy + texturefusion_amd.synth + tests/patch_inputs.py + tests/patch_ref.py only: no oracle, no GPU.

One camera (160 x 120), 5 mm voxels, one keyframe pose; every vertex is back-projected from an "interior" image position
(tests/patch_inputs.py) at z = 1.1, the keyframes' depth images are the usual [1.0, 1.2) noise, and the mesh colours are
derived from tests/patch_ref.py's own texcolor, so that the colour compare fires nowhere and the depth compare exactly
where a patch is built at z = 2.1.  Clusters, keyed by frame id (CLUSTERS below is the table):

  A general        white noise; the vertex counts that straddle a wave (64) and the host path's workgroup (256)
  B one vertex     covariance 0 / (N - 1) = 0 / 0: labs are NaN
  C two vertices   rank-1 covariances
  D constant       a black keyframe: texcolor is exactly 0 on every vertex, the source covariance exactly 0
  E grey           R = G = B: the source covariance has rank 1 (three equal rows)
  F low contrast   every channel 200 or 201: source variances of 2e-6 (the bilinear blend halves the two-level
                   image's 4e-6), far below the 1e-2 regulariser
  G identity       mesh colours are texcolor itself
  H mixed          six good patches, three wrongly mapped, one empty mesh
  I all wrong      learns nothing
  J all empty      learns nothing
  K colliding ids  64 frame ids on one probe chain of the device path's table, two patches each
  L cluster/patch  400 consecutive ids, one patch each

The meshes are dealt onto the chunk ids by a fixed-seed permutation, so the clusters interleave in chunk order and a
cluster's first patch by rank is not the first one built."""
import functools

import numpy as np

from tests import patch_inputs as PI
from tests import patch_ref as PR
from texturefusion_amd import synth

F = np.float32
CAM = PI.CAMERAS["small"]
RES = PI.RESOLUTIONS[0]
SLOT = PI.slot_size(RES)
AW, AH = 1920, 720        # 80 x 40 slots of 24 x 18
MAX_KEYFRAMES = 512       # tf_config.max_keyframes: the scene caches 474
HAS, CAUTION, WRONG, IMAGE, ADJ = 1, 2, 4, 8, 16  # TF_PATCH_*

KF = dict(A=10, B=11, C=12, D=13, E=14, F=15, G=16, H=17, I=18, J=19)
# K: ids that differ by multiples of 2^25.  The device path's table hashes (uint32) id by a 32-bit multiplication, drops
# the product's low 7 bits and masks.  Two ids that differ by j * 2^25 have products that differ by j * 2^25 * (an odd
# constant): only in product bits 25..31, i.e. hash bits 18..24.  The table this scene gets has 2048 entries (the
# smallest power of two >= 2 * 568 patches) -- mask bits 0..10, and no list a handle of 2^14 chunks can hold reaches bit
# 18 -- so all 64 ids share one home slot and form ONE probe chain of length 64; two patches per id race on every entry
# of it.  (63 * 2^25 + K0 < 2^31: the ids stay positive int32.)
K0, K_IDS = 1000, 64
K_FRAMES = tuple(K0 + j * 2 ** 25 for j in range(K_IDS))
L0, L_IDS = 5000, 400
L_FRAMES = tuple(range(L0, L0 + L_IDS))

# cluster -> (vertex counts of its good patches, of its wrongly mapped patches (built at z = 2.1), empty meshes)
CLUSTERS = {
    "A": ((1, 2, 5, 17, 63, 64, 65, 127, 128, 129, 192, 2240), (), 0),
    "B": ((1,), (), 0),
    "C": ((2,), (), 0),
    "D": ((64, 65, 300), (), 0),
    "E": ((40, 129, 200), (), 0),
    "F": ((65, 150, 300), (), 0),
    "G": ((17, 128, 200), (), 0),
    "H": ((3, 17, 64, 100, 129, 200), (5, 65, 150), 1),
    "I": ((), (40, 129), 0),
    "J": ((), (), 2),
}
K_COUNTS = (40, 65)
LEARNT = "ABCDEFGHKL"  # I and J learn nothing: has_adjusted stays clear
N_MESHES = sum(len(g) + len(w) + e for g, w, e in CLUSTERS.values()) + K_IDS * len(K_COUNTS) + L_IDS  # 568
N_FRAMES = len(KF) + K_IDS + L_IDS  # 474
REGEN_CLUSTERS, REGEN_EVERY = "AEHK", 3


def _images():
    """-> {frame id: (rgb u8[H,W,3], depth f32[H,W])}; K's 64 ids share one image, L's 400 another"""
    out = {}
    for k, (name, kid) in enumerate(sorted(KF.items())):
        rgb, depth, _ = PI.keyframe_images(CAM, 9000 + k)
        if name == "D":
            rgb = np.zeros_like(rgb)  # texcolor = 0 / 255 blended with any weights: exactly 0
        elif name == "E":
            rgb = np.repeat(rgb[..., :1], 3, -1)
        elif name == "F":
            rgb = (200 + (rgb & 1)).astype(np.uint8)
        out[kid] = (np.ascontiguousarray(rgb), depth)
    shared_k = PI.keyframe_images(CAM, 9100)[:2]
    shared_l = PI.keyframe_images(CAM, 9101)[:2]
    for kid in K_FRAMES:
        out[kid] = shared_k
    for kid in L_FRAMES:
        out[kid] = shared_l
    return out


def _gain(rng):
    """what the keyframe sees the mesh colours through: per-channel gain 0.7 .. 1.1, offset <= 0.05.  The largest colour
    difference this leaves is 0.3 per channel, 0.52 in norm: inside the colour compare's 0.6"""
    g, o = rng.uniform(0.7, 1.1, 3).astype(F), rng.uniform(0.0, 0.05, 3).astype(F)
    return lambda tex, rng: np.clip(tex * g + o, F(0), F(1)).astype(F)


def _colour_rule(name, rng):
    if name == "D":  # multiples of 1 / 256 in [0, 0.3]: sums of a few hundred are exact in f32 and f64 alike
        return lambda tex, rng: (rng.integers(0, 77, tex.shape) / 256.0).astype(F)
    if name == "E":
        g, o = np.array([0.7, 0.8, 0.9], F), np.array([0.01, 0.02, 0.03], F)
        return lambda tex, rng: (tex * g + o).astype(F)
    if name == "F":
        return lambda tex, rng: (tex + rng.uniform(-0.1, 0.1, tex.shape).astype(F)).astype(F)
    if name == "G":
        return lambda tex, rng: tex.copy()
    return _gain(rng)


@functools.lru_cache(maxsize=1)
def scene():
    """-> dict(cam, res, slot, pose, T16, keyframes {id: (rgb, depth)}, meshes [dict(cluster, kf, verts, colors, z)]),
    the meshes in the order they go onto the ascending chunk ids (mesh i has rank i)"""
    rng = np.random.Generator(np.random.PCG64(20240))
    pose = PI.general_pose()
    T16 = synth.pose_inverse16(pose)
    images = _images()
    plan = []  # (cluster, frame id, vertices, z, colour rule)
    for name, (good, wrong, empty) in sorted(CLUSTERS.items()):
        rule = _colour_rule(name, rng)
        plan += [(name, KF[name], n, 1.1, rule) for n in good]
        plan += [(name, KF[name], n, 2.1, rule) for n in wrong]  # the depth compare fires on every vertex
        plan += [(name, KF[name], 0, 1.1, rule)] * empty
    for kid in K_FRAMES:
        rule = _gain(rng)
        plan += [("K", kid, n, 1.1, rule) for n in K_COUNTS]
    # L: 5 .. 40 vertices, not 3 .. 40.  Three vertices span a plane: Cs has rank 2, and labs are NOT insensitive to its
    # null direction -- (Cs^1/2 Ct Cs^1/2)^1/2 couples it to the range through Ct, so T has a term
    # Di_null * sqrt(eps) * Di_range that maps a centred colour onto the null direction, eps being whatever the rounding
    # of the covariance's entries left of the zero eigenvalue (+-1e-9, clamped at 0): 100 * 3e-5 * 3 * |d|.  The
    # references themselves then stood 1e-6 .. 8.2e-5 apart on the eleven three-vertex clusters of this table's first
    # version (four of them beyond TOL: the oracle's f32 in-order sums against exact sums, the two solves agreeing to the
    # bit; measured by tests/test_cc_inputs_cpu.py), and 5.4e-6 on a four-vertex cluster whose smallest eigenvalue was
    # 3.6e-7.  From five vertices on the smallest
    # eigenvalue here is >= 8e-4 and the references agree to 2e-7.  (C's two vertices stay: every summation order of two
    # terms rounds alike, so all sides see the same covariance bits.)
    l_counts = 5 + rng.integers(0, 36, L_IDS)
    for kid, n in zip(L_FRAMES, l_counts):
        plan.append(("L", kid, int(n), 1.1, _gain(rng)))
    meshes = []
    for name, kid, n, z, rule in plan:
        rgb, depth = images[kid]
        if n == 0:
            meshes.append(dict(cluster=name, kf=kid, z=z, verts=np.zeros((0, 3), F), colors=np.zeros((0, 3), F)))
            continue
        verts = PI.back_project(CAM, pose, PI.interior_positions(n, CAM, SLOT, rng, z))
        tex = PR.project(verts, np.zeros((n, 3), F), T16, rgb, depth, CAM)["texcolor"]
        meshes.append(dict(cluster=name, kf=kid, z=z, verts=verts, colors=rule(tex, rng)))
    assert len(meshes) == N_MESHES and len(images) == N_FRAMES
    deal = np.random.Generator(np.random.PCG64(7)).permutation(len(meshes))
    return dict(cam=CAM, res=RES, slot=SLOT, pose=pose, T16=T16, keyframes=images, meshes=[meshes[i] for i in deal])


def predict(sc, labels=None):
    """What GeneratePatches leaves, by tests/patch_ref.py: dict(frameid, flags, nv, voff, texcolor, meshcolor, results).
    labels: the frame id per mesh (default: the mesh's own)."""
    meshes = sc["meshes"]
    if labels is None:
        labels = [m["kf"] for m in meshes]
    res = []
    for m, kid in zip(meshes, labels):
        rgb, depth = sc["keyframes"][int(kid)]
        res.append(PR.project(m["verts"], m["colors"], sc["T16"], rgb, depth, sc["cam"]))
    nv = np.array([len(m["verts"]) for m in meshes], np.int64)
    flags = np.array([HAS | IMAGE | (CAUTION if r["flag"] < 0 else 0) | (WRONG if r["wrong_mapping"] else 0)
                      for r in res], np.int32)
    return dict(frameid=np.asarray(labels, np.int32), flags=flags, nv=nv, voff=np.concatenate([[0], np.cumsum(nv)]),
                texcolor=np.concatenate([r["texcolor"] for r in res]).astype(F),
                meshcolor=np.concatenate([m["colors"] for m in meshes]).astype(F), results=res)


@functools.lru_cache(maxsize=1)
def predicted():
    return predict(scene())


def compensate_model(frameid, flags, nv):
    """Chisel::CompensateColor on the integers (Chisel.cpp:199-214, :242, :280) -> (clusters counted, flags behind it):
    the patches without has_adjusted cluster by frame id; a cluster whose correctly mapped patches hold a vertex is learnt
    and every member of it, wrongly mapped and empty ones included, gets has_adjusted"""
    frameid, flags, nv = np.asarray(frameid), np.asarray(flags).copy(), np.asarray(nv)
    todo = ((flags & HAS) > 0) & ((flags & ADJ) == 0)
    ids = np.unique(frameid[todo])
    for f in ids:
        mem = todo & (frameid == f)
        if nv[mem & ((flags & WRONG) == 0)].sum() > 0:
            flags[mem] |= ADJ
    return len(ids), flags


def regen_subset(sc):
    """step 7 of the GPU test: every third mesh, by rank, of the clusters A, E, H and K -- regenerated under A's keyframe"""
    pick = [i for i, m in enumerate(sc["meshes"]) if m["cluster"] in REGEN_CLUSTERS]
    return np.array(pick[::REGEN_EVERY], np.int64)


def vertex_mask(voff, patches):
    """bool[total vertices]: the vertices of the listed patches"""
    m = np.zeros(int(voff[-1]), bool)
    for p in patches:
        m[voff[p]:voff[p + 1]] = True
    return m
