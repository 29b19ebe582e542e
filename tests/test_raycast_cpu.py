"""CPU checks of the raycast feature.

Only the last test, the register / scratch budget of k_query and k_raycast compiled for gfx950, exercises the library
itself.  The others check the numpy restatement (tests/raycast_ref.py) against the CPU oracle's volume: GetSDF /
GetWeight / GetSDFAndGradient by hand on chosen voxels, the trilinear SDF against the analytic wall, and the restated
march.  They are checks of the reference the GPU tests (tests/test_gpu_raycast.py) hold the kernels to bit for bit, not
of the kernels, and so they pass without the library's raycast code."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import api as O
from texturefusion_amd import synth
from tests.raycast_ref import WALL_Z, RefVolume, wall_frames, wall_poses
from tests.util import RES5

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texturefusion_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
F = np.float32
@pytest.fixture(scope="module")
def wall():
    cam = synth.Camera()
    ov = O.Volume(RES5, O.camera_from(cam), O.default_integrator())
    for depth, rgba, pose in wall_frames(cam):
        ov.integrate_frame(depth, rgba, pose)
    ids = ov.list_chunks()
    ref = RefVolume.from_volume(ov, ids, RES5)
    yield ov, ids, ref
    ov.close()


def _voxel_centre(cid, x, y, z, res=RES5):
    return np.array([(8 * cid[0] + x + 0.5) * res, (8 * cid[1] + y + 0.5) * res, (8 * cid[2] + z + 0.5) * res], np.float32)


def _surface_chunks(ids, ref):
    """chunks holding voxels with weight > 0 on both sides of the wall"""
    out = []
    for cid in ids:
        j = ref.slot(*cid)
        w, sd = ref.w[j], ref.sdf[j]
        if (w > 0).any() and (sd[w > 0] > 0).any() and (sd[w > 0] < 0).any():
            out.append(cid)
    return np.array(out, np.int32)


def test_get_sdf_and_weight_hand_checked(wall):
    """GetSDF / GetWeight at voxel centres are the stored voxel; a point on a voxel or chunk face gets one of the two
    voxels it touches; absent chunks are invalid"""
    ov, ids, ref = wall
    surf = _surface_chunks(ids, ref)
    assert len(surf) > 20
    rng = np.random.default_rng(1)
    for cid in surf[rng.choice(len(surf), 8, replace=False)]:
        s, w, _ = ov.get_chunk(cid)
        for x, y, z in ((0, 0, 0), (7, 7, 7), (3, 4, 5), (0, 7, 2)):
            q = ref.query(_voxel_centre(cid, x, y, z)[None])
            vi = (z * 8 + y) * 8 + x
            assert q["flags"][0] & 2 and q["weight"][0] == w[vi]
            assert bool(q["flags"][0] & 1) == (float(w[vi]) > 1e-12)
            if w[vi] > 0:
                assert q["sdf"][0] == s[vi]
        # on the x face between voxels 2 and 3 of row (y, z) = (4, 5), and on the chunk's own low x face
        for xf, cand in ((3, (2, 3)), (0, (-1, 0))):
            p = _voxel_centre(cid, xf, 4, 5)
            p[0] = F((8 * cid[0] + xf) * RES5)
            q = ref.query(p[None])
            if q["flags"][0] & 2:
                vals = []
                for xc in cand:
                    c2 = np.array(cid) + np.array([xc // 8, 0, 0])
                    if ov.has_chunk(c2):
                        vals.append(ov.get_chunk(c2)[1][(5 * 8 + 4) * 8 + (xc % 8)])
                assert q["weight"][0] in vals
    q = ref.query(np.array([[10.0, 10.0, 10.0]], np.float32))  # an absent chunk
    assert q["flags"][0] == 0 and q["sdf"][0] == 0 and q["weight"][0] == 0


def test_gradient_across_the_six_chunk_faces(wall):
    """GetSDFAndGradient on the faces of a chunk reads the adjacent chunk at the wrapped index; a missing neighbour
    chunk or a neighbour value >= 1 makes it invalid"""
    ov, ids, ref = wall
    surf = _surface_chunks(ids, ref)
    idset = {tuple(c) for c in ids.tolist()}
    checked = {"cross": 0, "missing": 0}
    for cid in surf:
        for a in range(3):
            for face in (0, 7):
                for zl in range(8):
                    loc = [3, 4, zl]
                    loc[a] = face
                    g, ok = ref.gradient(_voxel_centre(cid, *loc)[None])
                    nb = list(cid)
                    nb[a] += 1 if face == 7 else -1
                    if tuple(nb) not in idset:
                        assert not ok[0]
                        checked["missing"] += 1
                        continue
                    vals = []  # the six neighbours by hand from the raw arrays
                    for k in range(6):
                        ax, sg = k >> 1, (1 if k & 1 else -1)
                        l2 = list(loc)
                        l2[ax] += sg
                        c2 = list(cid)
                        if l2[ax] < 0 or l2[ax] > 7:
                            c2[ax] += sg
                            l2[ax] %= 8
                        if tuple(c2) not in idset:
                            vals.append(None)
                            continue
                        vals.append(ov.get_chunk(np.array(c2, np.int32))[0][(l2[2] * 8 + l2[1]) * 8 + l2[0]])
                    exp_ok = all(v is not None and v < 1 for v in vals)
                    assert ok[0] == exp_ok
                    if exp_ok:
                        exp = np.array([vals[1] - vals[0], vals[3] - vals[2], vals[5] - vals[4]], np.float32)
                        assert np.array_equal(g[0], exp)
                        checked["cross"] += 1
    assert checked["cross"] > 50 and checked["missing"] > 0, checked


def test_trilinear_sdf_of_the_wall_matches_the_plane(wall):
    """the wall's trilinear SDF is the camera-z distance to the plane inside the truncation band"""
    _, _, ref = wall
    rng = np.random.default_rng(2)
    n = 4000
    p = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.3, 0.3, n), WALL_Z + rng.uniform(-0.008, 0.008, n)], 1)
    p = p.astype(np.float32)
    s, ok, rgb, okc = ref.trilinear(p)
    assert ok.mean() > 0.99
    err = np.abs(s[ok] - (F(WALL_Z) - p[ok, 2]))
    assert err.max() < 1e-4, err.max()
    assert okc.mean() > 0.99 and np.all(rgb[okc] == np.array([200, 100, 50], np.uint8))


def test_march_renders_the_wall_back_at_its_depth(wall):
    """the restated step rule, from the middle pose: the wall at its integrated depth (the GPU test holds the kernel
    to this restatement)"""
    _, _, ref = wall
    cam = synth.Camera(160, 120, 131.25, 131.25, 79.5, 59.5)
    d = ref.raycast_depth(wall_poses()[0], cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, 0.1, 3.0, 1024)
    hit = d > 0
    # (the outermost four rows / columns of this 4x coarser camera -- 16 pixels of the integrated images -- also hold
    # rays whose trilinear corners the integrator left unobserved; the full-image figure is the GPU test's)
    assert hit[4:-4, 4:-4].mean() > 0.999 and hit.mean() > 0.98
    assert np.abs(d[hit] - F(WALL_Z)).max() < RES5 / 2


def test_march_of_an_empty_volume_and_a_pose_looking_away(wall):
    _, _, ref = wall
    empty = RefVolume(np.zeros((0, 3), np.int32), np.zeros((0, 512)), np.zeros((0, 512)), np.zeros((0, 2048)), RES5)
    assert not empty.raycast_depth(wall_poses()[0], 131, 131, 79.5, 59.5, 160, 120, 0.1, 3.0, 256).any()
    away = synth.pose_yaw(np.pi)
    assert not ref.raycast_depth(away, 131, 131, 79.5, 59.5, 160, 120, 0.1, 3.0, 256).any()


# k_query / k_raycast resource budget.  Both kernels are gathers through the chunk hash: latency-bound, so occupancy is
# what hides the probes.  k_raycast: 77 VGPRs measured (six waves per SIMD: the march keeps ray origin / direction, t, the
# previous sample and the chunk cache live across the 8-corner gather, whose slots and values take 16 more); budget 80 =
# still six waves.  k_query: 84 measured (the colour sampler's eight ushort4 corners live next to the SDF corners and the
# gradient's state); budget 96 = five waves.  Neither may own private memory.
BUDGET = {"k_raycast": 80, "k_query": 96}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_ray_kernels_stay_within_their_register_budget():
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "tf_ray.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    for frag, max_vgpr in BUDGET.items():
        hits = {k: v for k, v in usage.items() if frag in k}
        assert hits, "kernel %s not found" % frag
        for k, v in hits.items():
            assert v["ScratchSize"] == 0, "%s uses %d B/lane of private memory" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d)" % (k, v["VGPRs"], max_vgpr)
