"""CPU checks of GetDistanceFromSurface / RefineFrameInVoxel.

The first test compiles k_surface_dist and k_refine_frame for gfx950 and holds them to their register / scratch budget.
The others check the numpy restatement (tests/refine_ref.py) that the GPU tests (tests/test_gpu_refine.py) hold the
kernels to bit for bit: against a line-by-line scalar transcription of Structure/Chisel.h:251-451 in np.float32 scalars
on the CPU oracle's wall and S-room volumes, and for what refinement does to a noisy depth image of the wall."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import api as O
from texturefusion_amd import synth
from tests import refine_ref
from tests.raycast_ref import WALL_Z, RefVolume, wall_frames
from tests.util import RES5

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texturefusion_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
F = np.float32

# k_surface_dist / k_refine_frame resource budget.  Both are chains of dependent gathers through the chunk hash, so
# occupancy is what hides their latency: at most 64 allocated VGPRs keeps the register-limited bound at 8 waves per SIMD
# (MI355X: 512 VGPRs per lane and SIMD, allocated in blocks of 8), and the compiler's occupancy remark must say 8 (the
# SGPR count can cap it too).  Measured: k_surface_dist 43 VGPRs, k_refine_frame 49.  Neither may own private memory.
BUDGET = {"k_surface_dist": 64, "k_refine_frame": 64}
MIN_WAVES = 8


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_refine_kernels_stay_within_their_register_budget():
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
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    for frag, max_vgpr in BUDGET.items():
        hits = {k: v for k, v in usage.items() if frag in k}
        assert hits, "kernel %s not found" % frag
        for k, v in hits.items():
            assert v["ScratchSize"] == 0, "%s uses %d B/lane of private memory" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d)" % (k, v["VGPRs"], max_vgpr)
            assert v["Occupancy"] >= MIN_WAVES, "%s: %d waves per SIMD" % (k, v["Occupancy"])


# ---- a line-by-line transcription of Chisel.h:251-451 in np.float32 scalars ------------------------------------------
class ScalarChisel:
    """GetDistanceFromSurface / RefineFrameInVoxel as the reference writes them, one point at a time; the chunk map is a
    dict {(x, y, z): (sdf[512], weight[512])}.  Where the reference converts floor / ceil of a float to int, a value that
    is not finite or beyond +-(2^23 - 1) makes that corner absent (the library's definition)."""

    def __init__(self, chunks, res):
        self.chunks = chunks
        self.res = F(res)

    @staticmethod
    def _to_int(f):
        f = F(f)
        if not (abs(f) <= F(8388607.0)):
            return None
        return int(f)

    def GetDistanceFromSurface(self, global_vertex):
        tsdfWeight = F(0)
        global_vertex = [F(global_vertex[a]) - self.res / F(2) for a in range(3)]
        roundingVoxelStep = F(1.0) / self.res
        rasterizedPose = [global_vertex[a] * roundingVoxelStep for a in range(3)]
        with np.errstate(invalid="ignore"):
            distX = rasterizedPose[0] - np.floor(rasterizedPose[0])
            distY = rasterizedPose[1] - np.floor(rasterizedPose[1])
            distZ = rasterizedPose[2] - np.floor(rasterizedPose[2])
            one = F(1)
            spatialWeight = [(one - distX) * (one - distY) * (one - distZ), (one - distX) * (one - distY) * (distZ),
                             (one - distX) * (distY) * (one - distZ), (one - distX) * (distY) * (distZ),
                             (distX) * (one - distY) * (one - distZ), (distX) * (one - distY) * (distZ),
                             (distX) * (distY) * (one - distZ), (distX) * (distY) * (distZ)]
        fl = [self._to_int(np.floor(rasterizedPose[a])) for a in range(3)]
        ce = [self._to_int(np.ceil(rasterizedPose[a])) for a in range(3)]
        V = [(fl[0], fl[1], fl[2]), (fl[0], fl[1], ce[2]), (fl[0], ce[1], fl[2]), (fl[0], ce[1], ce[2]),
             (ce[0], fl[1], fl[2]), (ce[0], fl[1], ce[2]), (ce[0], ce[1], fl[2]), (ce[0], ce[1], ce[2])]
        weight = F(0)
        distance = F(0)
        for k in range(8):
            if any(c is None for c in V[k]):
                continue
            cid = tuple(int(math.floor(F(V[k][a]) / F(8))) for a in range(3))
            if cid in self.chunks:
                sdf, w = self.chunks[cid]
                vid = (V[k][0] - cid[0] * 8) + (V[k][1] - cid[1] * 8) * 8 + (V[k][2] - cid[2] * 8) * 8 * 8
                weight += spatialWeight[k] * w[vid]
                distance += sdf[vid] * spatialWeight[k] * w[vid]
                tsdfWeight += w[vid] * spatialWeight[k]
        if weight > 0:
            distance = distance / weight
            tsdfWeight = tsdfWeight / weight
        return F(distance), F(tsdfWeight)

    def RefinePixel(self, depthImage, weight, i, j, pose, cam):
        """the body of RefineFrameInVoxel's loop for pixel (i, j); rotation rows summed a0 b0 + (a1 b1 + a2 b2)"""
        width = cam.width
        cx, cy, fx, fy = (F(int(F(a))) for a in (cam.cx, cam.cy, cam.fx, cam.fy))  # int getters read into float
        P = np.asarray(pose, np.float32).reshape(3, 4)
        depth = depthImage[i * width + j]
        if float(depth) < 0.05 or float(depth) > 3:
            return
        dir_ = (F(F(j) - cx) / fx, F(F(i) - cy) / fy, F(1))

        def vertex(dep):
            return [(P[r, 0] * dir_[0] + (P[r, 1] * dir_[1] + P[r, 2] * dir_[2])) * dep + P[r, 3] for r in range(3)]

        with np.errstate(invalid="ignore", over="ignore"):
            updated_distance, tsdfWeight = self.GetDistanceFromSurface(vertex(depth))
            depth_init = depth
            for _ in range(5):
                depth += updated_distance
                updated_distance, tsdfWeight = self.GetDistanceFromSurface(vertex(depth))
            depth += updated_distance
            depthImage[i * width + j] = depth
            weight[i * width + j] = tsdfWeight
            if abs(float(updated_distance)) > 5e-3:
                depthImage[i * width + j] = 0
                weight[i * width + j] = 0
            if depthImage[i * width + j] > F(cam.far) or depthImage[i * width + j] < F(cam.near):
                depthImage[i * width + j] = 0
                weight[i * width + j] = 0
            if abs(float(depthImage[i * width + j] - depth_init)) > 0.1:
                depthImage[i * width + j] = 0
                weight[i * width + j] = 0


def _oracle_volume(frames, cam):
    ov = O.Volume(RES5, O.camera_from(cam), O.default_integrator())
    for depth, rgba, pose in frames:
        ov.integrate_frame(depth, rgba, pose)
    ids = ov.list_chunks()
    ref = RefVolume.from_volume(ov, ids, RES5)
    chunks = {tuple(int(c) for c in cid): (ref.sdf[ref.slot(*cid)], ref.w[ref.slot(*cid)]) for cid in ids}
    ov.close()
    return ref, ScalarChisel(chunks, RES5), ids


@pytest.fixture(scope="module")
def wall():
    cam = synth.Camera()
    frames = wall_frames(cam)
    ref, sc, ids = _oracle_volume(frames, cam)
    return ref, sc, ids, cam, frames


@pytest.fixture(scope="module")
def room():
    cam = synth.Camera()
    frames = []
    for k in range(4):
        depth, rgba, _, pose = synth.room_frame(k, cam, with_quality=False, wobble=0.1)
        frames.append((depth, rgba, pose))
    ref, sc, ids = _oracle_volume(frames, cam)
    return ref, sc, ids, cam, frames


def _probe_points(ids, rng, res=RES5):
    """points whose rasterized coordinates are integral (corners repeat), on chunk faces, random near chunks, and next to
    the chunk set (some corners absent)"""
    pick = ids[rng.choice(len(ids), min(len(ids), 60), replace=False)].astype(np.float64)
    r, e = float(res), 8 * float(res)
    half = r / 2
    out = [pick * e + half, (pick + 1) * e + half, pick * e + half + r * rng.integers(0, 8, pick.shape),
           pick * e + half + r * np.array([3.0, 0.5, 7.0]), (pick + [0.5, 0.5, 0]) * e, (pick - [0.3, 0.1, 0.2]) * e,
           (pick + rng.uniform(0, 1, pick.shape)) * e, (pick + [1.0, 1.0, 1.0]) * e + r * 0.25]
    return np.concatenate(out).astype(np.float32)


@pytest.mark.parametrize("scene", ["wall", "room"])
def test_restated_distance_matches_the_scalar_transcription(scene, wall, room):
    ref, sc, ids = (wall if scene == "wall" else room)[:3]
    rng = np.random.default_rng(21)
    pts = np.concatenate([_probe_points(ids, rng), np.array([[np.nan, 0, 1], [1e30, 0, 0], [-1e30, 1, 1],
                                                               [0, np.inf, 0], [-0.3, -0.2, -0.1]], np.float32)])
    d, tw = refine_ref.surface_dist(ref, pts)
    n_pos = 0
    for k, p in enumerate(pts):
        ed, etw = sc.GetDistanceFromSurface(p)
        assert F(ed).tobytes() == d[k].tobytes() and F(etw).tobytes() == tw[k].tobytes(), (k, p, ed, d[k], etw, tw[k])
        n_pos += bool(etw > 0)
    assert n_pos > 100  # the points reach observed voxels, not only absent chunks


@pytest.mark.parametrize("scene", ["wall", "room"])
def test_restated_refinement_matches_the_scalar_transcription(scene, wall, room):
    ref, sc, ids, cam, frames = wall if scene == "wall" else room
    depth0, _, pose = frames[0]
    rng = np.random.default_rng(22)
    depth = depth0 + rng.uniform(-0.003, 0.003, depth0.shape).astype(np.float32) * (depth0 > 0)
    flat = depth.reshape(-1).copy()
    flat[:: 97] = 0.0
    flat[5:: 211] = np.nan
    flat[7:: 307] = 0.04
    flat[9:: 401] = 3.5
    # a few hundred pixels: random, image borders, the principal point row / column (integral ray coordinates)
    W, H = cam.width, cam.height
    pix = [(int(i), int(j)) for i, j in zip(rng.integers(0, H, 300), rng.integers(0, W, 300))]
    pix += [(0, 0), (H - 1, W - 1), (int(cam.cy), int(cam.cx)), (int(cam.cy), 5), (7, int(cam.cx))]
    pix += [(i, j) for i in range(0, H, 60) for j in range(0, W, 80)]
    pix += [(p // W, p % W) for p in (5, 7, 9, 97, 211 + 5, 307 + 7)]
    sent = np.full(W * H, F(-7.0))
    exp_d, exp_w = refine_ref.refine_frame(ref, flat.reshape(H, W), pose, cam, weight=sent.reshape(H, W))
    got_d, got_w = flat.copy(), sent.copy()
    accepted = 0
    for i, j in pix:
        sc.RefinePixel(got_d, got_w, i, j, pose, cam)
        o = i * W + j
        assert got_d[o].tobytes() == exp_d.reshape(-1)[o].tobytes(), (i, j, got_d[o], exp_d.reshape(-1)[o])
        assert got_w[o].tobytes() == exp_w.reshape(-1)[o].tobytes(), (i, j, got_w[o], exp_w.reshape(-1)[o])
        accepted += bool(got_w[o] > 0)
    assert accepted > 100
    # the NaN pixel passes through: NaN depth, weight 0; the skipped ones keep both values
    assert np.isnan(exp_d.reshape(-1)[5]) and exp_w.reshape(-1)[5] == 0
    for o in (0, 7, 9):
        assert exp_d.reshape(-1)[o] == flat[o] and exp_w.reshape(-1)[o] == F(-7.0)


# |refined - true depth| of accepted pixels after +-3 mm of uniform noise on the integrated wall depth (every valid pixel
# is accepted), measured on the restatement: median 1.2e-7 m, 99th percentile 3.4e-4 m, RMS 1.2e-4 m against the noise's
# 1.7e-3 m.  A tail of 0.1 % of the pixels ends 1.5 .. 4.3 mm off (max 4.29e-3 m): the walk stops where the weighted
# corners' SDF reads 0 within the reference's 5e-3 acceptance, not on the plane.
REFINE_Q99, REFINE_MAX = 5e-4, 5e-3


def test_refinement_pulls_a_noisy_wall_onto_the_surface(wall):
    ref, _, _, cam, frames = wall
    depth0, _, pose = frames[0]
    true_z = F(WALL_Z - float(pose[2, 3]))
    rng = np.random.default_rng(23)
    valid = depth0 > 0
    noise = rng.uniform(-0.003, 0.003, depth0.shape).astype(np.float32)
    noisy = np.where(valid, depth0 + noise, depth0).astype(np.float32)
    d, w = refine_ref.refine_frame(ref, noisy, pose, cam)
    acc = (w > 0) & valid
    assert acc[valid].mean() > 0.98, acc[valid].mean()
    err = np.abs(d[acc] - true_z)
    before = np.abs(noisy[acc] - true_z)
    assert np.quantile(err, 0.99) < REFINE_Q99 and np.median(err) < 1e-5, np.quantile(err, [0.5, 0.99])
    assert err.max() < REFINE_MAX, err.max()
    assert np.sqrt((err.astype(np.float64) ** 2).mean()) < 0.1 * np.sqrt((before.astype(np.float64) ** 2).mean())
    assert np.all(d[~acc & valid] == 0) and np.all(w[~valid] == 0) and np.all(d[~valid] == 0)
