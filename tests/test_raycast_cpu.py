"""CPU checks of the raycast feature.

Only the register / scratch budget of k_query and k_raycast compiled for gfx950 exercises the library itself.  The
others check the numpy restatement (tests/raycast_ref.py) against the CPU oracle's volume: GetSDF / GetWeight /
GetSDFAndGradient by hand on chosen voxels, the trilinear SDF against the analytic wall, and the restated march; and, on
the hand-built volumes of tests/ray_inputs.py, that every case reaches the branch it is named for (the restatement's
trace), that depth, normal, vertex and colour of the planar ones agree with their closed form, and that every rule of
the march and of the normal is told from its neighbour by some case.  They are checks of the reference the GPU tests
(tests/test_gpu_raycast.py, tests/test_gpu_ray_edges.py) hold the kernels to bit for bit, not of the kernels, and so they
pass without the library's raycast code."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import api as O
from texturefusion_amd import synth
from tests import ray_inputs as RI
from tests import raycast_ref as RR
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


# ---- the hand-built volumes of tests/ray_inputs.py ----------------------------------------------------------------------
# cases in which every pixel of the image takes the named branch
EVERY = ("front", "front_zero", "behind", "inside", "gap_hold", "gap_fail", "gap_equal", "dy_zero", "far_short", "far_beyond",
         "near_beyond", "tile_9x1", "tile_1x1", "tile_8x8")


@pytest.fixture(scope="module")
def hand_maps():
    return {name: RI.ref_maps(c) for name, c in RI.cases().items()}


def test_the_names_and_the_cases_agree():
    assert sorted(RI.NAMES) == sorted(RI.cases()) and set(RI.KILLS) == set(RR._FLIPS) and set(RI.KILLS.values()) <= set(RI.NAMES)
    for name, c in RI.cases().items():
        cam = c["cam"]
        assert 1 <= cam.width <= 24 and 1 <= cam.height <= 17 and len(c["ids"]) <= 64 and c["why"], name
        assert c["res"] in (RI.HAND_RES, RES5)
    assert {float(c["res"]) for c in RI.cases().values()} == {float(RI.HAND_RES), float(RES5)}
    assert {(c["cam"].width, c["cam"].height) for c in RI.cases().values()} >= {(13, 9), (9, 1), (1, 1), (8, 8)}


@pytest.mark.parametrize("name", RI.NAMES)
def test_every_case_reaches_its_branch(name, hand_maps):
    c, o = RI.cases()[name], hand_maps[name]
    tr = o["trace"]
    reach = c["reach"](o)
    px = c["cam"].width * c["cam"].height
    print("%s: %d of %d pixels reach it; ends %s, jumps %d..%d, invalid %d..%d, gap rejections %d, samples %d..%d -- %s" % (
        name, reach.sum(), px, np.bincount(tr["end"].ravel(), minlength=6)[1:].tolist(), tr["jumps"].min(), tr["jumps"].max(),
        tr["invalid"].min(), tr["invalid"].max(), tr["gap"].sum(), tr["steps"].min(), tr["steps"].max(), c["why"]))
    assert reach.sum() >= min(4, px), c["why"]
    if name in EVERY:
        assert reach.all(), c["why"]
    hit = tr["end"] == RR.END_HIT
    assert np.array_equal(hit, o["depth"] > 0) and np.array_equal(hit, o["rgba"][..., 3] == 255)
    assert not o["vertex"][:, ~hit].any() and not o["normal"][:, ~hit].any() and not o["rgba"][~hit].any()
    assert np.array_equal(o["depth"], RI.ref_volume(c).raycast_depth(c["pose"], c["cam"].fx, c["cam"].fy, c["cam"].cx, c["cam"].cy,
                                                                     c["cam"].width, c["cam"].height, c["near"], c["far"], c["max_steps"]))


def test_the_cases_cover_the_normal_and_the_chunk_borders(hand_maps):
    m = np.concatenate([o["trace"]["m"].reshape(3, -1) for o in hand_maps.values()], 1)
    for a in range(3):
        for v in (1, 2, 3):
            assert (m[a] == v).sum() >= 4, "axis %d never shows m == %d" % (a, v)
    o = hand_maps["gap_hold"]  # (the crossing lies in the weight-0 cell: no x or y tap, the z difference alone is no normal)
    assert (o["trace"]["m"][:2] == 0).all() and (o["trace"]["m"][2] == 2).all() and not o["normal"].any() and (o["depth"] > 0).all()
    n = np.concatenate([RI.corner_chunks(hand_maps[k], RI.cases()[k]["res"]).ravel() for k in ("neg_x", "neg_y", "neg_z")])
    assert (n == 2).sum() >= 4 and (n == 4).sum() >= 4 and (n == 8).sum() >= 4
    for a, k in enumerate(("neg_x", "neg_y", "neg_z")):  # negative chunk and voxel coordinates: cell -1 on the marched axis, both signs on the others
        cell = np.floor(hand_maps[k]["vertex"].astype(np.float64) / float(RI.cases()[k]["res"]) - 0.5).reshape(3, -1)
        assert (cell[a] == -1).all() and all((cell[b] < 0).any() and (cell[b] >= 0).any() for b in range(3) if b != a)


def test_the_step_cap_splits_one_image(hand_maps):
    c, o = RI.cases()["step_cap"], hand_maps["step_cap"]
    more = RI.ref_maps(dict(c, max_steps=c["max_steps"] + 1))
    last = (o["trace"]["end"] == RR.END_HIT) & (o["trace"]["steps"] == c["max_steps"])
    short = (o["trace"]["end"] == RR.END_STEPS) & (more["trace"]["end"] == RR.END_HIT)
    assert last.sum() >= 4 and short.sum() >= 4, (last.sum(), short.sum())


def _rays64(c):
    cam, P = c["cam"], c["pose"].astype(np.float64)
    u = (np.arange(cam.width) - (int(cam.cx) + 0.5)) / int(cam.fx)
    v = (np.arange(cam.height) - (int(cam.cy) + 0.5)) / int(cam.fy)
    uu, vv = np.meshgrid(u, v)
    return np.einsum("rc,hwc->rhw", P[:, :3], np.stack([uu, vv, np.ones_like(uu)], -1)), P[:, 3]


# Largest deviations of the restatement from the closed form over the planar cases, as measured by this test (printed):
# depth 5.76e-8 m at 10 mm voxels (step_cap, the tilted view) and 1.71e-8 m at 5 mm (normal_box); a normal component
# 3.05e-6 (normal_box).  Asserted at four times that; far below res / 100 and 1e-4, so every case is well conditioned.
DEPTH_BOUND = {float(RI.HAND_RES): 2.31e-7, float(RES5): 6.84e-8}
NORMAL_BOUND = 1.22e-5


def test_the_restatement_against_the_closed_form(hand_maps):
    worst_d, worst_n, seen = {}, 0.0, 0
    for name, c in RI.cases().items():
        if c["plane"] is None:
            continue
        o = hand_maps[name]
        hit = o["depth"] > 0
        if not hit.any():
            continue
        n, p0 = (np.asarray(a, np.float64) for a in c["plane"])
        d, org = _rays64(c)
        t = ((p0 - org) @ n) / np.einsum("r,rhw->hw", n, d)
        ed = np.abs(o["depth"].astype(np.float64) - t)[hit].max()
        worst_d[float(c["res"])] = max(worst_d.get(float(c["res"]), 0.0), ed)
        ok = hit & (o["trace"]["m"] > 0).all(0)
        en = np.abs(o["normal"].astype(np.float64) - n[:, None, None])[:, ok].max() if ok.any() else 0.0
        worst_n = max(worst_n, en)
        seen += int(((o["trace"]["m"] == 1) | (o["trace"]["m"] == 2)).any(0)[ok].sum())
        print("%s: depth within %.2e m, normal within %.2e" % (name, ed, en))
        assert ed <= DEPTH_BOUND[float(c["res"])] and en <= NORMAL_BOUND, name
    print("largest: depth %s, normal %.2e; %d pixels with a one-sided difference" % (worst_d, worst_n, seen))
    assert seen >= 100  # the one-sided differences are held to the plane's normal too: the factor 2 and its sign
    assert all(b < r / 100 for r, b in DEPTH_BOUND.items()) and NORMAL_BOUND < 1e-4


@pytest.mark.parametrize("name", RI.NAMES)
def test_vertex_is_the_ray_at_the_depth_bit_for_bit(name, hand_maps):
    c, o = RI.cases()[name], hand_maps[name]
    cam, P = c["cam"], c["pose"]
    hit = o["depth"] > 0
    yy, xx = np.mgrid[0:cam.height, 0:cam.width]
    dcx = (xx.astype(np.float32) - (F(int(cam.cx)) + F(0.5))) / F(int(cam.fx))
    dcy = (yy.astype(np.float32) - (F(int(cam.cy)) + F(0.5))) / F(int(cam.fy))
    for r in range(3):
        d = (P[r, 0] * dcx + P[r, 1] * dcy) + P[r, 2]
        exp = np.where(hit, P[r, 3] + o["depth"] * d, F(0))
        assert np.array_equal(o["vertex"][r].view(np.uint32), exp.astype(np.float32).view(np.uint32)), (name, r)


def _colour64(c, points):
    """trilinear colour in float64 at world points -> (rgb before rounding [n, 3], valid [n], safe [n]: no coordinate
    within 1e-6 voxels of a cell border, where f32 and f64 may pick different cells)"""
    ref = RI.ref_volume(c)
    g = points.astype(np.float64) * float(F(1) / c["res"]) - 0.5
    i = np.floor(g).astype(np.int64)
    f = g - i
    safe = (np.minimum(f, 1 - f) > 1e-6).all(1)
    out, ok = np.zeros((len(points), 3)), np.ones(len(points), bool)
    for k in range(8):
        off = np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1])
        v = i + off
        sl = ref.slot(v[:, 0] >> 3, v[:, 1] >> 3, v[:, 2] >> 3)
        q = ref.col[np.maximum(sl, 0), ((v[:, 2] & 7) * 8 + (v[:, 1] & 7)) * 8 + (v[:, 0] & 7)].astype(np.float64)
        ok &= (sl >= 0) & (q[:, 3] > 0)
        wgt = np.prod(np.where(off == 1, f, 1 - f), 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            out += np.where(ok[:, None], wgt[:, None] * q[:, :3] / q[:, 3:4], 0.0)
    return out, ok, safe


@pytest.mark.parametrize("name", ["colour", "gap_hold", "gap_equal"])
def test_colour_against_means_in_float64(name, hand_maps):
    c, o = RI.cases()[name], hand_maps[name]
    hit = o["depth"] > 0
    x, ok, safe = _colour64(c, o["vertex"][:, hit].T)
    got = o["rgba"][hit]
    assert (got[:, 3] == 255).all() and safe.sum() >= 0.9 * len(safe)
    assert np.array_equal(got[~ok, :3], np.zeros(((~ok).sum(), 3), np.uint8))
    off_tie = np.abs(x + 0.5 - np.round(x + 0.5)) > 1e-3  # (f32 and f64 may round a mean within 1e-3 of a tie apart)
    exp = np.minimum(255, np.floor(x + 0.5)).astype(np.uint8)
    cmp = (ok & safe)[:, None] & off_tie
    assert np.array_equal(got[:, :3][cmp], exp[cmp]) and cmp[:, 1].sum() >= 4 and cmp[:, 2].sum() >= 4
    if name == "colour":
        assert (~ok).sum() >= 4 and ok.sum() >= 4
        assert (got[ok, 0] == 4).all(), "a mean of 3.5 at every corner is 3.5 exactly: rounds up to 4"
        assert (got[ok, 2] == 255).all() and len(np.unique(got[ok, 1])) >= 4 and (x[ok, 1] % 1 != 0).any()
    else:  # the hit's cell holds a corner with weight 0 and count > 0: no SDF there, colour all the same
        s, oks, _, okc = RI.ref_volume(c).trilinear(np.ascontiguousarray(o["vertex"][:, hit].T))
        assert not oks.any() and okc.all() and ok.all()


@pytest.mark.parametrize("flip", RR._FLIPS)
def test_each_rule_is_told_apart(flip, hand_maps):
    name = RI.KILLS[flip]
    a, b = hand_maps[name], RI.ref_maps(RI.cases()[name], flip)
    changed = {k: int((a[k] != b[k]).sum()) for k in ("depth", "vertex", "normal", "rgba")}
    print("%s on %s: %s" % (flip, name, changed))
    assert any(changed.values()), "%s is not told from the kernel's rule by %s" % (flip, name)
