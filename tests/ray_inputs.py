"""Hand-built volumes for the raycaster (k_raycast) at its decision edges, shared by tests/test_raycast_cpu.py (which proves
on the restatement's trace that every case reaches the branch it names, holds the planar ones to their closed form and shows
that every rule of the march is told apart) and tests/test_gpu_ray_edges.py (which holds the kernel to the restatement bit
for bit on them): the GPU tests cannot drift to inputs that no longer reach their edge.

numpy + texturefusion_amd.synth + tests/raycast_ref.py only: no oracle, no GPU.

A case is a dict: ids / sdf / weight / colour as set_chunk takes them, res, cam (a synth.Camera, 1 x 1 .. 24 x 17), pose,
near, far, max_steps, a one-line why, `reach` (maps of RefVolume.raycast_maps -> the mask of the pixels that take the named
branch) and, where the surface is a plane, `plane` = (unit normal the raycaster must report, a world point on it).

Coordinates: g = p / res - 0.5 are voxel-centre coordinates (voxel V has its centre at g = V); the SDFs are linear in g,
sdf = unit * (c - n . g), so the trilinear sampler reproduces them up to rounding, one-sided differences included.  `unit`
is res (a metric SDF: the step rule takes 0.75 sdf) or 2^-9 (dyadic values, and every step is one voxel).

  front            the plane g_z = 27.5 of one chunk layer (both sides observed), 13 x 9, the camera five absent chunks away
  front_zero       the same, dyadic, from a camera on the voxel grid: one sample lands on s == 0, the hit is that sample's t
  behind           a back face (- -> +) and, three chunks on, a front face that must not be hit
  inside           the back face from a start inside its negative side: nothing to pair the first sample with
  gap_hold         + stretch, weight-0 voxels, - stretch: the pair is 3 voxels apart, the crossing lies in the weight-0 cell
                   (its colour is valid there: weight 0, count > 0), the z normal is one-sided
  gap_fail         the same 5 voxels apart: no hit;  gap_equal  exactly 4 voxels apart in f32: a hit
  neg_x, neg_y,    the plane p_a = 0 seen along -a from p_a > 0: chunks -1 | 0 on every axis, the central pixels' eight corners
  neg_z            lie in eight chunks, the outer ones in four and two
  dy_zero          front under a pose whose middle row is (0, 0, 0, ty): dy == 0, the INFINITY arm of the chunk DDA
  far_short,       front with far = the float below the t of the sample that closes the crossing, and that t itself
  far_beyond
  step_cap         front from a tilted pose, max_steps = K: pixels that hit on sample K and pixels that would on K + 1
  near_beyond      front with near behind the surface and its band
  normal_box       a tilted plane, observed in a box of 4 x 4 voxel columns: m = 2, 3, 1 on x and on y
  normal_thin_back,  the tilted plane observed in a band that ends 1.9 voxels behind (in front of) the surface: plus (minus)
  normal_thin_front  taps fall out of it, m = 1 (2) on every axis next to m = 3
  normal_m0        the fronto-parallel plane observed in two voxel columns: no x tap, depth > 0 and normal 0
  colour           front with counts of 2: R 3.5 everywhere (rounds at .5), G a non-integral ramp, B 300 (the cap), and no
                   colour from voxel column 1 on (count 0): 0, 0, 0, 255 there
  tile_9x1, tile_1x1, tile_8x8   front through cameras that fill their tiles partly, or exactly
"""
import functools

import numpy as np

from tests import raycast_ref as RR
from tests.align_inputs import HAND_RES
from tests.util import RES5
from texturefusion_amd import synth

F = np.float32
DYADIC = 2.0 ** -9
N122 = np.array([1.0, 2.0, 2.0]) / 3.0
MAX_CHUNKS = 1 << 10


def _cam(w, h, f=200.0):
    return synth.Camera(w, h, f, f, float(w // 2), float(h // 2), 0.01, 2.0)


def _pose(R, q, res):
    """rotation R, origin at q voxel widths (q integral: on the voxel grid)"""
    p = np.zeros((3, 4), np.float32)
    p[:, :3] = np.asarray(R, np.float32)
    p[:, 3] = (np.asarray(q, np.float64) * float(res)).astype(np.float32)
    return p


EYE = np.eye(3)
LOOK = {0: [[0, 0, -1], [0, 1, 0], [1, 0, 0]], 1: [[1, 0, 0], [0, 0, -1], [0, 1, 0]], 2: [[1, 0, 0], [0, -1, 0], [0, 0, -1]]}  # along -axis


def _fill(chunks, sdf_fn, w_fn=None, col_fn=None):
    """chunks of ids; the functions take the voxels' global indices V [512, 3] (voxel = x + 8 y + 64 z)"""
    ids = np.asarray(sorted(set(tuple(c) for c in chunks)), np.int32).reshape(-1, 3)
    i = np.arange(8)
    z, y, x = np.meshgrid(i, i, i, indexing="ij")
    loc = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
    sdf, w, col = [], [], []
    for c in ids:
        V = 8 * c.astype(np.int64) + loc
        sdf.append(np.asarray(sdf_fn(V), np.float64).astype(np.float32))
        w.append(np.ones(512, np.float32) if w_fn is None else np.asarray(w_fn(V), np.float32))
        col.append(np.zeros((512, 4), np.uint16) if col_fn is None else np.asarray(col_fn(V), np.uint16))
    return ids, np.stack(sdf), np.stack(w), np.stack(col).reshape(len(ids), 2048)


def _box(xs, ys, zs):
    return [(x, y, z) for x in xs for y in ys for z in zs]


def _linear(unit, n, c):
    n = np.asarray(n, np.float64)
    return lambda V: unit * (c - V @ n)


def _case(vol, res, cam, pose, why, reach, near=0.01, far=2.0, max_steps=256, plane=None):
    ids, sdf, w, col = vol
    assert len(ids) <= 64 and cam.width <= 24 and cam.height <= 17
    return dict(ids=ids, sdf=sdf, weight=w, colour=col, res=F(res), cam=cam, pose=np.asarray(pose, np.float32), near=near,
                far=far, max_steps=max_steps, why=why, reach=reach, plane=plane)


def ref_volume(c):
    return RR.RefVolume(c["ids"], c["sdf"], c["weight"], c["colour"], c["res"])


def ref_maps(c, flip=None):
    """RefVolume.raycast_maps of a case"""
    cam = c["cam"]
    return ref_volume(c).raycast_maps(c["pose"], cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, c["near"], c["far"],
                                      c["max_steps"], _flip=flip)


def _world(g, res):
    return (np.asarray(g, np.float64) + 0.5) * float(res)


# ---- the plain slab ---------------------------------------------------------------------------------------------------
FRONT_CHUNKS = _box((-1, 0), (-1, 0), (3,))
FRONT_POSE = _pose(EYE, (0, 0, -8), HAND_RES)
FRONT_PLANE = ((0.0, 0.0, -1.0), _world((0, 0, 27.5), HAND_RES))


def _front_volume(col_fn=None):
    return _fill(FRONT_CHUNKS, _linear(float(HAND_RES), (0, 0, 1), 27.5), None, col_fn)


def _front(cam=None, **kw):
    why = kw.pop("why", "a front-facing plane behind absent chunks: every pixel hits, each after >= 4 chunk jumps")
    reach = kw.pop("reach", lambda o: (o["trace"]["end"] == RR.END_HIT) & (o["trace"]["jumps"] >= 4))
    return _case(_front_volume(), HAND_RES, cam or _cam(13, 9), kw.pop("pose", FRONT_POSE), why, reach, plane=FRONT_PLANE, **kw)


def _uniform_t_end(c):
    t = ref_maps(c)["trace"]["t_end"]
    assert (t == t.flat[0]).all(), "the rays of a fronto-parallel view march in step"
    return t.flat[0]


def _front_zero():
    """searches the grid origins and starts for one whose third sample has g_z == 27.5 exactly: s == 0 there"""
    vol = _fill(FRONT_CHUNKS, _linear(DYADIC, (0, 0, 1), 27.5))
    reach = lambda o: (o["trace"]["end"] == RR.END_HIT) & (o["depth"] == o["trace"]["t_end"])
    for q in (26, 25, 24, 0):
        for near in (0.0, 0.01, 0.26, 0.25, 0.27):
            c = _case(vol, HAND_RES, _cam(13, 9), _pose(EYE, (0, 0, q), HAND_RES), "a sample exactly on s == 0: the refined hit is "
                      "the sample's own t", reach, near=near, plane=FRONT_PLANE)
            if q * 0.01 + near < 0.275 and reach(ref_maps(c)).all():
                return c
    raise AssertionError("no start puts a sample on s == 0")


def _two_faces():
    back, front = _linear(float(HAND_RES), (0, 0, -1), -27.5), _linear(float(HAND_RES), (0, 0, 1), 51.5)
    return _fill(FRONT_CHUNKS + _box((-1, 0), (-1, 0), (6,)), lambda V: np.where(V[:, 2] < 40, back(V), front(V)))


# ---- the gap rule: dyadic values, every step one voxel, samples at g_z = 24.25 + k ---------------------------------------
GAP_POSE = _pose(EYE, (0, 0, 24), HAND_RES)


def _gap_colour(V):
    return np.stack([V[:, 0] * 0 + 14, 40 + 6 * (V[:, 0] & 7), 90 + 10 * (V[:, 1] & 7), V[:, 0] * 0 + 2], 1)


def _gap(dead, why, reach, near=0.0075):
    vol = _fill(FRONT_CHUNKS, _linear(DYADIC, (0, 0, 1), 26.5), lambda V: (~np.isin(V[:, 2], dead)).astype(np.float32), _gap_colour)
    return _case(vol, HAND_RES, _cam(13, 9), GAP_POSE, why, reach, near=near, plane=((0.0, 0.0, -1.0), _world((0, 0, 26.5), HAND_RES)))


def _gap_equal():
    """searches the starts for one at which the four voxel steps from the + sample add up to 4 res exactly in f32"""
    reach = lambda o: (o["trace"]["end"] == RR.END_HIT) & (o["trace"]["invalid"] == 3) & (o["trace"]["gap"] == 0)
    res = F(HAND_RES)
    for k in range(1, 16):
        near = F(k / 16.0) * res
        t = near
        for _ in range(4):
            t = F(t + res)
        if F(t - near) == F(4) * res:
            c = _gap((26, 27), "the pair exactly kRayGap voxels apart (t - pt == gap in f32): still a hit", reach, near=float(near))
            if reach(ref_maps(c)).all():
                return c
    raise AssertionError("no start makes t - pt == gap")


# ---- views along the negative axes: the plane p_a = 0 ---------------------------------------------------------------------
def _neg(a, res, q):
    n = np.zeros(3)
    n[a] = -1.0
    vol = _fill(_box((-1, 0), (-1, 0), (-1, 0)), _linear(float(res), n, 0.5))  # sdf = res (g_a + 0.5) = p_a
    o = np.zeros(3)
    o[a] = q
    normal = tuple(-n)

    def reach(out):  # the eight corners of the hit in eight chunks: cell -1 on every axis
        g = out["vertex"].astype(np.float64) / float(res) - 0.5
        return (out["trace"]["end"] == RR.END_HIT) & (np.floor(g) == -1).all(0) & (out["trace"]["jumps"] >= 1)

    return _case(vol, res, _cam(15, 15), _pose(LOOK[a], o, res), "seen along -%s from chunk 2 into chunks -1 | 0: negative chunk and "
                 "voxel coordinates, hits whose corners lie in 8 chunks" % "xyz"[a], reach, plane=(normal, np.zeros(3)))


def corner_chunks(out, res):
    """per pixel, in how many chunks the eight corners of the hit's cell lie (0 on a miss)"""
    g = np.floor(out["vertex"].astype(np.float64) / float(res) - 0.5).astype(np.int64)
    n = np.prod(1 + ((g & 7) == 7), 0)
    return np.where(out["depth"] > 0, n, 0)


# ---- limits ---------------------------------------------------------------------------------------------------------------
STEP_POSE = synth.pose_euler(0.2, 0.15, 0.1, (-0.075, 0.05, -0.08))


def _step_cap():
    cam = _cam(24, 17, 100.0)
    full = _front(cam, pose=STEP_POSE, max_steps=256)
    o = ref_maps(full)
    assert (o["trace"]["end"] == RR.END_HIT).all(), "the tilted view must see the plane in every pixel"
    steps = o["trace"]["steps"]
    for k in range(int(steps.min()), int(steps.max())):
        if (steps == k).sum() >= 4 and (steps == k + 1).sum() >= 4:
            return _front(cam, pose=STEP_POSE, max_steps=k, why="max_steps = %d: pixels that hit on their last allowed sample, "
                          "pixels that run out one sample short" % k,
                          reach=lambda m, k=k: (m["trace"]["steps"] == k) & (m["trace"]["end"] == RR.END_HIT))
    raise AssertionError("no step count splits the image")


# ---- normals ----------------------------------------------------------------------------------------------------------------
def _m_counts(out, a):
    return [int((out["trace"]["m"][a] == v).sum()) for v in (0, 1, 2, 3)]


def _normal_box():
    inside = lambda V: ((V[:, 0] >= 2) & (V[:, 0] <= 5) & (V[:, 1] >= 2) & (V[:, 1] <= 5)).astype(np.float32)
    vol = _fill([(0, 0, 5)], _linear(float(RES5), N122, 32.5), inside)
    reach = lambda o: ((o["trace"]["m"][0] == 1) | (o["trace"]["m"][0] == 2)) & (o["trace"]["m"][2] == 3)
    return _case(vol, RES5, _cam(24, 17), _pose(EYE, (4, 4, 0), RES5), "a tilted plane observed in 4 x 4 voxel columns: one-sided x and y "
                 "differences (m = 1, 2) beside central ones", reach, plane=(tuple(-N122), _world((3.5, 3.5, 43.5), RES5)))


def _normal_thin(lo, hi, m, why):
    f = _linear(float(HAND_RES), N122, 64.0 / 3.0)
    band = lambda V: ((f(V) >= lo * float(HAND_RES)) & (f(V) <= hi * float(HAND_RES))).astype(np.float32)
    vol = _fill(_box((-1, 0), (-1, 0), (3, 4)), f, band)
    reach = lambda o: (o["trace"]["m"] == m).any(0) & (o["trace"]["m"] > 0).all(0)
    return _case(vol, HAND_RES, _cam(24, 17), _pose(EYE, (0, 0, 0), HAND_RES), why, reach, plane=(tuple(-N122), _world((0, 0, 32), HAND_RES)))


def _normal_m0():
    two = lambda V: ((V[:, 0] == 3) | (V[:, 0] == 4)).astype(np.float32)
    vol = _fill([(0, 0, 5)], _linear(float(RES5), (0, 0, 1), 43.5), two)
    reach = lambda o: (o["depth"] > 0) & (o["trace"]["m"][0] == 0) & (o["normal"] == 0).all(0)
    return _case(vol, RES5, _cam(24, 17), _pose(EYE, (4, 4, 0), RES5), "observed in two voxel columns: no x tap is valid, depth > 0 and "
                 "normal 0", reach)


# ---- colour -----------------------------------------------------------------------------------------------------------------
def _colour_fn(V):
    n = np.where(V[:, 0] >= 1, 0, 2)
    return np.stack([V[:, 0] * 0 + 7, 2 * (40 + 3 * (V[:, 0] & 7) + 5 * (V[:, 1] & 7)) + 1, V[:, 0] * 0 + 600, n], 1)


def _colour():
    reach = lambda o: (o["rgba"][..., 3] == 255) & (o["rgba"][..., :3] == 0).all(-1)  # hits without colour
    c = _front(why="counts of 2: R 3.5 (rounds at .5), G a non-integral ramp, B 300 (capped at 255); count 0 from voxel column 1 on: "
               "0, 0, 0 with alpha 255", reach=reach)
    c["ids"], c["sdf"], c["weight"], c["colour"] = _front_volume(_colour_fn)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case"""
    far_t = float(_uniform_t_end(_front()))
    dy0 = FRONT_POSE.copy()
    dy0[1] = (0.0, 0.0, 0.0, 0.004)
    dy0[0, 3] = 0.003
    miss_far = lambda o: (o["trace"]["end"] == RR.END_FAR) & (o["depth"] == 0)
    c = {
        "front": _front(),
        "front_zero": _front_zero(),
        "behind": _case(_two_faces(), HAND_RES, _cam(13, 9), FRONT_POSE, "a back face, then a front face: the - -> + break ends every ray, "
                        "the second face is not hit", lambda o: (o["trace"]["end"] == RR.END_BACK) & (o["depth"] == 0)),
        "inside": _case(_two_faces(), HAND_RES, _cam(13, 9), GAP_POSE, "the first valid sample is <= 0 at near, nothing to pair it with: a "
                        "back break", lambda o: (o["trace"]["end"] == RR.END_BACK) & (o["trace"]["jumps"] == 0), near=0.0075),
        "gap_hold": _gap((26,), "+ sample, two invalid samples, - sample 3 voxels on: pt / ps survive, a hit in the weight-0 cell",
                         lambda o: (o["trace"]["end"] == RR.END_HIT) & (o["trace"]["invalid"] == 2) & (o["trace"]["gap"] == 0)),
        "gap_fail": _gap((26, 27, 28), "+ sample, four invalid samples, - sample 5 voxels on: the pairing is refused, no hit",
                         lambda o: (o["trace"]["end"] == RR.END_FAR) & (o["trace"]["gap"] == 1) & (o["depth"] == 0)),
        "gap_equal": _gap_equal(),
        "neg_x": _neg(0, RES5, 20),
        "neg_y": _neg(1, HAND_RES, 20),
        "neg_z": _neg(2, RES5, 20),
        "dy_zero": _front(pose=dy0, why="the pose's middle row is (0, 0, 0, ty): dy == 0 for every ray, the chunk jumps take the "
                          "INFINITY arm"),
        "far_short": _front(far=float(np.nextafter(F(far_t), F(0))), why="far one float short of the sample that closes the crossing: "
                            "no hit", reach=miss_far),
        "far_beyond": _front(far=far_t, why="far == the t of the sample that closes the crossing: t <= far admits it",
                             reach=lambda o: (o["trace"]["end"] == RR.END_HIT) & (o["trace"]["t_end"] == F(far_t))),
        "step_cap": _step_cap(),
        "near_beyond": _front(near=0.5, why="near behind the surface and its band: nothing but absent chunks", reach=miss_far),
        "normal_box": _normal_box(),
        "normal_thin_back": _normal_thin(-1.9, 4.0, 1, "the band ends 1.9 voxels behind the surface: plus taps fall out, m = 1"),
        "normal_thin_front": _normal_thin(-4.0, 1.9, 2, "the band ends 1.9 voxels in front of the surface: minus taps fall out, m = 2"),
        "normal_m0": _normal_m0(),
        "colour": _colour(),
        "tile_9x1": _front(_cam(9, 1)),
        "tile_1x1": _front(_cam(1, 1)),
        "tile_8x8": _front(_cam(8, 8)),
    }
    return c


NAMES = ("front", "front_zero", "behind", "inside", "gap_hold", "gap_fail", "gap_equal", "neg_x", "neg_y", "neg_z", "dy_zero",
         "far_short", "far_beyond", "step_cap", "near_beyond", "normal_box", "normal_thin_back", "normal_thin_front", "normal_m0",
         "colour", "tile_9x1", "tile_1x1", "tile_8x8")
# the flips of raycast_ref._FLIPS and the case that tells each from the kernel's rule
KILLS = {"gap_lt": "gap_equal", "hit_lt": "front_zero", "far_lt": "far_beyond", "no_back": "behind", "no_eps": "neg_z",
         "one_sided_1": "normal_box", "one_sided_sign": "normal_thin_back", "reset_on_invalid": "gap_hold"}
