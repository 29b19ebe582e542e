"""Hand-built chunks for the voxel update (K-A) at its arithmetic edges, shared by tests/test_ka_cpu.py (which proves, with
tests/ka_ref.py and the oracle alone, that every case hits the edge it names) and tests/test_gpu_ka_edges.py /
tests/test_gpu_ka_math.py (which run them through the device): the GPU tests cannot drift to inputs the census never saw.

numpy + texturefusion_amd.synth + tests/ka_ref.py only: no oracle, no GPU.

Every case is a `Case`: camera, resolution, integrator, one pose and one depth image per frame (one frame, except J),
an RGBA and a quality image, an explicit id list and the preset contents of every listed chunk.  64 x 48 cameras, lists of
1 - 30 chunks.  Where an edge needs an exact float (a depth that makes sd equal a threshold, a weight that makes
w + wD equal 0.5) the builder searches the few floats around the real-number solution for one that gives the equality
in float32 and asserts that it found one: a case that no longer hits its edge fails while it is built.

  A  borders     identity pose, 5 mm voxels, chunks ~0.25 m away (about one pixel per voxel) along the four image
                 borders: voxels project onto X = -1, 0, 1, W-2, W-1, W and Y likewise.  A_top's first row is off the
                 image (nothing may change although later rows are valid), A_bottom stalls in the middle, A_centre is
                 fully valid, A_left has off-image lanes in its early rows only: with colour and quality the sentinel is
                 ASSIGNED mid-chunk and later rows add to it.  A2: the same borders under a quarter turn about the
                 optical axis, where the lanes of a row differ in Y instead of X
  B  ties        res 2^-8, fx = fy = 64, identity rotation, t = (2^-9, 2^-9, 2^-9): slice z = 0 of the chunks at id.z = 8
                 has p.z = 2^-2 exactly and u = 8 id.x + x + 31.5, v likewise -- ties for even and odd integers.
                 B2: the same under a camera with non-integral fx, fy, cx, cy (the reference truncates them)
  C  at / behind the camera   res 2^-8, t = (2^-9, 2^-9, 2^-9), chunks (0,0,0), (0,0,-1), (-1,-1,-1), (-1,-1,0),
                 (0,0,1): voxel 0 of chunk (0,0,0) IS the camera centre (0 / 0), its slice z = 0 has p.z == 0
                 exactly, chunk (0,0,-1) has negative p.z whose mirrored projection lands inside the image.  C1: identity
                 rotation (p.z constant per row); C2: a quarter turn about y (exact 0 / +-1 entries), which puts p.z == 0
                 lanes into rows that have valid lanes; C3: C2 under fy = 400 and t.z = -2^-9, where chunk (0,0,0) has exactly one
                 processed row: lanes 1 .. 7 on the principal point, lane 0 at 0 / 0 -- the only off-image lane of the
                 chunk, so the quality sum shows whether 0 / 0 (x86: integer indefinite) is classified as off the image
  D  the guard   res 2^-8 (band 32 res = 2^-3 exactly), the camera looking down the cube's diagonal, chunk (0, 0, 4) and
                 eight neighbours.  The translation is chosen so that chunk (0, 0, 4) projects around the principal
                 point and its o.z is: the band itself (D_eq, D_neg_eq: `>` fails, the generic division runs), one float
                 above it (D_pos_above, D_neg_above: the fast path) and one float below it (D_pos_below, D_neg_below),
                 for chunks in front of (pos) and behind (neg) the camera; the neighbours lie on both sides of the
                 guard in every one of them.  The smallest |p.z| of a fast-path chunk is about 23 res here: a voxel
                 centre is never further than 8 sqrt(3) res from its chunk's origin, so nothing closer to the camera
                 plane exists inside the guard.  D_x_under ... D_z_over: translations that put |o.x|, |o.y| or |o.z|
                 just under and just over 2^20; nothing updates there, stall, sentinel and flag must still match
  E  thresholds  res 2^-10, tilted pose, near = 2^-12, far = 3 * 2^-6, chunks 0.8 - 6 cm in front of the camera; for
                 named voxels (each with a pixel no other voxel of the list projects to) the depth pixel is set so
                 that d == near, d == far, sd == lower, sd == upper, sd == +-thrCol exactly, and to both float
                 neighbours of each
  F  keep        preset weights around the keep threshold w + nw > 0.5 (integrator weight 2^-7, so that wD ~ 0.27 and
                 the presets are positive): w + wD == 0.5 exactly, the next float above; for flag 0 w == wD (sum 0),
                 w == 0, w just above wD + 0.5, w == -0.0
  G  extreme     preset (s, w) from +-inf, NaN, 3e38 with |s| > 1, subnormal s, subnormal w, subnormal product,
                 negative w.  The only case in which NaNs may be stored
  H  colour      image bytes 255 (alpha 0 / 1 / 255 by pixel), preset channels 65535 (flag 1 wraps) and 0 (flag 0
                 wraps) next to small non-zero neighbours in the same dword, counts 119 / 120 / 121 / 200 / 0x8000 /
                 0xFFFF; holes in the depth image leave single lanes of updated rows without an update
  I  quality     B's geometry off the ties (one pixel per voxel in slice 0) with a quality image of 1e8, 1, -1e8, 1e-3
                 in a period-4 layout: a row's lanes read two full periods, so the row sums and their running total
                 depend on the order lane 0..7, row after row; in the chunks at id.x = -4 the sentinel is assigned in
                 rows 0 .. 7 and rows 8 .. 31 add to it
  J  groups      J1 / J2 / J6: 1, 2 and 6 depth frames with different poses over one list of centre and border chunks
                 (the frames stall at different rows); preset w = 0.3 - wD in one chunk drops to reset after frame 1
                 (flag 1) and is rebuilt by frame 2
"""
import dataclasses
import functools

import numpy as np

from tests import ka_ref as KR
from texturefusion_amd import synth

F = np.float32
W, H = 64, 48
CAM = synth.Camera(W, H, 52.5, 52.5, 31.5, 23.5, 0.01, 5.0)       # (the reference truncates: 52, 52, 31, 23)
CAM_POW2 = synth.Camera(W, H, 64.0, 64.0, 31.0, 23.0, 0.01, 5.0)
CAM_FRAC = synth.Camera(W, H, 52.75, 51.25, 31.9, 23.1, 0.01, 5.0)
CAM_TALL = synth.Camera(W, H, 52.5, 400.5, 31.5, 23.5, 0.01, 5.0)
CAM_NEAR = synth.Camera(W, H, 52.5, 52.5, 31.5, 23.5, float(2.0 ** -12), float(3 * 2.0 ** -6))
RES5 = F(0.005)
RES8 = F(2.0 ** -8)
RES10 = F(2.0 ** -10)
IG = (F(0.0019), F(0.00152), F(0.001504), F(6.0), F(1.0))          # MobileFusion::initChiselMap
IG_LIGHT = IG[:4] + (F(2.0 ** -7),)


@dataclasses.dataclass
class Case:
    name: str
    cam: synth.Camera
    res: np.float32
    ig: tuple
    poses: list
    depths: list
    rgba: np.ndarray
    quality: np.ndarray
    ids: np.ndarray
    preset: dict          # (x, y, z) -> (sdf f32[512], weight f32[512], colour u16[2048])
    named: dict = dataclasses.field(default_factory=dict)   # what the builder aimed at: name -> (chunk index, voxel)

    def cam_tuple(self):
        c = self.cam
        return (c.width, c.height, c.fx, c.fy, c.cx, c.cy, c.near, c.far)

    def chunk(self, i):
        return self.preset[tuple(int(v) for v in self.ids[i])]


def fresh():
    return np.full(512, 999.0, F), np.zeros(512, F), np.zeros(2048, np.uint16)


def pose_rt(R=None, t=(0, 0, 0)):
    p = np.zeros((3, 4), F)
    p[:, :3] = np.eye(3, dtype=F) if R is None else np.asarray(R, F)
    p[:, 3] = np.asarray(t, F)
    return p


def roll(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


def images(seed):
    """an RGBA image with every byte value and a smooth positive quality image"""
    rng = np.random.default_rng(seed)
    rgba = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    rgba[..., 3] = (rng.random((H, W)) > 0.2)
    q = (0.25 + rng.random((H, W))).astype(F)
    return rgba, q


def plane(d):
    return np.full((H, W), d, F)


def steer(depth):
    """Pixel (0, 0) is never read by the voxel update (a valid lane has X > 0 and Y > 0), but the fused frame's selection
    takes its bounding box over every pixel of depth + 0.2: a pixel of -0.2 there makes the box start at z = 0, which is what
    lets the selection find the preset chunks of E - H by itself (E's are nearer than 0.2 m)."""
    depth[0, 0] = F(-0.2)
    return depth


def geometry(case, i, frame=0):
    """the projection of chunk i of the case (tests/ka_ref.py on the case's own images)"""
    s, w, c = case.chunk(i)
    return KR.voxel_update(case.depths[frame], case.rgba, case.quality, case.cam_tuple(), case.ig, case.poses[frame], 1,
                           case.ids[i], case.res, s, w, c)


def _make(name, cam, res, ig, poses, depths, ids, seed, preset=None, rgba=None, quality=None):
    ids = np.asarray(ids, np.int32).reshape(-1, 3)
    assert 1 <= len(ids) <= 30
    im = images(seed)
    ps = {tuple(int(v) for v in c): fresh() for c in ids}
    if preset:
        ps.update(preset)
    return Case(name, cam, F(res), ig, [np.asarray(p, F) for p in poses], [np.asarray(d, F) for d in depths],
                im[0] if rgba is None else rgba, im[1] if quality is None else quality, ids, ps)


def ulps(x, n):
    """the float32 n steps away from x"""
    x = F(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, F(np.inf) if n > 0 else F(-np.inf))
    return x


def solve(fn, guess, want, span=6):
    """a float32 x within `span` steps of `guess` with fn(x) == want bit for bit, or None"""
    want = F(want)
    for n in sorted(range(-span, span + 1), key=abs):
        x = ulps(guess, n)
        if F(fn(x)).view(np.uint32) == want.view(np.uint32):
            return x
    return None


# ---- A -----------------------------------------------------------------------------------------------------------------
A_Z = 6  # chunk id.z: p.z from 0.2425 to 0.2775


def _case_a():
    # about 1.07 .. 0.94 pixels per voxel: a chunk is 8 pixels wide.  Chunk columns -4 .. 3 cover X = -2 .. 63, rows -3 .. 2
    # cover Y = -1 .. 49 (t shifts the grid by fractions of a voxel so that the border values all occur)
    pose = pose_rt(t=(0.0012, 0.0031, 0.0))
    ids = [[0, 0, A_Z], [-1, -1, A_Z]]
    ids += [[-4, j, A_Z] for j in (-3, -1, 0, 2)] + [[3, j, A_Z] for j in (-3, -1, 0, 2)]
    ids += [[i, -3, A_Z] for i in (-3, -1, 1, 2)] + [[i, 2, A_Z] for i in (-3, -1, 1, 2)]
    ids += [[-4, 0, A_Z + 1], [3, 0, A_Z - 1], [0, -3, A_Z + 1], [0, 2, A_Z - 1]]
    # (quality of the order of 1e4: a row's sum is more than the sentinel's ulp of 8192, so additions after it show)
    return _make("A", CAM, RES5, IG, [pose], [plane(0.262)], ids, 1, quality=(images(1)[1] * F(16384.0)).astype(F))


def _case_a2():
    # a quarter turn about the optical axis (exact 0 / +-1 entries): a row's eight lanes now differ in Y, so Y = -1, 0, H-1
    # and H occur in rows that are processed (under the identity pose a row shares one Y, and such a row is dead)
    pose = pose_rt([[0, -1, 0], [1, 0, 0], [0, 0, 1]], (-0.0044, -0.0012, 0.0))
    ids = [[0, 0, A_Z]] + [[i, j, A_Z] for i in (2, -3) for j in (-4, -2, 0, 1, 3)] + [[i, j, A_Z] for j in (-4, 3) for i in (-2, 0, 1)]
    return _make("A2", CAM, RES5, IG, [pose], [plane(0.262)], ids, 12, quality=(images(12)[1] * F(16384.0)).astype(F))


# ---- B -----------------------------------------------------------------------------------------------------------------
def _case_b(cam, name):
    h = F(2.0 ** -9)
    ids = [[i, j, 8] for i in (-3, -1, 0, 2) for j in (-2, 0, 1)]
    return _make(name, cam, RES8, IG, [pose_rt(t=(h, h, h))], [plane(0.262)], ids, 2)


# ---- C -----------------------------------------------------------------------------------------------------------------
C_IDS = [[0, 0, 0], [0, 0, -1], [-1, -1, -1], [-1, -1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0]]


def _case_c(quarter, name, cam=CAM, tz=1):
    h = F(2.0 ** -9)
    R = [[0, 0, 1], [0, 1, 0], [-1, 0, 0]] if quarter else None
    d = plane(0.0117)
    d[::3, ::2] = 0.035
    return _make(name, cam, RES8, IG, [pose_rt(R, (h, h, tz * h))], [d], C_IDS, 3)


# ---- D -----------------------------------------------------------------------------------------------------------------
D_IDS = [[0, 0, 4], [0, 0, 3], [0, 0, 5], [1, 0, 4], [-1, 0, 4], [0, 1, 4], [0, -1, 4], [1, 1, 5], [-1, -1, 3]]
D_R = np.asarray(synth.pose_euler(2.3, -0.62, 0.3))[:, :3].astype(np.float64)  # the camera looks down the cube's diagonal
D_BAND = F(0.125)  # 32 res
TWO20 = 1048576.0


def _case_d(name, sign, step):
    """chunk (0, 0, 4) gets o.z == sign * (the float `step` steps from the band) and projects around the image centre"""
    want = F(sign) * ulps(D_BAND, step)
    mid = (D_R.T @ np.array([4.0, 4.0, 4.0])) * float(RES8)          # the chunk's centre relative to its origin, camera frame
    t0 = np.array([0.0, 0.0, 0.125]) - D_R @ np.array([-mid[0], -mid[1], float(want)])
    cid = np.array(D_IDS[0], np.int32)

    # o.z is a rounded sum of three rounded products: not every float is reachable by moving t along one axis, so the
    # translation is jittered by less than a micrometre (fixed seed) until the sum lands on the float wanted
    rng = np.random.default_rng(4)
    for _ in range(20000):
        t = (t0 + rng.uniform(-1e-6, 1e-6, 3)).astype(F)
        if KR.chunk_scalars(IG, pose_rt(D_R, t), cid, RES8)[0][2] == want:
            break
    else:
        raise AssertionError("case %s: no translation gives o.z == %r" % (name, want))
    d = plane(0.125)
    d[::2, 1::3] = 0.1
    d[1::2, ::3] = 0.15
    return _make(name, CAM, RES8, IG, [pose_rt(D_R, t)], [d], D_IDS, 4)


def _cases_d():
    out = [_case_d("D_eq", 1, 0), _case_d("D_pos_above", 1, 1), _case_d("D_pos_below", 1, -1),
           _case_d("D_neg_eq", -1, 0), _case_d("D_neg_above", -1, 1), _case_d("D_neg_below", -1, -1)]
    under = float(ulps(TWO20, -1))
    for ax, nm in enumerate("xyz"):
        for lab, val in (("under", under), ("over", TWO20)):
            t = [0.0, 0.0, 0.0]
            t[ax] = -val
            if ax == 2:
                t[2] = -(val - 0.25)  # (the listed chunks add up to 0.16 to o.z)
            ids = [[0, 0, 8], [1, 0, 8], [0, -1, 9]] if ax < 2 else [[0, 0, 4], [0, 0, 8], [0, 0, 12]]
            out.append(_make("D_%s_%s" % (nm, lab), CAM, RES8, IG, [pose_rt(None, t)], [plane(0.27)], ids, 5))
    return out


# ---- E -----------------------------------------------------------------------------------------------------------------
E_TARGETS = ("near", "far", "lower", "upper", "thr_pos", "thr_neg")


def _case_e():
    pose = pose_rt(np.asarray(synth.pose_euler(0.21, -0.13, 0.4))[:, :3], (0.0041, 0.0038, 0.0))
    ids = [[0, 0, k] for k in range(1, 8)] + [[-1, 0, 3], [0, -1, 4], [-1, -1, 5], [1, 0, 6], [0, 1, 7], [1, 1, 7]]
    c = _make("E", CAM_NEAR, RES10, IG, [pose], [steer(plane(0.035))], ids, 6)
    g = [geometry(c, i) for i in range(len(ids))]
    # voxels whose pixel no other voxel of the list reads
    allidx = np.concatenate([x["idx"][x["valid"] & x["live"]] for x in g])
    cnt = np.bincount(allidx, minlength=W * H)
    depth = c.depths[0].reshape(-1)
    near, far = F(CAM_NEAR.near), F(CAM_NEAR.far)
    used = set()
    for tgt in E_TARGETS:
        for step in (0, -1, 1):
            done = False
            for i, x in enumerate(g):
                if done:
                    break
                thr, up = x["thr_col"], x["upper"]
                for k in np.flatnonzero((x["valid"] & x["live"]).reshape(-1)):
                    pix = int(x["idx"].reshape(-1)[k])
                    if cnt[pix] != 1 or pix in used:
                        continue
                    pz = x["pz"].reshape(-1)[k]
                    sub = lambda d: F(F(d) - pz)
                    if tgt in ("near", "far"):
                        d = ulps(near if tgt == "near" else far, step)
                        ok = KR.LOWER < sub(d) < up  # the band alone would update: the depth test decides
                    else:
                        want = ulps({"lower": KR.LOWER, "upper": up, "thr_pos": thr, "thr_neg": -thr}[tgt], step)
                        d = solve(sub, F(pz + want), want)
                        ok = d is not None and near < d < far
                    if ok:
                        depth[pix] = d
                        used.add(pix)
                        c.named["%s%+d" % (tgt, step)] = (i, int(k))
                        done = True
                        break
            assert done, "case E: no voxel can hit %s%+d" % (tgt, step)
    return c


# ---- F, G, H: one geometry -----------------------------------------------------------------------------------------------
FGH_IDS = [[0, 0, 10], [-1, 0, 10], [0, -1, 10]]  # p.z from 0.4025 to 0.4375; d = 0.415 puts every voxel inside the TSDF band


def _fgh(name, ig, seed, presets, depth=None, rgba=None):
    pose = pose_rt(t=(0.0007, -0.0011, 0.0))
    return _make(name, CAM, RES5, ig, [pose], [steer(plane(0.415) if depth is None else depth)], FGH_IDS, seed, presets, rgba=rgba)


def _case_f():
    c = _fgh("F", IG_LIGHT, 7, None)
    for i in range(len(c.ids)):
        wD = geometry(c, i)["wD"]
        add = lambda w: F(F(w) + wD)
        sub = lambda w: F(F(w) - wD)
        half_eq, half_up = solve(add, F(F(0.5) - wD), F(0.5)), solve(add, F(F(0.5) - wD), ulps(0.5, 1))
        hi0 = next(ulps(wD + F(0.5), n) for n in range(-3, 8) if sub(ulps(wD + F(0.5), n)) > F(0.5))  # the first w that survives flag 0
        assert half_eq is not None and half_up is not None and not sub(ulps(hi0, -1)) > F(0.5)
        vals = np.array([half_eq, half_up, wD, 0.0, hi0, -0.0, ulps(half_eq, -1), F(wD + F(0.5)), 3.0, 0.6], F)
        s, w, col = c.chunk(i)
        w[:] = vals[np.arange(512) % len(vals)]
        s[:] = (0.004 * ((np.arange(512) % 7) - 3)).astype(F)
        c.named["w%d" % i] = vals
    return c


G_STATES = [(np.inf, 1.0), (-np.inf, 1.0), (np.nan, 1.0), (0.5, np.inf), (0.5, -np.inf), (0.5, np.nan), (2.0, 3e38), (-2.0, 3e38),
            (1e-40, 1.0), (-1e-40, 2.0), (0.5, 1e-40), (0.5, -1e-40), (1e-20, 1e-20), (-1e-19, 1e-21), (0.5, -3.0), (-0.5, -40.0),
            (np.inf, 0.0), (0.0, np.inf), (3e38, 3e38), (999.0, 0.0), (0.01, 7.0)]


def _case_g():
    c = _fgh("G", IG, 8, None)
    st = np.array(G_STATES, F)
    for i in range(len(c.ids)):
        s, w, col = c.chunk(i)
        k = (np.arange(512) + 5 * i) % len(st)
        s[:], w[:] = st[k, 0], st[k, 1]
    return c


H_COLOURS = [(65535, 5, 65535, 119), (5, 65535, 7, 120), (65535, 65535, 65535, 121), (0, 9, 0, 3), (9, 0, 11, 0), (0, 0, 0, 200),
             (65400, 1, 65300, 118), (300, 65500, 1, 0x8000), (1, 2, 3, 0xFFFF), (65535, 1, 0, 0x7FFF), (100, 200, 300, 200),
             (0, 1, 65535, 65535 - 254), (40000, 50000, 60000, 122)]


def _case_h():
    rgba = np.full((H, W, 4), 255, np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    rgba[..., 3] = np.array([0, 1, 255], np.uint8)[(xx + 2 * yy) % 3]
    depth = plane(0.42)
    depth[(xx + 3 * yy) % 5 == 0] = 0.0   # holes: single lanes of updated rows without an update
    c = _fgh("H", IG, 9, None, depth=depth, rgba=rgba)
    hc = np.array(H_COLOURS, np.uint16)
    for i in range(len(c.ids)):
        s, w, col = c.chunk(i)
        col[:] = hc[(np.arange(512) + 3 * i) % len(hc)].reshape(-1)
    return c


# ---- I -----------------------------------------------------------------------------------------------------------------
I_IDS = [[0, 0, 8], [-4, 0, 8], [1, -1, 8], [-4, -2, 8], [-2, 1, 8], [3, 0, 8]]


def _case_i():
    # B's geometry off the ties: in slice 0 (p.z = 2^-2, fx = 64, res = 2^-8) X = 8 id.x + x + 31 and Y = 8 id.y + y + 24, one
    # pixel per voxel; the depth plane puts slices 0 .. 3 into the colour band.  The quality image has period 4 along both
    # axes, so a row's eight lanes read two full periods (1e8, 1, -1e8, 1e-3 from some phase): summed lane 0 .. 7 a row
    # gives 1e-3, 0, 1 or 1.001 by phase, any other order something else, and the chunk totals stay small enough to show it.
    # The chunks at id.x = -4 have X = -1 in lane 0 of slice 0 only: the sentinel is assigned in rows 0 .. 7, rows 8 .. 31 add
    yy, xx = np.mgrid[0:H, 0:W]
    q = np.array([1e8, 1.0, -1e8, 1e-3], F)[(xx + yy) % 4]
    pose = pose_rt(t=(0.75 / 256, 0.25 / 256, 2.0 ** -9))
    return _make("I", CAM_POW2, RES8, IG, [pose], [plane(0.2505)], I_IDS, 10, quality=q)


# ---- J -----------------------------------------------------------------------------------------------------------------
J_POSES = [pose_rt(t=(0.0012, 0.0031, 0.0)),
           np.asarray(synth.pose_euler(0.05, -0.02, 0.01, (0.006, -0.004, 0.001))),
           np.asarray(synth.pose_euler(-0.04, 0.03, -0.02, (-0.005, 0.007, -0.002))),
           np.asarray(synth.pose_euler(0.02, 0.06, 0.1, (0.0, 0.012, 0.003))),
           np.asarray(synth.pose_euler(-0.08, -0.05, 0.0, (0.011, 0.0, -0.001))),
           np.asarray(synth.pose_euler(0.0, 0.0, -0.15, (-0.009, -0.009, 0.002)))]
J_DEPTHS = (0.262, 0.258, 0.266, 0.26, 0.27, 0.255)
J_IDS = [[0, 0, A_Z], [-1, -1, A_Z], [-4, 0, A_Z], [3, -1, A_Z], [0, -3, A_Z], [1, 2, A_Z], [-4, -3, A_Z], [3, 2, A_Z], [0, 0, A_Z + 1]]


def _case_j(n):
    c = _make("J%d" % n, CAM, RES5, IG, J_POSES[:n], [plane(d) for d in J_DEPTHS[:n]], J_IDS, 11)
    wD = geometry(c, 0)["wD"]
    s, w, col = c.chunk(0)
    w[:] = F(F(0.3) - wD)   # frame 1 leaves 0.3 (reset), frame 2 rebuilds
    w[1::2] = F(wD + F(0.4))  # under flag 0: 0.4 after frame 1 (reset)
    s[:] = F(0.002)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, in the order of the module docstring"""
    out = [_case_a(), _case_a2(), _case_b(CAM_POW2, "B"), _case_b(CAM_FRAC, "B2"), _case_c(False, "C1"), _case_c(True, "C2"), _case_c(True, "C3", CAM_TALL, -1)]
    out += _cases_d()
    out += [_case_e(), _case_f(), _case_g(), _case_h(), _case_i(), _case_j(1), _case_j(2), _case_j(6)]
    return {c.name: c for c in out}


SINGLE = ("A", "A2", "B", "B2", "C1", "C2", "C3", "D_eq", "D_pos_above", "D_pos_below", "D_neg_eq", "D_neg_above", "D_neg_below", "D_x_under", "D_x_over",
          "D_y_under", "D_y_over", "D_z_under", "D_z_over", "E", "F", "G", "H", "I")
GROUPS = ("J1", "J2", "J6")
ALL = SINGLE + GROUPS
NAN_ALLOWED = ("G",)
FUSED = ("E", "F", "G", "H")


def guard_safe(o, res):
    """the fast-division predicate, restated from tf_kernels.hip:744-746 (`div_safe`).  It exists only so that the census can
    prove that chunks on both sides of it are exercised; no expected value depends on it"""
    o = np.asarray(o, F)
    band = F(F(32.0) * F(res))
    return bool(abs(o[2]) > band and abs(o[2]) < F(TWO20) and abs(o[0]) < F(TWO20) and abs(o[1]) < F(TWO20)
                and F(res) > F(1e-6) and F(res) < F(16.0))
