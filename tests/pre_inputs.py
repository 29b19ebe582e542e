"""Hand-built inputs for the frame pre-processing passes (tf_pre_*, texturefusion_amd/csrc/tf_pre.hip) at the edges
the room frames of test_gpu_pre.py never reach: every strict comparison fed a value on its boundary, projections that
leave the image, fall behind the camera or onto V.z == 0, non-finite and denormal readings, image sizes whose pixel
count is a multiple of neither 64 nor 256, the loader's weight image (0), and in-place dependency chains as long as
the image is tall.

Each case is a function returning a SimpleNamespace: its camera, its arrays, and `promise`, a function that takes the
REFERENCE outputs (tests/pre_ref.py) and asserts the coverage the case exists for.  The promises are conditions on the
inputs: a case that misses one is changed, never the condition.  tests/test_pre_cpu.py checks them on the CPU;
tests/test_gpu_pre_edges.py runs the same cases on the device against the oracle.

Widths that are no multiple of 8 exist for the five passes whose reference is defined per pixel; the device's camera
(tf_set_camera) does not take them, so they are checked between the two CPU statements only."""
from types import SimpleNamespace as NS

import numpy as np

from texturefusion_amd import synth
from tests import pre_ref as R

F = np.float32
SIZES8 = [(24, 13), (40, 29), (72, 53)]                    # W % 8 == 0, W * H % 64 != 0
SIZES_ODD = [(w, 5) for w in (11, 12, 19, 20, 21, 27)]     # around the normal map's j < W - 10 group rule
PROJ_SIZES = [(40, 29), (72, 53)]
I34 = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(F)


def exact_cam(W, H):
    """fx = fy = 128 and an integer principal point: with depth 1, ((j - cx) / fx * d) / d * fx + cx is exactly j,
    and the pixel at (cy, cx) has the view vector (0, 0, 1) exactly"""
    return synth.Camera(width=W, height=H, fx=128.0, fy=128.0, cx=float(W // 2), cy=float(H // 2))


def room_cam(W, H):
    """the small test camera of test_gpu_pre.py scaled to W x H (a 62 degree field of view)"""
    return synth.Camera(width=W, height=H, fx=131.25 * W / 160, fy=131.25 * W / 160, cx=W / 2 - 0.5, cy=H / 2 - 0.5)


def below(x):
    """one ulp nearer to zero"""
    return np.nextafter(F(x), F(0))


def plane(cam, a, b, c):
    j, i = np.meshgrid(np.arange(cam.width), np.arange(cam.height))
    return (c / (1.0 - a * (j - cam.cx) / cam.fx - b * (i - cam.cy) / cam.fy)).astype(F)


def _unit(n):
    return np.linalg.norm(n.astype(np.float64), axis=0)


# ---- extractNormalMapSIMD -------------------------------------------------------------------------------------------
def nm_plane(W, H):
    """a tilted plane, valid everywhere: shows WHICH pixels the pass writes.  Rows 1 .. H - 2 (none at H = 2, one at
    H = 3), columns 1 .. 8 * groups (no group at W = 11, one at W = 12 and 19, two at W = 20)"""
    cam = room_cam(W, H)
    depth = plane(cam, 0.3, -0.2, 1.5)

    def promise(n):
        written = np.zeros((H, W), bool)
        written[1:H - 1, 1:R.normal_map_columns(W)] = True
        assert np.array_equal(_unit(n) > 0.99, written)
        assert (n[:, ~written] == 0).all()
    return NS(name="nm_plane_%dx%d" % (W, H), cam=cam, depth=depth, promise=promise)


def nm_thresholds():
    """u3 = right - left and v3 = below - above exactly +-0.3f (rejected) and one ulp inside (kept): the neighbours
    are 0 and the threshold itself, so the difference is exact"""
    W, H = 24, 13
    cam = exact_cam(W, H)
    depth = np.ones((H, W), F)
    t, s = F(0.3), below(0.3)
    spots = {}
    for (i, j), (lo, hi), keep in (((2, 3), (0, t), False), ((2, 8), (0, s), True), ((2, 13), (t, 0), False),
                                   ((4, 3), (s, 0), True)):
        depth[i, j - 1], depth[i, j + 1] = lo, hi
        spots[(i, j)] = keep
    for (i, j), (lo, hi), keep in (((7, 3), (0, t), False), ((7, 8), (0, s), True), ((7, 13), (t, 0), False),
                                   ((10, 3), (s, 0), True)):
        depth[i - 1, j], depth[i + 1, j] = lo, hi
        spots[(i, j)] = keep

    def promise(n):
        for (i, j), keep in spots.items():
            assert (_unit(n)[i, j] > 0.99) == keep, (i, j)
    return NS(name="nm_thresholds", cam=cam, depth=depth, promise=promise)


def nm_tiny():
    """a nearly constant tiny depth c gives the normal (0, 0, (2c / fx)(2c / fy)) before scaling: c runs through
    6.4e-5 down the image, 0.4 % either side, where the squared length crosses 1e-24f.  Rows are rejected above and
    kept below, with every difference far inside 0.3"""
    W, H = 40, 29
    cam = exact_cam(W, H)
    c = 6.4e-5 * (0.996 + 0.008 * np.arange(H) / (H - 1))
    depth = np.repeat(c[:, None], W, 1).astype(F)
    depth += (F(1e-10) * np.arange(W, dtype=F))[None, :]  # the tiny tilt

    def promise(n):
        kept = _unit(n)[1:H - 1, 1:R.normal_map_columns(W)] > 0.99
        assert kept[-1].all() and not kept[0].any() and 0.3 < kept.mean() < 0.7
        assert np.abs(depth).max() < 0.1
    return NS(name="nm_tiny", cam=cam, depth=depth, promise=promise)


def nm_nonfinite():
    """NaN, +Inf, an Inf pair and denormals next to finite readings: all four neighbours of each are rejected, and
    no NaN reaches the output"""
    W, H = 40, 29
    cam = room_cam(W, H)
    depth = plane(cam, 0.1, 0.1, 1.2)
    bad = {(5, 5): np.nan, (5, 12): np.inf, (12, 5): np.inf, (12, 7): np.inf, (12, 14): 1e-40, (20, 20): np.nan,
           (20, 21): np.inf}
    for at, v in bad.items():
        depth[at] = v
    depth[22:26, 3:9] = F(1e-40)  # a denormal patch: differences 0, squared length 0

    def promise(n):
        assert np.isfinite(n).all()
        u = _unit(n)
        for (i, j) in bad:
            for at in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
                assert u[at] == 0, at
        assert (u[23:25, 4:8] == 0).all() and (u > 0.99).mean() > 0.5
    return NS(name="nm_nonfinite", cam=cam, depth=depth, promise=promise)


def nm_exact_length():
    """the flat depth 6.4e-5f under the exact camera has the squared length EXACTLY 1e-24f, which the strict
    comparison rejects; four ulps more depth and it is kept"""
    W, H = 24, 13
    cam = exact_cam(W, H)
    lo = F(6.4e-5)
    hi = lo + F(4) * np.spacing(lo)
    depth = np.full((H, W), lo, F)
    depth[7:] = hi

    def length(c):
        z = (((F(0) + c) + c) / F(128)) * (((F(0) + c) + c) / F(128))  # u3 = v3 = 0: the normal is (0, 0, u1 * v2)
        return (F(0) + F(0)) + z * z

    def promise(n):
        assert length(lo) == F(1e-24) and length(hi) > F(1e-24)
        u = _unit(n)[:, 1:R.normal_map_columns(W)]
        assert (u[1:6] == 0).all() and (u[9:12] > 0.99).all()
    return NS(name="nm_exact_length", cam=cam, depth=depth, promise=promise)


def normal_map_cases():
    sizes = SIZES8 + SIZES_ODD + [(24, 2), (24, 3)]
    return [nm_plane(w, h) for w, h in sizes] + [nm_thresholds(), nm_tiny(), nm_exact_length(), nm_nonfinite()]


# ---- refineDepthUseNormalSIMD / checkColorQuality / estimateColorQuality ---------------------------------------------
def _facing(cam):
    n = np.zeros((3, cam.height, cam.width), F)
    n[2] = 1
    return n


def _random_normals(cam, seed):
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(3, cam.height, cam.width))
    return (n / np.linalg.norm(n, axis=0)).astype(F)


def rdn_threshold(nz, flips):
    """at the principal point view . normal IS n_z: the pixel is zeroed for |q| < 0.1f, strictly"""
    cam = exact_cam(24, 13)
    pp = (int(cam.cy), int(cam.cx))
    n = _facing(cam)
    n[:, pp[0], pp[1]] = (0.6, -0.7, nz)
    depth = np.ones((cam.height, cam.width), F)

    def promise(n2, d2):
        zeroed = np.argwhere(d2 == 0).tolist()
        assert zeroed == ([list(pp)] if flips else []), zeroed
        assert (n2[:, pp[0], pp[1]] == 0).all() == flips
    return NS(name="rdn_nz_%s" % np.float32(nz).view(np.uint32), cam=cam, normal=n, depth=depth, promise=promise)


def rdn_random(W, H):
    cam = room_cam(W, H)
    n = _random_normals(cam, 7 * W + H)
    depth = plane(cam, 0.1, -0.1, 1.3)

    def promise(n2, d2):
        assert 0 < (d2 == 0).sum() < d2.size
        assert np.array_equal(d2 == 0, (n2 == 0).all(0))
    return NS(name="rdn_random_%dx%d" % (W, H), cam=cam, normal=n, depth=depth, promise=promise)


def refine_depth_normal_cases():
    t = F(0.1)
    return ([rdn_threshold(t, False), rdn_threshold(below(t), True), rdn_threshold(-t, False),
             rdn_threshold(-below(t), True)] + [rdn_random(w, h) for w, h in SIZES8 + SIZES_ODD])


def cv_threshold(nz, flag):
    """at the principal point |q| is |n_z|: flagged for (double)|q| >= 0.2, and 0.2f widens to just above 0.2"""
    cam = exact_cam(24, 13)
    pp = (int(cam.cy), int(cam.cx))
    n = _facing(cam)
    n[:, pp[0], pp[1]] = (0.6, -0.7, nz)

    def promise(f):
        assert np.argwhere(f == 0).tolist() == ([] if flag else [list(pp)])
    return NS(name="cv_nz_%s" % np.float32(nz).view(np.uint32), cam=cam, normal=n, promise=promise)


def cv_random(W, H):
    cam = room_cam(W, H)

    def promise(f):
        assert 0 < f.sum() < f.size and set(np.unique(f)) == {0, 1}
    return NS(name="cv_random_%dx%d" % (W, H), cam=cam, normal=_random_normals(cam, 11 * W + H), promise=promise)


def color_valid_cases():
    t = F(0.2)
    return ([cv_threshold(t, 1), cv_threshold(below(t), 0), cv_threshold(-t, 1), cv_threshold(-below(t), 0)] +
            [cv_random(w, h) for w, h in SIZES8 + SIZES_ODD])


def _mixed_derivative(rgb):
    g = np.pad(R.gray8(rgb), 1, mode="reflect")  # numpy "reflect" = BORDER_REFLECT_101
    return (g[2:, 2:] - g[2:, :-2] - g[:-2, 2:] + g[:-2, :-2]).astype(F)


def cq_depth_sign():
    """depth > 0 decides between the raw derivative and |derivative| * |view . normal|: 0, -1 and NaN are not
    above 0, the denormal 1e-40f is"""
    cam = exact_cam(24, 13)
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (cam.height, cam.width, 3), dtype=np.uint8)
    depth = np.ones((cam.height, cam.width), F)
    spots = {(3, 4): (F(0), False), (3, 15): (F(1e-40), True), (8, 4): (F(-1), False), (8, 15): (F(np.nan), False)}
    for at, (v, _) in spots.items():
        depth[at] = v
    n = _facing(cam)
    n[0] = 0.5  # tilted, so that |view . normal| is not 1

    def promise(q):
        s = _mixed_derivative(rgb)
        for at, (_, scaled) in spots.items():
            assert s[at] != 0, at
            if scaled:
                assert q[at] > 0 and q[at] != abs(s[at]), at
            else:
                assert q[at] == s[at], at
        assert depth[3, 15] != 0 and abs(depth[3, 15]) < np.finfo(F).tiny
    return NS(name="cq_depth_sign", cam=cam, depth=depth, normal=n, rgb=rgb, promise=promise)


def cq_random(W, H):
    """random colours, holes and normals; at H = 2 or W = 2 BORDER_REFLECT_101 folds both neighbours onto the one
    other row or column and the derivative vanishes"""
    cam = room_cam(W, H)
    rng = np.random.default_rng(13 * W + H)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    depth = np.where(rng.random((H, W)) < 0.7, 1.0, 0.0).astype(F)
    depth[0, 0], depth[-1, -1] = 1, 0

    def promise(q):
        if H == 2 or W == 2:
            assert (q == 0).all()
        else:
            assert (q[depth == 0] < 0).any() and (q[depth > 0] > 0).any() and (q[depth > 0] >= 0).all()
    return NS(name="cq_random_%dx%d" % (W, H), cam=cam, depth=depth, normal=_random_normals(cam, 17 * W + H), rgb=rgb,
              promise=promise)


def color_quality_cases():
    return [cq_depth_sign()] + [cq_random(w, h) for w, h in SIZES8 + SIZES_ODD + [(2, 2), (8, 2), (2, 5), (24, 2)]]


# ---- the two refinement passes: shared projection cases -------------------------------------------------------------
def _rot(axis, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    a, b = [(1, 2), (2, 0), (0, 1)][axis]
    M = np.eye(3)
    M[a, a], M[a, b], M[b, a], M[b, b] = c, -s, s, c
    return M


def _T(Rm=np.eye(3), t=(0, 0, 0)):
    return np.hstack([Rm, np.asarray(t, np.float64)[:, None]]).astype(F)


def _sides(rx, ry, valid, W, H, lo):
    """a projection leaves the image on each of its four sides, and at least a fifth stays inside"""
    with np.errstate(invalid="ignore"):
        assert (rx <= lo).any() and (rx >= W - lo).any() and (ry <= lo).any() and (ry >= H - lo).any()
    assert valid.mean() >= 0.2, valid.mean()


def _projection_inputs(kind, W, H):
    """-> cam, moving (the image the pass projects), other (the image it gathers from), T, check(V, rx, ry, valid)"""
    cam = room_cam(W, H)
    moving, other = plane(cam, 0.1, -0.05, 1.2), plane(cam, 0.08, -0.06, 1.21)
    T = _T(t=(0.004, -0.003, 0.002))
    check = lambda V, rx, ry, valid: None  # noqa: E731
    rng = np.random.default_rng(W + H)
    if kind == "roll30":
        T = _T(_rot(2, 30.0), (0.05, -0.03, 0.01))
        check = lambda V, rx, ry, valid: _sides(rx, ry, valid, W, H, 1)  # noqa: E731
    elif kind == "behind":
        T = _T(_rot(1, 180.0))

        def check(V, rx, ry, valid):
            assert (V[2] < 0).all() and valid.any()  # the image test alone lets such pixels through
    elif kind == "vz_zero":
        moving = np.ones((H, W), F)
        T = _T(t=(0, 0, -1))

        def check(V, rx, ry, valid):
            assert (V[2] == 0).all() and not valid.any()
    elif kind in ("holes_t0", "holes_tz"):
        moving[rng.random((H, W)) < 0.2] = 0
        moving[H // 2, W // 2] = 0
        T = _T(t=(0, 0.01, 0.0 if kind == "holes_t0" else 0.05))

        def check(V, rx, ry, valid):
            hole = moving == 0
            assert hole.sum() > 20
            if kind == "holes_t0":  # 0 / 0 and 0.01 / 0
                assert np.isnan(rx[hole]).all() and np.isinf(ry[hole]).all() and not valid[hole].any()
            else:                   # a hole projects as the point t itself: inside the image
                assert (V[2][hole] == F(0.05)).all() and valid[hole].all()
    elif kind in ("nonfinite_moving", "nonfinite_other"):
        img = moving if kind == "nonfinite_moving" else other
        pick = rng.random((H, W))
        img[pick < 0.05] = np.nan
        img[pick > 0.95] = np.inf
        img[H // 2, W // 2 - 1:W // 2 + 1] = (np.nan, np.inf)

        def check(V, rx, ry, valid):
            assert np.isnan(img).sum() > 5 and np.isposinf(img).sum() > 5 and np.isfinite(img).mean() > 0.8
    elif kind == "other_zero":
        other = np.zeros((H, W), F)
    elif kind == "step01":
        # the gathered image steps by exactly 0.1f in every 2x2 neighbourhood of its left half (0.2f - 0.1f is exact)
        # and by one ulp less in its right half; half a pixel of shift puts the bilinear value near 0.15
        a, b, b1 = F(0.1), F(0.2), below(0.2)
        odd = np.indices((H, W)).sum(0) % 2 == 1
        other = np.where(odd, np.where(np.arange(W)[None, :] < W // 2, b, b1), a).astype(F)
        moving = np.full((H, W), 0.15, F)
        T = _T(t=(0.5 * 0.15 / cam.fx, 0.5 * 0.15 / cam.fy, 0))

        def check(V, rx, ry, valid):
            dj = np.abs(other[:, 1:] - other[:, :-1])
            assert (dj[:, :W // 2 - 1] == a).all() and (dj[:, W // 2:] < a).all() and (dj[:, W // 2:] > F(0.0999)).all()
            assert valid.mean() > 0.5
    else:
        raise KeyError(kind)
    return cam, moving, other, T, check


PROJ_KINDS = ["roll30", "behind", "vz_zero", "holes_t0", "holes_tz", "nonfinite_moving", "nonfinite_other", "other_zero",
              "step01"]


def newframe_projection_case(kind, W, H):
    cam, moving, other, T, check = _projection_inputs(kind, W, H)

    def promise(out):
        check(*R.newframe_projection(moving, cam, T))
        if kind in ("roll30", "holes_tz", "nonfinite_other", "nonfinite_moving"):
            assert 0 < (out > 0).sum() < out.size
        if kind in ("behind", "vz_zero", "other_zero"):
            assert (out == 0).all()
    return NS(name="new_%s_%dx%d" % (kind, W, H), cam=cam, depth_ref=other, depth_new=moving, T=T, promise=promise)


def newframe_exact(W, H):
    """exact camera, identity motion: rx = j + 0.5 exactly, so a pixel is kept exactly for 1 <= j <= W - 2 and
    1 <= i <= H - 2 (1 < rx < W - 1, strictly)"""
    cam = exact_cam(W, H)
    one = np.ones((H, W), F)

    def promise(out):
        inner = np.zeros((H, W), bool)
        inner[1:H - 1, 1:W - 1] = True
        assert np.array_equal(out > 0, inner)
    return NS(name="new_exact_%dx%d" % (W, H), cam=cam, depth_ref=one, depth_new=one.copy(), T=I34.copy(), promise=promise)


def newframe_random(W, H):
    """the per-pixel form of the pass at every width, multiples of 8 or not"""
    cam = room_cam(W, H)
    rng = np.random.default_rng(19 * W + H)
    ref = plane(cam, 0.1, -0.05, 1.2)
    new = (ref * (1 + 0.04 * rng.normal(size=(H, W)))).astype(F)

    def promise(out):
        inner = out[1:H - 1, 1:W - 1]
        assert 0 < (inner > 0).sum() < inner.size
    return NS(name="new_random_%dx%d" % (W, H), cam=cam, depth_ref=ref, depth_new=new, T=_T(t=(0.002, 0.001, -0.003)),
              promise=promise)


def refine_newframe_cases():
    return ([newframe_exact(w, h) for w, h in SIZES8] + [newframe_random(w, h) for w, h in SIZES8 + SIZES_ODD] +
            [newframe_projection_case(k, w, h) for k in PROJ_KINDS for w, h in PROJ_SIZES])


# ---- refineKeyframesSIMD --------------------------------------------------------------------------------------------
WEIGHTS = {"w0": 0.0, "w1": 1.0, "w7": 7.0, "wdenormal": 1e-40}


def weight_image(kind, W, H):
    """0 is what the loader gives a fresh keyframe (Tools/DatasetWrapper.hpp:220), so the first refinement of every
    keyframe runs with it"""
    if kind == "wmixed":
        rng = np.random.default_rng(W * H)
        return rng.choice(np.array(list(WEIGHTS.values()) + [2.0, 30.0], F), size=(H, W)).astype(F)
    return np.full((H, W), WEIGHTS[kind], F)


def keyframe_case(name, cam, depth_ref, weight, depth_new, T, check=None, rounds=None):
    """promise(depth, weight, rounds) with rounds from the Jacobi form"""
    def promise(d, w, k):
        if check:
            check(d, w)
        if rounds:
            assert rounds(k), k
    return NS(name=name, cam=cam, depth_ref=depth_ref, weight=weight, depth_new=depth_new, T=T, promise=promise)


def keyframe_projection_case(kind, W, H, wkind="w1"):
    cam, moving, other, T, check = _projection_inputs(kind, W, H)
    if kind == "roll30":
        check = lambda V, rx, ry, valid: _sides(rx, ry, valid, W, H, 2)  # noqa: E731
    w0 = weight_image(wkind, W, H)

    def outcome(d, w):
        check(*R.keyframe_projection(moving, cam, T))
        grew = w != w0
        if kind in ("roll30", "holes_t0", "nonfinite_other", "nonfinite_moving", "step01"):
            assert 0 < grew.sum() < grew.size
        if kind in ("behind", "vz_zero", "other_zero"):
            assert not grew.any() and np.array_equal(d.view(np.uint32), moving.view(np.uint32))
        if kind == "step01":  # both halves are refined: through the fallback on the left, the bilinear tap on the right
            assert grew[5:-5, 5:W // 2 - 3].all() and grew[5:-5, W // 2 + 3:-5].all()
    return keyframe_case("key_%s_%s_%dx%d" % (kind, wkind, W, H), cam, moving, w0, other, T, outcome)


def keyframe_exact(W, H):
    """exact camera, identity motion: rx = j exactly, refined exactly for 2 < j < W - 2 and 2 < i < H - 2"""
    cam = exact_cam(W, H)
    one = np.ones((H, W), F)

    def outcome(d, w):
        inner = np.zeros((H, W), bool)
        inner[3:H - 2, 3:W - 2] = True
        assert np.array_equal(w == 2, inner) and (w[~inner] == 1).all()
    return keyframe_case("key_exact_%dx%d" % (W, H), cam, one, one.copy(), (one * F(1.02)).astype(F), I34.copy(), outcome)


def keyframe_chain(W, H, wkind, rounds):
    """A chain as long as the image is tall.  The new frame is a checkerboard, so no 2x2 neighbourhood is smooth and
    every valid pixel takes the nearest-neighbour fallback; T puts that neighbour one row up, in a group already
    rewritten.  With weight 0 the update (d * w + vZ) / (w + 1) is vZ alone and a change passes down undamped: one
    round per row.  With weight 1 it halves per link and dies out after about 14 rounds."""
    cam = synth.Camera(width=W, height=H, fx=131.25, fy=131.25, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    i, j = np.indices((H, W))
    depth = (1 + 1e-4 * i + 1e-5 * j).astype(F)
    new = (1 + 0.2 * ((i + j) % 2)).astype(F)
    T = I34.copy()
    T[1, 3] = F(-1 / cam.fy)
    return keyframe_case("key_chain_%s_%dx%d" % (wkind, W, H), cam, depth, weight_image(wkind, W, H), new, T, None, rounds)


def _rel(pose_a, pose_b):
    A = np.vstack([pose_a.astype(np.float64), [0, 0, 0, 1]])
    B = np.vstack([pose_b.astype(np.float64), [0, 0, 0, 1]])
    return (np.linalg.inv(A) @ B)[:3].astype(F)


def keyframe_room_w0():
    """the frame pair of test_frame_passes_match_the_oracle at 160x120, with the loader's weight 0 instead of 1"""
    cam = room_cam(160, 120)
    d0, _, _, pose0 = synth.room_frame(10, cam, with_quality=False, wobble=0.05)
    d1, _, _, pose1 = synth.room_frame(12, cam, with_quality=False, wobble=0.05)

    def outcome(d, w):
        assert (w == 1).mean() > 0.5 and set(np.unique(w)) == {0, 1}
    return keyframe_case("key_room_w0_160x120", cam, d0, np.zeros_like(d0), d1, _rel(pose1, pose0), outcome,
                         lambda k: k >= 2)


def refine_keyframe_cases():
    return ([keyframe_exact(w, h) for w, h in SIZES8] +
            [keyframe_projection_case(k, w, h) for k in PROJ_KINDS for w, h in PROJ_SIZES] +
            [keyframe_projection_case("roll30", 40, 29, wk) for wk in ("w0", "w7", "wdenormal", "wmixed")] +
            [keyframe_projection_case("step01", 24, 13, "w0"), keyframe_projection_case("roll30", 24, 13, "wmixed")] +
            [keyframe_chain(16, 64, "w0", lambda k: k == 61), keyframe_chain(16, 300, "w0", lambda k: k >= 290),
             keyframe_chain(16, 64, "w1", lambda k: 10 <= k <= 20), keyframe_room_w0()])


# ---- DatasetWrapper::framePreprocess --------------------------------------------------------------------------------
def _raw(W, H, seed, lo=800, hi=3500):
    rng = np.random.default_rng(seed)
    z = lo + (hi - lo) * (np.arange(W)[None, :] / W) + 200 * (np.arange(H)[:, None] > H // 2) + rng.normal(0, 4, (H, W))
    z[rng.random((H, W)) < 0.05] = 0
    return np.clip(z, 0, 65535).astype(np.uint16)


def frame_depth_cases():
    """(name, z u16, maximum_depth, depth_scale, d, promise(z_out, refined))"""
    def filtered(zo, ref):
        assert (ref > 0).mean() > 0.5 and len(np.unique(ref)) > 10

    def all_cut(zo, ref):
        assert (zo == 0).all() and (ref == 0).all()

    def near_the_top(zo, ref):
        # the u16 conversion of out * depth_scale is undefined from 65536.0 on: the case must stay below
        assert (ref * F(1000.0)).max() < 65536.0 and zo.max() >= 65500 and len(np.unique(ref)) > 10
    far = np.full((13, 24), 5000, np.uint16)
    far[::3, ::5] = 65535
    top = _raw(24, 13, 5, 65300, 65535)
    top[top == 0] = 65535
    top[4, 4:9] = 65535
    return [NS(name="fd_d15_24x13", z=_raw(24, 13, 1), maximum_depth=4.0, depth_scale=1000.0, d=15, promise=filtered),
            NS(name="fd_d1_24x13", z=_raw(24, 13, 2), maximum_depth=4.0, depth_scale=1000.0, d=1, promise=filtered),
            NS(name="fd_d9_8x8", z=_raw(8, 8, 3), maximum_depth=4.0, depth_scale=1000.0, d=9, promise=filtered),
            NS(name="fd_d7_72x53", z=_raw(72, 53, 4), maximum_depth=3.0, depth_scale=1000.0, d=7, promise=filtered),
            NS(name="fd_all_cut_24x13", z=far, maximum_depth=4.0, depth_scale=1000.0, d=9, promise=all_cut),
            NS(name="fd_top_24x13", z=top, maximum_depth=100.0, depth_scale=1000.0, d=9, promise=near_the_top)]


FRAME_DEPTH_REJECTED_D = (16, 0, -3)  # radius 8, and d <= 0 -> radius lrint(1.5 * sigma_space) = 15: both above 7
