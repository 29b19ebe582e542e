"""numpy float32 restatement of the six BasicAPI image passes (BasicAPI.cpp:378-443, 506-636, 728-905), written from
the reference source and the conventions tf_pre.hip states in its header: the vec8 operator order without FMA (numpy
f32 never fuses), the correctly rounded 1 / sqrt for _mm256_rsqrt_ps, zero where cv::Mat::create leaves garbage.
It is the second, independent statement the oracle is compared with bit for bit (tests/test_pre_cpu.py), and its
Jacobi form of refineKeyframesSIMD is the only thing that says how many rounds a case needs on the device.

Every function takes and returns float32 arrays (normal maps planar [3][H][W]) and leaves its arguments alone."""
import numpy as np

F = np.float32


def _f(a):
    return np.ascontiguousarray(a, np.float32)


def _ji(cam):
    """column / row numbers as float32, broadcastable to [H][W]"""
    return np.arange(cam.width, dtype=F)[None, :], np.arange(cam.height, dtype=F)[:, None]


def _k(cam):
    return F(cam.fx), F(cam.fy), F(cam.cx), F(cam.cy)


def normal_map_columns(W):
    """columns extractNormalMapSIMD writes: 8-wide groups from j = 1 while j < W - 10 -> range(1, stop)"""
    return 1 + 8 * len(range(1, W - 10, 8))


def normal_map(depth, cam):
    """extractNormalMapSIMD (:849-905): cross product of the two central differences of the back-projected vertex"""
    d = _f(depth)
    H, W = d.shape
    n = np.zeros((3, H, W), F)
    stop = normal_map_columns(W)
    if H < 3 or stop == 1:
        return n
    fx, fy, cx, cy = _k(cam)
    j, i = _ji(cam)
    j, i = j[:, 1:stop], i[1:H - 1]
    with np.errstate(all="ignore"):
        dr, dl = d[1:H - 1, 2:stop + 1], d[1:H - 1, 0:stop - 1]
        db, dt = d[2:H, 1:stop], d[0:H - 2, 1:stop]
        lane = (j - F(1)) % F(8)
        xs = (lane + (j - lane)) - cx  # inc + vec8(j) - vec8(cx)
        ys = i - cy
        u3, v3 = dr - dl, db - dt
        u1 = ((xs * u3 + dr) + dl) / fx
        u2 = (ys * u3) / fy
        v1 = (xs * v3) / fx
        v2 = ((ys * v3 + db) + dt) / fy
        x = u2 * v3 - u3 * v2
        y = u3 * v1 - u1 * v3
        z = u1 * v2 - u2 * v1
        nsq = (x * x + y * y) + z * z
        valid = (u3 < F(0.3)) & (u3 > F(-0.3)) & (v3 < F(0.3)) & (v3 > F(-0.3)) & (nsq > F(1e-24))
        r = F(1) / np.sqrt(nsq)
        for k, c in enumerate((x, y, z)):
            n[k, 1:H - 1, 1:stop] = np.where(valid, c * r, F(0))
    return n


def view_dot_simd(normal, cam):
    """view . normal as refineDepthUseNormalSIMD forms it: the view vector scaled by 1 / sqrt, sums left to right"""
    n = _f(normal)
    fx, fy, cx, cy = _k(cam)
    j, i = _ji(cam)
    vX, vY, vZ = (j - cx) / fx, (i - cy) / fy, F(1)
    r = F(1) / np.sqrt((vX * vX + vY * vY) + vZ * vZ)
    with np.errstate(all="ignore"):
        return ((vX * r) * n[0] + (vY * r) * n[1]) + (vZ * r) * n[2]


def refine_depth_normal(normal, depth, cam):
    """refineDepthUseNormalSIMD (:728-781): depth and normal zeroed where -0.1 < view . normal < 0.1"""
    n, d = _f(normal).copy(), _f(depth).copy()
    q = view_dot_simd(n, cam)
    hit = (q > F(-0.1)) & (q < F(0.1))
    d[hit] = 0
    n[:, hit] = 0
    return n, d


def view_dot_eigen(normal, cam):
    """view . normal as the two Eigen passes form it: Vector3f(...).normalize() (x*x + (y*y + z*z), division by the
    root), then the fixed-size dot p0 + (p1 + p2)"""
    n = _f(normal)
    fx, fy, cx, cy = _k(cam)
    j, i = _ji(cam)
    x, y = (j - cx) / fx + F(0) * i, (i - cy) / fy + F(0) * j
    z = np.ones_like(x)
    root = np.sqrt(x * x + (y * y + z * z))
    with np.errstate(all="ignore"):
        return (x / root) * n[0] + ((y / root) * n[1] + (z / root) * n[2])


def color_valid(normal, cam):
    """checkColorQuality (:783-806): 1 where |view . normal| >= 0.2, the comparison in double"""
    q = view_dot_eigen(normal, cam)
    with np.errstate(invalid="ignore"):
        return (np.abs(q).astype(np.float64) >= 0.2).astype(np.uint8)


def gray8(rgb):
    """cv::cvtColor(CV_RGB2GRAY) on 8-bit pixels: 14-bit fixed point, rounded"""
    c = np.ascontiguousarray(rgb, np.uint8).astype(np.int64)
    return (4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14


def color_quality(depth, normal, rgb, cam):
    """estimateColorQuality (:815-847): the mixed 3x3 derivative of the gray image (BORDER_REFLECT_101), times
    |view . normal| in magnitude where depth > 0"""
    d = _f(depth)
    H, W = d.shape
    g = gray8(rgb)
    im, ip = np.arange(H) - 1, np.arange(H) + 1
    jm, jp = np.arange(W) - 1, np.arange(W) + 1
    im[0], ip[-1], jm[0], jp[-1] = 1, H - 2, 1, W - 2
    s = (g[ip][:, jp] - g[ip][:, jm] - g[im][:, jp] + g[im][:, jm]).astype(F)
    with np.errstate(invalid="ignore"):
        return np.where(d > 0, np.abs(s) * np.abs(view_dot_eigen(normal, cam)), s).astype(F)


def project(d, i, j, cam, T):
    """the vertex of pixel (i, j) at depth d, moved by [R | t]: (V0, V1, V2), each ((r0 X + r1 Y) + r2 d) + t"""
    fx, fy, cx, cy = _k(cam)
    T = _f(T).reshape(3, 4)
    with np.errstate(all="ignore"):
        lx, ly = ((j - cx) / fx) * d, ((i - cy) / fy) * d
        return [((T[r, 0] * lx + T[r, 1] * ly) + T[r, 2] * d) + T[r, 3] for r in range(3)]


def _rne_index(x):
    return np.rint(x).astype(np.int64)  # _mm256_cvtps_epi32, only ever read for in-range lanes


def newframe_projection(depth_new, cam, T):
    """-> V (3 images), rx, ry, valid of refineNewframesSIMD (with its cx + 0.5, formed in double)"""
    d = _f(depth_new)
    fx, fy, cx, cy = _k(cam)
    j, i = _ji(cam)
    V = project(d, i, j, cam, T)
    cxh, cyh = F(np.float64(cx) + 0.5), F(np.float64(cy) + 0.5)
    with np.errstate(all="ignore"):
        rx, ry = (V[0] / V[2]) * fx + cxh, (V[1] / V[2]) * fy + cyh
        valid = (rx > F(1)) & (rx < F(cam.width - 1)) & (ry > F(1)) & (ry < F(cam.height - 1))
    return V, rx, ry, valid


def refine_newframe(depth_ref, depth_new, cam, T):
    """refineNewframesSIMD (:378-443): a pixel of the new frame stays where the keyframe's depth at its projection
    is within 5 % of its own"""
    ref, d = _f(depth_ref), _f(depth_new)
    V, rx, ry, valid = newframe_projection(d, cam, T)
    with np.errstate(all="ignore"):
        at = np.where(valid, _rne_index(np.where(valid, np.floor(rx) + np.floor(ry) * F(cam.width), F(0))), 0)
        nd = np.where(valid, ref.reshape(-1)[at], F(0))
        diff = nd - V[2]
        keep = (diff > F(-0.05) * V[2]) & (diff < F(0.05) * V[2])
    return np.where(keep, d, F(0)).astype(F)


def keyframe_projection(depth_ref, cam, T):
    """-> V, rx, ry, valid of refineKeyframesSIMD for the whole image"""
    d = _f(depth_ref)
    fx, fy, cx, cy = _k(cam)
    j, i = _ji(cam)
    V = project(d, i, j, cam, T)
    with np.errstate(all="ignore"):
        rx, ry = (V[0] / V[2]) * fx + cx, (V[1] / V[2]) * fy + cy
        valid = (rx > F(2)) & (rx < F(cam.width - 2)) & (ry > F(2)) & (ry < F(cam.height - 2))
    return V, rx, ry, valid


def _keyframe_pixels(i, j, d, w, new, cam, T, nearest):
    """refineKeyframesSIMD for the pixels (i, j) (float32 arrays) with depth d and weight w.  nearest(index, valid)
    reads the keyframe's own map at flat indices: WHICH version of it is the caller's business.
    -> (depth, weight, uses) where uses marks the pixels that took the nearest-neighbour fallback and kept it"""
    fx, fy, cx, cy = _k(cam)
    W, H = cam.width, cam.height
    T = _f(T).reshape(3, 4)
    flat = new.reshape(-1)
    with np.errstate(all="ignore"):
        V = project(d, i, j, cam, T)
        rx, ry = (V[0] / V[2]) * fx + cx, (V[1] / V[2]) * fy + cy
        valid = (rx > F(2)) & (rx < F(W - 2)) & (ry > F(2)) & (ry < F(H - 2))
        fxr, fyr = np.floor(rx), np.floor(ry)
        q = np.where(valid, _rne_index(np.where(valid, fxr + fyr * F(W), F(0))), 0)
        qn = np.where(valid, _rne_index(np.where(valid, np.floor(rx + F(0.5)) + np.floor(ry + F(0.5)) * F(W), F(0))), 0)
        ul, ur = np.where(valid, flat[q], F(0)), np.where(valid, flat[np.minimum(q + 1, flat.size - 1)], F(0))
        bl = np.where(valid, flat[np.minimum(q + W, flat.size - 1)], F(0))
        br = np.where(valid, flat[np.minimum(q + W + 1, flat.size - 1)], F(0))
        nn = np.where(valid, nearest(qn, valid), F(0))
        dx, dy = rx - fxr, ry - fyr
        smooth = (((ul - ur) < F(0.1)) & ((ul - ur) > F(-0.1)) & ((ul - bl) < F(0.1)) & ((ul - bl) > F(-0.1)) &
                  ((ul - br) < F(0.1)) & ((ul - br) > F(-0.1)))
        one = F(1)
        bil = ((((one - dx) * (one - dy)) * ul + ((one - dx) * dy) * ur) + (dx * (one - dy)) * bl) + (dx * dy) * br
        bil = np.where(smooth, bil, nn)
        diff = bil - V[2]
        ok = (diff > F(-0.05) * V[2]) & (diff < F(0.05) * V[2])
        scale = bil / V[2]
        X, Y, Z = V[0] * scale - T[0, 3], V[1] * scale - T[1, 3], V[2] * scale - T[2, 3]
        vZ = (T[0, 2] * X + T[1, 2] * Y) + T[2, 2] * Z  # row 2 of R^T
        nd = np.where(ok, (d * w + vZ) / (w + one), d)
        nw = np.where(ok, w + one, w)
    return nd.astype(F), nw.astype(F), valid & ~smooth & ok


def _need_groups(W):
    if W % 8:
        raise ValueError("refineKeyframesSIMD steps 8 pixels at a time: width %d has no defined result" % W)


def refine_keyframe_sequential(depth_ref, weight_ref, depth_new, cam, T):
    """refineKeyframesSIMD (:506-636) as the reference runs it: rows top to bottom, 8 pixels at a time, each group
    stored before the next is loaded, the fallback reading the map as it stands -> (depth, weight)"""
    d, w, new = _f(depth_ref).copy(), _f(weight_ref).copy(), _f(depth_new)
    H, W = d.shape
    _need_groups(W)
    flat = d.reshape(-1)
    lane = np.arange(8, dtype=F)
    for i in range(H):
        for j0 in range(0, W, 8):
            nd, nw, _ = _keyframe_pixels(np.full(8, i, F), lane + F(j0), d[i, j0:j0 + 8], w[i, j0:j0 + 8], new, cam, T,
                                         lambda qn, valid: flat[qn])
            d[i, j0:j0 + 8], w[i, j0:j0 + 8] = nd, nw
    return d, w


def refine_keyframe_jacobi(depth_ref, weight_ref, depth_new, cam, T, max_rounds=None):
    """The same result as a fixed point, the way the device computes it: every round evaluates ALL pixels, the
    fallback reading the previous round's estimate where the index lies in an earlier 8-pixel group and the original
    map elsewhere.  -> (depth, weight, rounds): rounds counts every round run up to and including the first that
    changes no bit, which is what a device that stops as early as it can reports.  Group g is final after round g,
    so W * H / 8 + 1 rounds always suffice (the default max_rounds)."""
    orig, w0, new = _f(depth_ref), _f(weight_ref), _f(depth_new)
    H, W = orig.shape
    _need_groups(W)
    j, i = _ji(cam)
    i, j = i + F(0) * j, j + F(0) * i
    group = np.arange(H * W).reshape(H, W) >> 3
    oflat = orig.reshape(-1)
    est = orig
    limit = H * W // 8 + 1 if max_rounds is None else max_rounds
    for k in range(limit + 1):
        eflat = est.reshape(-1)
        nd, nw, _ = _keyframe_pixels(i, j, orig, w0, new, cam, T,
                                     lambda qn, valid: np.where((qn >> 3) < group, eflat[qn], oflat[qn]))
        if np.array_equal(nd.view(np.uint32), est.view(np.uint32)):
            return nd, nw, k + 1
        est = nd
    raise AssertionError("no fixed point in %d rounds" % limit)
