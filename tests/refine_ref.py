"""numpy float32 restatement of k_surface_dist and k_refine_frame (tf_ray.hip), a helper of the refine tests, not a test
module.

surface_dist: Chisel::GetDistanceFromSurface (Structure/Chisel.h:251-342) operation for operation in f32 -- the point
shifted by res / 2, multiplied by the rounded reciprocal of res, floor / ceil corners in the reference's order, corner
weights as left-to-right products, sums over the corners whose chunk exists, then the division where the summed weight
is > 0.  A corner coordinate that is not finite or beyond +-(2^23 - 1) is absent.  refine_frame: RefineFrameInVoxel
(:377-451) over it, six walks along the pixel's ray and the three rejection tests.  Both run over the chunk set of a
raycast_ref.RefVolume; the library is built with -ffp-contract=off, so the device results are reproduced bit for bit.
"""
import numpy as np

F = np.float32
VOX_LIMIT = F(8388607.0)


def surface_dist(ref, points):
    """(dist [n], tsdf_weight [n]) of GetDistanceFromSurface at world points [n, 3] over RefVolume ref"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(p)
    half, step = ref.res / F(2), F(1) / ref.res
    with np.errstate(invalid="ignore", over="ignore"):
        r = (p - half) * step
        fl, ce = np.floor(r), np.ceil(r)
        frac = r - fl
        okf, okc = np.abs(fl) <= VOX_LIMIT, np.abs(ce) <= VOX_LIMIT
    fli = np.where(okf, fl, F(0)).astype(np.int64)
    cei = np.where(okc, ce, F(0)).astype(np.int64)
    weight, dist, tw = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for k in range(8):
        s = ((k >> 2) & 1, (k >> 1) & 1, k & 1)  # ceil on x / y / z
        V = [cei[:, a] if s[a] else fli[:, a] for a in range(3)]
        ok = np.ones(n, bool)
        for a in range(3):
            ok &= okc[:, a] if s[a] else okf[:, a]
        sl = np.where(ok, ref.slot(V[0] >> 3, V[1] >> 3, V[2] >> 3), -1)
        has = sl >= 0
        ax = [frac[:, a] if s[a] else F(1) - frac[:, a] for a in range(3)]
        with np.errstate(invalid="ignore"):
            sw = (ax[0] * ax[1]) * ax[2]
        vi = ((V[2] & 7) * 8 + (V[1] & 7)) * 8 + (V[0] & 7)
        sd, w = ref.sdf[np.maximum(sl, 0), vi], ref.w[np.maximum(sl, 0), vi]
        with np.errstate(invalid="ignore", over="ignore"):
            weight = np.where(has, weight + sw * w, weight)
            dist = np.where(has, dist + (sd * sw) * w, dist)
            tw = np.where(has, tw + w * sw, tw)
    pos = weight > F(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = np.where(pos, dist / np.where(pos, weight, F(1)), dist)
        tw = np.where(pos, tw / np.where(pos, weight, F(1)), tw)
    return dist.astype(np.float32), tw.astype(np.float32)


def pixel_rays(pose, fx, fy, cx, cy, W, H):
    """R * ((j - cx) / fx, (i - cy) / fy, 1) per pixel ([3, H * W]) with the int-truncated intrinsics, rows summed as
    a0 b0 + (a1 b1 + a2 b2); fx .. cy as given to tf_set_camera"""
    fxi, fyi, cxi, cyi = (F(int(F(a))) for a in (fx, fy, cx, cy))
    P = np.asarray(pose, np.float32).reshape(3, 4)
    yy, xx = np.mgrid[0:H, 0:W]
    with np.errstate(divide="ignore", invalid="ignore"):
        dx = (xx.reshape(-1).astype(np.float32) - cxi) / fxi
        dy = (yy.reshape(-1).astype(np.float32) - cyi) / fyi
    return np.stack([P[r, 0] * dx + (P[r, 1] * dy + P[r, 2]) for r in range(3)]), P[:, 3].copy()


def refine_frame(ref, depth, pose, cam, weight=None):
    """RefineFrameInVoxel: (depth [H, W], weight [H, W]) as tf_refine_frame_in_voxel leaves them; cam: synth.Camera-like
    (fx, fy, cx, cy, width, height, near, far); weight = the caller's weight image (None = zeros)"""
    W, H = cam.width, cam.height
    d0 = np.array(depth, np.float32).reshape(-1)
    wout = np.zeros(W * H, np.float32) if weight is None else np.array(weight, np.float32).reshape(-1)
    dout = d0.copy()
    with np.errstate(invalid="ignore"):
        act = ~((d0.astype(np.float64) < 0.05) | (d0.astype(np.float64) > 3.0))
    idx = np.nonzero(act)[0]
    rays, t = pixel_rays(pose, cam.fx, cam.fy, cam.cx, cam.cy, W, H)
    rr = rays[:, idx]
    dep = d0[idx].copy()
    init = dep.copy()
    d = tw = None
    for _ in range(6):
        with np.errstate(invalid="ignore", over="ignore"):
            v = np.stack([rr[a] * dep + t[a] for a in range(3)], 1)
        d, tw = surface_dist(ref, v)
        with np.errstate(invalid="ignore", over="ignore"):
            dep = dep + d
    tw = tw.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        bad = np.abs(d).astype(np.float64) > 5e-3
        dep[bad], tw[bad] = F(0), F(0)
        bad = (dep > F(cam.far)) | (dep < F(cam.near))
        dep[bad], tw[bad] = F(0), F(0)
        bad = np.abs(dep - init).astype(np.float64) > 0.1
        dep[bad], tw[bad] = F(0), F(0)
    dout[idx], wout[idx] = dep, tw
    return dout.reshape(H, W), wout.reshape(H, W)
