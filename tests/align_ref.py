"""numpy restatement of tf_align.hip (a helper of the alignment tests, not a test module).

Rows (residual, gradient, q = R pc, flags) are computed in float32, operation for operation as k_align_rows does (the
library is built with -ffp-contract=off), on top of raycast_ref.RefVolume.trilinear: the device's maps are reproduced
bit for bit.  The sums are taken with math.fsum over the same exact f64 products the device adds, so they are the exact
sums rounded once; the solve uses numpy.linalg and the pose update is done in f64.
"""
import math

import numpy as np

F = np.float32
CONVERGED, MAX_ITERS, TOO_FEW, SINGULAR = 0, 1, 2, 3
IU = np.triu_indices(6)

DEFAULTS = dict(levels=[(4, 4), (2, 3), (1, 2)], min_depth=0.05, max_depth=5.0, max_residual=0.03, huber=0.01, damping=0.0,
                eps_t=1e-5, eps_r=1e-5, min_valid=100)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def rows(ref, depth, pose, cam, stride, p):
    """One evaluation's rows at the sampled pixels.  cam: synth.Camera-like (intrinsics truncated here).  Returns a dict:
    maps r [H, W] f32, grad [3, H, W] f32, flags [H, W] u32 as tf_align_residuals writes them, and per sampled pixel
    (row-major over the sampled grid) the arrays s, g [n, 3], q [n, 3], fl."""
    H, W = cam.height, cam.width
    depth = np.asarray(depth, np.float32).reshape(H, W)
    P = np.asarray(pose, np.float32).reshape(3, 4)
    res = ref.res
    fxi, fyi, cxs, cys = F(int(cam.fx)), F(int(cam.fy)), F(int(cam.cx)) + F(0.5), F(int(cam.cy)) + F(0.5)
    ys, xs = np.arange(0, H, stride), np.arange(0, W, stride)
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    yy, xx = yy.reshape(-1), xx.reshape(-1)
    z = depth[yy, xx]
    with np.errstate(invalid="ignore"):
        b0 = np.isfinite(z) & (z >= F(p["min_depth"])) & (z <= F(p["max_depth"]))
    zz = np.where(b0, z, F(1))
    dcx = (xx.astype(np.float32) - cxs) / fxi
    dcy = (yy.astype(np.float32) - cys) / fyi
    pcx, pcy = dcx * zz, dcy * zz
    q = np.stack([(P[r, 0] * pcx + P[r, 1] * pcy) + P[r, 2] * zz for r in range(3)], 1)
    pw = np.stack([P[r, 3] + q[:, r] for r in range(3)], 1)
    s, ok, _, _ = ref.trilinear(pw, want_rgb=False)
    b1 = b0 & ok
    taps_ok = np.ones(len(z), bool)
    sp, sm = np.zeros((len(z), 3), np.float32), np.zeros((len(z), 3), np.float32)
    for ax in range(3):
        for sign, dst in ((-1, sm), (1, sp)):
            pt = pw.copy()
            pt[:, ax] = pt[:, ax] + (res if sign > 0 else -res)
            t, okt, _, _ = ref.trilinear(pt, want_rgb=False)
            dst[:, ax] = t
            taps_ok &= okt
    b2 = b1 & taps_ok
    g = (sp - sm) * (F(0.5) / res)
    with np.errstate(invalid="ignore"):
        b3 = b2 & (np.abs(s) <= F(p["max_residual"]))
    fl = (b0 * 1 + b1 * 2 + b2 * 4 + b3 * 8).astype(np.uint32)
    s = np.where(b1, s, F(0)).astype(np.float32)
    g = np.where(b2[:, None], g, F(0)).astype(np.float32)
    rm, gm, fm = np.zeros((H, W), np.float32), np.zeros((3, H, W), np.float32), np.zeros((H, W), np.uint32)
    rm[yy, xx], fm[yy, xx] = s, fl
    for a in range(3):
        gm[a, yy, xx] = g[:, a]
    return dict(r=rm, grad=gm, flags=fm, s=s, g=g, q=q.astype(np.float32), fl=fl)


def sums(rw, p):
    """The sums of one evaluation from its rows: A21 (upper entries row by row), b, sum_r2, sum_wr2 (math.fsum of the exact
    f64 terms), n_valid, n_sampled, and per sum the total of |term| (the error bound of an f64 sum in any order)."""
    v = rw["fl"] == 15
    g, q, r = rw["g"][v], rw["q"][v], rw["s"][v]
    J = np.concatenate([g, np.stack([q[:, 1] * g[:, 2] - q[:, 2] * g[:, 1], q[:, 2] * g[:, 0] - q[:, 0] * g[:, 2],
                                     q[:, 0] * g[:, 1] - q[:, 1] * g[:, 0]], 1)], 1).astype(np.float32)
    ar = np.abs(r)
    hub = F(p["huber"])
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where((hub == 0) | (ar <= hub), F(1), hub / ar).astype(np.float32)
    wJ = (w[:, None] * J).astype(np.float32)
    wr = (w * r).astype(np.float32)
    J64, wJ64, r64 = J.astype(np.float64), wJ.astype(np.float64), r.astype(np.float64)
    terms = [wJ64[:, i] * J64[:, j] for i, j in zip(*IU)] + [wJ64[:, i] * r64 for i in range(6)]
    terms += [r64 * r64, wr.astype(np.float64) * r64]
    tot = np.array([math.fsum(t) for t in terms])
    mag = np.array([math.fsum(np.abs(t)) for t in terms])
    return dict(A21=tot[:21], b=tot[21:27], sum_r2=tot[27], sum_wr2=tot[28], mag=mag, n_valid=int(v.sum()),
                n_sampled=len(rw["fl"]))


def full(A21):
    A = np.zeros((6, 6))
    A[IU] = A21
    return A + np.triu(A, 1).T


def pivots_ok(M):
    """the pivot test of tf_align_solve.h: every Cholesky pivot above 1e-12 * the largest diagonal entry"""
    thresh = 1e-12 * max(M.diagonal().max(), 0.0)
    L = np.zeros((6, 6))
    for j in range(6):
        piv = M[j, j] - (L[j, :j] ** 2).sum()
        if not piv > thresh:
            return False
        L[j, j] = math.sqrt(piv)
        for i in range(j + 1, 6):
            L[i, j] = (M[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return True


def solve(A21, b, damping):
    """xi = -(A + damping diag(A))^-1 b, or None where the pivot test fails"""
    A = full(A21)
    M = A + float(damping) * np.diag(A.diagonal())
    if not pivots_ok(M):
        return None
    return -np.linalg.solve(M, np.asarray(b, np.float64))


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = math.sqrt(float(w @ w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    if th < 1e-8:
        a, b = 1.0, 0.5
    else:
        a, b = math.sin(th) / th, 2.0 * math.sin(0.5 * th) ** 2 / (th * th)
    return np.eye(3) + a * K + b * (K @ K)


def update(pose, xi):
    P = np.array(pose, np.float64).reshape(3, 4)
    P[:, :3] = rodrigues(xi[3:]) @ P[:, :3]
    P[:, 3] += xi[:3]
    return P


def align(ref, depth, pose, cam, p):
    """tf_align_frame restated -> (result dict as Volume.align_frame's, log as Volume.align_log's)"""
    P = np.asarray(pose, np.float32).reshape(3, 4).astype(np.float64)
    log, status, stop = [], MAX_ITERS, False
    levels = p["levels"]
    first = None

    def evaluate(level, stride):
        rw = rows(ref, depth, P.astype(np.float32), cam, stride, p)
        sm = sums(rw, p)
        rec = dict(level=level, stride=stride, n_sampled=sm["n_sampled"], n_valid=sm["n_valid"], sum_r2=sm["sum_r2"],
                   sum_wr2=sm["sum_wr2"], A21=sm["A21"], A=full(sm["A21"]), b=sm["b"], xi=np.zeros(6), pose=P.copy(),
                   mag=sm["mag"])
        log.append(rec)
        return rec

    for l, (stride, iters) in enumerate(levels):
        for _ in range(iters):
            rec = evaluate(l, stride)
            if rec["n_valid"] < p["min_valid"]:
                status, stop = TOO_FEW, True
                break
            xi = solve(rec["A21"], rec["b"], p["damping"])
            if xi is None:
                status, stop = SINGULAR, True
                break
            rec["xi"] = xi
            P = update(P, xi)
            if np.linalg.norm(xi[:3]) < F(p["eps_t"]) and np.linalg.norm(xi[3:]) < F(p["eps_r"]):
                if l == len(levels) - 1:
                    status = CONVERGED
                break
        if stop:
            break
    if not stop:
        rec = evaluate(len(levels) - 1, levels[-1][0])
        if rec["n_valid"] < p["min_valid"]:
            status = TOO_FEW
    first, last = log[0], log[-1]
    rms = lambda r: F(math.sqrt(r["sum_r2"] / r["n_valid"])) if r["n_valid"] > 0 else F(0)
    res = dict(status=status, evaluations=len(log), n_sampled=last["n_sampled"], n_valid_first=first["n_valid"],
               n_valid_last=last["n_valid"], rms_first=rms(first), rms_last=rms(last), pose=P.astype(np.float32))
    return res, log


def pose_distance(a, b):
    """(translation distance, rotation angle in radians) between two 3 x 4 poses"""
    a, b = np.asarray(a, np.float64).reshape(3, 4), np.asarray(b, np.float64).reshape(3, 4)
    R = a[:, :3] @ b[:, :3].T
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])  # sin(angle) * axis
    return float(np.linalg.norm(a[:, 3] - b[:, 3])), float(math.atan2(np.linalg.norm(v), (np.trace(R) - 1) / 2))
