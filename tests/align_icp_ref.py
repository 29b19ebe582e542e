"""numpy restatement of tf_align_icp.hip (a helper of the projective-ICP tests, not a test module).

rows() restates k_icp_rows in float32, operation for operation (the library is built with -ffp-contract=off): the
device's r, flags and assoc maps are reproduced bit for bit.  The sums, the solve and the pose update are align_ref's
(its sums() takes the rows' s, g, q and fl: here s = r and g = the model normal).  The level loop is align_ref.align's,
restated here only because that one calls its own rows().
"""
import math

import numpy as np

from tests.align_ref import CONVERGED, MAX_ITERS, SINGULAR, TOO_FEW, F, full, solve, sums, update  # noqa: F401

DEFAULTS = dict(levels=[(4, 6), (2, 4), (1, 3)], min_depth=0.05, max_depth=5.0, max_residual=0.15, max_distance=0.15,
                huber=0.02, damping=0.0, eps_t=1e-5, eps_r=1e-5, min_valid=100)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def rows(depth, pose, Vm, Nm, model_pose, cam, stride, p):
    """One evaluation's rows at the sampled pixels.  Vm, Nm: f32 [3, H, W] world-frame model maps rendered from model_pose
    with the same camera.  Returns maps r [H, W] f32, flags [H, W] u32, assoc [H, W] i32 as tf_align_icp_residuals writes
    them, and per sampled pixel (row-major over the sampled grid) s (= r), g (= the model normal) [n, 3], q [n, 3], fl."""
    H, W = cam.height, cam.width
    depth = np.asarray(depth, np.float32).reshape(H, W)
    P = np.asarray(pose, np.float32).reshape(3, 4)
    M = np.asarray(model_pose, np.float32).reshape(3, 4)
    Vm = np.asarray(Vm, np.float32).reshape(3, H * W)
    Nm = np.asarray(Nm, np.float32).reshape(3, H * W)
    fxi, fyi, cxs, cys = F(int(cam.fx)), F(int(cam.fy)), F(int(cam.cx)) + F(0.5), F(int(cam.cy)) + F(0.5)
    ys, xs = np.arange(0, H, stride), np.arange(0, W, stride)
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    yy, xx = yy.reshape(-1), xx.reshape(-1)
    z = depth[yy, xx]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        b0 = np.isfinite(z) & (z >= F(p["min_depth"])) & (z <= F(p["max_depth"]))
        zz = np.where(b0, z, F(1))
        dcx = (xx.astype(np.float32) - cxs) / fxi
        dcy = (yy.astype(np.float32) - cys) / fyi
        pcx, pcy = dcx * zz, dcy * zz
        q = np.stack([(P[r, 0] * pcx + P[r, 1] * pcy) + P[r, 2] * zz for r in range(3)], 1)
        pw = np.stack([P[r, 3] + q[:, r] for r in range(3)], 1)
        d = np.stack([pw[:, r] - M[r, 3] for r in range(3)], 1)
        pm = np.stack([(M[0, c] * d[:, 0] + M[1, c] * d[:, 1]) + M[2, c] * d[:, 2] for c in range(3)], 1)
        uf = np.floor(((fxi * pm[:, 0]) / pm[:, 2] + cxs) + F(0.5))
        vf = np.floor(((fyi * pm[:, 1]) / pm[:, 2] + cys) + F(0.5))
        b1 = b0 & (pm[:, 2] > F(p["min_depth"])) & (uf >= 0) & (uf < F(W)) & (vf >= 0) & (vf < F(H))
        idx = np.where(b1, vf.astype(np.float64) * W + uf.astype(np.float64), 0)
        idx = np.where(b1, idx, 0).astype(np.int64)
        vm, nm = Vm[:, idx].T, Nm[:, idx].T
        b2 = b1 & ((nm[:, 0] * nm[:, 0] + nm[:, 1] * nm[:, 1]) + nm[:, 2] * nm[:, 2] > F(0.5))
        e = pw - vm
        r = (nm[:, 0] * e[:, 0] + nm[:, 1] * e[:, 1]) + nm[:, 2] * e[:, 2]
        ee = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        md = F(p["max_distance"])
        b3 = b2 & (ee <= md * md) & (np.abs(r) <= F(p["max_residual"]))
    fl = (b0 * 1 + b1 * 2 + b2 * 4 + b3 * 8).astype(np.uint32)
    r = np.where(b2, r, F(0)).astype(np.float32)
    g = np.where(b2[:, None], nm, F(0)).astype(np.float32)
    rm, fm, am = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint32), np.full((H, W), -1, np.int32)
    rm[yy, xx], fm[yy, xx], am[yy, xx] = r, fl, np.where(b1, idx, -1).astype(np.int32)
    return dict(r=rm, flags=fm, assoc=am, s=r, g=g, q=q.astype(np.float32), fl=fl)


def align(depth, pose, Vm, Nm, model_pose, cam, p):
    """tf_align_frame_icp_device restated -> (result dict as Volume.align_frame_icp's, log as Volume.align_icp_log's)"""
    P = np.asarray(pose, np.float32).reshape(3, 4).astype(np.float64)
    log, status, stop = [], MAX_ITERS, False
    levels = p["levels"]

    def evaluate(level, stride):
        sm = sums(rows(depth, P.astype(np.float32), Vm, Nm, model_pose, cam, stride, p), p)
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
