"""numpy restatement of tf_align_icp_gate.hip (a helper of the gated projective-ICP tests, not a test module).

frame_normals() restates the frame normal in float32, operation for operation; rows() puts flag bits 4 and 5 on top of
align_icp_ref.rows (r, assoc, bits 0 to 3, s, g and q are that function's, untouched); align() is align_icp_ref.align with
these rows.  A pixel is valid iff flags == 63, so the `fl` handed to align_ref.sums is 15 exactly there."""
import math

import numpy as np

from tests import align_icp_ref as K
from tests.align_ref import CONVERGED, MAX_ITERS, SINGULAR, TOO_FEW, F, full, solve, sums, update  # noqa: F401

COS20 = F(0.9396926)  # cosf(20 degrees)
GATE = dict(min_normal_cos=COS20, max_depth_jump=F(0.1))  # tf_align_icp_gate_default


def gate(**kw):
    g = dict(GATE)
    g.update(kw)
    return g


def _sampled(cam, stride):
    ys, xs = np.arange(0, cam.height, stride), np.arange(0, cam.width, stride)
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    return yy.reshape(-1), xx.reshape(-1)


def frame_normals(depth, cam, stride, p, g):
    """The frame normals at the sampled pixels -> dict(n [3, H, W] f32 as tf_align_icp_frame_normals writes it; per sampled
    pixel (row-major over the sampled grid) nrm [n, 3], l2 [n], ok [n])."""
    H, W, s = cam.height, cam.width, int(stride)
    depth = np.asarray(depth, np.float32).reshape(H, W)
    fxi, fyi, cxs, cys = F(int(cam.fx)), F(int(cam.fy)), F(int(cam.cx)) + F(0.5), F(int(cam.cy)) + F(0.5)
    lo, hi, mj = F(p["min_depth"]), F(p["max_depth"]), F(g["max_depth_jump"])
    yy, xx = _sampled(cam, s)
    in4 = (xx - s >= 0) & (xx + s < W) & (yy - s >= 0) & (yy + s < H)

    def tap(dy, dx):
        return depth[np.where(in4, yy + dy, yy), np.where(in4, xx + dx, xx)]

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        inr = lambda z: np.isfinite(z) & (z >= lo) & (z <= hi)
        z0, zl, zr, zu, zd = depth[yy, xx], tap(0, -s), tap(0, s), tap(-s, 0), tap(s, 0)
        ok = inr(z0) & in4
        for z in (zl, zr, zu, zd):
            ok = ok & inr(z) & (np.abs(z - z0) <= mj)
        dc = lambda v, c, f: (v.astype(np.float32) - c) / f
        dcx, dcy = dc(xx, cxs, fxi), dc(yy, cys, fyi)
        dcxl, dcxr, dcyu, dcyd = dc(xx - s, cxs, fxi), dc(xx + s, cxs, fxi), dc(yy - s, cys, fyi), dc(yy + s, cys, fyi)
        ax, ay, az = dcxr * zr - dcxl * zl, dcy * zr - dcy * zl, zr - zl
        bx, by, bz = dcx * zd - dcx * zu, dcyd * zd - dcyu * zu, zd - zu
        nx, ny, nz = by * az - bz * ay, bz * ax - bx * az, bx * ay - by * ax
        l2 = (nx * nx + ny * ny) + nz * nz
        ok = ok & np.isfinite(l2) & (l2 > 0)
    nrm = np.where(ok[:, None], np.stack([nx, ny, nz], 1), F(0)).astype(np.float32)
    l2 = np.where(ok, l2, F(0)).astype(np.float32)
    out = np.zeros((3, H, W), np.float32)
    out[:, yy, xx] = nrm.T
    return dict(n=out, nrm=nrm, l2=l2, ok=ok)


def rows(depth, pose, Vm, Nm, model_pose, cam, stride, p, g):
    """align_icp_ref.rows with the gate: flags with bits 4 and 5, fl = 15 exactly where flags == 63 (what the sums take),
    fl15 = the ungated bits 0 to 3 per sampled pixel; everything else as that function returns it."""
    rw = K.rows(depth, pose, Vm, Nm, model_pose, cam, stride, p)
    fn = frame_normals(depth, cam, stride, p, g)
    P = np.asarray(pose, np.float32).reshape(3, 4)
    n, nm = fn["nrm"], rw["g"]
    c2 = F(g["min_normal_cos"]) * F(g["min_normal_cos"])
    with np.errstate(invalid="ignore", over="ignore"):
        nw = np.stack([(P[r, 0] * n[:, 0] + P[r, 1] * n[:, 1]) + P[r, 2] * n[:, 2] for r in range(3)], 1)
        d = (nw[:, 0] * nm[:, 0] + nw[:, 1] * nm[:, 1]) + nw[:, 2] * nm[:, 2]
        m2 = (nm[:, 0] * nm[:, 0] + nm[:, 1] * nm[:, 1]) + nm[:, 2] * nm[:, 2]
        b4 = (rw["fl"] == 15) & fn["ok"]
        b5 = b4 & (d > 0) & (d * d >= (c2 * fn["l2"]) * m2)
    fl = (rw["fl"] + b4 * 16 + b5 * 32).astype(np.uint32)
    yy, xx = _sampled(cam, stride)
    fm = rw["flags"].copy()
    fm[yy, xx] = fl
    out = dict(rw)
    out.update(flags=fm, fl63=fl, fl15=rw["fl"], fl=np.where(fl == 63, 15, fl & 7).astype(np.uint32), d=d)
    return out


def align(depth, pose, Vm, Nm, model_pose, cam, p, g):
    """tf_align_frame_icp_device with the gate set, restated: align_icp_ref.align's loop over these rows"""
    P = np.asarray(pose, np.float32).reshape(3, 4).astype(np.float64)
    log, status, stop = [], MAX_ITERS, False
    levels = p["levels"]

    def evaluate(level, stride):
        sm = sums(rows(depth, P.astype(np.float32), Vm, Nm, model_pose, cam, stride, p, g), p)
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
