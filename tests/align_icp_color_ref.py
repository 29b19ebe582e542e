"""numpy restatement of tf_align_icp_color.hip (a helper of the colour-ICP tests, not a test module).

model_maps() restates k_cicp_lum and k_cicp_grad, rows() the photometric row on top of align_icp_ref.rows (or, with a gate,
align_icp_gate_ref.rows: r, assoc, bits 0 to 5, s, g and q are those functions', untouched), both in float32, operation for
operation (the library is built with -ffp-contract=off): the device's maps are reproduced bit for bit.  sums() gives
align_ref.sums of the two rows (exact sums with their error bounds).  align() goes further than the other restatements: its
sums are taken in the device's own order (device_sums: the tile's tree of tf_align_tree.h, the workgroup's eight tiles in
wave order, the solve launch's eight groups of tf_align_rows.h), its step is tf_align_solve.h's Cholesky solve and pose
update operation for operation in f64, so that pose and log can be compared bit for bit -- as far as sin() of the two
mathematical libraries agrees.
"""
import math

import numpy as np

from tests import align_color_ref as CR
from tests import align_icp_gate_ref as G
from tests import align_icp_ref as K
from tests import align_ref as R

F = np.float32
NAN = np.frombuffer(np.uint32(0x7FC00000).tobytes(), np.float32)[0]  # what a gradient that does not exist is stored as

DEFAULTS = dict(K.DEFAULTS, photo_weight=0.1, max_photo_residual=0.25, huber_photo=0.05, max_depth_jump=0.1)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def model_maps(ref, Vm, Nm, model_pose, cam, p):
    """The model maps of a call -> dict(L, Gu, Gv, Z [H, W] f32) as tf_align_icp_color_model_maps writes the first three;
    ref: the volume (raycast_ref.RefVolume) the intensity is sampled from, None: a volume without colour."""
    H, W = cam.height, cam.width
    Vm = np.asarray(Vm, np.float32).reshape(3, H * W)
    Nm = np.asarray(Nm, np.float32).reshape(3, H * W)
    M = np.asarray(model_pose, np.float32).reshape(3, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        hit = (Nm[0] * Nm[0] + Nm[1] * Nm[1]) + Nm[2] * Nm[2] > F(0.5)
        d = [Vm[r] - M[r, 3] for r in range(3)]
        Z = ((M[0, 2] * d[0] + M[1, 2] * d[1]) + M[2, 2] * d[2]).astype(np.float32)
        L = np.full(H * W, F(-1), np.float32)
        if ref is not None and hit.any():
            pts = np.ascontiguousarray(Vm[:, hit].T)
            _, _, lum, okl = CR.trilinear_lum(ref, pts)
            L[hit] = np.where(okl, lum, F(-1))
        L, Z = L.reshape(H, W), Z.reshape(H, W)
        mj = F(p["max_depth_jump"])

        def diff(axis):
            g = np.full((H, W), NAN, np.float32)
            lo = [slice(None), slice(None)]
            hi = [slice(None), slice(None)]
            mid = [slice(None), slice(None)]
            lo[axis], hi[axis], mid[axis] = slice(0, -2), slice(2, None), slice(1, -1)
            lo, hi, mid = tuple(lo), tuple(hi), tuple(mid)
            ok = (L[lo] >= 0) & (L[hi] >= 0) & (np.abs(Z[lo] - Z[mid]) <= mj) & (np.abs(Z[hi] - Z[mid]) <= mj)
            g[mid] = np.where(ok, (L[hi] - L[lo]) * F(0.5), NAN)
            return g

        return dict(L=L, Gu=diff(1), Gv=diff(0), Z=Z)


def rows(maps, depth, rgba, pose, Vm, Nm, model_pose, cam, stride, p, gate=None):
    """One evaluation's rows at the sampled pixels; maps: model_maps' dict.  Returns the geometric rows' dict (align_icp_ref.rows',
    or align_icp_gate_ref.rows' where gate is given) with flags carrying bits 8 and 9, the maps rc [H, W] and gradc [3, H, W],
    and per sampled pixel sc (= rc), gc [n, 3], flc (15 where bit 9 is set, else 0: what the photometric sums take)."""
    H, W = cam.height, cam.width
    geo = K.rows(depth, pose, Vm, Nm, model_pose, cam, stride, p) if gate is None else \
        G.rows(depth, pose, Vm, Nm, model_pose, cam, stride, p, gate)
    rgba = np.asarray(rgba, np.uint8).reshape(H, W, 4)
    depth = np.asarray(depth, np.float32).reshape(H, W)
    P = np.asarray(pose, np.float32).reshape(3, 4)
    M = np.asarray(model_pose, np.float32).reshape(3, 4)
    fxi, fyi, cxs, cys = F(int(cam.fx)), F(int(cam.fy)), F(int(cam.cx)) + F(0.5), F(int(cam.cy)) + F(0.5)
    ys, xs = np.arange(0, H, stride), np.arange(0, W, stride)
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    yy, xx = yy.reshape(-1), xx.reshape(-1)
    z = depth[yy, xx]
    px = rgba[yy, xx].astype(np.float32)
    full = geo["fl63"] if gate is not None else geo["fl"]  # bits 0 to 3 (to 5 with the gate) per sampled pixel
    gvalid = full == (63 if gate is not None else 15)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        zz = np.where((full & 1) != 0, z, F(1))
        dcx = (xx.astype(np.float32) - cxs) / fxi
        dcy = (yy.astype(np.float32) - cys) / fyi
        pcx, pcy = dcx * zz, dcy * zz
        q = np.stack([(P[r, 0] * pcx + P[r, 1] * pcy) + P[r, 2] * zz for r in range(3)], 1)
        pw = np.stack([P[r, 3] + q[:, r] for r in range(3)], 1)
        d = np.stack([pw[:, r] - M[r, 3] for r in range(3)], 1)
        pm = np.stack([(M[0, c] * d[:, 0] + M[1, c] * d[:, 1]) + M[2, c] * d[:, 2] for c in range(3)], 1)
        mx, my, mz = pm[:, 0], pm[:, 1], pm[:, 2]
        uc, vc = (fxi * mx) / mz + cxs, (fyi * my) / mz + cys
        uf, vf = np.floor(uc + F(0.5)), np.floor(vc + F(0.5))
        am = geo["assoc"][yy, xx]
        i = np.maximum(am, 0)
        l, gu, gv = (maps[k].reshape(-1)[i] for k in ("L", "Gu", "Gv"))
        usable = (am >= 0) & (l >= 0) & ~np.isnan(gu) & ~np.isnan(gv)
        b8 = gvalid & (px[:, 3] != 0) & usable
        lf = CR.luma(px[:, 0], px[:, 1], px[:, 2]) * CR.INV255
        du, dv = uc - uf, vc - vf
        rc = (l + (gu * du + gv * dv)) - lf
        a, b = (fxi * gu) / mz, (fyi * gv) / mz
        c = -((a * mx + b * my) / mz)
        gc = np.stack([(M[r, 0] * a + M[r, 1] * b) + M[r, 2] * c for r in range(3)], 1)
        b9 = b8 & (np.abs(rc) <= F(p["max_photo_residual"]))
    rc = np.where(b8, rc, F(0)).astype(np.float32)
    gc = np.where(b8[:, None], gc, F(0)).astype(np.float32)
    out = dict(geo)
    fm = geo["flags"].copy()
    fm[yy, xx] = fm[yy, xx] + (b8 * 256 + b9 * 512).astype(np.uint32)
    rcm = np.zeros((H, W), np.float32)
    rcm[yy, xx] = rc
    gcm = np.zeros((3, H, W), np.float32)
    for k in range(3):
        gcm[k, yy, xx] = gc[:, k]
    out.update(flags=fm, rc=rcm, gradc=gcm, sc=rc, gc=gc, flc=np.where(b9, 15, 0).astype(np.uint32))
    return out


def sums(rw, p):
    """(geometric sums, photometric sums) of one evaluation, each as align_ref.sums returns them"""
    geo = R.sums(rw, p)
    pho = R.sums(dict(fl=rw["flc"], g=rw["gc"], q=rw["q"], s=rw["sc"]), dict(huber=p["huber_photo"]))
    return geo, pho


def _row_terms(g, q, r, valid, huber):
    """the 29 f64 terms of every sampled pixel's row, [n, 29], zero where the pixel is not valid (al_row_sums, al_tile_sum)"""
    J = np.concatenate([g, np.stack([q[:, 1] * g[:, 2] - q[:, 2] * g[:, 1], q[:, 2] * g[:, 0] - q[:, 0] * g[:, 2],
                                     q[:, 0] * g[:, 1] - q[:, 1] * g[:, 0]], 1)], 1).astype(np.float32)
    ar = np.abs(r)
    hub = F(huber)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where((hub == 0) | (ar <= hub), F(1), hub / ar).astype(np.float32)
    w = np.where(valid, w, F(0))
    r = np.where(valid, r, F(0)).astype(np.float32)
    J = np.where(valid[:, None], J, F(0)).astype(np.float32)
    wJ, wr = (w[:, None] * J).astype(np.float32), (w * r).astype(np.float32)
    J64, wJ64, r64 = J.astype(np.float64), wJ.astype(np.float64), r.astype(np.float64)
    cols = [wJ64[:, i] * J64[:, j] for i, j in zip(*R.IU)] + [wJ64[:, i] * r64 for i in range(6)]
    cols += [r64 * r64, wr.astype(np.float64) * r64]
    return np.stack(cols, 1)


def device_sums(terms, cam, stride):
    """The sums of [n, k] per-pixel f64 terms (row-major over the sampled grid) in the device's order -> [k]"""
    ny, nx = -(-cam.height // stride), -(-cam.width // stride)
    tx, ty = (nx + 7) // 8, (ny + 7) // 8
    k = terms.shape[1]
    grid = np.zeros((ty * 8, tx * 8, k))
    grid[:ny, :nx] = terms.reshape(ny, nx, k)
    # lane = 8 y + x inside a tile, tile = ty_ * tx + tx_
    t = grid.reshape(ty, 8, tx, 8, k).transpose(0, 2, 1, 3, 4).reshape(ty * tx, 64, k)
    n = 64
    while n > 1:  # the tree: xor 32, 16, 8, 4, 2, 1
        t = t[:, :n // 2] + t[:, n // 2:n]
        n //= 2
    tiles = t[:, 0]
    n_rows = (len(tiles) + 7) // 8
    tiles = np.concatenate([tiles, np.zeros((n_rows * 8 - len(tiles), k))]).reshape(n_rows, 8, k)
    rows_ = tiles[:, 0].copy()
    for w in range(1, 8):  # al_store_rows
        rows_ = rows_ + tiles[:, w]
    red = np.zeros((8, k))
    for tt in range(n_rows):  # al_add_rows
        red[tt % 8] = red[tt % 8] + rows_[tt]
    tot = red[0].copy()
    for g in range(1, 8):  # al_total
        tot = tot + red[g]
    return tot


def solve_exact(A21, b, damping):
    """align_solve6 of tf_align_solve.h in Python floats, operation for operation; None where a pivot fails"""
    A = R.full(np.asarray(A21, np.float64))
    M = [[float(A[i, j]) + float(damping) * float(A[i, j]) if i == j else float(A[i, j]) for j in range(6)] for i in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    dmax = 0.0
    for i in range(6):
        dmax = M[i][i] if M[i][i] > dmax else dmax
    thresh = 1e-12 * dmax
    for j in range(6):
        piv = M[j][j]
        for k in range(j):
            piv = piv - L[j][k] * L[j][k]
        if not piv > thresh:
            return None
        d = math.sqrt(piv)
        L[j][j] = d
        for i in range(j + 1, 6):
            sm = M[i][j]
            for k in range(j):
                sm = sm - L[i][k] * L[j][k]
            L[i][j] = sm / d
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        sm = float(b[i])
        for k in range(i):
            sm = sm - L[i][k] * y[k]
        y[i] = sm / L[i][i]
    for i in range(5, -1, -1):
        sm = y[i]
        for k in range(i + 1, 6):
            sm = sm - L[k][i] * x[k]
        x[i] = sm / L[i][i]
    return np.array([-v for v in x])


def update_exact(pose, xi):
    """align_update of tf_align_solve.h in Python floats, operation for operation"""
    w = [float(v) for v in xi[3:]]
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = math.sqrt(th2)
    a, b = 1.0, 0.5
    if th >= 1e-8:
        sh = math.sin(0.5 * th)
        a = math.sin(th) / th
        b = 2.0 * (sh * sh) / th2
    K = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    E = [0.0] * 9
    for i in range(3):
        for j in range(3):
            k2 = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j]
            E[3 * i + j] = ((1.0 if i == j else 0.0) + a * K[3 * i + j]) + b * k2
    P = [float(v) for v in np.asarray(pose, np.float64).reshape(12)]
    out = list(P)
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = (E[3 * i] * P[j] + E[3 * i + 1] * P[4 + j]) + E[3 * i + 2] * P[8 + j]
        out[4 * i + 3] = P[4 * i + 3] + float(xi[i])
    return np.array(out).reshape(3, 4)


def _device_eval_sums(rw, p, cam, stride):
    """both rows' sums in the device's order, as sums() returns them (mag: the exact sums')"""
    sg, sc = sums(rw, p)
    tg = device_sums(_row_terms(rw["g"], rw["q"], rw["s"], rw["fl"] == 15, p["huber"]), cam, stride)
    tc = device_sums(_row_terms(rw["gc"], rw["q"], rw["sc"], rw["flc"] == 15, p["huber_photo"]), cam, stride)
    for d, t in ((sg, tg), (sc, tc)):
        d.update(A21=t[:21], b=t[21:27], sum_r2=t[27], sum_wr2=t[28])
    return sg, sc


def align(ref, depth, rgba, pose, Vm, Nm, model_pose, cam, p, gate=None):
    """tf_align_frame_icp_color_device restated -> (result dict as Volume.align_frame_icp_color's, log as
    Volume.align_icp_color_log's)"""
    P = np.asarray(pose, np.float32).reshape(3, 4).astype(np.float64)
    l2 = float(F(p["photo_weight"])) * float(F(p["photo_weight"]))
    maps = model_maps(ref, Vm, Nm, model_pose, cam, p)
    log, status, stop = [], R.MAX_ITERS, False
    levels = p["levels"]

    def evaluate(level, stride):
        rw = rows(maps, depth, rgba, P.astype(np.float32), Vm, Nm, model_pose, cam, stride, p, gate)
        sg, sc = _device_eval_sums(rw, p, cam, stride)
        rec = dict(level=level, stride=stride, n_sampled=sg["n_sampled"], n_valid=sg["n_valid"], sum_r2=sg["sum_r2"],
                   sum_wr2=sg["sum_wr2"], A21=sg["A21"], A=R.full(sg["A21"]), b=sg["b"], xi=np.zeros(6), pose=P.copy(),
                   mag=sg["mag"], n_photo=sc["n_valid"], sum_rc2=sc["sum_r2"], sum_wrc2=sc["sum_wr2"], Ac21=sc["A21"],
                   Ac=R.full(sc["A21"]), bc=sc["b"], mag_c=sc["mag"])
        rec["M21"], rec["bM"] = rec["A21"] + l2 * rec["Ac21"], rec["b"] + l2 * rec["bc"]
        log.append(rec)
        return rec

    for l, (stride, iters) in enumerate(levels):
        for _ in range(iters):
            rec = evaluate(l, stride)
            if rec["n_valid"] < p["min_valid"]:
                status, stop = R.TOO_FEW, True
                break
            xi = solve_exact(rec["M21"], rec["bM"], p["damping"])
            if xi is None:
                status, stop = R.SINGULAR, True
                break
            rec["xi"] = xi
            P = update_exact(P, xi)
            if np.linalg.norm(xi[:3]) < F(p["eps_t"]) and np.linalg.norm(xi[3:]) < F(p["eps_r"]):
                if l == len(levels) - 1:
                    status = R.CONVERGED
                break
        if stop:
            break
    if not stop:
        rec = evaluate(len(levels) - 1, levels[-1][0])
        if rec["n_valid"] < p["min_valid"]:
            status = R.TOO_FEW
    first, last = log[0], log[-1]
    rms = lambda s2, n: F(math.sqrt(s2 / n)) if n > 0 else F(0)
    res = dict(status=status, evaluations=len(log), n_sampled=last["n_sampled"], n_valid_first=first["n_valid"],
               n_valid_last=last["n_valid"], rms_first=rms(first["sum_r2"], first["n_valid"]),
               rms_last=rms(last["sum_r2"], last["n_valid"]), pose=P.astype(np.float32), n_photo_first=first["n_photo"],
               n_photo_last=last["n_photo"], rms_photo_first=rms(first["sum_rc2"], first["n_photo"]),
               rms_photo_last=rms(last["sum_rc2"], last["n_photo"]))
    return res, log
