"""numpy restatement of tf_align_color.hip (a helper of the colour-aided alignment tests, not a test module).

The maps (r, grad, rc, gradc, flags) are computed in float32, operation for operation as k_calign_rows and
tri_sample_lum do (the library is built with -ffp-contract=off): the device's maps are reproduced bit for bit.  The
geometric and the photometric sums are align_ref.sums (math.fsum over the exact f64 terms) of the respective rows; the
solve and the loop are align_ref's with the joined system M = A_g + l2 A_c, b = b_g + l2 b_c.
"""
import math

import numpy as np

from tests import align_ref as R
from tests.raycast_ref import VOX_LIMIT, _floor_in, _tri8

F = np.float32
KR, KG, KB = F(0.299), F(0.587), F(0.114)
INV255 = F(1.0) / F(255.0)

DEFAULTS = dict(R.DEFAULTS, photo_weight=0.1, max_photo_residual=0.25, huber_photo=0.05)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def luma(r, g, b):
    return (KR * r + KG * g) + KB * b


def trilinear_lum(ref, p):
    """tri_sample_lum at the points p [n, 3] f32 -> (sdf [n], sdf valid [n], intensity [n], intensity valid [n]); the SDF
    and its validity are RefVolume.trilinear's"""
    ir = F(1) / ref.res
    n = len(p)
    g = [p[:, a] * ir - F(0.5) for a in range(3)]
    ok = np.ones(n, bool)
    i, f = [], []
    for a in range(3):
        ia, oka = _floor_in(g[a], VOX_LIMIT)
        ok &= oka
        i.append(ia)
        f.append(g[a] - np.floor(g[a]))
    c = np.zeros((8, n), np.float32)
    l = np.zeros((8, n), np.float32)
    okl = ok.copy()
    inr = ok.copy()
    for k in range(8):
        vx, vy, vz = i[0] + (k & 1), i[1] + ((k >> 1) & 1), i[2] + ((k >> 2) & 1)
        sl = np.where(inr, ref.slot(vx >> 3, vy >> 3, vz >> 3), -1)
        vi = ((vz & 7) * 8 + (vy & 7)) * 8 + (vx & 7)
        s0 = np.maximum(sl, 0)
        ok_k = sl >= 0
        c[k] = np.where(ok_k, ref.sdf[s0, vi], F(0))
        q = ref.col[s0, vi].astype(np.float32)
        has = ok_k & (ref.col[s0, vi, 3] > 0)
        cnt = np.where(has, q[:, 3], F(1))
        l[k] = np.where(has, luma(q[:, 0] / cnt, q[:, 1] / cnt, q[:, 2] / cnt), F(0))
        okl &= has
        ok &= ok_k & (ref.w[s0, vi] > F(0))
    sdf = np.where(ok, _tri8(c, *f), F(0))
    lum = np.where(okl, _tri8(l, *f) * INV255, F(0))
    return sdf.astype(np.float32), ok, lum.astype(np.float32), okl


def rows(ref, depth, rgba, pose, cam, stride, p):
    """One evaluation's rows at the sampled pixels.  Returns a dict: the maps r, rc [H, W] f32, grad, gradc [3, H, W] f32,
    flags [H, W] u32 as tf_align_color_residuals writes them, and per sampled pixel (row-major over the sampled grid) the
    arrays s, g [n, 3], sc (= rc), gc [n, 3], q [n, 3], fl."""
    H, W = cam.height, cam.width
    depth = np.asarray(depth, np.float32).reshape(H, W)
    rgba = np.asarray(rgba, np.uint8).reshape(H, W, 4)
    P = np.asarray(pose, np.float32).reshape(3, 4)
    res = ref.res
    fxi, fyi, cxs, cys = F(int(cam.fx)), F(int(cam.fy)), F(int(cam.cx)) + F(0.5), F(int(cam.cy)) + F(0.5)
    ys, xs = np.arange(0, H, stride), np.arange(0, W, stride)
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    yy, xx = yy.reshape(-1), xx.reshape(-1)
    z = depth[yy, xx]
    px = rgba[yy, xx].astype(np.float32)
    with np.errstate(invalid="ignore"):
        b0 = np.isfinite(z) & (z >= F(p["min_depth"])) & (z <= F(p["max_depth"]))
    zz = np.where(b0, z, F(1))
    dcx = (xx.astype(np.float32) - cxs) / fxi
    dcy = (yy.astype(np.float32) - cys) / fyi
    pcx, pcy = dcx * zz, dcy * zz
    q = np.stack([(P[r, 0] * pcx + P[r, 1] * pcy) + P[r, 2] * zz for r in range(3)], 1)
    pw = np.stack([P[r, 3] + q[:, r] for r in range(3)], 1)
    s, ok, lc, okl = trilinear_lum(ref, pw)
    b1 = b0 & ok
    taps_ok, taps_okl = np.ones(len(z), bool), np.ones(len(z), bool)
    n = len(z)
    sp, sm, lp, lm = (np.zeros((n, 3), np.float32) for _ in range(4))
    for ax in range(3):
        for sign, ds, dl in ((-1, sm, lm), (1, sp, lp)):
            pt = pw.copy()
            pt[:, ax] = pt[:, ax] + (res if sign > 0 else -res)
            t, okt, l, oklt = trilinear_lum(ref, pt)
            ds[:, ax], dl[:, ax] = t, l
            taps_ok &= okt
            taps_okl &= oklt
    b2 = b1 & taps_ok
    h2 = F(0.5) / res
    g = (sp - sm) * h2
    with np.errstate(invalid="ignore"):
        b3 = b2 & (np.abs(s) <= F(p["max_residual"]))
    b4 = b3 & (px[:, 3] != 0) & okl
    lf = luma(px[:, 0], px[:, 1], px[:, 2]) * INV255
    rc = lc - lf
    b5 = b4 & taps_okl
    gc = (lp - lm) * h2
    b6 = b5 & (np.abs(rc) <= F(p["max_photo_residual"]))
    fl = (b0 * 1 + b1 * 2 + b2 * 4 + b3 * 8 + b4 * 16 + b5 * 32 + b6 * 64).astype(np.uint32)
    s = np.where(b1, s, F(0)).astype(np.float32)
    g = np.where(b2[:, None], g, F(0)).astype(np.float32)
    rc = np.where(b4, rc, F(0)).astype(np.float32)
    gc = np.where(b5[:, None], gc, F(0)).astype(np.float32)
    out = dict(s=s, g=g, sc=rc, gc=gc, q=q.astype(np.float32), fl=fl)
    for name, val in (("r", s), ("rc", rc)):
        m = np.zeros((H, W), np.float32)
        m[yy, xx] = val
        out[name] = m
    for name, val in (("grad", g), ("gradc", gc)):
        m = np.zeros((3, H, W), np.float32)
        for a in range(3):
            m[a, yy, xx] = val[:, a]
        out[name] = m
    fm = np.zeros((H, W), np.uint32)
    fm[yy, xx] = fl
    out["flags"] = fm
    return out


def sums(rw, p):
    """(geometric sums, photometric sums) of one evaluation, each as align_ref.sums returns them; the photometric ones run
    over the pixels with flags == 127, with rc, gc and huber_photo in the places of s, g and huber"""
    geo = R.sums(dict(fl=rw["fl"] & np.uint32(15), g=rw["g"], q=rw["q"], s=rw["s"]), p)
    pho = R.sums(dict(fl=np.where(rw["fl"] == 127, 15, 0), g=rw["gc"], q=rw["q"], s=rw["sc"]), dict(huber=p["huber_photo"]))
    return geo, pho


def align(ref, depth, rgba, pose, cam, p):
    """tf_align_frame_color restated -> (result dict as Volume.align_frame_color's, log as Volume.align_color_log's)"""
    P = np.asarray(pose, np.float32).reshape(3, 4).astype(np.float64)
    l2 = float(F(p["photo_weight"])) * float(F(p["photo_weight"]))
    log, status, stop = [], R.MAX_ITERS, False
    levels = p["levels"]

    def evaluate(level, stride):
        rw = rows(ref, depth, rgba, P.astype(np.float32), cam, stride, p)
        sg, sc = sums(rw, p)
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
            xi = R.solve(rec["M21"], rec["bM"], p["damping"])
            if xi is None:
                status, stop = R.SINGULAR, True
                break
            rec["xi"] = xi
            P = R.update(P, xi)
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
