"""numpy restatement of tf_align_exposure.hip (a helper of the exposure-compensation tests, not a test module).

The rows are the two photometric aligners' own (align_color_ref.rows, align_icp_color_ref.rows: the model's side of rc is
taken from them with a black frame, whose luma is an exact zero) with the frame's luma compensated in float32, operation for
operation: Lfe = gain_f * Lf + offset_f, rc = L - Lfe.  All three rows' sums are taken in the device's order
(align_icp_color_ref.device_sums), the elimination of the pair, the 6 x 6 solve, the pose update and the pair's step in
Python floats, operation for operation as tf_align_exposure_solve.h and tf_align_solve.h have them, so that pose, pair and
both logs can be compared bit for bit.
"""
import math

import numpy as np

from tests import align_color_ref as CR
from tests import align_icp_color_ref as X
from tests import align_ref as R

F = np.float32
IU = R.IU

DEFAULT = dict(unknowns=2, carry=0, gain0=1.0, offset0=0.0, min_gain=0.25, max_gain=4.0)


def setting(**kw):
    e = dict(DEFAULT)
    e.update(kw)
    return e


def expose(rgba, gain, offset):
    """the frame as a camera at another exposure sees it: every colour channel rint(g * v + 255 * o) where alpha != 0"""
    out = np.asarray(rgba, np.uint8).copy()
    seen = out[..., 3] != 0
    v = np.rint(gain * out[..., :3].astype(np.float64) + 255.0 * offset)
    assert v[seen].min() >= 0 and v[seen].max() <= 255
    out[..., :3] = np.where(seen[..., None], v, out[..., :3]).astype(np.uint8)
    return out


def _black(rgba):
    out = np.asarray(rgba, np.uint8).copy()
    out[..., :3] = 0
    return out


def _sampled(rgba, cam, stride):
    H, W = cam.height, cam.width
    rgba = np.asarray(rgba, np.uint8).reshape(H, W, 4)
    ys, xs = np.arange(0, H, stride), np.arange(0, W, stride)
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    yy, xx = yy.reshape(-1), xx.reshape(-1)
    px = rgba[yy, xx].astype(np.float32)
    return yy, xx, (CR.luma(px[:, 0], px[:, 1], px[:, 2]) * CR.INV255).astype(np.float32)


def _compensate(lf, pair):
    """Lfe = gain_f * Lf + offset_f in f32, both operations rounded"""
    g, o = F(pair[0]), F(pair[1])
    return ((g * lf).astype(np.float32) + o).astype(np.float32)


def _spread(cam, yy, xx, val):
    m = np.zeros((cam.height, cam.width), val.dtype)
    m[yy, xx] = val
    return m


def rows_sdf(ref, depth, rgba, pose, cam, stride, p, pair):
    """tf_align_frame_color's rows with the pair (gain, offset) -> align_color_ref.rows' dict with rc, flags, sc and fl by the
    compensated residual, and lf (the uncompensated luma, per sampled pixel), gvalid, pvalid"""
    base = CR.rows(ref, depth, _black(rgba), pose, cam, stride, dict(p, max_photo_residual=np.inf))
    yy, xx, lf = _sampled(rgba, cam, stride)
    fl = base["fl"]
    b4, b5 = (fl & 16) != 0, (fl & 32) != 0
    rc = np.where(b4, base["sc"] - _compensate(lf, pair), F(0)).astype(np.float32)  # base["sc"] is L(pw) where bit 4 is set
    with np.errstate(invalid="ignore"):
        b6 = b5 & (np.abs(rc) <= F(p["max_photo_residual"]))
    fl = ((fl & np.uint32(63)) | (b6 * 64).astype(np.uint32)).astype(np.uint32)
    out = dict(base)
    out.update(fl=fl, sc=rc, lf=lf, rc=_spread(cam, yy, xx, rc), flags=_spread(cam, yy, xx, fl), gvalid=(fl & 15) == 15,
               pvalid=fl == 127)
    return out


def rows_icp(maps, depth, rgba, pose, Vm, Nm, model_pose, cam, stride, p, pair, gate=None):
    """tf_align_frame_icp_color's rows with the pair -> align_icp_color_ref.rows' dict the same way"""
    base = X.rows(maps, depth, _black(rgba), pose, Vm, Nm, model_pose, cam, stride, dict(p, max_photo_residual=np.inf), gate)
    yy, xx, lf = _sampled(rgba, cam, stride)
    fm = base["flags"][yy, xx]
    b8 = (fm & 256) != 0
    rc = np.where(b8, base["sc"] - _compensate(lf, pair), F(0)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        b9 = b8 & (np.abs(rc) <= F(p["max_photo_residual"]))
    fm = ((fm & np.uint32(511)) | (b9 * 512).astype(np.uint32)).astype(np.uint32)
    low = 63 if gate is not None else 15
    out = dict(base)
    out.update(sc=rc, lf=lf, rc=_spread(cam, yy, xx, rc), flags=_spread(cam, yy, xx, fm), gvalid=(fm & 255) == low, pvalid=b9,
               flc=np.where(b9, 15, 0).astype(np.uint32))
    return out


def exposure_terms(gc, q, rc, lf, valid, huber):
    """the 17 f64 terms of every sampled pixel's exposure row, [n, 17]: P[6] Q[6] S_w S_l S_ll S_r S_lr (al_exposure_row_sums)"""
    J = np.concatenate([gc, np.stack([q[:, 1] * gc[:, 2] - q[:, 2] * gc[:, 1], q[:, 2] * gc[:, 0] - q[:, 0] * gc[:, 2],
                                      q[:, 0] * gc[:, 1] - q[:, 1] * gc[:, 0]], 1)], 1).astype(np.float32)
    ar = np.abs(rc)
    hub = F(huber)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where((hub == 0) | (ar <= hub), F(1), hub / ar).astype(np.float32)
    w = np.where(valid, w, F(0)).astype(np.float32)
    rc = np.where(valid, rc, F(0)).astype(np.float32)
    lf = np.where(valid, lf, F(0)).astype(np.float32)
    J = np.where(valid[:, None], J, F(0)).astype(np.float32)
    wJ = (w[:, None] * J).astype(np.float32).astype(np.float64)
    wl = (w * lf).astype(np.float32).astype(np.float64)
    w64, lf64, rc64 = w.astype(np.float64), lf.astype(np.float64), rc.astype(np.float64)
    cols = [wJ[:, i] for i in range(6)] + [wJ[:, i] * lf64 for i in range(6)]
    cols += [w64, w64 * lf64, wl * lf64, w64 * rc64, wl * rc64]
    return np.stack(cols, 1)


def eval_sums(rw, p, cam, stride):
    """(geometric, photometric, exposure) sums of one evaluation in the device's order"""
    tg = X.device_sums(X._row_terms(rw["g"], rw["q"], rw["s"], rw["gvalid"], p["huber"]), cam, stride)
    tc = X.device_sums(X._row_terms(rw["gc"], rw["q"], rw["sc"], rw["pvalid"], p["huber_photo"]), cam, stride)
    te = X.device_sums(exposure_terms(rw["gc"], rw["q"], rw["sc"], rw["lf"], rw["pvalid"], p["huber_photo"]), cam, stride)
    geo = dict(A21=tg[:21], b=tg[21:27], sum_r2=tg[27], sum_wr2=tg[28], n_valid=int(rw["gvalid"].sum()), n_sampled=len(rw["gvalid"]))
    pho = dict(A21=tc[:21], b=tc[21:27], sum_r2=tc[27], sum_wr2=tc[28], n_valid=int(rw["pvalid"].sum()))
    return geo, pho, te


# ---- tf_align_exposure_solve.h in Python floats, operation for operation -------------------------------------------------
def eliminate(S, unknowns, Ac21, bc):
    """-> (Ac' [21], bc' [6], el): el = dict(rank, l00, l10, l11, Y [2][6], z [2])"""
    S = [float(v) for v in S]
    P, Q, sw, sl, sll, sr, slr = S[0:6], S[6:12], S[12], S[13], S[14], S[15], S[16]
    thresh = 1e-12 * (sw if sw > sll else sll)
    rank, l00, l10, l11 = 0, 1.0, 0.0, 1.0
    if unknowns >= 1 and sw > thresh:
        rank, l00 = 1, math.sqrt(sw)
    if unknowns == 2 and rank == 1:
        t10 = sl / l00
        p1 = sll - t10 * t10
        floor2 = sll / 8388608.0  # 2^-23 of S_ll: twice the f32 rounding of wl
        if p1 > (thresh if thresh > floor2 else floor2):
            rank, l10, l11 = 2, t10, math.sqrt(p1)
    z0 = sr / l00 if rank >= 1 else 0.0
    z1 = (slr - l10 * z0) / l11 if rank == 2 else 0.0
    Y0 = [P[i] / l00 if rank >= 1 else 0.0 for i in range(6)]
    Y1 = [(Q[i] - l10 * Y0[i]) / l11 if rank == 2 else 0.0 for i in range(6)]
    A = [float(v) for v in Ac21]
    b = [float(v) for v in bc]
    u = 0
    for i in range(6):
        for j in range(i, 6):
            A[u] = (A[u] - Y0[i] * Y0[j]) - Y1[i] * Y1[j]
            u += 1
        b[i] = (b[i] - Y0[i] * z0) - Y1[i] * z1
    return np.array(A), np.array(b), dict(rank=rank, l00=l00, l10=l10, l11=l11, Y=[Y0, Y1], z=[z0, z1])


def step(S, el, xi):
    """-> (d offset, d gain) for the twist xi"""
    S = [float(v) for v in S]
    t0, t1 = S[15], S[16]
    for i in range(6):
        t0 = t0 + S[i] * float(xi[i])
        t1 = t1 + S[6 + i] * float(xi[i])
    if el["rank"] == 2:
        u0 = t0 / el["l00"]
        u1 = (t1 - el["l10"] * u0) / el["l11"]
        d1 = u1 / el["l11"]
        return (u0 - el["l10"] * d1) / el["l00"], d1
    if el["rank"] == 1:
        return (t0 / el["l00"]) / el["l00"], 0.0
    return 0.0, 0.0


def apply(pair, rank, de, min_gain, max_gain):
    """pair = (gain, offset) -> the pair after the step; min_gain, max_gain: f64 (the device's are the setting's f32 widened)"""
    g, o = float(pair[0]), float(pair[1])
    if rank >= 1:
        o = o + de[0]
    if rank == 2:
        g = g + de[1]
        lo = g if g > min_gain else min_gain
        g = lo if lo < max_gain else max_gain
    return g, o


def solve_joint(geo, pho, S, l2, damping):
    """the full 8 x 8 Gauss-Newton system in (xi, offset, gain) solved directly (numpy.linalg.solve) -> (xi, d offset, d gain);
    what the eliminated step must equal"""
    A, Ac = R.full(np.asarray(geo["A21"])), R.full(np.asarray(pho["A21"]))
    S = np.asarray(S, np.float64)
    Cm = np.stack([S[0:6], S[6:12]], 1)
    Fm = np.array([[S[12], S[13]], [S[13], S[14]]])
    h = np.array([S[15], S[16]])
    M = np.zeros((8, 8))
    M[:6, :6] = A + l2 * Ac
    M[:6, 6:] = -l2 * Cm
    M[6:, :6] = -l2 * Cm.T
    M[6:, 6:] = l2 * Fm
    M[np.arange(6), np.arange(6)] *= 1.0 + damping
    rhs = -np.concatenate([np.asarray(geo["b"]) + l2 * np.asarray(pho["b"]), -l2 * h])
    x = np.linalg.solve(M, rhs)
    return x[:6], x[6], x[7]


# ---- the loop ------------------------------------------------------------------------------------------------------------
def _align(rows_at, cam, p, e, pose, pair):
    """rows_at(P32, stride, pair) -> rows.  Returns (result, colour log, exposure log, final pair)"""
    P = np.asarray(pose, np.float32).reshape(3, 4).astype(np.float64)
    pair = (float(pair[0]), float(pair[1]))
    l2 = float(F(p["photo_weight"])) * float(F(p["photo_weight"]))
    log, xlog, status, stop = [], [], R.MAX_ITERS, False
    levels = p["levels"]

    def evaluate(level, stride):
        rw = rows_at(P.astype(np.float32), stride, (F(pair[0]), F(pair[1])))
        sg, sc, S = eval_sums(rw, p, cam, stride)
        A2, b2, el = eliminate(S, e["unknowns"], sc["A21"], sc["b"])
        rec = dict(level=level, stride=stride, n_sampled=sg["n_sampled"], n_valid=sg["n_valid"], sum_r2=sg["sum_r2"],
                   sum_wr2=sg["sum_wr2"], A21=sg["A21"], A=R.full(sg["A21"]), b=sg["b"], xi=np.zeros(6), pose=P.copy(),
                   n_photo=sc["n_valid"], sum_rc2=sc["sum_r2"], sum_wrc2=sc["sum_wr2"], Ac21=sc["A21"], Ac=R.full(sc["A21"]),
                   bc=sc["b"])
        rec["M21"], rec["bM"] = rec["A21"] + l2 * A2, rec["b"] + l2 * b2
        log.append(rec)
        xlog.append(dict(gain=pair[0], offset=pair[1], rank=el["rank"], n_photo=sc["n_valid"], S=np.array(S), d_offset=0.0,
                         d_gain=0.0, el=el))
        return rec, xlog[-1]

    for l, (stride, iters) in enumerate(levels):
        for _ in range(iters):
            rec, xr = evaluate(l, stride)
            if rec["n_valid"] < p["min_valid"]:
                status, stop = R.TOO_FEW, True
                break
            xi = X.solve_exact(rec["M21"], rec["bM"], p["damping"])
            if xi is None:
                status, stop = R.SINGULAR, True
                break
            rec["xi"] = xi
            P = X.update_exact(P, xi)
            de = step(xr["S"], xr["el"], xi)
            pair = apply(pair, xr["rank"], de, float(F(e["min_gain"])), float(F(e["max_gain"])))
            xr["d_offset"], xr["d_gain"] = de
            if np.linalg.norm(xi[:3]) < F(p["eps_t"]) and np.linalg.norm(xi[3:]) < F(p["eps_r"]):
                if l == len(levels) - 1:
                    status = R.CONVERGED
                break
        if stop:
            break
    if not stop:
        rec, _ = evaluate(len(levels) - 1, levels[-1][0])
        if rec["n_valid"] < p["min_valid"]:
            status = R.TOO_FEW
    first, last = log[0], log[-1]
    rms = lambda s2, n: F(math.sqrt(s2 / n)) if n > 0 else F(0)
    res = dict(status=status, evaluations=len(log), n_sampled=last["n_sampled"], n_valid_first=first["n_valid"],
               n_valid_last=last["n_valid"], rms_first=rms(first["sum_r2"], first["n_valid"]),
               rms_last=rms(last["sum_r2"], last["n_valid"]), pose=P.astype(np.float32), n_photo_first=first["n_photo"],
               n_photo_last=last["n_photo"], rms_photo_first=rms(first["sum_rc2"], first["n_photo"]),
               rms_photo_last=rms(last["sum_rc2"], last["n_photo"]))
    return res, log, xlog, pair


def start_pair(e, pair=None):
    """the cell after tf_align_set_exposure(e): (gain0, offset0) as f32 values"""
    return (float(F(e["gain0"])), float(F(e["offset0"]))) if pair is None else pair


def align_sdf(ref, depth, rgba, pose, cam, p, e, pair=None):
    """tf_align_frame_color with the setting e on, from the cell's pair (None: the setting's start pair)"""
    return _align(lambda P32, stride, pr: rows_sdf(ref, depth, rgba, P32, cam, stride, p, pr), cam, p, e, pose, start_pair(e, pair))


def align_icp(ref, depth, rgba, pose, Vm, Nm, model_pose, cam, p, e, pair=None):
    """tf_align_frame_icp_color_device with the setting e on"""
    maps = X.model_maps(ref, Vm, Nm, model_pose, cam, p)
    return _align(lambda P32, stride, pr: rows_icp(maps, depth, rgba, P32, Vm, Nm, model_pose, cam, stride, p, pr), cam, p, e,
                  pose, start_pair(e, pair))
