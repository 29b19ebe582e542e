"""numpy restatement of tf_align_group.hip on top of tests/align_ref.py (a helper of the group alignment tests, not a test
module).

A frame's rows are align_ref.rows' -- the device's per-pixel text is k_align_rows'.  What differs is the lever of the
rotational part of the Jacobian: the twist of a body is taken about its anchor's camera centre (the anchor is the body's
first frame), so a later frame k uses a = (t_k - t_anchor) + q componentwise in f32, from the f32 poses the rows are
sampled at, in place of q.  A body's sums are math.fsum over the exact f64 terms of all its frames (the device adds each
frame's sums as tf_align_frame does and then the frames in ascending order: an f64 sum of the same terms in another order).
A step moves every frame of the body by the same rigid motion about the anchor's centre c of before the step:
R_k <- E R_k, t_k <- (c + E (t_k - c)) + v, in f64.  Bodies do not interact, so each is run on its own.
"""
import math

import numpy as np

from tests import align_ref as R

F = np.float32


def lever(rw, pose_k, pose_a, is_anchor):
    """the rows of frame k with q replaced by the body's lever (the anchor keeps q)"""
    if is_anchor:
        return rw
    tk, ta = np.asarray(pose_k, np.float32).reshape(3, 4)[:, 3], np.asarray(pose_a, np.float32).reshape(3, 4)[:, 3]
    out = dict(rw)
    out["q"] = ((tk - ta).astype(np.float32)[None, :] + rw["q"]).astype(np.float32)
    return out


def body_rows(ref, depths, poses32, cam, stride, p):
    """the rows of a body's frames at their f32 poses, levers applied, as one set: s, g, q (the lever), fl concatenated in
    frame order; per_frame = the valid count of each frame"""
    rws = [lever(R.rows(ref, d, P, cam, stride, p), P, poses32[0], k == 0) for k, (d, P) in enumerate(zip(depths, poses32))]
    out = {key: np.concatenate([rw[key] for rw in rws]) for key in ("s", "g", "q", "fl")}
    out["per_frame"] = [int((rw["fl"] == 15).sum()) for rw in rws]
    return out


def update_about(P, E, c, v):
    """one frame [R | t] (f64 3 x 4) moved by the twist (v, E) about the centre c"""
    Q = np.array(P, np.float64).reshape(3, 4)
    Q[:, :3] = E @ Q[:, :3]
    Q[:, 3] = (c + E @ (Q[:, 3] - c)) + v
    return Q


def align_body(ref, depths, poses, cam, p):
    """one rigid body (frame 0 is its anchor) -> (result dict as align_ref.align's with pose = the anchor's, log, the frames'
    end poses [n, 3, 4] f64, frame_valid_first, frame_valid_last)"""
    Ps = [np.asarray(P, np.float32).reshape(3, 4).astype(np.float64) for P in poses]
    log, status, stop = [], R.MAX_ITERS, False
    levels = p["levels"]
    fv = []

    def evaluate(level, stride):
        rw = body_rows(ref, depths, [P.astype(np.float32) for P in Ps], cam, stride, p)
        sm = R.sums(rw, p)
        rec = dict(level=level, stride=stride, n_sampled=sm["n_sampled"], n_valid=sm["n_valid"], sum_r2=sm["sum_r2"],
                   sum_wr2=sm["sum_wr2"], A21=sm["A21"], A=R.full(sm["A21"]), b=sm["b"], xi=np.zeros(6), pose=Ps[0].copy(),
                   mag=sm["mag"])
        log.append(rec)
        fv.append(rw["per_frame"])
        return rec

    for l, (stride, iters) in enumerate(levels):
        for _ in range(iters):
            rec = evaluate(l, stride)
            if rec["n_valid"] < p["min_valid"]:
                status, stop = R.TOO_FEW, True
                break
            xi = R.solve(rec["A21"], rec["b"], p["damping"])
            if xi is None:
                status, stop = R.SINGULAR, True
                break
            rec["xi"] = xi
            E, c = R.rodrigues(xi[3:]), Ps[0][:, 3].copy()
            Ps = [update_about(P, E, c, xi[:3]) for P in Ps]
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
    rms = lambda r: F(math.sqrt(r["sum_r2"] / r["n_valid"])) if r["n_valid"] > 0 else F(0)
    res = dict(status=status, evaluations=len(log), n_sampled=last["n_sampled"], n_valid_first=first["n_valid"],
               n_valid_last=last["n_valid"], rms_first=rms(first), rms_last=rms(last), pose=Ps[0].astype(np.float32))
    return res, log, np.stack(Ps), fv[0], fv[-1]


def align_group(ref, depths, poses, cam, p, body=None):
    """tf_align_group restated -> dict(n_frames, n_bodies, body = [result dict per body], log = [log per body],
    pose [n, 3, 4] f32, pose64 (the f64 poses behind it), frame_valid_first, frame_valid_last [n])"""
    n = len(depths)
    body = [0] * n if body is None else [int(b) for b in body]
    assert len(poses) == n == len(body) and 1 <= n <= 7 and body[0] == 0
    assert all(body[k] <= 1 + max(body[:k]) for k in range(1, n))
    nb = max(body) + 1
    out = dict(n_frames=n, n_bodies=nb, body=[], log=[], pose64=np.zeros((n, 3, 4)), frame_valid_first=np.zeros(n, np.int32),
               frame_valid_last=np.zeros(n, np.int32))
    for b in range(nb):
        ks = [k for k in range(n) if body[k] == b]
        res, log, Ps, f0, f1 = align_body(ref, [depths[k] for k in ks], [poses[k] for k in ks], cam, p)
        out["body"].append(res)
        out["log"].append(log)
        for i, k in enumerate(ks):
            out["pose64"][k], out["frame_valid_first"][k], out["frame_valid_last"][k] = Ps[i], f0[i], f1[i]
    out["pose"] = out["pose64"].astype(np.float32)
    return out


def group_distance(a, b):
    """the largest (translation, rotation) distance between corresponding frames of two pose sets"""
    d = [R.pose_distance(x, y) for x, y in zip(a, b)]
    return max(x[0] for x in d), max(x[1] for x in d)
