"""The chunk selection (K-B + K-C: tfo_bbox + tfo_select of oracle/tf_oracle.c) restated in numpy float32, one operation
per rounding, with switchable mistakes.  It does NOT replace the oracle as the device's reference: it exists so that
tests/test_select_cpu.py can prove that each hand-built case of tests/select_inputs.py hinges on the decision it is named
after -- the unmutated restatement equals the oracle in ids, order and n_coarse, and the mutant a case names gives another
list or another n_coarse on that case.

What makes it bit-equal: every product and sum is a float32 array operation of its own (numpy neither fuses nor reorders
them), the three-term products accumulate sequentially (dot3_seq), and the truncation distance is evaluated in double
exactly as tfo_truncation does.  All coarse blocks are probed at once as arrays, then all chunks of the hit blocks; the
order of the list is the reference's push_back order (x, y, z outer to inner over blocks, then i, j, k inside a block).

The mutants (select(..., mutant=name)); each changes exactly one decision:

  trunc              pixel by truncation instead of round-to-nearest-even
  half_away          ties rounded away from zero
  plus_half          +0.5 added before rounding (K-A's projection)
  no_int_intrinsics  fx, fy, cx, cy used without truncation to int (in the box and in the probes)
  border0            X > 0 and Y > 0 instead of > 1 (K-A's rule)
  border_hi          W > X and H > Y instead of W - 1 > X, H - 1 > Y
  ge_near_far        >= on the near and far planes
  no_depth_valid     depthValid ignored
  ge_band            >= on both edges of the band
  coarse_trunc       the fine test uses its coarse block's truncation distance
  float_step_rule    the step rule decided in float with f32(0.01) itself counted as above 10 mm (res >= 0.01f).  The strict
                     float comparison res > 0.01f is NOT a mutant: f32(0.01) < 0.01 < the next float, so it is the same
                     predicate as the reference's (double)res > 0.01 on every float and no case could tell them apart.  What
                     the f32(0.01) case pins is on which side of the rule that one float falls
  no_margin          the box not widened by one chunk on each side
  no_offset          the +0.2 left out of the box
  swap_dtn           the coarse / fine negative margins swapped

Frames whose box is not representable (a corner that is NaN, or whose chunk index does not fit an int) raise Undefined:
the reference casts an out-of-range float to int there, which no restatement can pin."""
import numpy as np

F = np.float32
D = np.float64
INT32_MIN = -(2 ** 31)

MUTANTS = ("trunc", "half_away", "plus_half", "no_int_intrinsics", "border0", "border_hi", "ge_near_far", "no_depth_valid",
           "ge_band", "coarse_trunc", "float_step_rule", "no_margin", "no_offset", "swap_dtn")
EVENTS = ("probes", "tie", "pz_le0", "x1", "x2", "xw2", "xw1", "y1", "y2", "yh2", "yh1")


class Undefined(ValueError):
    """the box has no finite, int-representable corners: the reference's behaviour is undefined"""


def _intrinsics(cam, mutant):
    k = [cam.fx, cam.fy, cam.cx, cam.cy]
    if mutant != "no_int_intrinsics":
        k = [int(x) for x in k]  # PinholeCamera::GetFx() returns int
    return [F(x) for x in k]


def truncation(ig, z):
    """tfo_truncation: |quad * z^2 + (float)(lin * z) + cons| * scale, the square and the sums in double"""
    z = np.asarray(z, F)
    quad, lin, cons, scale = (F(x) for x in ig[:4])
    zz = z.astype(D) * z.astype(D)
    lz = lin * z
    v = D(quad) * zz + lz.astype(D) + D(cons)
    return (np.abs(v) * D(scale)).astype(F)


def step_rule(res, mutant=None):
    """-> (step, diag, negTrunc) of ChunkManager.h:398-405"""
    res = F(res)
    if mutant == "float_step_rule":
        coarse_voxels = bool(res >= F(0.01))
    else:
        coarse_voxels = float(res) > 0.01  # (float vs double literal)
    if not coarse_voxels:
        return 4, F(F(8.0) * res) / F(2.0), F(0.03)
    diag = F(D(F(8.0) * res) * np.sqrt(D(3.0)))
    return 1, diag, F(D(0.05) * D(res) / D(0.005))


def bbox(depth, cam, pose, res, mutant=None):
    """tfo_bbox -> (min_id[3], max_id[3]) as Python ints"""
    depth = np.asarray(depth, F).reshape(cam.height, cam.width)
    P = np.asarray(pose, F).reshape(3, 4)
    fx, fy, cx, cy = _intrinsics(cam, mutant)
    with np.errstate(all="ignore"):
        ly = ((np.arange(cam.height, dtype=F) - cy) / fy)[:, None]
        lx = ((np.arange(cam.width, dtype=F) - cx) / fx)[None, :]
        dz = depth if mutant == "no_offset" else depth + F(0.2)
        vx, vy = lx * dz, ly * dz
        mn, mx = [], []
        for a in range(3):
            p = P[a, 0] * vx
            p = p + P[a, 1] * vy
            p = p + P[a, 2] * dz
            p = p + P[a, 3]
            # (p > max) ? p : max from -1e8, (p < min) ? p : min from 1e8: a NaN never wins a comparison
            mx.append(np.fmax(np.fmax.reduce(p, axis=None), F(-1e8)))
            mn.append(np.fmin(np.fmin.reduce(p, axis=None), F(1e8)))
        f = F(1.0) / (F(8.0) * F(res))  # GetIDAt
        lo = [np.floor(F(m * f)) for m in mn]
        hi = [np.floor(F(m * f)) for m in mx]
    for t in lo + hi:
        if not abs(float(t)) < 2.0 ** 31 - 8:  # (NaN included)
            raise Undefined("box corner %r chunks" % float(t))
    return [int(t) for t in lo], [int(t) for t in hi]


def _dot3_seq(r, v0, v1, v2):
    s = r[0] * v0
    s = s + r[1] * v1
    s = s + r[2] * v2
    return s


def _cvt(u, mutant):
    """_mm256_cvtps_epi32: round to nearest even; NaN and out of range -> 0x80000000.  int64 array"""
    if mutant == "plus_half":
        u = u + F(0.5)
    if mutant == "trunc":
        r = np.trunc(u)
    elif mutant == "half_away":
        r = (np.sign(u).astype(D) * np.floor(np.abs(u.astype(D)) + 0.5)).astype(F)
    else:
        r = np.rint(u)
    ok = (r >= F(-2147483648.0)) & (r < F(2147483648.0))
    return np.where(ok, np.where(ok, r, 0).astype(np.int64), INT32_MIN)


class _Probe:
    """CheckCornerIntersectingSIMD on arrays of origins"""

    def __init__(self, depth, cam, mutant, events):
        self.depth = np.asarray(depth, F).reshape(-1)
        self.W, self.H = cam.width, cam.height
        self.near, self.far = F(cam.near), F(cam.far)
        self.fx, self.fy, self.cx, self.cy = _intrinsics(cam, mutant)
        self.mutant = mutant
        self.ev = events

    def table(self, oc, off):
        """oc: [3][N] f32, off: [3][8] -> dict of [N, 8] arrays (X, Y, valid, pz, d, sd)"""
        m = self.mutant
        px = oc[0][:, None] + off[0][None, :]
        py = oc[1][:, None] + off[1][None, :]
        pz = oc[2][:, None] + off[2][None, :]
        u = (px / pz) * self.fx + self.cx  # no +0.5 here
        v = (py / pz) * self.fy + self.cy
        X, Y = _cvt(u, m), _cvt(v, m)
        W, H = self.W, self.H
        lo = 0 if m == "border0" else 1
        wx, hy = (W, H) if m == "border_hi" else (W - 1, H - 1)
        valid = (X > lo) & (wx > X) & (Y > lo) & (hy > Y)
        idx = np.where(valid, Y * W + X, 0)
        d = np.where(valid, self.depth[idx], F(0.0))
        sd = d - pz
        ev = self.ev
        if ev is not None:
            xin, yin = (X > 1) & (W - 1 > X), (Y > 1) & (H - 1 > Y)
            ev["probes"] += X.size
            ev["pz_le0"] += int(np.count_nonzero(pz <= 0))
            fin = np.isfinite(u) & np.isfinite(v)
            uu, vv = np.where(fin, u, F(0)), np.where(fin, v, F(0))
            ev["tie"] += int(np.count_nonzero(fin & ((uu - np.floor(uu) == F(0.5)) | (vv - np.floor(vv) == F(0.5)))))
            for k, c, n, other in (("x1", X, 1, yin), ("x2", X, 2, yin), ("xw2", X, W - 2, yin), ("xw1", X, W - 1, yin),
                                   ("y1", Y, 1, xin), ("y2", Y, 2, xin), ("yh2", Y, H - 2, xin), ("yh1", Y, H - 1, xin)):
                ev[k] += int(np.count_nonzero((c == n) & other))
        return dict(X=X, Y=Y, valid=valid, pz=pz, d=d, sd=sd, u=u, v=v)

    def hit(self, oc, dtp, dtn, off):
        m = self.mutant
        t = self.table(oc, off)
        sd, ndtn, dtp = t["sd"], -np.asarray(dtn, F), np.asarray(dtp, F)[:, None]
        if m == "ge_band":
            inside = (sd >= ndtn) & (dtp >= sd)
        else:
            inside = (sd > ndtn) & (dtp > sd)
        if m == "no_depth_valid":
            dv = np.ones(len(oc[2]), bool)
        elif m == "ge_near_far":
            dv = (oc[2] >= self.near) & (self.far >= oc[2])
        else:
            dv = (oc[2] > self.near) & (self.far > oc[2])
        return (t["valid"] & inside).any(axis=1) & dv


def _consts(pose, res, step):
    P = np.asarray(pose, F).reshape(3, 4)
    res = F(res)
    rot = P[:, :3].T.copy()  # rotation = R^T
    tc = [_dot3_seq(rot[i], P[0, 3], P[1, 3], P[2, 3]) for i in range(3)]
    r = [[(rot[i][c] * F(8.0)) * res for i in range(3)] for c in range(3)]  # r0, r1, r2: columns scaled by 8, then res
    half = res * F(0.5)
    coarse, fine = np.zeros((3, 8), F), np.zeros((3, 8), F)
    for x in range(2):
        for y in range(2):
            for z in range(2):
                k = x + y * 2 + z * 4
                for a in range(3):
                    d = _dot3_seq(rot[a], F(x * 8), F(y * 8), F(z * 8))
                    coarse[a, k] = (d * res) * F(step) + half
                    fine[a, k] = (d * res) * F(1.0) + half
    return rot, tc, r, coarse, fine


def _fine_origin(rot, tc, res, i, j, k):
    """[3][N] camera-frame origins of the chunks (i, j, k): rotation * (id * 8 * res) - translation"""
    org = [(8 * c).astype(F) * F(res) for c in (i, j, k)]
    return [_dot3_seq(rot[a], org[0], org[1], org[2]) - tc[a] for a in range(3)]


def select(depth, cam, ig, pose, res, mutant=None):
    """tfo_select -> (ids int32 [n, 3] in push_back order, n_coarse, events)"""
    assert mutant is None or mutant in MUTANTS, mutant
    res = F(res)
    ev = dict.fromkeys(EVENTS, 0)
    lo, hi = bbox(depth, cam, pose, res, mutant)
    step, diag, neg = step_rule(res, mutant)
    rot, tc, r, coarse, fine = _consts(pose, res, step)
    pr = _Probe(depth, cam, mutant, ev)
    margin = 0 if mutant == "no_margin" else 1
    axes = [np.arange(lo[a] - margin, hi[a] + margin + 1, step, dtype=np.int64) for a in range(3)]
    n_coarse = len(axes[0]) * len(axes[1]) * len(axes[2])
    if n_coarse == 0:
        return np.zeros((0, 3), np.int32), 0, ev
    x, y, z = (g.reshape(-1) for g in np.meshgrid(*axes, indexing="ij"))
    with np.errstate(all="ignore"):
        oc = []
        for a in range(3):
            ox = r[0][a] * x.astype(F) - tc[a]
            oy = ox + r[1][a] * y.astype(F)
            oc.append(oy + z.astype(F) * r[2][a])
        trunc = truncation(ig, oc[2])
        big, small = neg + diag * F(step), neg + diag
        dtn_c, dtn_f = (small, big) if mutant == "swap_dtn" else (big, small)
        hit = pr.hit(oc, trunc + diag * F(step), dtn_c, coarse)
        if not hit.any():
            return np.zeros((0, 3), np.int32), n_coarse, ev
        s = np.arange(step, dtype=np.int64)
        di, dj, dk = (g.reshape(-1) for g in np.meshgrid(s, s, s, indexing="ij"))
        i = (x[hit][:, None] + di[None, :]).reshape(-1)
        j = (y[hit][:, None] + dj[None, :]).reshape(-1)
        k = (z[hit][:, None] + dk[None, :]).reshape(-1)
        of = _fine_origin(rot, tc, res, i, j, k)
        tr = np.repeat(trunc[hit], step ** 3) if mutant == "coarse_trunc" else truncation(ig, of[2])
        fhit = pr.hit(of, tr + diag, dtn_f, fine)
    ids = np.stack([i[fhit], j[fhit], k[fhit]], axis=1).astype(np.int32)
    return ids, n_coarse, ev


def chunk_probes(depth, cam, ig, pose, res, cid):
    """The fine test of one chunk, for builders that put a pixel exactly on a threshold: dict of [8] arrays X, Y, valid, pz,
    d, sd, plus the scalars dtp, dtn and depth_valid"""
    res = F(res)
    step, diag, neg = step_rule(res)
    rot, tc, r, coarse, fine = _consts(pose, res, step)
    c = [np.array([int(v)], np.int64) for v in cid]
    with np.errstate(all="ignore"):
        of = _fine_origin(rot, tc, res, *c)
        t = _Probe(depth, cam, None, None).table(of, fine)
        out = {k: v[0] for k, v in t.items()}
        out["dtp"] = F(truncation(ig, of[2])[0] + diag)
    out["dtn"] = F(neg + diag)
    out["depth_valid"] = bool(of[2][0] > F(cam.near) and F(cam.far) > of[2][0])
    return out
