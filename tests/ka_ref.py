"""numpy restatement of the voxel update (K-A): tfo_voxel_update and tfo_chunk_scalars of oracle/tf_oracle.c, i.e.
ProjectionIntegrator::voxelUpdateSIMD (utils/ProjectionIntegrator.cpp:67-426) for ONE chunk and one frame.

float32 throughout, every operation rounded on its own (numpy rounds each array operation; nothing is fused); the two
places the reference computes in double (the truncation polynomial, the colour threshold and the half-pixel shift) are
double here.  The row stall is kept: a row of eight voxels without a valid lane does not advance `pos` (:176-178), so
that row and every later one of the chunk is dead -- `rows` of the result is the number of processed rows.

numpy only: no oracle, no GPU.  tests/test_ka_cpu.py holds this file against both oracle kernels bit for bit; its
intermediates (per row and lane) are what that file uses to prove that every case of tests/ka_inputs.py hits the edge
it names."""
import numpy as np

F = np.float32
INT_MIN = np.int32(-2 ** 31)
QOOB = F(-99999999999.0)  # "out of observation" (:221-222): assigned, not accumulated
LOWER = F(-0.03)          # :314
SIGMA = F(1e-4)           # :126
RESET_SDF = F(999.0)


def cvt_rne(x):
    """_mm256_cvtps_epi32 under the default MXCSR: nearest-even; NaN and |x| >= 2^31 give 0x80000000"""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        ok = (x >= F(-2147483648.0)) & (x < F(2147483648.0))
        r = np.rint(np.where(ok, x, F(0))).astype(np.int64)
    return np.where(ok, r, np.int64(INT_MIN)).astype(np.int32)


def dot3_tree(a0, a1, a2, b0, b1, b2):
    """the fixed-size Eigen dot of the oracle: a0*b0 + (a1*b1 + a2*b2), each step rounded"""
    p0, p1, p2 = F(a0) * F(b0), F(a1) * F(b1), F(a2) * F(b2)
    return F(p0 + F(p1 + p2))


def truncation(ig, z):
    """QuadraticTruncator::GetTruncationDistance: |q*z^2 + l*z + c| * s, polynomial in double, l*z in float.
    ig = (quad, lin, cons, scale, weight) as float32"""
    quad, lin, cons, scale = (F(v) for v in ig[:4])
    z = F(z)
    with np.errstate(all="ignore"):
        zz = np.float64(z) * np.float64(z)
        lz = F(lin * z)
        v = np.float64(quad) * zz + np.float64(lz) + np.float64(cons)
        return F(np.abs(v) * np.float64(scale))


def chunk_scalars(ig, pose, cid, res):
    """tfo_chunk_scalars: (origin in camera [3], truncation, weight) of one chunk"""
    pose = np.asarray(pose, F).reshape(3, 4)
    res = F(res)
    with np.errstate(all="ignore"):
        d = [F(F(F(8 * int(cid[a])) * res) - pose[a, 3]) for a in range(3)]
        o = np.array([dot3_tree(pose[0, a], pose[1, a], pose[2, a], d[0], d[1], d[2]) for a in range(3)], F)
        tr = truncation(ig, o[2])
        w = F(F(ig[4]) / F(F(2.0) * tr))
    return o, tr, w


def centroids(pose, res):
    """tfo_centroids: c[a][i] = (R^T (x,y,z))_a * res + res/2, i = (z*8+y)*8+x -> float32[3, 512]"""
    pose = np.asarray(pose, F).reshape(3, 4)
    res = F(res)
    half = F(res * F(0.5))
    i = np.arange(512)
    fx, fy, fz = (i & 7).astype(F), ((i >> 3) & 7).astype(F), (i >> 6).astype(F)
    out = np.empty((3, 512), F)
    for a in range(3):
        p0, p1, p2 = pose[0, a] * fx, pose[1, a] * fy, pose[2, a] * fz
        d = (p0 + (p1 + p2).astype(F)).astype(F)
        out[a] = ((d * res).astype(F) + half).astype(F)
    return out


def constants(cam, res):
    """per-frame constants of voxelUpdateSIMD; cam = (W, H, fx, fy, cx, cy, near, far).  The intrinsics go through the
    reference's int getters (:79-82): truncated towards zero"""
    res = F(res)
    res_diag = F(np.sqrt(np.float64(3.0)) * np.float64(res))
    c = dict(W=int(cam[0]), H=int(cam[1]), near=F(cam[6]), far=F(cam[7]), res_diag=res_diag)
    c["fxi"], c["fyi"] = F(int(F(cam[2]))), F(int(F(cam[3])))
    cxi, cyi = F(int(F(cam[4]))), F(int(F(cam[5])))
    c["cxs"], c["cys"] = F(np.float64(cxi) + 0.5), F(np.float64(cyi) + 0.5)
    c["thr_col"] = F(np.float64(F(res_diag / F(2.0))) + 0.01)
    return c


def voxel_update(depth, rgba, quality, cam, ig, pose, flag, cid, res, sdf, weight, color):
    """One chunk, one frame.  sdf, weight: float32[512]; color: uint16[2048]; none of them is modified.
    Returns dict(sdf, weight, color, quality, updated, rows, + the intermediates, each [64 rows, 8 lanes]:
    X, Y, valid, oob, pz, px, py, u, v, idx, d, sd, upd, F, num, den, nwt, live (row was processed), row_tsdf, row_color
    (row was rewritten), o / trunc / wD / upper / thr_col (scalars))."""
    k = constants(cam, res)
    W, H = k["W"], k["H"]
    o, trunc, wD = chunk_scalars(ig, pose, cid, res)
    if not flag:
        wD = F(wD * F(-1.0))
    cen = centroids(pose, res)
    upper = F(trunc + k["res_diag"])
    thr = k["thr_col"]
    depth = np.asarray(depth, F).reshape(-1)
    sdf = np.asarray(sdf, F).copy()
    weight = np.asarray(weight, F).copy()
    color = np.asarray(color, np.uint16).copy().reshape(512, 4)
    with np.errstate(all="ignore"):
        px = (o[0] + cen[0]).astype(F).reshape(64, 8)
        py = (o[1] + cen[1]).astype(F).reshape(64, 8)
        pz = (o[2] + cen[2]).astype(F).reshape(64, 8)
        u = (((px / pz).astype(F) * k["fxi"]).astype(F) + k["cxs"]).astype(F)
        v = (((py / pz).astype(F) * k["fyi"]).astype(F) + k["cys"]).astype(F)
        X, Y = cvt_rne(u), cvt_rne(v)
        valid = (X > 0) & (W - 1 > X) & (Y > 0) & (H - 1 > Y)
        oob = (0 > X) | (X > W - 1) | (0 > Y) | (Y > H - 1)
        dead = np.flatnonzero(~valid.any(axis=1))
        rows = int(dead[0]) if len(dead) else 64
        live = np.zeros((64, 8), bool)
        live[:rows] = True
        idx = (Y.astype(np.int64) * W + X.astype(np.int64))
        idx = np.where(valid, idx, 0)
        d = np.where(valid & live, depth[idx], F(0)).astype(F)
        sd = (d - pz).astype(F)
        upd = valid & live & (sd > -thr) & (thr > sd)
        Fm = live & (d > k["near"]) & (k["far"] > d) & (sd > LOWER) & (upper > sd)
        row_color = upd.any(axis=1) & (rgba is not None)
        row_tsdf = Fm.any(axis=1)
        # TSDF: every lane of a rewritten row (:319-341)
        s2, w2 = sdf.reshape(64, 8), weight.reshape(64, 8)
        nw = np.where(Fm, wD, F(0)).astype(F)
        num = ((s2 * w2).astype(F) + (sd * nw).astype(F)).astype(F)
        nwt = (w2 + nw).astype(F)
        den = (nwt + SIGMA).astype(F)
        ns = (num / den).astype(F)
        keep = nwt > F(0.5)
        wr = row_tsdf[:, None] & np.ones((1, 8), bool)
        new_s = np.where(wr, np.where(keep, ns, RESET_SDF), s2).astype(F)
        new_w = np.where(wr, np.where(keep, nwt, F(0)), w2).astype(F)
        # colour and the quality sum, in row order (:201-306)
        qsum = F(0)
        if rgba is not None:
            pix = np.asarray(rgba, np.uint8).reshape(-1, 4)
            qimg = None if quality is None else np.asarray(quality, F).reshape(-1)
            c3 = color.reshape(64, 8, 4)
            for r in range(rows):
                if oob[r].any():
                    qsum = QOOB
                if not upd[r].any():
                    continue
                if qimg is not None:
                    s = F(0)
                    for l in range(8):
                        s = F(s + (qimg[idx[r, l]] if upd[r, l] else F(0)))
                    qsum = F(qsum + s)
                inp = np.where(upd[r][:, None], pix[idx[r]], 0).astype(np.uint16)
                if flag:
                    n = (c3[r] + inp).astype(np.uint16)
                    over = n[:, 3].astype(np.int16) > 120  # the signed compare of :281-287
                    n = np.where(over[:, None], n >> 2, n).astype(np.uint16)
                else:
                    n = (c3[r] - inp).astype(np.uint16)
                c3[r] = n
    return dict(sdf=new_s.reshape(512), weight=new_w.reshape(512), color=color.reshape(2048), quality=F(qsum),
                updated=bool(row_tsdf.any()), rows=rows, X=X, Y=Y, valid=valid, oob=oob & live, pz=pz, px=px, py=py, u=u, v=v,
                idx=idx, d=d, sd=sd, upd=upd, F=Fm, num=num, den=den, nwt=nwt, live=live, row_tsdf=row_tsdf,
                row_color=row_color, o=o, trunc=trunc, wD=wD, upper=upper, thr_col=thr)


def depth_group(depths, cam, ig, poses, flag, cid, res, sdf, weight):
    """n depth-only frames, each with its own pose, over one chunk: the single-frame update applied n times (what
    tf_integrate_depth_group promises to equal).  Returns (sdf, weight, updated, [per-frame results])."""
    col = np.zeros(2048, np.uint16)
    upd, per = False, []
    for dep, pose in zip(depths, poses):
        r = voxel_update(dep, None, None, cam, ig, pose, flag, cid, res, sdf, weight, col)
        sdf, weight = r["sdf"], r["weight"]
        upd = upd or r["updated"]
        per.append(r)
    return sdf, weight, upd, per


def same_floats(a, b, nan_equal=False):
    """bit-for-bit equality of two float32 arrays; with nan_equal a NaN equals a NaN whatever its sign and payload (x86
    produces the negative default NaN, the GPU the positive one) -- but only at the same positions"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    if not nan_equal:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])
