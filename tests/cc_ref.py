"""Chisel::CompensateColor (Structure/Chisel.cpp:198-286, computeMeanAndCov Patch.cpp:342-348) restated with EXACT sums:
every statement as the reference forms it in f32 (centred values, their products, the transfer), the two reductions
accumulated in f64 -- whose own error, at most N u sum|x| = 1e-11 relative for the 1e5 vertices used here, vanishes in the
rounding of the means and covariances to f32 -- and the 3x3 solve by the oracle's color_transfer.  It is the reference for
sums over so many vertices that the oracle's own f32 in-order accumulation leaves the stage's bound: over the 74 936
vertices of the wall scene as ONE cluster the oracle is 3.8e-5 from this evaluation (two clusters: 8.2e-6), measured on
the CPU with both fed the oracle's own patches."""
import numpy as np

from oracle import api as O


def _eigh(A):
    w, V = np.linalg.eigh(np.asarray(A, np.float64))
    return np.maximum(w, 0.0), V


def transfer_f64(cov_src, cov_tar):
    """The transfer matrix of Chisel.cpp:247-266 as the matrix function it is,

        T = f(Cs) . (Cs^1/2 Ct Cs^1/2)^1/2 . f(Cs),    f(x) = 1 / (sqrt(max(x, 0)) + 1e-2),

    by numpy.linalg.eigh (LAPACK's tridiagonal QR) in f64: no line of the Jacobi text that tf_cc_solve.h and the oracle
    share.  With Cs = U diag(w) U^T: f(Cs) = U Di U^T, Cs^1/2 Ct Cs^1/2 = U media U^T with media = D U^T Ct U D, and its
    root is U Um Dm Um^T U^T from media = Um diag(wm) Um^T.  The four f32 roundings of tf_cc_solve.h are applied where it
    applies them: D = f32(sqrt(w)), media rounded entry by entry and its upper triangle mirrored, Dm = f32(sqrt(wm)),
    Di = f32(1 / (D + 1e-2)).  Where Cs has a repeated eigenvalue (Cs = 0, a grey keyframe's rank-1 Cs) eigh's U is
    another basis of that eigenspace than Jacobi's, so media is rounded in another basis: a relative 2^-24 of entries that
    T depends on continuously; tests/test_cc_inputs_cpu.py measures it against the Jacobi text on every cluster.

    Compare labs, never T.  On a rank-deficient Cs the components of T on the null space of Cs are ill-conditioned: an
    eigenvalue of 1e-9 where 0 is meant makes D 3e-5, media's entry there 1e-9 |Ct|, and T's component
    Di^2 sqrt(1e-9 |Ct|) -- about 1e4 * 1e-5 = 0.1.  The vertices that receive labs = T (texcolor - mean_src) + mean_tar
    are exactly the vertices the covariance was taken over: texcolor - mean_src has no component on the null space of
    Cs (up to the rounding of the mean), so labs do not feel what T does TO a null-space input.  They do feel the
    block of T that maps the range of Cs ONTO the null direction, Di_null * sqrt(eps) * Di_range: two solves fed the
    same covariance bits agree on it (0 to 6e-8 in labs over the clusters of tests/cc_inputs.py, rank 0, 1 and 3), but
    two summations that differ in the covariance's last bits do not where the zero eigenvalue is made of rounding
    alone -- see the note on cluster L in tests/cc_inputs.py.

    A covariance that is not finite (a one-vertex cluster: 0 / 0) gives a T of NaN, as the Jacobi text does."""
    cs = np.asarray(cov_src, np.float32).reshape(3, 3).astype(np.float64)
    ct = np.asarray(cov_tar, np.float32).reshape(3, 3).astype(np.float64)
    if not (np.isfinite(cs).all() and np.isfinite(ct).all()):
        return np.full((3, 3), np.nan, np.float32)
    w, U = _eigh((cs + cs.T) / 2)
    D = np.sqrt(w).astype(np.float32).astype(np.float64)
    media = (D[:, None] * (U.T @ ct @ U) * D[None, :]).astype(np.float32)
    media = (np.triu(media) + np.triu(media, 1).T).astype(np.float64)
    wm, Um = _eigh(media)
    Dm = np.sqrt(wm).astype(np.float32).astype(np.float64)
    Di = (1.0 / (D + 1e-2)).astype(np.float32).astype(np.float64)
    f_cs = (U * Di) @ U.T
    root = U @ ((Um * Dm) @ Um.T) @ U.T
    return (f_cs @ root @ f_cs).astype(np.float32)


def labs_exact_sums(frameid, wrong, adjusted, voff, texcolor, meshcolor, solve=O.color_transfer):
    """labs of every patch that is not adjusted yet (NaN where the reference writes none), has_adjusted afterwards;
    solve(cov_src, cov_tar) -> T is the oracle's Jacobi text or transfer_f64"""
    tex = np.ascontiguousarray(texcolor, np.float32)
    mesh = np.ascontiguousarray(meshcolor, np.float32)
    labs = np.full_like(tex, np.nan)
    adj = np.asarray(adjusted).astype(bool).copy()
    todo = ~adj
    for f in np.unique(np.asarray(frameid)[todo]):
        members = [p for p in np.flatnonzero(todo) if frameid[p] == f]
        good = [p for p in members if not wrong[p]]
        v = np.concatenate([np.arange(voff[p], voff[p + 1]) for p in good]) if good else np.zeros(0, np.int64)
        if len(v) == 0:
            continue  # Chisel.cpp:242: nothing learnt, has_adjusted stays false
        n = len(v)
        nm1 = np.float64(np.float32(n) - np.float32(1))
        mean, cov = [], []
        for x in (tex[v], mesh[v]):
            m = (x.astype(np.float64).sum(0) / n).astype(np.float32)
            d = x - m
            c = np.zeros((3, 3), np.float32)
            with np.errstate(invalid="ignore", divide="ignore"):  # (one vertex: 0 / (N - 1) = 0 / 0, Patch.cpp:347)
                for i in range(3):
                    for j in range(3):
                        c[i, j] = np.float32((d[:, i] * d[:, j]).astype(np.float64).sum() / nm1)
            mean.append(m)
            cov.append(c)
        T = np.asarray(solve(cov[0], cov[1]), np.float32).reshape(3, 3)
        for p in members:
            adj[p] = True
            if wrong[p]:
                continue
            a, b = voff[p], voff[p + 1]
            d = tex[a:b] - mean[0]
            for i in range(3):
                acc = T[i, 0] * d[:, 0]
                acc = acc + T[i, 1] * d[:, 1]
                acc = acc + T[i, 2] * d[:, 2]
                labs[a:b, i] = acc + mean[1][i]
    return labs, adj
