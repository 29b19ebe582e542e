"""Chisel::CompensateColor (Structure/Chisel.cpp:198-286, computeMeanAndCov Patch.cpp:342-348) restated with EXACT sums:
every statement as the reference forms it in f32 (centred values, their products, the transfer), the two reductions
accumulated in f64 -- whose own error, at most N u sum|x| = 1e-11 relative for the 1e5 vertices used here, vanishes in the
rounding of the means and covariances to f32 -- and the 3x3 solve by the oracle's color_transfer.  It is the reference for
sums over so many vertices that the oracle's own f32 in-order accumulation leaves the stage's bound: over the 74 936
vertices of the wall scene as ONE cluster the oracle is 3.8e-5 from this evaluation (two clusters: 8.2e-6), measured on
the CPU with both fed the oracle's own patches."""
import numpy as np

from oracle import api as O


def labs_exact_sums(frameid, wrong, adjusted, voff, texcolor, meshcolor):
    """labs of every patch that is not adjusted yet (NaN where the reference writes none), has_adjusted afterwards"""
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
            for i in range(3):
                for j in range(3):
                    c[i, j] = np.float32((d[:, i] * d[:, j]).astype(np.float64).sum() / nm1)
            mean.append(m)
            cov.append(c)
        T = O.color_transfer(cov[0], cov[1])
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
