"""The inline device helpers the voxel update is built from, each on chosen operands, through tests/hip/libka_math_probe.so
(one-line kernels around the unmodified helpers of tf_devfn.h / tf_voxel_math.h, built by build() with the library's flags):

  div2_by(n, recip_refined(d))       == float32 n / d, bit for bit, zero mismatches, on four operand sets
  cvt_sat_rne / cvt_rne_hw           == the x86 conversion where it is defined, and the same `valid` / off-image
                                        predicates where the two saturate differently
  truncation / chunk_pre / centroid_table   == tfo_truncation / tfo_chunk_scalars / tfo_centroids, bit for bit
  f2key / key2f, pack_id / unpack_id / hash_key

The next attempt to extend the division sequence (to the TSDF quotient, to the mesher) starts from a test that pins it."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import api as O
from tests import ka_inputs as KI
from tests import ka_ref as KR

pytestmark = pytest.mark.gpu

F = np.float32
_SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip", "libka_math_probe.so")


@pytest.fixture(scope="module")
def probe(gpu_required):
    if not os.path.exists(_SO):
        pytest.fail("%s is missing: build() makes it (tests/hip/Makefile)" % _SO)
    L = C.CDLL(_SO)
    fp, ip, i64 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int64
    L.ka_div2.argtypes = [i64, fp, fp, fp, fp, fp]
    L.ka_cvt_sat_rne.argtypes = [i64, fp, ip]
    L.ka_cvt_rne_hw.argtypes = [i64, fp, ip]
    L.ka_truncation.argtypes = [i64, fp, fp, fp]
    L.ka_chunk_pre.argtypes = [i64, ip, fp, fp, C.c_float, C.c_float, fp]
    L.ka_centroid_table.argtypes = [fp, C.c_float, fp]
    L.ka_float_keys.argtypes = [i64, fp, C.POINTER(C.c_uint32), fp]
    L.ka_chunk_ids.argtypes = [i64, ip, C.POINTER(C.c_uint64), ip, C.POINTER(C.c_uint32)]
    return L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _div2(L, a0, a1, d):
    a0, a1, d = (np.ascontiguousarray(x, F) for x in (a0, a1, d))
    q0, q1 = np.empty_like(d), np.empty_like(d)
    assert L.ka_div2(len(d), _fp(a0), _fp(a1), _fp(d), _fp(q0), _fp(q1)) == 0
    return q0, q1


def _assert_quotients(L, a0, a1, d, what):
    a0, a1, d = (np.ascontiguousarray(x, F) for x in (a0, a1, d))
    q0, q1 = _div2(L, a0, a1, d)
    for a, q in ((a0, q0), (a1, q1)):
        want = (a / d).astype(F)
        bad = np.flatnonzero(want.view(np.uint32) != q.view(np.uint32))
        assert len(bad) == 0, "%s: %d of %d quotients differ from n / d, first n = %r, d = %r: %r vs %r" % (
            what, len(bad), len(d), a[bad[0]], d[bad[0]], q[bad[0]], want[bad[0]])


def _log_uniform(rng, n, e_lo, e_hi):
    """|x| = 2^e * m with e uniform in [e_lo, e_hi) and a uniform 24-bit significand, random sign"""
    e = rng.integers(e_lo, e_hi, n)
    m = 1.0 + rng.integers(0, 1 << 23, n) / float(1 << 23)
    x = np.ldexp(m, e) * rng.choice([-1.0, 1.0], n)
    out = x.astype(F)
    assert np.array_equal(out.astype(np.float64), x)
    return out


def test_division_sequence_log_uniform_pairs(probe):
    """2^20 pairs inside the guard's operand range: |d| in [2^-18, 2^21), n = 0 or |n| in [2^-44, 2^21), every sign.
    The zero numerators are +0: the kernels' numerators are sums o + c of a chunk origin and a centroid, a sum of two
    floats is -0 only if both are, and a centroid d * res + res / 2 never is (test_negative_zero_numerator has the rest)"""
    rng = np.random.default_rng(20261019)
    n = 1 << 20
    d = _log_uniform(rng, n, -18, 21)
    a0, a1 = _log_uniform(rng, n, -44, 21), _log_uniform(rng, n, -44, 21)
    a0[::16] = 0.0
    a1[5::16] = 0.0
    for s0 in (1, -1):
        for sd in (1, -1):
            assert ((np.sign(a0) == s0) & (np.sign(d) == sd)).sum() > 1000
    _assert_quotients(probe, a0, a1, d, "log-uniform pairs")


def test_division_sequence_near_midpoints(probe):
    """2^18 hard roundings: n = RN(m * d) with m a 25-bit midpoint between two floats (the product is exact in float64)"""
    rng = np.random.default_rng(7)
    n = 1 << 18
    d = _log_uniform(rng, n, -10, 10)
    nums = []
    for _ in range(2):
        m = np.ldexp((1 << 24) + 2 * rng.integers(0, 1 << 23, n) + 1, rng.integers(-34, -14, n))  # odd 25-bit integers, scaled
        prod = m * d.astype(np.float64)  # 25 x 24 significant bits: exact
        nums.append(prod.astype(F))
    _assert_quotients(probe, nums[0], nums[1], d, "near-midpoint quotients")


def test_division_sequence_powers_of_two_and_neighbours(probe):
    def around(e_lo, e_hi):
        p = np.ldexp(1.0, np.arange(e_lo, e_hi + 1)).astype(F)
        v = np.concatenate([p, np.nextafter(p, F(0)), np.nextafter(p, F(np.inf))])
        return np.concatenate([v, -v])

    d = around(-18, 21)
    a = np.concatenate([around(-44, 21), np.array([0.0], F)])
    dd, aa = np.meshgrid(d, a)
    dd, aa = dd.reshape(-1), aa.reshape(-1)
    _assert_quotients(probe, aa, aa[::-1].copy(), dd, "powers of two and their neighbours")


def test_negative_zero_numerator(probe):
    """Outside the sequence's domain, pinned so that nobody extends it unawares: without v_div_fixup the sequence returns
    +0 for -0 / d with d > 0 (the residual fma(-d, -0, -0) is +0, and +0 + -0 is +0), where `/` gives -0; the other three
    sign combinations of a zero numerator are exact (measured on the MI355X: 120 of 120 pairs with n = -0, d > 0 differ,
    none of the others).  The projection cannot see it: no case of tests/ka_inputs.py has a -0 numerator, and
    u = q * fx + (cx + 0.5) is the same float for either zero."""
    for name, c in KI.cases().items():
        for i in range(len(c.ids)):
            g = KI.geometry(c, i)
            for k in ("px", "py"):
                assert not np.signbit(g[k][g[k] == 0]).any(), "%s chunk %d: a -0 numerator" % (name, i)
    p = np.ldexp(1.0, np.arange(-18, 22)).astype(F)
    d = np.concatenate([p, -p, np.nextafter(p, F(0)), -np.nextafter(p, F(np.inf))])
    for zero in (F(0.0), F(-0.0)):
        n = np.full(len(d), zero, F)
        q0, q1 = _div2(probe, n, n, d)
        want = (n / d).astype(F)
        assert (q0 == 0).all() and np.array_equal(q0.view(np.uint32), q1.view(np.uint32))
        exact = ~(np.signbit(n) & (d > 0))
        assert np.array_equal(q0.view(np.uint32)[exact], want.view(np.uint32)[exact])
        for fx, cxs in ((F(52.0), F(31.5)), (F(64.0), F(0.5))):
            assert np.array_equal((q0 * fx + cxs).view(np.uint32), (want * fx + cxs).view(np.uint32))


def test_division_sequence_on_the_cases_own_operands(probe):
    """the exact (p.x, p.y, p.z) of cases B (ties) and D (both sides of the guard)"""
    px, py, pz = [], [], []
    for name in ("B", "B2", "D_eq", "D_pos_above", "D_pos_below", "D_neg_eq", "D_neg_above", "D_neg_below"):
        c = KI.cases()[name]
        for i in range(len(c.ids)):
            g = KI.geometry(c, i)
            px.append(g["px"].reshape(-1)); py.append(g["py"].reshape(-1)); pz.append(g["pz"].reshape(-1))
    px, py, pz = np.concatenate(px), np.concatenate(py), np.concatenate(pz)
    assert len(pz) > 30000 and (pz != 0).all()
    _assert_quotients(probe, px, py, pz, "p.x / p.z and p.y / p.z of cases B and D")


def _cvt(L, fn, x):
    x = np.ascontiguousarray(x, F)
    r = np.empty(len(x), np.int32)
    assert getattr(L, fn)(len(x), _fp(x), _ip(r)) == 0
    return r


def _kernel_predicates(X, n):
    """`valid` and off-image of one axis as the kernels compute them (tf_kernels.hip: two unsigned range tests)"""
    Xu = X.astype(np.int64) & 0xFFFFFFFF
    valid = ((Xu - 1) & 0xFFFFFFFF) < ((n - 2) & 0xFFFFFFFF)
    oob = Xu > ((n - 1) & 0xFFFFFFFF)
    return valid, oob


def _reference_predicates(X, n):
    X = X.astype(np.int64)
    return (X > 0) & (n - 1 > X), (0 > X) | (X > n - 1)


def test_float_to_int_conversions(probe):
    rng = np.random.default_rng(3)
    k = rng.integers(-(1 << 22), 1 << 22, 4096)
    ties = (k + 0.5).astype(F)
    assert np.array_equal(ties.astype(np.float64), k + 0.5)
    inside = np.concatenate([ties, _log_uniform(rng, 1 << 16, -30, 31), rng.uniform(-70, 1400, 1 << 14).astype(F),
                             np.array([0.0, -0.0, 0.5, -0.5, 1.5, 2.5, -1.5, 2147483520.0, -2147483648.0, 1e-40, -1e-40], F)])
    inside = inside[np.abs(inside.astype(np.float64)) <= 2147483648.0]
    inside = inside[inside != F(2147483648.0)]
    want = KR.cvt_rne(inside)
    for fn in ("ka_cvt_sat_rne", "ka_cvt_rne_hw"):
        assert np.array_equal(_cvt(probe, fn, inside), want), fn + " inside the int range"
        assert np.array_equal(_cvt(probe, fn, ties), KR.cvt_rne(ties)), fn + " at ties"
    # where x86 gives the integer indefinite and the GPU saturates: the same predicates
    beyond = np.array([2147483648.0, -2147483904.0, 4294967296.0, -4294967296.0, 1e20, -1e20, 3e38, -3e38, np.inf, -np.inf], F)
    ref = KR.cvt_rne(beyond)
    assert (ref == KR.INT_MIN).all()
    for fn, x in (("ka_cvt_sat_rne", np.concatenate([beyond, np.array([np.nan, -np.nan], F)])), ("ka_cvt_rne_hw", beyond)):
        got = _cvt(probe, fn, x)
        for n in (2, 64, 1280):
            gv, go = _kernel_predicates(got, n)
            rv, ro = _reference_predicates(np.full(len(x), KR.INT_MIN, np.int32), n)
            assert np.array_equal(gv, rv) and np.array_equal(go, ro), "%s beyond the int range, image size %d: %s" % (fn, n, got)
    # ... and the unsigned form of the predicates is the reference's on every value that can occur
    for n in (2, 64, 1280):
        X = np.concatenate([np.arange(-3, n + 3), np.array([KR.INT_MIN, KR.INT_MIN + 1, 2 ** 31 - 1, 2 ** 31 - 2])]).astype(np.int32)
        assert all(np.array_equal(a, b) for a, b in zip(_kernel_predicates(X, n), _reference_predicates(X, n)))


INTEGRATORS = (KI.IG, (F(0.004), F(-0.003), F(0.0007), F(3.5), F(0.25)), (F(0.0), F(0.0), F(0.0), F(6.0), F(1.0)))


def _random_pose(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.concatenate([R, rng.uniform(-2, 2, (3, 1))], 1).astype(F)


def test_truncation_chunk_scalars_and_centroids(probe):
    rng = np.random.default_rng(11)
    z = np.concatenate([np.array([0.0, -0.0, 1e-30, -1e-30, 1e-40, -1e-40, -0.7, -3.0, 1e6, -1e6, 0.4, 2.5], F),
                        rng.uniform(-4, 8, 500).astype(F)])
    for ig in INTEGRATORS:
        ig5 = np.array(ig, F)
        got = np.empty(len(z), F)
        assert probe.ka_truncation(len(z), _fp(ig5), _fp(z), _fp(got)) == 0
        oig = O.Integrator(*ig)
        want = np.array([O.truncation(oig, v) for v in z], F)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "truncation, integrator %s" % (ig,)
    ids = np.concatenate([rng.integers(-300, 300, (200, 3)), np.array([[0, 0, 0], [1 << 19, -(1 << 19), 7], [-1, -1, -1]])]).astype(np.int32)
    poses = [KI.pose_rt(), KI.cases()["D_eq"].poses[0], KI.cases()["C2"].poses[0]] + [_random_pose(rng) for _ in range(5)]
    for res in (KI.RES5, KI.RES8, F(0.0123)):
        res_diag = F(np.sqrt(np.float64(3.0)) * np.float64(res))  # ProjectionIntegrator.cpp:77
        for pose in poses:
            p12 = np.ascontiguousarray(pose, F).reshape(12)
            cen = np.empty((3, 512), F)
            assert probe.ka_centroid_table(_fp(p12), res, _fp(cen)) == 0
            assert np.array_equal(cen.view(np.uint32), O.centroids(pose, res).view(np.uint32)), "centroid table"
            for ig in INTEGRATORS[:2]:
                out = np.empty((len(ids), 8), F)
                ig5 = np.array(ig, F)
                assert probe.ka_chunk_pre(len(ids), _ip(ids), _fp(p12), _fp(ig5), res, res_diag, _fp(out)) == 0
                oig = O.Integrator(*ig)
                for i, cid in enumerate(ids):
                    o, tr, w = O.chunk_scalars(oig, pose, cid, res)
                    want = np.array([o[0], o[1], o[2], tr, w, F(F(tr) + res_diag)], F)
                    assert np.array_equal(out[i, :6].view(np.uint32), want.view(np.uint32)), "chunk_pre of %s: %s vs %s" % (cid, out[i], want)


def test_float_keys(probe):
    tiny = np.finfo(F).tiny
    pos = np.array([0.0, 1e-45, 1e-40, float(np.nextafter(tiny, F(0))), tiny, 1e-20, 0.5, 1.0, float(np.nextafter(F(1), F(2))), 1e8, 3.4e38, np.inf], F)
    f = np.concatenate([-pos[::-1], pos])
    assert np.signbit(f[len(pos) - 1]) and not np.signbit(f[len(pos)]) and (np.diff(f.astype(np.float64)) >= 0).all()
    key, back = np.empty(len(f), np.uint32), np.empty(len(f), F)
    assert probe.ka_float_keys(len(f), _fp(f), key.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(back)) == 0
    assert (np.diff(key.astype(np.int64)) > 0).all(), "keys strictly increasing, -0 below +0: %s" % key
    assert np.array_equal(back.view(np.uint32), f.view(np.uint32)), "round trip"


def test_chunk_id_packing_and_hash(probe):
    ax = [0, 1, -1, -(1 << 20), (1 << 20) - 1]
    xyz = np.array([[x, y, z] for x in ax for y in ax for z in ax], np.int32)
    key, back, h = np.empty(len(xyz), np.uint64), np.empty_like(xyz), np.empty(len(xyz), np.uint32)
    assert probe.ka_chunk_ids(len(xyz), _ip(xyz), key.ctypes.data_as(C.POINTER(C.c_uint64)), _ip(back),
                              h.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    assert np.array_equal(back, xyz), "pack_id / unpack_id round trip"
    assert len(set(key.tolist())) == len(xyz)
    for k, hv in zip(key.tolist(), h.tolist()):
        p = (k * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        assert hv == ((p >> 32) ^ (p & 0xFFFFFFFF)), "hash_key"
