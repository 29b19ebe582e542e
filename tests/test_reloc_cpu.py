"""Relocalisation without a GPU: the restatement (tests/reloc_ref.py) is exact whatever the order of summation, s_grey does
not see a brightness offset, tf_reloc_score.h on the host gives the restatement's bits, the input scene (tests/
reloc_inputs.py) is what the device tests need it to be -- keyframes far apart, every ray a hit, every query ranking its own
keyframe first, the far keyframes no start for the tracker -- and the C++ mirror compiles."""
import ctypes as C
import itertools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import align_icp_inputs as II
from tests import align_icp_ref as K
from tests import align_inputs as I
from tests import align_ref as R
from tests import reloc_inputs as QI
from tests import reloc_ref as Q
from texturefusion_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++")
SHAPE = (I.CAM.height, I.CAM.width)


@pytest.fixture(scope="module")
def scene():
    """keyframe descriptors {kf_id: (G, Z, S)} at the default parameters, ids 10 .."""
    p = Q.params()
    return p, {10 + k: Q.describe(*QI.frame(pose), p) for k, pose in enumerate(QI.keyframe_poses())}


def _bits(x):
    return struct.pack("<d", x)


# ---- 1. exactness -------------------------------------------------------------------------------------------------------
def test_descriptor_and_score_do_not_depend_on_the_order_of_summation(scene):
    p, rows = scene
    rng = np.random.default_rng(5)
    depth, rgb = QI.frame(QI.query_pose(1, 1))
    depth = depth.copy()
    depth[rng.random(depth.shape) < 0.1] = np.nan
    want = Q.describe(depth, rgb, p)
    for _ in range(3):
        got = Q.describe(depth, rgb, p, rng=rng)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert (want[1] >= 0).sum() > 300 and (want[1] < 0).sum() > 50
    s0 = Q.score(want, rows[11], p, SHAPE)
    perm = rng.permutation(len(want[0]))
    s1 = Q.score((want[0][perm], want[1][perm], want[2]), (rows[11][0][perm], rows[11][1][perm], rows[11][2]), p, SHAPE)
    assert _bits(s0[0]) == _bits(s1[0]) and s0[1] == s1[1] and np.isfinite(s0[0])


def test_grey_score_does_not_see_a_brightness_offset(scene):
    p, rows = scene
    depth, rgb = QI.frame(QI.query_pose(2, 0))
    assert rgb.max() <= 245 and rgb.min() >= 10  # +10 saturates nowhere
    n, bw, bh = 1200, 4, 4
    for kf_id, k in rows.items():
        a = Q.sums(Q.describe(depth, rgb, p), k)
        b = Q.sums(Q.describe(depth, rgb + np.uint8(10), p), k)
        assert a[1] != b[1] and a[0] != b[0]  # the sums do change
        ga, gb = Q.grey_score(a[0], a[1], n, bw, bh), Q.grey_score(b[0], b[1], n, bw, bh)
        assert _bits(ga) == _bits(gb) and ga > 0.0


def test_default_params_round_trip():
    p = capi.RelocParams()
    assert {k: getattr(p, k) for k in Q.DEFAULTS} == {k: (v if isinstance(v, int) else float(np.float32(v))) for k, v in Q.DEFAULTS.items()}
    r = capi.RelocaliseParams()
    assert (r.max_tries, r.min_stage, r.min_valid_fraction, r.max_rms) == (3, 2, 0.5, float(np.float32(0.01)))
    assert bytes(r.icp) == bytes(capi.AlignIcpParams()) and bytes(r.sdf) == bytes(capi.AlignParams())


# ---- 2. the shared header on the host -----------------------------------------------------------------------------------
@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_score_header_on_the_host_gives_the_restatements_bits(scene, tmp_path):
    p, rows = scene
    exe = str(tmp_path / "reloc_score_print")
    src = os.path.join(ROOT, "tests", "cpp_reloc", "reloc_score_print.cpp")
    r = subprocess.run([CXX, "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", src, "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cases = []
    for k, rung in itertools.product(range(len(rows)), range(2)):
        q = Q.describe(*QI.frame(QI.query_pose(k, rung)), p)
        for kf_id, row in rows.items():
            cases.append(Q.sums(q, row) + (1200, 4, 4, 1.0, 2.55e4, 300))
    # the edges: sums near the top of their ranges (a 128-bit N), a negative sum, no overlap, too little overlap
    cases += [(2 ** 63 - 5, -(2 ** 36) + 3, 12345678901, 700, 1200, 16, 16, 0.37, 1.5e3, 300),
              (10 ** 17, 10 ** 9 + 7, 0, 0, 1200, 4, 4, 1.0, 2.55e4, 0), (10 ** 12, -10 ** 6, 999, 299, 1200, 4, 4, 1.0, 2.55e4, 300),
              (0, 0, 0, 1, 1, 1, 1, 1.0, 1.0, 1)]
    text = "".join("%d %d %d %d %d %d %d %.9g %.9g %d\n" % c for c in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60).stdout.split("\n")
    assert len(out) == len(cases) + 1
    for line, (sd2, sd, sz2, m, n, bw, bh, gw, dw, mo) in zip(out, cases):
        g = Q.grey_score(sd2, sd, n, bw, bh)
        s = float("inf") if m < mo else float(np.float32(gw)) * g + float(np.float32(dw)) * Q.depth_score(sz2, m)
        assert line.split() == [_bits(g)[::-1].hex(), _bits(s)[::-1].hex()], (line, sd2, sd, sz2, m)
    assert Q.score((np.zeros(1200, np.uint32), np.full(1200, -1, np.int32), 0), rows[10], p, SHAPE)[0] == float("inf")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_struct_sizes_match_a_compiled_probe(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tf_fusion.h"\nint main() {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(tf_reloc_params), sizeof(tf_relocalise_params),\n'
                   '         offsetof(tf_relocalise_params, sdf), sizeof(tf_reloc_try), offsetof(tf_reloc_try, track),\n'
                   '         sizeof(tf_relocalise_result), offsetof(tf_relocalise_result, pose), offsetof(tf_relocalise_result, tries));\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    r = subprocess.run([CXX, "-std=c++14", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    P, T, X = capi.RelocaliseParamsC, capi.RelocTry, capi.RelocaliseResult
    assert got == [C.sizeof(capi.RelocParamsC), C.sizeof(P), P.sdf.offset, C.sizeof(T), T.track.offset, C.sizeof(X), X.pose.offset,
                   X.tries.offset]


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_mirror_program_compiles(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp_reloc", "mirror_reloc.cpp")
    r = subprocess.run([CXX, "-std=c++14", "-O0", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-c", src,
                        "-o", str(tmp_path / "mirror_reloc.o")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- 3. the input scene -------------------------------------------------------------------------------------------------
def test_keyframes_lie_far_apart_and_every_ray_hits():
    poses = QI.keyframe_poses()
    assert len(poses) >= 5
    for a, b in itertools.combinations(poses, 2):
        t, r = QI.apart(a, b)
        assert t >= QI.MIN_APART_T or r >= QI.MIN_APART_R, (t, r)
    for k, pose in enumerate(poses):
        assert QI.all_rays_hit(pose), k
        for rung in range(len(QI.QUERY_RUNGS)):
            assert QI.all_rays_hit(QI.query_pose(k, rung)), (k, rung)
    for far in QI.far_poses():  # the far keyframes see the faces too: their descriptors have depth everywhere
        assert (QI.frame(far)[0] > 0).mean() > 0.9
        for pose in poses:
            assert QI.apart(far, pose)[0] > 1.0


def test_every_query_ranks_its_own_keyframe_first(scene):
    p, rows = scene
    for k in range(len(rows)):
        for rung, (metres, degrees) in enumerate(QI.QUERY_RUNGS):
            q = Q.describe(*QI.frame(QI.query_pose(k, rung)), p)
            ranked = Q.rank(q, rows, p, SHAPE)
            print("keyframe %d, %.0f mm / %.0f deg: first %d at %.1f over %d blocks, second %d at %.1f, margin %.1f" % (
                10 + k, 1e3 * metres, degrees, ranked[0][0], ranked[0][1], ranked[0][2], ranked[1][0], ranked[1][1],
                ranked[1][1] - ranked[0][1]))
            assert len(ranked) == len(rows) and ranked[0][0] == 10 + k
            assert ranked[1][1] > ranked[0][1]


def _tracker_restated(ref, depth, start):
    """tf_track_frame restated (the ICP on analytic maps of the start, then the SDF alignment from its pose) and
    tf_relocalise's acceptance test at its defaults -> (accepted, text)"""
    V, N = II.hand_model_maps(start)
    icp, _ = K.align(depth, start, V, N, start, I.CAM, K.params())
    if icp["status"] > K.MAX_ITERS:
        return False, "icp status %d, %d valid" % (icp["status"], icp["n_valid_last"])
    sdf, _ = R.align(ref, depth, icp["pose"], I.CAM, R.params())
    ok = (sdf["status"] <= R.MAX_ITERS and sdf["n_sampled"] > 0 and sdf["n_valid_last"] >= 0.5 * sdf["n_sampled"] and
          sdf["rms_last"] <= 0.01)
    return ok, "icp status %d, sdf status %d, %d of %d valid, rms %.3g" % (icp["status"], sdf["status"], sdf["n_valid_last"],
                                                                         sdf["n_sampled"], sdf["rms_last"])


def test_the_tracker_holds_from_the_near_keyframe_and_not_from_the_far_ones(scene):
    from tests.raycast_ref import RefVolume
    p, rows = scene
    ref = RefVolume(*I.hand_corner(), I.HAND_RES)
    j = 3
    depth, rgb = QI.frame(QI.query_pose(j, 1))
    ok, text = _tracker_restated(ref, depth, QI.keyframe_poses()[j])
    print("from keyframe %d: %s" % (10 + j, text))
    assert ok
    q = Q.describe(depth, rgb, p)
    for k, far in enumerate(QI.far_poses()):
        ok, text = _tracker_restated(ref, depth, far)
        s, m = Q.score(q, Q.describe(*QI.frame(far), p), p, SHAPE)
        print("from far keyframe %d (%.2f m, %.1f deg off): %s; score %.1f over %d blocks" % ((k,) + QI.apart(far, QI.query_pose(j, 1)) + (text, s, m)))
        assert not ok and np.isfinite(s)  # a candidate that no try accepts
