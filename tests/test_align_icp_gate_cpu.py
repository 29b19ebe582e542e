"""The ICP's normal-compatibility gate without a GPU: what the numpy restatement (tests/align_icp_gate_ref.py) does on the
hand-built corner rendered WITHOUT its edge mask -- the pairs across an edge that the ungated association accepts, that the
gate removes all of them and keeps the good ones, what that does to a whole alignment -- the orientation of the frame
normal, the hand-built plane's cases, and the ABI.

The counts of the first test were taken with tests/align_icp_ref.py and a prototype of the gate before the device code
existed.  A restatement that gives other numbers differs from the text of tf_align_icp_gate.hip's header: the reason is to be
found, not the numbers changed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import align_icp_gate_inputs as GI
from tests import align_icp_gate_ref as G
from tests import align_icp_inputs as II
from tests import align_icp_ref as K
from tests import align_inputs as I
from tests import align_ref as R
from texturefusion_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++")
F = np.float32

# (start, stride) -> (valid ungated, of those on the wrong plane, right pairs kept by the gate, right pairs): first
# evaluation, default parameters, gate cos 20 deg / 0.1 m, analytic maps at the start pose
TABLE = {
    ((0.040, 2.0), 4): (1200, 41, 1000, 1159),
    ((0.060, 3.0), 4): (1200, 58, 983, 1142),
    ((0.080, 5.0), 4): (1200, 101, 943, 1099),
    ((0.120, 8.0), 4): (1187, 166, 869, 1021),
    ((0.120, 8.0), 1): (18958, 2678, 15696, 16280),
}
KEPT_FLOOR = 0.8  # a floor under the lowest share of right pairs kept that was observed (0.851), not a measurement


@pytest.fixture(scope="module")
def corner():
    return I.hand_pose(), GI.corner_unmasked(), GI.true_axis()


def _first_evaluation(corner, rung, stride):
    true, depth, axis = corner
    start = II.ladder_start(*rung)
    V, N = II.hand_model_maps(start)
    rw = G.rows(depth, start, V, N, start, I.CAM, stride, K.params(), G.gate())
    yy, xx = G._sampled(I.CAM, stride)
    on_plane = rw["g"].argmax(1) == axis[yy, xx]  # the associated model normal's axis against the pixel's true plane
    v15, v63 = rw["fl15"] == 15, rw["fl63"] == 63
    return dict(valid=int(v15.sum()), wrong=int((v15 & ~on_plane).sum()), wrong_gated=int((v63 & ~on_plane).sum()),
                kept=int((v63 & on_plane).sum()), right=int((v15 & on_plane).sum()))


@pytest.mark.parametrize("stride", [4, 2, 1])
def test_the_gate_removes_every_pair_across_an_edge_and_keeps_the_good_ones(corner, stride):
    for rung in II.LADDER:
        f = _first_evaluation(corner, rung, stride)
        print("%.0f mm / %.0f deg, stride %d: %d valid ungated, %d on the wrong plane, %d of them left by the gate, %d / %d right "
              "pairs kept" % (1e3 * rung[0], rung[1], stride, f["valid"], f["wrong"], f["wrong_gated"], f["kept"], f["right"]))
        if (rung, stride) in TABLE:
            assert (f["valid"], f["wrong"], f["kept"], f["right"]) == TABLE[(rung, stride)]
        assert f["wrong"] > 0 and f["wrong_gated"] == 0
        assert f["kept"] >= KEPT_FLOOR * f["right"]


@pytest.mark.parametrize("rung", II.LADDER)
def test_whole_alignments_with_and_without_the_gate(corner, rung):
    true, depth, _ = corner
    start = II.ladder_start(*rung)
    V, N = II.hand_model_maps(start)
    p, g = K.params(), G.gate()
    ends = {}
    for name, img in (("unmasked", depth), ("masked", I.hand_depth(true))):
        ru, lu = K.align(img, start, V, N, start, I.CAM, p)
        rg, lg = G.align(img, start, V, N, start, I.CAM, p, g)
        ends[name] = (R.pose_distance(ru["pose"], true), len(lu), R.pose_distance(rg["pose"], true), len(lg))
        print("%.0f mm / %.0f deg, %s: ungated %d evaluations, %.3g m %.3g rad; gated %d evaluations, %.3g m %.3g rad" % (
            1e3 * rung[0], rung[1], name, len(lu), *ends[name][0], len(lg), *ends[name][2]))
        assert ru["status"] == rg["status"] == R.CONVERGED
    (ut, ur), nu, (gt, gr), ng = ends["unmasked"]
    assert gt <= II.ICP_TOL_T and gr <= II.ICP_TOL_R and ng <= nu
    assert ut > II.ICP_TOL_T  # the pairs across the edges bias the ungated solve
    (ut, ur), nu, (gt, gr), ng = ends["masked"]
    assert ut <= II.ICP_TOL_T and ur <= II.ICP_TOL_R and gt <= II.ICP_TOL_T and gr <= II.ICP_TOL_R


@pytest.mark.parametrize("stride", [4, 2, 1])
def test_the_frame_normal_faces_the_camera(corner, stride):
    """every frame normal that exists on the corner has a positive d with the analytic model normal at the true pose"""
    true, depth, _ = corner
    V, N = II.hand_model_maps(true)
    rw = G.rows(depth, true, V, N, true, I.CAM, stride, K.params(), G.gate())
    fn = G.frame_normals(depth, I.CAM, stride, K.params(), G.gate())
    assert fn["ok"].sum() > 0.8 * len(fn["ok"]) and (rw["fl15"][fn["ok"]] == 15).all()
    assert (rw["d"][fn["ok"]] > 0).all()
    # ... and the map form holds the same normals, 0 where there is none or the pixel is not sampled
    yy, xx = G._sampled(I.CAM, stride)
    m = np.zeros(depth.shape, bool)
    m[yy[fn["ok"]], xx[fn["ok"]]] = True
    assert (np.abs(fn["n"]).sum(0) > 0)[m].all() and not fn["n"][:, ~m].any()


@pytest.mark.parametrize("cam", [GI.CAM, GI.CAM_ODD], ids=["160x120", "152x116"])
@pytest.mark.parametrize("stride", [1, 2, 4])
def test_the_hand_built_plane_shows_every_case(cam, stride):
    depth, V, N = GI.plane(cam, stride)
    sampled, inner = GI.border_masks(cam, stride)
    for name, gk in GI.GATES.items():
        rw = G.rows(depth, GI.EYE, V, N, GI.EYE, cam, stride, K.params(), G.gate(**gk))
        fl = rw["flags"]
        for case, (x, y) in GI.centres().items():
            assert fl[y, x] == GI.EXPECT[name][case], (name, case, int(fl[y, x]))
        assert fl[GI.PLAIN[1], GI.PLAIN[0]] == 63, name  # at cosine 1: d d == l2 m2 exactly
        assert not (fl[sampled & ~inner] & 16).any() and not fl[~sampled].any()
        xl, yl = (cam.width - 1) // stride * stride, (cam.height - 1) // stride * stride  # the last sampled column and row
        for x, y in ((0, 24), (xl, 24), (24, 0), (24, yl)):  # a neighbour outside the image on each side
            assert fl[y, x] == 15 and not inner[y, x]
        assert xl + stride >= cam.width and yl + stride >= cam.height
    fn = G.frame_normals(depth, cam, stride, K.params(), G.gate(**GI.GATES["default_cos"]))
    mx, my = GI.centres()["miss"]
    assert fn["n"][2, my, mx] < 0 and not fn["n"][:2, my, mx].any()  # a model miss under a pixel that has a frame normal


# ---- the ABI ------------------------------------------------------------------------------------------------------------
GATE_SYMBOLS = ("tf_align_icp_gate_default", "tf_align_icp_set_gate", "tf_align_icp_get_gate", "tf_align_icp_frame_normals",
                "tf_align_icp_frame_normals_device")


def test_gate_symbols_are_exported_and_bound():
    L = capi.lib()
    for s in GATE_SYMBOLS:
        assert s in capi.SYMBOLS and hasattr(L, s) and getattr(L, s).argtypes is not None, s
    for m in ("align_icp_set_gate", "align_icp_get_gate", "align_icp_frame_normals", "align_icp_frame_normals_device"):
        assert callable(getattr(capi.Volume, m))


def test_gate_defaults_round_trip():
    g = capi.AlignIcpGate()
    assert g.min_normal_cos == G.COS20 == F(np.cos(np.radians(20.0))) and g.max_depth_jump == F(0.1)
    assert F(G.GATE["min_normal_cos"]) == g.min_normal_cos and F(G.GATE["max_depth_jump"]) == g.max_depth_jump
    q = capi.AlignIcpGate(min_normal_cos=0.5, max_depth_jump=np.inf)
    assert q.min_normal_cos == 0.5 and q.max_depth_jump == np.inf
    with pytest.raises(TypeError):
        capi.AlignIcpGate(no_such_field=1)
    assert C.sizeof(capi.AlignIcpGateC) == 8
    assert capi.lib().tf_align_icp_gate_default(None) == capi.TF_ERR_INVALID


def test_the_icp_params_struct_did_not_grow():
    assert C.sizeof(capi.AlignIcpParamsC) == 68 + 16  # embedded in tf_relocalise_params


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_gate_struct_matches_a_compiled_probe(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tf_fusion.h"\nint main() {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(tf_align_icp_gate), offsetof(tf_align_icp_gate, max_depth_jump),\n'
                   '         sizeof(tf_align_icp_params));\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    r = subprocess.run([CXX, "-std=c++14", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [C.sizeof(capi.AlignIcpGateC), capi.AlignIcpGateC.max_depth_jump.offset, C.sizeof(capi.AlignIcpParamsC)]


def test_invalid_arguments_are_refused_ahead_of_the_device():
    L = capi.lib()
    g, on = capi.AlignIcpGate(), C.c_int32(7)
    p = capi.AlignIcpParams()
    z = (C.c_float * 12)()
    assert L.tf_align_icp_set_gate(None, C.byref(g)) == capi.TF_ERR_INVALID
    assert L.tf_align_icp_get_gate(None, C.byref(g), C.byref(on)) == capi.TF_ERR_INVALID and on.value == 7
    assert L.tf_align_icp_frame_normals(None, z, C.byref(p), C.byref(g), z) == capi.TF_ERR_INVALID
    assert L.tf_align_icp_frame_normals_device(None, None, C.byref(p), C.byref(g), None) == capi.TF_ERR_INVALID
