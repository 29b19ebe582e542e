"""The hand-built pre-processing cases (tests/pre_inputs.py) on the CPU: the numpy restatement (tests/pre_ref.py)
equals the oracle bit for bit on every case, the Jacobi form of refineKeyframesSIMD equals its sequential form, and
every case meets the coverage it promises -- computed from the restatement's outputs alone, so that the device test
(tests/test_gpu_pre_edges.py) compares against inputs known to sit on the edges they are named after."""
import numpy as np
import pytest

from oracle import api as O
from tests import pre_inputs as I
from tests import pre_ref as R


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ids(cases):
    return [c.name for c in cases]


NORMAL_MAP = I.normal_map_cases()
DEPTH_NORMAL = I.refine_depth_normal_cases()
COLOR_VALID = I.color_valid_cases()
COLOR_QUALITY = I.color_quality_cases()
NEWFRAME = I.refine_newframe_cases()
KEYFRAME = I.refine_keyframe_cases()
FRAME_DEPTH = I.frame_depth_cases()


def test_case_names_are_unique():
    for cases in (NORMAL_MAP, DEPTH_NORMAL, COLOR_VALID, COLOR_QUALITY, NEWFRAME, KEYFRAME, FRAME_DEPTH):
        assert len(set(_ids(cases))) == len(cases)


@pytest.mark.parametrize("case", NORMAL_MAP, ids=_ids(NORMAL_MAP))
def test_normal_map(case):
    n = R.normal_map(case.depth, case.cam)
    assert _same(n, O.pre_normal_map(case.depth, case.cam))
    case.promise(n)


@pytest.mark.parametrize("case", DEPTH_NORMAL, ids=_ids(DEPTH_NORMAL))
def test_refine_depth_normal(case):
    n2, d2 = R.refine_depth_normal(case.normal, case.depth, case.cam)
    n_o, d_o = O.pre_refine_depth_normal(case.normal, case.depth, case.cam)
    assert _same(n2, n_o) and _same(d2, d_o)
    case.promise(n2, d2)


@pytest.mark.parametrize("case", COLOR_VALID, ids=_ids(COLOR_VALID))
def test_color_valid(case):
    f = R.color_valid(case.normal, case.cam)
    assert np.array_equal(f, O.pre_color_valid(case.normal, case.cam))
    case.promise(f)


@pytest.mark.parametrize("case", COLOR_QUALITY, ids=_ids(COLOR_QUALITY))
def test_color_quality(case):
    q = R.color_quality(case.depth, case.normal, case.rgb, case.cam)
    assert _same(q, O.pre_color_quality(case.depth, case.normal, case.rgb, case.cam))
    case.promise(q)


@pytest.mark.parametrize("case", NEWFRAME, ids=_ids(NEWFRAME))
def test_refine_newframe(case):
    out = R.refine_newframe(case.depth_ref, case.depth_new, case.cam, case.T)
    assert _same(out, O.pre_refine_newframe(case.depth_ref, case.depth_new, case.cam, case.T))
    case.promise(out)


@pytest.mark.parametrize("case", KEYFRAME, ids=_ids(KEYFRAME))
def test_refine_keyframe(case):
    args = (case.depth_ref, case.weight, case.depth_new, case.cam, case.T)
    d_s, w_s = R.refine_keyframe_sequential(*args)
    d_j, w_j, rounds = R.refine_keyframe_jacobi(*args)
    d_o, w_o = O.pre_refine_keyframe(*args)
    assert _same(d_s, d_o) and _same(w_s, w_o), "the restatement differs from the oracle"
    assert _same(d_j, d_s) and _same(w_j, w_s), "the fixed point differs from the sequential sweep"
    assert rounds <= case.cam.width * case.cam.height // 8 + 1
    case.promise(d_s, w_s, rounds)


def test_chain_round_counts():
    """the numbers DESIGN.md quotes: a weight-0 chain takes one round per row, a weight-1 chain dies out"""
    counts = {}
    for c in KEYFRAME:
        if c.name.startswith(("key_chain", "key_room")):
            counts[c.name] = R.refine_keyframe_jacobi(c.depth_ref, c.weight, c.depth_new, c.cam, c.T)[2]
    assert counts["key_chain_w0_16x64"] == 61
    assert counts["key_chain_w0_16x300"] >= 290
    assert counts["key_chain_w0_16x300"] > 256, "the case exists to pass the old 256-round cap"
    assert counts["key_chain_w1_16x64"] < 30


@pytest.mark.parametrize("case", FRAME_DEPTH, ids=_ids(FRAME_DEPTH))
def test_frame_depth_cases_cover_what_they_promise(case):
    zo, ref = O.pre_frame_depth(case.z, case.maximum_depth, case.depth_scale, case.d)
    case.promise(zo, ref)
    assert case.z.shape[1] % 8 == 0


@pytest.mark.parametrize("width", [11, 12, 19, 20, 21, 27, 2, 1])
def test_keyframe_pass_refuses_widths_without_whole_groups(width):
    """refineKeyframesSIMD loads and stores 8 pixels at a time: at W % 8 != 0 the last group of a row runs into the
    next one (and past the image in the last row), which has no result to match.  The oracle's wrapper and both
    forms of the restatement refuse such widths instead of reading past the arrays."""
    cam = I.room_cam(width, 5)
    d = np.ones((5, width), np.float32)
    for fn in (O.pre_refine_keyframe, R.refine_keyframe_sequential, R.refine_keyframe_jacobi):
        with pytest.raises(ValueError):
            fn(d, d, d, cam, I.I34)


def test_color_quality_needs_two_columns():
    """BORDER_REFLECT_101 has no neighbour to fold onto in a one-pixel-wide image"""
    cam = I.room_cam(1, 5)
    with pytest.raises(ValueError):
        O.pre_color_quality(np.ones((5, 1), np.float32), np.zeros((3, 5, 1), np.float32), np.zeros((5, 1, 3), np.uint8), cam)
