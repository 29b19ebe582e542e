"""The integrator parameters of tests/test_gpu_integrator_params.py on the oracle alone: every (parameter set, weight)
pair the GPU test uses changes the voxels of the room against the MobileFusion default -- the weights of the chunks both
runs hold, and the chunk list wherever the truncation changes -- and none produces NaN.  A device that ignored
tf_set_truncation / tf_set_weight therefore cannot pass the GPU test, and the GPU test may compare every voxel bit for bit.
Also: de-integration under a non-unit weight is not an exact inverse (the GPU test then pins its rounding), and weight 3
reaches the w > 50 class of K-A's ballots and the mesher within the textured run."""
import functools

import numpy as np
import pytest

from tests import integrator_params as P


@functools.lru_cache(maxsize=None)
def _default(flow, color=True):
    if flow == "call_by_call":
        return P.oracle_call_by_call(P.DEFAULT, color)
    return P.oracle_stream(P.DEFAULT)


def _used_cases():
    cases = P.CALL_BY_CALL + P.STREAMED + P.TEXTURED + [P.KEYFRAME] + P.READERS
    cases += [(P.SETTER_TRUNCATION, 1.0), (0, P.SETTER_WEIGHT)]
    return sorted(set(cases))


@pytest.mark.parametrize("case", _used_cases(), ids=lambda c: "set%d-w%g" % c)
def test_every_case_changes_the_streamed_room(case):
    lists_differ = P.assert_differs(P.oracle_stream(case), _default("stream"), "stream %s" % (case,))
    assert lists_differ == (P.SETS[case[0]] != P.SETS[0]), "the chunk list follows the truncation alone"


@pytest.mark.parametrize("color", [True, False], ids=["colour", "depth_only"])
@pytest.mark.parametrize("case", P.CALL_BY_CALL, ids=lambda c: "set%d-w%g" % c)
def test_every_call_by_call_case_changes_the_voxels(case, color):
    P.assert_differs(P.oracle_call_by_call(case, color), _default("call_by_call", color), "call by call %s" % (case,))


@pytest.mark.parametrize("w", P.DEINTEGRATE_WEIGHTS)
def test_deintegration_leaves_a_rounding_residue(w):
    """Frames 0..2 integrated, 0 and 1 de-integrated: the weights left are those of frame 2 alone plus a residue of the
    float additions and subtractions -- non-zero, so the device must round exactly as the oracle does."""
    case = next(c for c in P.CALL_BY_CALL if c[1] == w)
    ov = P.oracle_call_by_call(case)
    only = P.oracle_volume(case)
    P.frame_call_by_call(only, P.room(P.ROOM_FRAMES[-1]), True, P.ROOM_FRAMES[-1])
    ids, _, wt = P.volume_arrays(ov)
    oids, _, owt = P.volume_arrays(only)
    assert np.array_equal(ids, oids) or len(ids) > len(oids)
    row = {tuple(c): i for i, c in enumerate(ids.tolist())}
    sel = np.array([row[tuple(c)] for c in oids.tolist()])
    res = wt[sel] - owt
    both = (wt[sel] > 0) & (owt > 0)
    assert both.sum() > 10000
    assert (res[both] != 0).sum() > 100, "de-integration left no residue"
    assert np.abs(res[both]).max() < 1e-3 * np.abs(owt[both]).max()  # (a rounding residue, not a missed frame)
    assert ((wt > 0) & (wt != np.round(wt))).any()


def test_weight_three_reaches_the_heavy_class_within_the_textured_run():
    heavy = lambda case: int((P.volume_arrays(P.oracle_textured(case)[0])[2] > 50).sum())
    case = next(c for c in P.TEXTURED if c[1] == 3.0 and c[0] == 0)
    assert heavy(P.DEFAULT) == 0 and heavy(case) > 100000
