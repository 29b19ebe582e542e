"""Inputs of the exposure-compensation tests (a helper, not a test module): the textured hand plane of
align_color_inputs.py seen by a camera at another exposure, the starts of both photometric aligners, and the recorded
measurements the device tests rest on."""
import numpy as np

from tests import align_color_inputs as CI
from tests import align_exposure_ref as E
from tests import align_icp_color_inputs as XI
from tests import align_inputs as I

CAM = I.CAM
# (gain, offset) of the exposed frames: every colour channel rint(g * v + 255 * o).  None clips the texture's 28..228.
EXPOSURES = [(0.8, 0.06), (1.1, -0.04), (0.6, 0.10)]
SDF_STARTS = [1, 3]               # of align_color_inputs.hand_starts()
ICP_STARTS = [(0.010, 0.0), (0.030, 0.0)]  # rungs of align_icp_color_inputs.PLANE_RUNGS: 10 mm and 30 mm in the plane
MAP_PAIR = (1.25, -0.07)          # the start pair of the map tests

# Measured by tests/test_align_exposure_cpu.py with the restatement (tests/align_exposure_ref.py), printed by
#   python -m pytest tests/test_align_exposure_cpu.py -s -k measurement
# On the unmodified frame the estimate is not (1, 0): the trilinear field loses some of the texture's contrast.  (g_id, o_id)
# is that estimate (the mean over the starts); an exposed frame's estimate should be (g_id / g, o_id - g_id * o / g), and
# DEV_G, DEV_O are the largest deviations from that over every exposure and start.  The device tests allow twice them, for
# the u8 rounding of the frame.
# tf_align_frame_color (CI.PARAMS, starts 1 and 3): both starts give 0.988436, 0.005818; the deviations are 1.97e-3, 1.14e-3.
SDF_ID = (0.988436, 0.005818)
SDF_DEV_G, SDF_DEV_O = 2.0e-3, 1.2e-3
# tf_align_frame_icp_color (defaults, from 10 and 30 mm): 0.988802, 0.005675 and 0.988886, 0.005627; deviations 2.00e-3, 1.17e-3.
ICP_ID = (0.988844, 0.005651)
ICP_DEV_G, ICP_DEV_O = 2.1e-3, 1.2e-3


def predicted(ident, g, o):
    """the pair an exposed frame should end at, from the unmodified frame's"""
    return ident[0] / g, ident[1] - ident[0] * o / g


def plane_frame(exposure=None):
    """(depth, rgba) of the textured plane from hand_pose(), rgba as a camera at `exposure` (gain, offset) sees it"""
    depth, rgba = CI.hand_frame(I.hand_pose())
    return depth, (rgba if exposure is None else E.expose(rgba, *exposure))


def sdf_start(k):
    dt, rv = CI.hand_starts()[k]
    return I.perturb(I.hand_pose(), dt, rv)


def icp_start(rung):
    return XI.plane_start(*rung)


def grey_frame(level=150):
    """the plane's depth with one grey level in every pixel: the gain cannot be told from the offset"""
    depth, rgba = CI.hand_frame(I.hand_pose())
    out = rgba.copy()
    out[..., :3] = np.where(rgba[..., 3:] != 0, level, 0)
    return depth, out
