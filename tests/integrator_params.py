"""The integrator parameters the device is tested under (tests/test_gpu_integrator_params.py) and the oracle's side of
the flows it runs them through.  tests/test_integrator_params_cpu.py runs the same oracle flows without a GPU and checks
that every choice below changes the voxels (so a device that ignored tf_set_truncation / tf_set_weight could not pass)
and produces no NaN (so the GPU test may compare every voxel bit for bit).

The parameter sets are those pinned to the compiled reference (tests/test_ref_pin.py) plus one wide band; each flow runs
a subset of (parameter set, weight) pairs so that the GPU file takes about a minute."""
import numpy as np

from oracle import api as O
from texturefusion_amd import synth
from tests.test_ref_pin import PARAM_SETS, WEIGHTS
from tests.util import RES5

F = np.float32
CAM = synth.Camera()
# the MobileFusion terms at scale 8: a truncation of 0.06-0.25 m over the room, above the selection's fixed negTrunc
# (0.03 m at 5 mm, tf_host_math.h) everywhere -- the positive band of K-A's test is then the wider one
WIDE = (0.0019, 0.00152, 0.001504, 8.0)
SETS = list(PARAM_SETS) + [WIDE]
DEFAULT = (0, 1.0)  # (index into SETS, weight): MobileFusion.h:245-249

# (index into SETS, weight) per flow.  Weight 1e-3 leaves every update below the 0.5 weight floor of K-A (the voxel is
# reset) except where the truncation is tiny: it is paired with set 3, whose truncation crosses zero at z = 1.71 m
CALL_BY_CALL = [(0, 0.5), (1, 3.0), (2, 1.0), (3, WEIGHTS[3]), (4, 0.5), (5, 3.0)]
DEINTEGRATE_WEIGHTS = (0.5, 3.0)
STREAMED = [(1, 0.5), (3, 3.0), (5, 1.0)]
TEXTURED = [(0, 3.0), (1, 0.5), (2, 1.0), (4, 1.0)]  # (set 2 at weight 0.5 leaves the room without a mesh)
KEYFRAME = (3, 0.5)
READERS = [(3, WEIGHTS[3]), (4, 3.0)]
SETTER_TRUNCATION = 4  # the set the ordering flow switches to (from the default)
SETTER_WEIGHT = 3.0

ROOM_FRAMES = range(3)         # call-by-call: three colour frames
STREAM_FRAMES = range(7)       # streamed / setter-ordering flows
TEXTURED_FRAMES = range(5)     # the default weight stays below the w > 50 class here, weight 3 reaches it at frame 1
READER_FRAMES = range(6)


def integrator(case):
    """(index into SETS, weight) -> O.Integrator"""
    k, w = case
    return O.Integrator(*[F(p) for p in SETS[k]], F(w))


def oracle_volume(case):
    return O.Volume(RES5, O.camera_from(CAM), integrator(case))


def room(k, quality=True, wobble=0.0):
    return synth.room_frame(k, CAM, with_quality=quality, wobble=wobble)


def frame_call_by_call(ov, frame, color=True, kf_id=-1):
    """prepare -> integrate -> finalize of one frame (colour + quality, or depth only); returns (ids, needs, new, valid)"""
    depth, rgba, quality, pose = frame
    ids, new = ov.prepare(depth, pose)
    needs = np.zeros(len(ids), np.uint8)
    ov.integrate(depth, rgba if color else None, quality if color else None, pose, ids, needs, 1, kf_id)
    valid = ov.finalize(ids, needs, new)
    return ids, needs, new, valid


def deintegrate(ov, frame, valid, color=True, kf_id=-1):
    """ReIntegrateKeyframe with integrateFlag = 0 over the frame's validChunks (MobileFusion.cpp:135-143)"""
    depth, rgba, quality, pose = frame
    needs = np.ones(len(valid), np.uint8)
    ov.integrate(depth, rgba if color else None, quality if color else None, pose, valid, needs, 0, kf_id)
    return needs


def oracle_call_by_call(case, color=True):
    """the call-by-call flow on the oracle: ROOM_FRAMES integrated, then the first two de-integrated again"""
    ov = oracle_volume(case)
    frames = [room(k) for k in ROOM_FRAMES]
    valids = [frame_call_by_call(ov, f, color, k)[3] for k, f in enumerate(frames)]
    for k in (0, 1):
        deintegrate(ov, frames[k], valids[k], color, k)
    return ov


def oracle_stream(case, frames=STREAM_FRAMES):
    ov = oracle_volume(case)
    for k in frames:
        f = room(k, quality=False)
        ov.integrate_frame(f[0], f[1], f[3])
    return ov


def oracle_textured(case):
    ov = oracle_volume(case)
    oa = O.Atlas(RES5)
    for i, k in enumerate(TEXTURED_FRAMES):
        f = room(k, quality=False)
        ov.frame_textured(oa, f[0], f[1], f[3], synth.pose_inverse16(f[3]), 10 + i)
    return ov, oa


def volume_arrays(ov):
    """(sorted ids, sdf [n, 512], weight [n, 512]) of an oracle volume"""
    ids = ov.list_chunks()
    ids = ids[np.lexsort((ids[:, 2], ids[:, 1], ids[:, 0]))]
    got = [ov.get_chunk(c) for c in ids]
    return ids, np.array([g[0] for g in got], F).reshape(-1, 512), np.array([g[1] for g in got], F).reshape(-1, 512)


def assert_differs(ov, od, what=""):
    """ov (a non-default integrator) holds other voxel weights than od (the default one, same flow) in the chunks both
    hold, and no NaN; returns whether the chunk lists differ too"""
    ids, s, w = volume_arrays(ov)
    dids, ds, dw = volume_arrays(od)
    assert not np.isnan(s).any() and not np.isnan(w).any(), "%s: NaN voxels" % what
    key = lambda a: [tuple(r) for r in a.tolist()]
    drow = {c: i for i, c in enumerate(key(dids))}
    both = [(i, drow[c]) for i, c in enumerate(key(ids)) if c in drow]
    assert both, "%s: no chunk in common with the default run" % what
    a, b = np.array(both).T
    assert not np.array_equal(w[a].view(np.uint32), dw[b].view(np.uint32)), "%s: the integrator changed no voxel weight" % what
    return len(both) != len(ids) or len(both) != len(dids)
