"""SHA-256 digests of what the four aligners compute on the hand-built scenes of the tests: for telling whether a change to
their shared machinery (texturefusion_amd/csrc/tf_align_rows.h) moved a bit anywhere.

The scenes are tests/align_inputs.py's 160 x 120 corner and single plane, tests/align_color_inputs.py's textured plane,
tests/align_group_inputs.py's three frames and tests/align_icp_inputs.py's far starts.  For tf_align_frame,
tf_align_frame_color, tf_align_group and tf_align_frame_icp each, one digest per case over the result, every log record
and (where the aligner has them) the residual maps:
  s1        one level at stride 1, every step taken (eps 0)
  s3_small  one level at stride 3 on a 13 x 9 camera: tiles over both borders
  default   the default parameters (three levels)
  too_few   an all-zero depth image: TF_ALIGN_TOO_FEW
  singular  the single plane: TF_ALIGN_SINGULAR
the group once as one rigid body of three frames and once as three bodies.  Only texturefusion_amd.capi is called, so the
tool runs unchanged against another build of the library (TF_LIB=<path to its libtexfusion_hip.so>).  One JSON line:
{"digest": {case: hex}, "status": {case: the statuses reached}}.  Needs the GPU; a few seconds:

    timeout -k 10 120 python tools/align_digest.py
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import align_color_inputs as CI  # noqa: E402
from tests import align_group_inputs as GI  # noqa: E402
from tests import align_icp_inputs as II  # noqa: E402
from tests import align_inputs as I  # noqa: E402
from texturefusion_amd import capi, synth  # noqa: E402

SMALL = synth.Camera(13, 9, 11.0, 11.0, 6.5, 4.5)
TURN = np.radians(0.3) * np.array([0.6, -0.64, 0.48])


def _feed(h, x):
    """x, a nest of dicts, lists, arrays and numbers, into the hash: every value's bytes, keys in sorted order"""
    if isinstance(x, dict):
        for k in sorted(x):
            h.update(k.encode())
            _feed(h, x[k])
    elif isinstance(x, (list, tuple)):
        h.update(b"[%d]" % len(x))
        for y in x:
            _feed(h, y)
    elif isinstance(x, np.ndarray):
        h.update(np.ascontiguousarray(x).tobytes())
    elif isinstance(x, (int, np.integer)):
        h.update(np.int64(x).tobytes())
    else:
        h.update(np.float64(x).tobytes())  # (exact for an f32)


def _digest(*parts):
    h = hashlib.sha256()
    _feed(h, list(parts))
    return h.hexdigest()


def _volume(chunks):
    gv = capi.Volume(I.HAND_RES, I.CAM, max_chunks=1 << 10)
    ids, s, w, c = chunks
    for k in range(len(ids)):
        gv.set_chunk(ids[k], s[k], w[k], c[k])
    gv.sync()
    return gv


def _levels(make, **kw):
    return {"s1": make(levels=[(1, 3)], eps_t=0.0, eps_r=0.0, **kw), "s3": make(levels=[(3, 2)], eps_t=0.0, eps_r=0.0, min_valid=1, **kw),
            "default": make(**kw)}


def frame_cases(corner, plane, out, status):
    true = I.hand_pose()
    start = I.perturb(true, I.HAND_DELTA, TURN)
    depth = I.hand_depth(true)
    p = _levels(capi.AlignParams)

    def run(name, gv, d, par):
        res = gv.align_frame(d, start, par)
        out["frame/" + name] = _digest(res, gv.align_log(), gv.align_residuals(d, start, par))
        status["frame/" + name] = res["status"]

    run("s1", corner, depth, p["s1"])
    run("default", corner, depth, p["default"])
    run("too_few", corner, np.zeros_like(depth), p["default"])
    run("singular", plane, I.hand_depth(true, planes=1), p["s1"])
    corner.raycast_camera(SMALL)
    try:
        run("s3_small", corner, I.hand_depth(true, SMALL, edge_voxels=0.0), p["s3"])
    finally:
        corner.raycast_camera(None)


def color_cases(tex, out, status):
    true = I.hand_pose()
    dt, rv = CI.hand_starts()[3]
    start = I.perturb(true, dt, rv)
    depth, rgba = CI.hand_frame(true)
    p = _levels(capi.AlignColorParams)

    def run(name, d, c, par):
        res = tex.align_frame_color(d, c, start, par)
        out["color/" + name] = _digest(res, tex.align_color_log(), tex.align_color_residuals(d, c, start, par))
        status["color/" + name] = res["status"]

    run("s1", depth, rgba, p["s1"])
    run("default", depth, rgba, p["default"])
    run("too_few", np.zeros_like(depth), rgba, p["default"])
    run("singular", depth, rgba, capi.AlignColorParams(levels=[(1, 3)], photo_weight=0.0))  # the plane by depth alone
    tex.raycast_camera(SMALL)
    try:
        d, c = CI.hand_frame(true, SMALL, edge_voxels=0.0)
        run("s3_small", d, c, p["s3"])
    finally:
        tex.raycast_camera(None)


def group_cases(corner, plane, out, status):
    poses, depths = GI.hand_group()
    starts = GI.move_group(poses, I.HAND_DELTA, TURN)
    p = _levels(capi.AlignParams)

    def run(name, gv, ds, body, par):
        res = gv.align_group(ds, starts, body, par)
        out["group/" + name] = _digest(res, [gv.align_group_log(b) for b in range(res["n_bodies"])])
        status["group/" + name] = [b["status"] for b in res["body"]]

    for tag, body in (("rigid", None), ("bodies", [0, 1, 2])):  # (its masked keyframe alone is singular)
        run(tag + "_s1", corner, depths, body, p["s1"])
        run(tag + "_default", corner, depths, body, p["default"])
        run(tag + "_too_few", corner, [np.zeros_like(d) for d in depths], body, p["default"])
        run(tag + "_singular", plane, [I.hand_depth(P, planes=1) for P in poses], body, p["s1"])
        corner.raycast_camera(SMALL)
        try:
            run(tag + "_s3_small", corner, [I.hand_depth(P, SMALL, edge_voxels=0.0) for P in poses], body, p["s3"])
        finally:
            corner.raycast_camera(None)


def icp_cases(corner, plane, out, status):
    true = I.hand_pose()
    start = II.ladder_start(0.080, 5.0)
    depth = I.hand_depth(true)
    V, N = II.hand_model_maps(start)
    p = _levels(capi.AlignIcpParams)

    def run(name, gv, d, par, maps=True):
        res = gv.align_frame_icp(d, start, None, par)  # the model raycast at the start
        parts = [res, gv.align_icp_log(), gv.align_icp_residuals(d, start, None, par)]
        if maps:  # and one evaluation against the analytic maps
            parts.append(gv.align_icp_residuals(d, true, start, par, vertex=V, normal=N))
        out["icp/" + name] = _digest(*parts)
        status["icp/" + name] = res["status"]

    run("s1", corner, depth, p["s1"])
    run("default", corner, depth, p["default"])
    run("too_few", corner, np.zeros_like(depth), p["default"])
    run("singular", plane, I.hand_depth(true, planes=1), p["s1"], maps=False)
    corner.raycast_camera(SMALL)
    try:
        run("s3_small", corner, I.hand_depth(true, SMALL, edge_voxels=0.0), p["s3"], maps=False)
    finally:
        corner.raycast_camera(None)


def main():
    if capi.lib().tf_device_count() <= 0:
        sys.exit("no HIP device: the digests are of what the MI355X computes")
    corner, plane, tex = _volume(I.hand_corner()), _volume(I.hand_plane()), _volume(CI.hand_plane_textured())
    out, status = {}, {}
    try:
        frame_cases(corner, plane, out, status)
        color_cases(tex, out, status)
        group_cases(corner, plane, out, status)
        icp_cases(corner, plane, out, status)
    finally:
        for gv in (corner, plane, tex):
            gv.close()
    print(json.dumps({"digest": out, "status": status}, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
