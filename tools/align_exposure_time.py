"""Device time of the two photometric aligners with exposure compensation off and on (tf_align_set_exposure).

S-room (640x480 @ 5 mm, 2^19-slot pool), as tools/align_color_time.py: one full orbit is integrated, then ten orbit frames
(depth and colour) are aligned from their poses moved by 1 cm and turned by 0.5 degrees.  Times are HIP events on the
handle's stream around R back-to-back calls after W warm-up calls (enqueue only).  Reported for tf_align_frame_color_device
("sdf") and for tf_align_frame_icp_color_device with the model maps raycast once at the start pose ("icp"), each with the
setting off and -- where the library has it -- on (the defaults: gain and offset estimated):
  us_per_evaluation[stride]   (a call of 8 steps - a call of none) / 8 at one level of that stride, eps 0
  us_per_default_call         the default three-level call
and on_over_off[stride], the ratio of the two evaluations.  The off figures are what the parent commit's library gives: the
off path enqueues the same launches.  One JSON line.  Needs the GPU; run it under a time limit:

    timeout -k 10 900 python tools/align_exposure_time.py [--orbit 200] [--reps 20]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from texturefusion_amd import capi, synth  # noqa: E402
from align_time import _perturb  # noqa: E402
from raycast_time import Hip, timed  # noqa: E402


def run(hip, orbit, reps):
    cam = synth.Camera()
    res = np.float32(0.005)
    pool = 1 << 19
    stream = hip.stream()
    vol = capi.Volume(res, cam, max_chunks=pool, max_list=1 << 18, mesh_blocks=pool // 4, stream=stream)
    has_setting = hasattr(vol, "align_set_exposure")
    try:
        frames = []
        for k in range(orbit):
            d, rgba, _, pose = synth.room_frame(k, cam, with_quality=False)
            vol.integrate_frame_host(d, rgba, pose.reshape(12), None, k)
            if k % max(1, orbit // 10) == 0:
                frames.append((d, rgba, pose))
        vol.update_meshes()  # the neighbour table: the sampler reads it
        vol.sync()
        P = cam.width * cam.height
        rng = np.random.default_rng(0)
        icp_default = capi.AlignIcpColorParams()
        src, col, starts, vmaps, nmaps = [], [], [], [], []
        for d, rgba, pose in frames:
            b, c, dv, dn = hip.malloc(4 * P), hip.malloc(4 * P), hip.malloc(12 * P), hip.malloc(12 * P)
            hip.upload(b, d)
            hip.upload(c, np.ascontiguousarray(rgba, np.uint8))
            start = _perturb(pose, rng)
            vol.raycast_device(start, icp_default.icp.ray_near, icp_default.icp.ray_far, icp_default.icp.ray_max_steps, d_normal=dn,
                               d_vertex=dv)
            src.append(b)
            col.append(c)
            starts.append(start)
            vmaps.append(dv)
            nmaps.append(dn)
        vol.sync()
        d_res = hip.malloc(C.sizeof(capi.AlignColorResult))
        it = iter(range(1 << 30))

        def sdf(params):
            def fn():
                k = next(it) % len(src)
                vol.align_frame_color_device(src[k], col[k], starts[k], params, d_res)
            return fn

        def icp(params):
            def fn():
                k = next(it) % len(src)
                vol.align_frame_icp_color_device(src[k], col[k], starts[k], vmaps[k], nmaps[k], starts[k], params, d_res)
            return fn

        out = {}
        for setting in (["off", "on"] if has_setting else ["off"]):
            if has_setting:
                vol.align_set_exposure(capi.AlignExposure() if setting == "on" else None)
            out[setting] = {}
            for name, call, make in (("sdf", sdf, capi.AlignColorParams), ("icp", icp, capi.AlignIcpColorParams)):
                per_eval = {}
                for stride in (1, 2, 4):
                    t8 = timed(hip, stream, call(make(levels=[(stride, 8)], eps_t=0.0, eps_r=0.0)), 3, reps)
                    t0 = timed(hip, stream, call(make(levels=[(stride, 0)], eps_t=0.0, eps_r=0.0)), 3, reps)
                    per_eval[str(stride)] = round((t8 - t0) / 8, 2)
                out[setting][name] = {"us_per_evaluation": per_eval,
                                      "us_per_default_call": round(timed(hip, stream, call(make()), 3, reps), 1)}
        if has_setting:
            vol.align_set_exposure(None)
            out["on_over_off"] = {name: {s: round(out["on"][name]["us_per_evaluation"][s] / out["off"][name]["us_per_evaluation"][s], 3)
                                         for s in ("1", "2", "4") if out["off"][name]["us_per_evaluation"][s] > 0}
                                  for name in ("sdf", "icp")}
        vol.sync()
        for p in src + col + vmaps + nmaps + [d_res]:
            hip.h.hipFree(p)
        out.update({"scene": "room", "image": [cam.width, cam.height], "res_m": float(res), "orbit_frames": orbit,
                    "n_chunks": int(vol.stats().n_chunks), "reps": reps, "has_setting": has_setting})
        return out
    finally:
        vol.close()
        hip.h.hipStreamDestroy(stream)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--orbit", type=int, default=200, help="frames integrated before timing (the bench's pre-roll)")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    hip = Hip()
    if capi.lib().tf_device_count() <= 0:
        sys.exit("no HIP device: this tool measures the MI355X and has no CPU path")
    print(json.dumps(run(hip, args.orbit, args.reps)), flush=True)


if __name__ == "__main__":
    main()
