"""Device time of tf_refine_frame_in_voxel_device and tf_distance_from_surface_device on the S-room.

S-room (640x480 @ 5 mm, 2^19-slot pool): one full orbit (the bench's pre-roll) is integrated, then orbit depth images
with +-3 mm of noise are refined against the model (Chisel::RefineFrameInVoxel) and GetDistanceFromSurface is answered
for a million points near the surface.  Times are HIP events on the handle's stream around R back-to-back calls, after W
warm-up calls; each refine call works on a fresh copy of its depth image (a device-to-device copy on the same stream,
timed on its own and subtracted).  One JSON line.  Needs the GPU; run it under a time limit:

    timeout -k 10 900 python tools/refine_time.py [--orbit 200] [--reps 20]
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
from raycast_time import Hip, timed  # noqa: E402


def run(hip, orbit, reps, n_points):
    cam = synth.Camera()
    res = np.float32(0.005)
    pool = 1 << 19
    stream = hip.stream()
    vol = capi.Volume(res, cam, max_chunks=pool, max_list=1 << 18, mesh_blocks=pool // 4, stream=stream)
    hip.h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    try:
        frames = []
        for k in range(orbit):
            d, rgba, _, pose = synth.room_frame(k, cam, with_quality=False)
            vol.integrate_frame_host(d, rgba, pose.reshape(12), None, k)
            if k % max(1, orbit // 10) == 0:
                frames.append((d, pose))
        vol.sync()
        n_chunks = int(vol.stats().n_chunks)
        P = cam.width * cam.height
        rng = np.random.default_rng(0)
        src, poses = [], []
        for d, pose in frames:
            noisy = np.where(d > 0, d + rng.uniform(-0.003, 0.003, d.shape).astype(np.float32), d).astype(np.float32)
            b = hip.malloc(4 * P)
            hip.upload(b, noisy)
            src.append(b)
            poses.append(pose)
        work, wgt = hip.malloc(4 * P), hip.malloc(4 * P)
        it = iter(range(1 << 30))

        def copy_only():
            k = next(it) % len(src)
            hip.ck(hip.h.hipMemcpyAsync(work, src[k], 4 * P, 3, stream), "hipMemcpyAsync")

        def copy_refine():
            k = next(it) % len(src)
            hip.ck(hip.h.hipMemcpyAsync(work, src[k], 4 * P, 3, stream), "hipMemcpyAsync")
            vol.refine_frame_device(work, wgt, poses[k])

        us_copy = timed(hip, stream, copy_only, 3, reps)
        us_refine = timed(hip, stream, copy_refine, 3, reps) - us_copy
        hip.ck(hip.h.hipMemcpyAsync(work, src[0], 4 * P, 3, stream), "hipMemcpyAsync")
        vol.refine_frame_device(work, wgt, poses[0])
        vol.sync()
        w = np.empty(P, np.float32)
        hip.download(wgt, w)
        accepted = float((w > 0).mean())
        ids = vol.list_chunks()
        pts = ((ids[rng.integers(0, len(ids), n_points)] * 8 + rng.uniform(0, 8, (n_points, 3))) * float(res)).astype(np.float32)
        qb = [hip.malloc(12 * n_points), hip.malloc(4 * n_points), hip.malloc(4 * n_points)]
        hip.upload(qb[0], pts)

        def dist():
            vol.distance_from_surface_device(qb[0], n_points, qb[1], qb[2])

        us_dist = timed(hip, stream, dist, 3, reps)
        for p in src + [work, wgt] + qb:
            hip.h.hipFree(p)
        return {"scene": "room", "image": [cam.width, cam.height], "res_m": float(res), "orbit_frames": orbit,
                "n_chunks": n_chunks, "accepted_fraction": round(accepted, 4),
                "us_per_refine_frame": round(us_refine, 1), "us_per_depth_copy_subtracted": round(us_copy, 1),
                "us_per_million_distances": round(us_dist * 1e6 / n_points, 1), "reps": reps}
    finally:
        vol.close()
        hip.h.hipStreamDestroy(stream)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--orbit", type=int, default=200, help="frames integrated before timing (the bench's pre-roll)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=1 << 20)
    args = ap.parse_args()
    hip = Hip()
    if capi.lib().tf_device_count() <= 0:
        sys.exit("no HIP device: this tool measures the MI355X and has no CPU path")
    print(json.dumps(run(hip, args.orbit, args.reps, args.points)), flush=True)


if __name__ == "__main__":
    main()
