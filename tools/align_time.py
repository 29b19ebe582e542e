"""Device time of tf_align_frame_device on the S-room, with tf_refine_frame_in_voxel_device as the yardstick.

S-room (640x480 @ 5 mm, 2^19-slot pool): one full orbit (the bench's pre-roll) is integrated, then ten orbit depth images
are aligned from their poses moved by 1 cm and turned by 0.5 degrees.  Times are HIP events on the handle's stream around
R back-to-back calls after W warm-up calls (enqueue only: an alignment never waits for the host).  Reported:
  us_per_evaluation[stride]   (a call of 8 steps - a call of none) / 8 at one level of that stride, eps 0
  us_per_idle_launch_pair     (16 steps - none) / 16 with min_valid above the pixel count: every pair behind the first stops
  us_per_default_call         the default three-level call, and how many evaluations it took on the first view
  us_per_refine_frame         k_refine_frame on the same volume and views, its depth copy subtracted (tools/refine_time.py)
One JSON line.  Needs the GPU; run it under a time limit:

    timeout -k 10 900 python tools/align_time.py [--orbit 200] [--reps 20]

--counter-run N times nothing: it issues N one-evaluation calls at stride 1 and N refine calls and ends, for a run under a
profiler (kernel durations, or one set of hardware counters per run).
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


def _perturb(pose, rng):
    """1 cm along and 0.5 degrees about random directions (about the camera centre)"""
    t = rng.normal(size=3)
    w = rng.normal(size=3)
    t, w = 0.01 * t / np.linalg.norm(t), np.radians(0.5) * w / np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    th = np.linalg.norm(w)
    E = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    P = np.asarray(pose, np.float64).reshape(3, 4).copy()
    P[:, :3] = E @ P[:, :3]
    P[:, 3] += t
    return P.astype(np.float32)


def run(hip, orbit, reps, counter_run=0):
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
        vol.update_meshes()  # the neighbour table: the sampler reads it
        vol.sync()
        n_chunks = int(vol.stats().n_chunks)
        P = cam.width * cam.height
        rng = np.random.default_rng(0)
        src, starts, poses = [], [], []
        for d, pose in frames:
            b = hip.malloc(4 * P)
            hip.upload(b, d)
            src.append(b)
            poses.append(pose)
            starts.append(_perturb(pose, rng))
        d_res = hip.malloc(C.sizeof(capi.AlignResult))
        it = iter(range(1 << 30))

        def call(params):
            def fn():
                k = next(it) % len(src)
                vol.align_frame_device(src[k], starts[k], params, d_res)
            return fn

        if counter_run:  # for a profiler: a few single-evaluation calls at stride 1 and as many refine calls, nothing timed
            one = capi.AlignParams(levels=[(1, 0)])
            work, wgt = hip.malloc(4 * P), hip.malloc(4 * P)
            for k in range(counter_run):
                vol.align_frame_device(src[k % len(src)], starts[k % len(src)], one, d_res)
                hip.ck(hip.h.hipMemcpyAsync(work, src[k % len(src)], 4 * P, 3, stream), "hipMemcpyAsync")
                vol.refine_frame_device(work, wgt, poses[k % len(src)])
            vol.sync()
            for p in src + [work, wgt, d_res]:
                hip.h.hipFree(p)
            return {"counter_run": counter_run, "n_chunks": n_chunks}
        out = {}
        per_eval = {}
        for stride in (1, 2, 4):
            t8 = timed(hip, stream, call(capi.AlignParams(levels=[(stride, 8)], eps_t=0.0, eps_r=0.0)), 3, reps)
            t0 = timed(hip, stream, call(capi.AlignParams(levels=[(stride, 0)], eps_t=0.0, eps_r=0.0)), 3, reps)
            per_eval[str(stride)] = round((t8 - t0) / 8, 2)
            out["us_per_call_of_one_evaluation_stride_%d" % stride] = round(t0, 2)
        big = cam.width * cam.height + 1
        t16 = timed(hip, stream, call(capi.AlignParams(levels=[(1, 16)], min_valid=big)), 3, reps)
        t0 = timed(hip, stream, call(capi.AlignParams(levels=[(1, 0)], min_valid=big)), 3, reps)
        us_default = timed(hip, stream, call(capi.AlignParams()), 3, reps)
        vol.align_frame_device(src[0], starts[0], capi.AlignParams(), d_res)
        vol.sync()
        raw = np.empty(C.sizeof(capi.AlignResult), np.uint8)
        hip.download(d_res, raw)
        first = vol.align_result(raw)
        dt = float(np.linalg.norm(first["pose"][:, 3] - poses[0][:, 3]))
        # the yardstick on the same volume: k_refine_frame, its depth copy subtracted
        work, wgt = hip.malloc(4 * P), hip.malloc(4 * P)

        def copy_only():
            k = next(it) % len(src)
            hip.ck(hip.h.hipMemcpyAsync(work, src[k], 4 * P, 3, stream), "hipMemcpyAsync")

        def copy_refine():
            k = next(it) % len(src)
            hip.ck(hip.h.hipMemcpyAsync(work, src[k], 4 * P, 3, stream), "hipMemcpyAsync")
            vol.refine_frame_device(work, wgt, poses[k])

        us_copy = timed(hip, stream, copy_only, 3, reps)
        us_refine = timed(hip, stream, copy_refine, 3, reps) - us_copy
        vol.sync()
        for p in src + [work, wgt, d_res]:
            hip.h.hipFree(p)
        out.update({"scene": "room", "image": [cam.width, cam.height], "res_m": float(res), "orbit_frames": orbit,
                    "n_chunks": n_chunks, "us_per_evaluation": per_eval, "us_per_idle_launch_pair": round((t16 - t0) / 16, 2),
                    "us_per_default_call": round(us_default, 1), "default_call_evaluations": first["evaluations"],
                    "default_call_status": first["status"], "default_call_rms": [float(first["rms_first"]), float(first["rms_last"])],
                    "default_call_valid": [first["n_valid_last"], first["n_sampled"]], "default_call_m_from_orbit_pose": round(dt, 5),
                    "us_per_refine_frame": round(us_refine, 1),
                    "evaluation_over_refine": round(per_eval["1"] / us_refine, 3) if us_refine > 0 else None, "reps": reps})
        return out
    finally:
        vol.close()
        hip.h.hipStreamDestroy(stream)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--orbit", type=int, default=200, help="frames integrated before timing (the bench's pre-roll)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--counter-run", type=int, default=0, metavar="N",
                    help="no timing: N one-evaluation calls at stride 1 and N refine calls, for a run under a profiler")
    args = ap.parse_args()
    hip = Hip()
    if capi.lib().tf_device_count() <= 0:
        sys.exit("no HIP device: this tool measures the MI355X and has no CPU path")
    print(json.dumps(run(hip, args.orbit, args.reps, args.counter_run)), flush=True)


if __name__ == "__main__":
    main()
