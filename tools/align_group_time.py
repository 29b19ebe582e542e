"""Device time of tf_align_group_device on the S-room, with seven successive tf_align_frame_device calls as the yardstick.

S-room (640x480 @ 5 mm, 2^19-slot pool): one full orbit (the bench's pre-roll) is integrated, then seven consecutive orbit
depth images -- a keyframe group -- are aligned from poses moved by 1 cm and turned by 0.5 degrees.  Times are HIP events
on the handle's stream around R back-to-back calls after W warm-up calls (enqueue only: neither form waits for the host).
Reported:
  us_seven_frame_calls[3]      seven tf_align_frame_device calls, default parameters, one after the other  } three runs
  us_group_seven_bodies[3]     one tf_align_group_device call, the same frames as seven bodies             } each, alternating
  us_group_one_body            the same frames as one rigid body (all moved by one rigid motion)
  us_per_evaluation[n][stride] (a call of 8 steps - a call of none) / 8 at one level of that stride, eps 0, for a group call
                               of n = 1 and n = 7 frames (seven bodies), and frame[stride] for tf_align_frame_device
One JSON line.  Needs the GPU; run it under a time limit:

    timeout -k 10 900 python tools/align_group_time.py [--orbit 200] [--reps 20]

--counter-run N times nothing: it issues N one-evaluation group calls per stride (1, 2, 4) with seven frames, then with
one, and ends, for a run under a profiler (kernel durations of k_galign_rows and k_galign_solve).
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

N = capi.TF_ALIGN_GROUP_MAX_FRAMES


def _move_all(poses, rng):
    """every pose by the same rigid motion: 0.5 degrees about the first camera centre, then 1 cm"""
    moved = _perturb(poses[0], rng).astype(np.float64)
    P0 = np.asarray(poses[0], np.float64).reshape(3, 4)
    E, c = moved[:, :3] @ P0[:, :3].T, P0[:, 3]
    dt = moved[:, 3] - c
    out = []
    for P in poses:
        P = np.asarray(P, np.float64).reshape(3, 4)
        Q = np.concatenate([E @ P[:, :3], (c + E @ (P[:, 3] - c) + dt)[:, None]], 1)
        out.append(Q.astype(np.float32))
    return out


def run(hip, orbit, reps, counter_run=0):
    cam = synth.Camera()
    res = np.float32(0.005)
    pool = 1 << 19
    stream = hip.stream()
    vol = capi.Volume(res, cam, max_chunks=pool, max_list=1 << 18, mesh_blocks=pool // 4, stream=stream)
    try:
        first = orbit // 2
        frames = []
        for k in range(orbit):
            d, rgba, _, pose = synth.room_frame(k, cam, with_quality=False)
            vol.integrate_frame_host(d, rgba, pose.reshape(12), None, k)
            if first <= k < first + N:
                frames.append((d, pose))
        vol.update_meshes()  # the neighbour table: the sampler reads it
        vol.sync()
        n_chunks = int(vol.stats().n_chunks)
        P = cam.width * cam.height
        rng = np.random.default_rng(0)
        src = []
        for d, _ in frames:
            b = hip.malloc(4 * P)
            hip.upload(b, d)
            src.append(b)
        poses = [pose for _, pose in frames]
        starts = [_perturb(pose, rng) for pose in poses]
        rigid = _move_all(poses, rng)
        d_res = hip.malloc(C.sizeof(capi.AlignResult))
        d_gres = hip.malloc(C.sizeof(capi.AlignGroupResult))
        own = list(range(N))

        def frame_calls(params, n=N):
            def fn():
                for k in range(n):
                    vol.align_frame_device(src[k], starts[k], params, d_res)
            return fn

        def group_call(params, n=N, body=own, at=starts):
            def fn():
                vol.align_group_device(src[:n], at[:n], None if body is None else body[:n], params, d_gres)
            return fn

        if counter_run:
            for n in (N, 1):
                for stride in (1, 2, 4):
                    one = capi.AlignParams(levels=[(stride, 0)])
                    for _ in range(counter_run):
                        group_call(one, n)()
            vol.sync()
            for p in src + [d_res, d_gres]:
                hip.h.hipFree(p)
            return {"counter_run": counter_run, "n_chunks": n_chunks,
                    "launch_order": "seven frames at strides 1, 2, 4, then one frame at strides 1, 2, 4; N calls each"}
        default = capi.AlignParams()
        sep, grp = [], []
        for _ in range(3):
            sep.append(round(timed(hip, stream, frame_calls(default), 2, reps), 1))
            grp.append(round(timed(hip, stream, group_call(default), 2, reps), 1))
        one_body = timed(hip, stream, group_call(default, body=None, at=rigid), 2, reps)
        per_eval = {"frame": {}, "1": {}, "7": {}}
        for stride in (1, 2, 4):
            p8 = capi.AlignParams(levels=[(stride, 8)], eps_t=0.0, eps_r=0.0)
            p0 = capi.AlignParams(levels=[(stride, 0)], eps_t=0.0, eps_r=0.0)
            per_eval["frame"][str(stride)] = round((timed(hip, stream, frame_calls(p8, 1), 3, reps) -
                                                    timed(hip, stream, frame_calls(p0, 1), 3, reps)) / 8, 2)
            for n in (1, N):
                per_eval[str(n)][str(stride)] = round((timed(hip, stream, group_call(p8, n), 3, reps) -
                                                       timed(hip, stream, group_call(p0, n), 3, reps)) / 8, 2)
        # what the calls did: evaluations and residuals of the seven bodies, and of the one
        raw = np.empty(C.sizeof(capi.AlignGroupResult), np.uint8)
        group_call(default)()
        vol.sync()
        hip.download(d_gres, raw)
        seven = vol.align_group_result(raw)
        group_call(default, body=None, at=rigid)()
        vol.sync()
        hip.download(d_gres, raw)
        one = vol.align_group_result(raw)
        for p in src + [d_res, d_gres]:
            hip.h.hipFree(p)
        return {"scene": "room", "image": [cam.width, cam.height], "res_m": float(res), "orbit_frames": orbit,
                "group_frames": [first, first + N - 1], "n_chunks": n_chunks, "us_seven_frame_calls": sep,
                "us_group_seven_bodies": grp, "us_group_one_body": round(one_body, 1), "us_per_evaluation": per_eval,
                "seven_bodies_evaluations": [b["evaluations"] for b in seven["body"]],
                "seven_bodies_status": [b["status"] for b in seven["body"]],
                "one_body_evaluations": one["body"][0]["evaluations"], "one_body_status": one["body"][0]["status"],
                "one_body_rms": [float(one["body"][0]["rms_first"]), float(one["body"][0]["rms_last"])],
                "one_body_valid": [one["body"][0]["n_valid_last"], one["body"][0]["n_sampled"]], "reps": reps}
    finally:
        vol.close()
        hip.h.hipStreamDestroy(stream)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--orbit", type=int, default=200, help="frames integrated before timing (the bench's pre-roll)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--counter-run", type=int, default=0, metavar="N",
                    help="no timing: N one-evaluation group calls per stride with seven frames, then with one, for a profiler")
    args = ap.parse_args()
    hip = Hip()
    if capi.lib().tf_device_count() <= 0:
        sys.exit("no HIP device: this tool measures the MI355X and has no CPU path")
    print(json.dumps(run(hip, args.orbit, args.reps, args.counter_run)), flush=True)


if __name__ == "__main__":
    main()
