"""Device time of tf_align_frame_color_device on the S-room, with tf_align_frame_device (unchanged code) as the yardstick.

S-room (640x480 @ 5 mm, 2^19-slot pool): one full orbit (the bench's pre-roll) is integrated, then ten orbit frames (depth
and colour) are aligned from their poses moved by 1 cm and turned by 0.5 degrees, as tools/align_time.py does.  Times are
HIP events on the handle's stream around R back-to-back calls after W warm-up calls (enqueue only: an alignment never waits
for the host).  Reported, for the colour-aided and for the geometric call alike:
  us_per_evaluation[stride]   (a call of 8 steps - a call of none) / 8 at one level of that stride, eps 0
  us_per_default_call         the default three-level call, and how many evaluations it took on the first view
and color_over_geometric[stride], the ratio of the two evaluations.
One JSON line.  Needs the GPU; run it under a time limit:

    timeout -k 10 900 python tools/align_color_time.py [--orbit 200] [--reps 20]

--counter-run N times nothing: it issues N one-evaluation calls at stride 1 of either kind and ends, for a run under a
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
from align_time import _perturb  # noqa: E402
from raycast_time import Hip, timed  # noqa: E402


def run(hip, orbit, reps, counter_run=0):
    cam = synth.Camera()
    res = np.float32(0.005)
    pool = 1 << 19
    stream = hip.stream()
    vol = capi.Volume(res, cam, max_chunks=pool, max_list=1 << 18, mesh_blocks=pool // 4, stream=stream)
    try:
        frames = []
        for k in range(orbit):
            d, rgba, _, pose = synth.room_frame(k, cam, with_quality=False)
            vol.integrate_frame_host(d, rgba, pose.reshape(12), None, k)
            if k % max(1, orbit // 10) == 0:
                frames.append((d, rgba, pose))
        vol.update_meshes()  # the neighbour table: the sampler reads it
        vol.sync()
        n_chunks = int(vol.stats().n_chunks)
        P = cam.width * cam.height
        rng = np.random.default_rng(0)
        src, col, starts, poses = [], [], [], []
        for d, rgba, pose in frames:
            b, c = hip.malloc(4 * P), hip.malloc(4 * P)
            hip.upload(b, d)
            hip.upload(c, np.ascontiguousarray(rgba, np.uint8))
            src.append(b)
            col.append(c)
            poses.append(pose)
            starts.append(_perturb(pose, rng))
        d_res = hip.malloc(C.sizeof(capi.AlignColorResult))
        it = iter(range(1 << 30))

        def color(params):
            def fn():
                k = next(it) % len(src)
                vol.align_frame_color_device(src[k], col[k], starts[k], params, d_res)
            return fn

        def geometric(params):
            def fn():
                k = next(it) % len(src)
                vol.align_frame_device(src[k], starts[k], params, d_res)
            return fn

        if counter_run:  # for a profiler: a few single-evaluation calls at stride 1 of either kind, nothing timed
            for k in range(counter_run):
                vol.align_frame_color_device(src[k % len(src)], col[k % len(src)], starts[k % len(src)],
                                             capi.AlignColorParams(levels=[(1, 0)]), d_res)
                vol.align_frame_device(src[k % len(src)], starts[k % len(src)], capi.AlignParams(levels=[(1, 0)]), d_res)
            vol.sync()
            for p in src + col + [d_res]:
                hip.h.hipFree(p)
            return {"counter_run": counter_run, "n_chunks": n_chunks}
        out = {"color": {}, "geometric": {}}
        for name, call, make in (("geometric", geometric, capi.AlignParams), ("color", color, capi.AlignColorParams)):
            per_eval = {}
            for stride in (1, 2, 4):
                t8 = timed(hip, stream, call(make(levels=[(stride, 8)], eps_t=0.0, eps_r=0.0)), 3, reps)
                t0 = timed(hip, stream, call(make(levels=[(stride, 0)], eps_t=0.0, eps_r=0.0)), 3, reps)
                per_eval[str(stride)] = round((t8 - t0) / 8, 2)
            out[name]["us_per_evaluation"] = per_eval
            out[name]["us_per_default_call"] = round(timed(hip, stream, call(make()), 3, reps), 1)
        vol.align_frame_color_device(src[0], col[0], starts[0], capi.AlignColorParams(), d_res)
        vol.sync()
        raw = np.empty(C.sizeof(capi.AlignColorResult), np.uint8)
        hip.download(d_res, raw)
        first = vol.align_color_result(raw)
        vol.sync()
        for p in src + col + [d_res]:
            hip.h.hipFree(p)
        ce, ge = out["color"]["us_per_evaluation"], out["geometric"]["us_per_evaluation"]
        out.update({"scene": "room", "image": [cam.width, cam.height], "res_m": float(res), "orbit_frames": orbit,
                    "n_chunks": n_chunks, "color_over_geometric": {s: round(ce[s] / ge[s], 3) for s in ce if ge[s] > 0},
                    "default_call_evaluations": first["evaluations"], "default_call_status": first["status"],
                    "default_call_rms": [float(first["rms_first"]), float(first["rms_last"])],
                    "default_call_rms_photo": [float(first["rms_photo_first"]), float(first["rms_photo_last"])],
                    "default_call_valid": [first["n_photo_last"], first["n_valid_last"], first["n_sampled"]],
                    "default_call_m_from_orbit_pose": round(float(np.linalg.norm(first["pose"][:, 3] - poses[0][:, 3])), 5),
                    "reps": reps})
        return out
    finally:
        vol.close()
        hip.h.hipStreamDestroy(stream)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--orbit", type=int, default=200, help="frames integrated before timing (the bench's pre-roll)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--counter-run", type=int, default=0, metavar="N",
                    help="no timing: N one-evaluation calls at stride 1 of either kind, for a run under a profiler")
    args = ap.parse_args()
    hip = Hip()
    if capi.lib().tf_device_count() <= 0:
        sys.exit("no HIP device: this tool measures the MI355X and has no CPU path")
    print(json.dumps(run(hip, args.orbit, args.reps, args.counter_run)), flush=True)


if __name__ == "__main__":
    main()
