"""Wall time per frame of KinectFusion's loop -- track a frame against the model, test the result, integrate the frame at
the tracked pose -- run from the host and run on the stream.

S-room (640x480 @ 5 mm, 2^19-slot pool, the 200-frame orbit of bench.py's headline configuration): one orbit is integrated
at its true poses (the bench's pre-roll), then the loop goes round again: frame f is tracked from the pose frame f - 1 ended
at.  Two ways:
  host    tf_track_frame (host depth image: its upload, a wait per stage), the acceptance test on the host,
          tf_integrate_frames_device at the tracked pose where it passes: 3 host waits per frame (the staging pool's, one
          per stage) -- the only way to run this sequence without the device-pose entry points
  device  tf_track_integrate_device, one pose cell fed back, frames resident: 0 waits per frame, one tf_sync at the end
W warm-up frames, then K timed frames (wall clock, a device synchronisation on both sides), R runs of each way, interleaved,
every run on a fresh volume.  The two ways compute the same thing: the tool checks that every tf_track_result of the timed
window is byte-equal between the first runs.  One JSON line; --out also writes it to a file.

    timeout -k 10 900 python tools/track_loop_time.py [--steps 200] [--warmup 20] [--runs 3] [--textured] [--out FILE]

--textured times the same two loops with the textured unit in place of the integrate: every frame of the
pre-roll and every accepted frame is meshed and textured from its own image.
  host    tf_track_frame, the test on the host, the rigid inverse of the tracked pose on the host (tf_devpose.h's
          definition in numpy), tf_stream_frames_textured_device with it: entry points that need no device pose
  device  tf_track_texture_device, one pose cell fed back: 0 waits per frame

--counter-run N times nothing: pre-roll, then N frames of the device loop, for a run under a profiler (kernel durations).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from texturefusion_amd import capi, synth  # noqa: E402
from raycast_time import Hip  # noqa: E402

ORBIT = 200
TRK = C.sizeof(capi.TrackResult)


def inverse16(pose):
    """devpose_inverse16 (tf_devpose.h): [R^T | -R^T t; 0 0 0 1] of a 3 x 4 f32 pose, the translation's products and its two
    additions, left to right, in f64"""
    P = np.asarray(pose, np.float32).reshape(3, 4)
    R, t = P[:, :3].astype(np.float64), P[:, 3].astype(np.float64)
    T = np.zeros((4, 4), np.float32)
    T[:3, :3] = P[:, :3].T
    T[:3, 3] = -((R[0] * t[0] + R[1] * t[1]) + R[2] * t[2])
    T[3, 3] = 1.0
    return T.reshape(16)


def _accepted(t, acc):
    a = t.sdf if t.stage == 2 else t.icp
    F = np.float32
    return bool(t.stage >= acc.min_stage and a.n_sampled > 0 and
                F(a.n_valid_last) >= F(F(acc.min_valid_fraction) * F(a.n_sampled)) and F(a.rms_last) <= F(acc.max_rms))


class Scene:
    def __init__(self, hip):
        self.hip, self.cam = hip, synth.Camera()
        self.depth, self.poses, self.d_depth, self.d_rgba = [], [], [], []
        for k in range(ORBIT):
            d, rgba, _, pose = synth.room_frame(k, self.cam, with_quality=False)
            self.depth.append(np.ascontiguousarray(d, np.float32))
            self.poses.append(np.ascontiguousarray(pose, np.float32).reshape(12))
            pd, pc = hip.malloc(d.nbytes), hip.malloc(rgba.nbytes)
            hip.upload(pd, d)
            hip.upload(pc, rgba)
            self.d_depth.append(pd)
            self.d_rgba.append(pc)

    def volume(self, stream, textured=False):
        pool = 1 << 19
        vol = capi.Volume(np.float32(0.005), self.cam, max_chunks=pool, max_list=1 << 18, mesh_blocks=pool // 4, stream=stream)
        for k in range(ORBIT):  # the pre-roll: one orbit at its true poses
            if textured:
                vol.stream_frames_textured_device([self.d_depth[k]], [self.d_rgba[k]], [self.poses[k]], [inverse16(self.poses[k])], k)
            else:
                vol.integrate_frames_device([self.d_depth[k]], [self.d_rgba[k]], [self.poses[k]])
        vol.sync()
        return vol

    def free(self):
        for p in self.d_depth + self.d_rgba:
            self.hip.h.hipFree(p)


def host_loop(sc, vol, n, acc, icp, sdf, t_from, textured=False):
    """-> (seconds of frames [t_from, n), the results of those frames, frames accepted)"""
    f32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    pose, out, n_ok, t0 = sc.poses[ORBIT - 1].copy(), [], 0, 0.0
    for f in range(n):
        if f == t_from:
            vol.sync()
            t0 = time.perf_counter()
        k = f % ORBIT
        t = capi.TrackResult()
        rc = vol.L.tf_track_frame(vol.h, f32p(sc.depth[k]), f32p(pose), C.byref(icp), C.byref(sdf), C.byref(t))
        assert rc == capi.TF_OK, rc
        if _accepted(t, acc):
            pose = np.array(t.pose, np.float32)
            if textured:
                vol.stream_frames_textured_device([sc.d_depth[k]], [sc.d_rgba[k]], [pose], [inverse16(pose)], ORBIT + f)
            else:
                vol.integrate_frames_device([sc.d_depth[k]], [sc.d_rgba[k]], [pose])
            n_ok += 1
        if f >= t_from:
            out.append(bytes(t))
    vol.sync()
    return time.perf_counter() - t0, out, n_ok


def device_loop(sc, vol, n, acc, icp, sdf, t_from, d_out, d_cell, textured=False):
    cell = capi.DevicePose()
    cell.pose[:] = [float(x) for x in sc.poses[ORBIT - 1]]
    cell.valid = 1
    sc.hip.upload(d_cell, np.frombuffer(bytes(cell), np.uint8))
    t0 = 0.0
    for f in range(n):
        if f == t_from:
            vol.sync()
            t0 = time.perf_counter()
        k = f % ORBIT
        if textured:
            vol.track_texture_device(sc.d_depth[k], sc.d_rgba[k], d_cell, icp, sdf, acc, d_out + 256 * f, d_cell, ORBIT + f)
        else:
            vol.track_integrate_device(sc.d_depth[k], sc.d_rgba[k], d_cell, icp, sdf, acc, d_out + 256 * f, d_cell)
    vol.sync()
    dt = time.perf_counter() - t0
    raw = np.empty(256 * n, np.uint8)
    sc.hip.download(d_out, raw)
    out = [bytes(raw[256 * f:256 * f + TRK]) for f in range(t_from, n)]
    n_ok = sum(_accepted(capi.TrackResult.from_buffer_copy(bytes(raw[256 * f:256 * f + TRK])), acc) for f in range(n))
    return dt, out, n_ok


def run(hip, steps, warmup, runs, counter_run=0, textured=False):
    sc = Scene(hip)
    stream = hip.stream()
    n = warmup + steps
    d_out, d_cell = hip.malloc(256 * max(n, counter_run, 1)), hip.malloc(64)
    acc, icp, sdf = capi.TrackAccept(), capi.AlignIcpParams(), capi.AlignParams()
    try:
        if counter_run:
            vol = sc.volume(stream, textured)
            try:
                device_loop(sc, vol, counter_run, acc, icp, sdf, 0, d_out, d_cell, textured)
            finally:
                vol.close()
            return {"counter_run": counter_run}
        ms = {"host": [], "device": []}
        ok = {"host": [], "device": []}
        first = {}
        for r in range(runs):
            for way in ("host", "device"):
                vol = sc.volume(stream, textured)
                try:
                    if way == "host":
                        dt, out, n_ok = host_loop(sc, vol, n, acc, icp, sdf, warmup, textured)
                    else:
                        dt, out, n_ok = device_loop(sc, vol, n, acc, icp, sdf, warmup, d_out, d_cell, textured)
                finally:
                    vol.close()
                ms[way].append(round(1e3 * dt / steps, 4))
                ok[way].append(n_ok)
                first.setdefault(way, out)
        fig = lambda v: {"runs": v, "median": float(np.median(v)), "min": min(v), "max": max(v)}
        return {"scene": "room", "image": [sc.cam.width, sc.cam.height], "res_m": 0.005, "preroll_frames": ORBIT,
                "warmup_frames": warmup, "timed_frames": steps, "textured": bool(textured),
                "ms_per_frame_host_loop": fig(ms["host"]), "ms_per_frame_device_loop": fig(ms["device"]),
                "host_waits_per_frame": {"host_loop": 3, "device_loop": 0},
                "frames_accepted_of": n, "frames_accepted": ok,
                "results_byte_equal": first["host"] == first["device"],
                "note": "the host loop's tf_track_frame takes a host depth image: its 1.2 MB upload is inside the host figure"}
    finally:
        hip.h.hipFree(d_out)
        hip.h.hipFree(d_cell)
        sc.free()
        hip.h.hipStreamDestroy(stream)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--textured", action="store_true",
                    help="the textured unit in place of the integrate: tf_stream_frames_textured_device / tf_track_texture_device")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    ap.add_argument("--counter-run", type=int, default=0, metavar="N", help="no timing: N frames of the device loop, for a profiler")
    args = ap.parse_args()
    hip = Hip()
    if capi.lib().tf_device_count() <= 0:
        sys.exit("no HIP device: this tool measures the MI355X and has no CPU path")
    line = json.dumps(run(hip, args.steps, args.warmup, args.runs, args.counter_run, args.textured))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
