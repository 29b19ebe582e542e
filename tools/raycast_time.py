"""Device time of tf_raycast_device and tf_query_points_device on the bench's steady-state scenes.

S-room (640x480 @ 5 mm, 2^19-slot pool) and the S-hall (1280x960 @ 5 mm, 8x6x8 m, 2^21 slots): one full orbit (the
bench's pre-roll) is integrated, then the model is rendered from orbit poses and queried at a million points near the
surface.  Times are HIP events on the handle's stream around R back-to-back calls, after W warm-up calls.  One JSON line
per scene.  Needs the GPU; run it under a time limit:

    timeout -k 10 900 python tools/raycast_time.py [--scenes room,hall] [--orbit 200] [--reps 20]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from texturefusion_amd import capi, synth  # noqa: E402


class Hip:
    def __init__(self):
        capi.lib()
        self.h = C.CDLL("libamdhip64.so")
        vp = C.c_void_p
        self.h.hipStreamCreate.argtypes = [C.POINTER(vp)]
        self.h.hipStreamDestroy.argtypes = [vp]
        self.h.hipEventCreate.argtypes = [C.POINTER(vp)]
        self.h.hipEventDestroy.argtypes = [vp]
        self.h.hipEventRecord.argtypes = [vp, vp]
        self.h.hipEventSynchronize.argtypes = [vp]
        self.h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
        self.h.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
        self.h.hipFree.argtypes = [vp]
        self.h.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]

    def ck(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %d" % (what, rc))

    def stream(self):
        s = C.c_void_p()
        self.ck(self.h.hipStreamCreate(C.byref(s)), "hipStreamCreate")
        return s.value

    def event(self):
        e = C.c_void_p()
        self.ck(self.h.hipEventCreate(C.byref(e)), "hipEventCreate")
        return e.value

    def malloc(self, n):
        p = C.c_void_p()
        self.ck(self.h.hipMalloc(C.byref(p), n), "hipMalloc")
        return p.value

    def upload(self, dst, arr):
        arr = np.ascontiguousarray(arr)
        self.ck(self.h.hipMemcpy(dst, arr.ctypes.data, arr.nbytes, 1), "hipMemcpy")

    def download(self, src, arr):
        self.ck(self.h.hipMemcpy(arr.ctypes.data, src, arr.nbytes, 2), "hipMemcpy")


def timed(hip, stream, fn, warm, reps):
    """device microseconds per call of fn (enqueue only) between two events on the handle's stream"""
    for _ in range(warm):
        fn()
    a, b = hip.event(), hip.event()
    hip.ck(hip.h.hipEventRecord(a, stream), "hipEventRecord")
    for _ in range(reps):
        fn()
    hip.ck(hip.h.hipEventRecord(b, stream), "hipEventRecord")
    hip.ck(hip.h.hipEventSynchronize(b), "hipEventSynchronize")
    ms = C.c_float()
    hip.ck(hip.h.hipEventElapsedTime(C.byref(ms), a, b), "hipEventElapsedTime")
    hip.h.hipEventDestroy(a)
    hip.h.hipEventDestroy(b)
    return 1e3 * ms.value / reps


def run_scene(hip, name, orbit, reps, n_points):
    big = name == "hall"
    cam = synth.Camera.hires() if big else synth.Camera()
    res = np.float32(0.005)
    pool = (1 << 21) if big else (1 << 19)
    stream = hip.stream()
    vol = capi.Volume(res, cam, max_chunks=pool, max_list=(1 << 20) if big else (1 << 18), mesh_blocks=pool // 4,
                      stream=stream)
    try:
        poses = []
        for k in range(orbit):
            if big:
                d, rgba, _, pose = synth.room_frame(k, cam, half=(4.0, 3.0, 4.0), radius=0.5, with_quality=False)
            else:
                d, rgba, _, pose = synth.room_frame(k, cam, with_quality=False)
            vol.integrate_frame_host(d, rgba, pose.reshape(12), None, k)
            poses.append(pose)
        vol.sync()
        n_chunks = int(vol.stats().n_chunks)
        P = cam.width * cam.height
        bufs = [hip.malloc(4 * P), hip.malloc(12 * P), hip.malloc(4 * P), hip.malloc(12 * P)]
        far = 8.0 if big else 5.0
        views = poses[:: max(1, orbit // 10)]
        it = iter(range(1 << 30))

        def render_all():
            k = next(it)
            vol.raycast_device(views[k % len(views)], 0.1, far, 2048, *bufs)

        def render_depth():
            k = next(it)
            vol.raycast_device(views[k % len(views)], 0.1, far, 2048, bufs[0])

        us_all = timed(hip, stream, render_all, 3, reps)
        us_depth = timed(hip, stream, render_depth, 3, reps)
        vol.raycast_device(views[0], 0.1, far, 2048, bufs[0])
        vol.sync()
        depth = np.empty((cam.height, cam.width), np.float32)
        hip.download(bufs[0], depth)
        hit = float((depth > 0).mean())
        # a million points around the surface: uniform inside chunks that exist
        ids = vol.list_chunks()
        rng = np.random.default_rng(0)
        pts = ((ids[rng.integers(0, len(ids), n_points)] * 8 + rng.uniform(0, 8, (n_points, 3))) * float(res)).astype(np.float32)
        qb = [hip.malloc(12 * n_points)] + [hip.malloc(12 * n_points) for _ in range(6)]
        hip.upload(qb[0], pts)

        def query_all():
            vol.query_device(qb[0], n_points, 31, *qb[1:])

        def query_sdf():
            vol.query_device(qb[0], n_points, capi.Q_SDF, qb[1], 0, 0, 0, 0, qb[6])

        us_q_all = timed(hip, stream, query_all, 3, reps)
        us_q_sdf = timed(hip, stream, query_sdf, 3, reps)
        for p in bufs + qb:
            hip.h.hipFree(p)
        scale = 1e6 / n_points
        return {"scene": name, "image": [cam.width, cam.height], "res_m": float(res), "orbit_frames": orbit,
                "n_chunks": n_chunks, "hit_fraction": round(hit, 4),
                "us_per_render_all_outputs": round(us_all, 1), "us_per_render_depth_only": round(us_depth, 1),
                "us_per_million_queries_all": round(us_q_all * scale, 1),
                "us_per_million_queries_sdf": round(us_q_sdf * scale, 1), "reps": reps}
    finally:
        vol.close()
        hip.h.hipStreamDestroy(stream)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default="room,hall")
    ap.add_argument("--orbit", type=int, default=200, help="frames integrated before timing (the bench's pre-roll)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=1 << 20)
    args = ap.parse_args()
    hip = Hip()
    if capi.lib().tf_device_count() <= 0:
        sys.exit("no HIP device: this tool measures the MI355X and has no CPU path")
    for s in args.scenes.split(","):
        print(json.dumps(run_scene(hip, s, args.orbit, args.reps, args.points)), flush=True)


if __name__ == "__main__":
    main()
