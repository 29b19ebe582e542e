"""What the resident model stream (tf_model_stream_*, tf_model.hip) costs and saves, on the scene and protocol of
tools/render_time.py: S-room 640x480 @ 5 mm, 2^19-slot pool, one textured 200-frame orbit, ten orbit views, 3 warm-up + R calls.

  render   tf_render_model_device in mode 4 on a MISS (a call that may have changed the model goes before every render -- a
           tf_keyframe_release of a keyframe that does not exist: no device work, but no whitelisted reader either -- so
           every render packs) and on a HIT (renders back to back).  Host clock, first call to tf_sync, per call; the hit
           also between HIP events on the handle's stream.  This part runs on a library without tf_model_stream_* too
           (there every render packs: both figures are that library's one cost), which is how the commit before the
           stream is measured with the same script.
  pack     tf_model_stream_update_device alone, split list / rank / scan / write by HIP events (tf_model_stream_time),
           median of R packs, with the model's size.
  keyframe tools/prof_unit.py's keyframe unit (every 7th orbit frame a keyframe, six local frames, texture stage) on a
           second volume: after one orbit of pre-roll, 2 R keyframes that end alternately in tf_model_stream_update_device
           and in tf_draw_meshes_device, each followed by tf_sync -- host clock per keyframe, and the ending alone (from a
           synchronised stream to synchronised again).

One JSON line.  Needs the GPU; run it under a time limit:

    timeout -k 10 900 python tools/model_stream_time.py [--orbit 200] [--reps 20] [--parts render,pack,keyframe]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from texturefusion_amd import capi, synth  # noqa: E402
from raycast_time import Hip, timed  # noqa: E402

NEAR, FAR = 0.1, 5.0


def render_and_pack(hip, orbit, reps, parts):
    cam = synth.Camera()
    res = np.float32(0.005)
    pool = 1 << 19
    stream = hip.stream()
    vol = capi.Volume(res, cam, max_chunks=pool, max_list=1 << 18, mesh_blocks=pool // 4, stream=stream)
    out = {}
    try:
        poses = []
        for k in range(orbit):
            d, rgba, _, pose = synth.room_frame(k, cam, with_quality=False)
            vol.integrate_frame_host(d, rgba, pose.reshape(12), synth.pose_inverse16(pose), k)
            poses.append(pose)
        vol.sync()
        P = cam.width * cam.height
        bufs = [hip.malloc(4 * P), hip.malloc(4 * P), hip.malloc(4 * P)]
        views = poses[:: max(1, orbit // 10)]
        it = iter(range(1 << 30))
        has_stream = hasattr(vol, "model_stream_update")
        out["library_has_model_stream"] = has_stream

        def render():
            vol.render_model_device(views[next(it) % len(views)], NEAR, FAR, 4, *bufs)

        def render_behind_a_writer():
            vol._ck(vol.L.tf_keyframe_release(vol.h, -12345))
            render()

        def host_clock(fn):
            for _ in range(3):
                fn()
            vol.sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            vol.sync()
            return 1e6 * (time.perf_counter() - t0) / reps

        if "render" in parts:
            s0 = vol.model_stream_stats() if has_stream else None
            out["us_per_render_model_device_miss_host_clock"] = round(host_clock(render_behind_a_writer), 1)
            s1 = vol.model_stream_stats() if has_stream else None
            out["us_per_render_model_device_hit_host_clock"] = round(host_clock(render), 1)
            s2 = vol.model_stream_stats() if has_stream else None
            out["us_per_render_model_device_hit_events"] = round(timed(hip, stream, render, 3, reps), 1)
            if has_stream:
                out["miss_window"] = {"packs": s1["packs"] - s0["packs"], "hits": s1["hits"] - s0["hits"], "renders": reps + 3}
                out["hit_window"] = {"packs": s2["packs"] - s1["packs"], "hits": s2["hits"] - s1["hits"], "renders": reps + 3}
        if "pack" in parts and has_stream:
            nv, ni = vol.model_stream_update()
            g = vol.model_stream_get()
            ctl = np.zeros(8, np.uint32)
            hip.download(g["counts"], ctl)
            runs = [vol.model_stream_time() for _ in range(3 + reps)][3:]
            out["pack"] = {"n_vertices": nv, "n_indices": ni, "n_patches": int(ctl[2]), "stream_MB": round((48 * nv + 4 * ni) / 1e6, 1),
                           "cap_vertices": g["cap_vertices"], "cap_indices": g["cap_indices"], "packs_timed": reps,
                           "us_median": {k: round(statistics.median(r[k] for r in runs), 1) for k in ("list", "rank", "scan", "write")},
                           "us_min": {k: round(min(r[k] for r in runs), 1) for k in ("list", "rank", "scan", "write")},
                           "us_max": {k: round(max(r[k] for r in runs), 1) for k in ("list", "rank", "scan", "write")}}
            out["pack"]["us_median_total"] = round(sum(out["pack"]["us_median"].values()), 1)
        for p in bufs:
            hip.h.hipFree(p)
    finally:
        vol.close()
        hip.h.hipStreamDestroy(stream)
    return out


def keyframes(hip, reps):
    STRIDE, ORBIT, N_LOCAL = 7, 200, 6  # tools/prof_unit.py
    cam = synth.Camera()
    fr = [synth.room_frame(k, cam, with_quality=False) for k in range(ORBIT)]
    dd, dc = [], []
    for f in fr:
        dd.append(hip.malloc(f[0].nbytes)); hip.upload(dd[-1], f[0])
        dc.append(hip.malloc(f[1].nbytes)); hip.upload(dc[-1], f[1])
    poses = np.stack([f[3].reshape(12) for f in fr]).astype(np.float32)
    pinv = np.stack([synth.pose_inverse16(f[3]) for f in fr]).astype(np.float32)
    vol = capi.Volume(np.float32(0.005), cam, max_chunks=1 << 19, max_list=1 << 18, max_coarse=1 << 20)
    try:
        def unit(g):
            k0 = (STRIDE * g) % ORBIT
            loc = [(k0 + 1 + i) % ORBIT for i in range(N_LOCAL)]
            fresh = capi.Volume.unit_group(1000 + g, (dd[k0], dc[k0], 0, poses[k0]), [(dd[k], poses[k]) for k in loc])
            vol.keyframe_unit(fresh=fresh, moved=[], texture=True, pose_inv16=pinv[k0])

        n_pre = ORBIT // STRIDE
        for g in range(n_pre):
            unit(g)
        nv, ni = vol.model_stream_update()
        cap_v, cap_i = 2 * nv, 2 * ni
        vol.model_stream_reserve(cap_v, cap_i)
        dv, di = hip.malloc(48 * cap_v), hip.malloc(4 * cap_i)
        cv, ci = C.c_int64(0), C.c_int64(0)

        def end_stream():
            vol.model_stream_update_device()

        def end_draw():
            vol._ck(vol.L.tf_draw_meshes_device(vol.h, dv, di, cap_v, cap_i, C.byref(cv), C.byref(ci)))

        t = {"stream": [], "draw": []}
        t_end = {"stream": [], "draw": []}
        for j in range(2 * reps + 2):
            name, end = (("stream", end_stream), ("draw", end_draw))[j % 2]
            vol.sync()
            t0 = time.perf_counter()
            unit(n_pre + j)
            end()
            vol.sync()
            t1 = time.perf_counter()
            end()  # the ending alone, from a synchronised stream
            vol.sync()
            t2 = time.perf_counter()
            if j >= 2:  # (one warm-up keyframe per ending)
                t[name].append(1e6 * (t1 - t0))
                t_end[name].append(1e6 * (t2 - t1))
        nv2, ni2 = vol.model_stream_update()
        for p in [dv, di] + dd + dc:
            hip.h.hipFree(p)
        return {"keyframes_per_ending": reps, "n_vertices_first": nv, "n_vertices_last": nv2,
                "us_per_keyframe_ending_in_model_stream_update_device": round(statistics.median(t["stream"]), 1),
                "us_per_keyframe_ending_in_draw_meshes_device": round(statistics.median(t["draw"]), 1),
                "us_model_stream_update_device_then_sync_alone": round(statistics.median(t_end["stream"]), 1),
                "us_draw_meshes_device_then_sync_alone": round(statistics.median(t_end["draw"]), 1),
                "statistic": "median over the keyframes of each ending, host clock, every keyframe followed by tf_sync"}
    finally:
        vol.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--orbit", type=int, default=200, help="textured frames integrated before timing (the bench's pre-roll)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parts", default="render,pack,keyframe")
    args = ap.parse_args()
    parts = set(args.parts.split(","))
    hip = Hip()
    if capi.lib().tf_device_count() <= 0:
        sys.exit("no HIP device: this tool measures the MI355X and has no CPU path")
    out = {"scene": "room", "image": [640, 480], "res_m": 0.005, "orbit_frames": args.orbit, "reps": args.reps}
    if parts & {"render", "pack"}:
        out.update(render_and_pack(hip, args.orbit, args.reps, parts))
    if "keyframe" in parts and hasattr(capi.Volume, "model_stream_update"):  # (not on a library without the stream)
        out["keyframe"] = keyframes(hip, args.reps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
