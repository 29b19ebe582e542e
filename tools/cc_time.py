"""Time of Chisel::CompensateColor per call: the host-solved path tf_compensate_color against tf_compensate_color_device.

Two scenes.  "wall": the three-cluster scene of tests/test_gpu_cc_device.py (six wall frames at 1.2 m, keyframes 2, 5 and 7
dealt i % 3 over the meshes, 640x480 @ 5 mm).  "room": 90 frames of the bench's stream (S-room orbit, 640x480 @ 5 mm,
2^19-slot pool) and ONE keyframe behind them -- the last frame textures every mesh, one cluster.  CompensateColor consumes
its input (has_adjusted), so every timed call is preceded by an untimed GeneratePatches over the same list, which resets
the patches, and a tf_sync.  Per call:

    host_us    wall time of tf_compensate_color (it ends in its own wait)
    device_us  wall time from the enqueue of tf_compensate_color_device to the return of a tf_sync behind it
    enqueue_us of that, the time until tf_compensate_color_device returned

The two paths alternate call by call, R calls each after W warm-up calls; medians and minima are reported.  With
--profile a child run of this script under `rocprofv3 --kernel-trace --stats` adds the kernel time per call of both paths
(k_list_patches + k_cc_* against k_ccd_*).  One JSON line.  Needs the GPU; run it under a time limit:

    timeout -k 10 900 python tools/cc_time.py [--reps 20] [--profile]

(--profile: each scene's child has 240 s of its own; a child that fails, is killed or runs out of time ends the script.)
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from texturefusion_amd import capi, synth  # noqa: E402

RES = np.float32(0.005)


def wall_scene():
    cam = synth.Camera()
    frames = []
    for k in range(6):
        d, rgba, q, pose = synth.wall_frame(1.2, cam, seed=k)
        rgba = synth._hash_colour(np.stack(np.meshgrid(np.arange(cam.width) * 0.01, np.arange(cam.height) * 0.01), -1)[..., [0, 1, 1]], 5)
        frames.append((d, rgba, pose))
    dark = (frames[1][0], (frames[1][1].astype(np.float32) * 0.7).astype(np.uint8), frames[1][2])
    far = (np.where(frames[2][0] > 0, frames[2][0] + 1.0, 0).astype(np.float32), frames[2][1], frames[2][2])
    vol = capi.Volume(RES, cam, max_chunks=1 << 15)
    for d, rgba, pose in frames:
        vol.frame_upload(d, rgba, None)
        vol.integrate_frame(pose, True)
    vol.update_meshes()
    ids = vol.compress_meshes()
    for k, f in ((2, frames[0]), (5, dark), (7, far)):
        vol.keyframe_cache(k, np.ascontiguousarray(f[1][..., :3]), f[0], synth.pose_inverse16(f[2]))
    labels = np.array([(2, 5, 7)[i % 3] for i in range(len(ids))], np.int32)
    return vol, ids, labels


def room_scene(n_frames=90):
    cam = synth.Camera()
    pool = 1 << 19
    vol = capi.Volume(RES, cam, max_chunks=pool, max_list=1 << 18, mesh_blocks=pool // 4)
    last = None
    for k in range(n_frames):
        d, rgba, _, pose = synth.room_frame(k, cam, with_quality=False)
        vol.integrate_frame_host(d, rgba, pose.reshape(12), None, k)
        last = (d, rgba, pose)
    vol.sync()
    vol.update_meshes()
    ids = vol.compress_meshes()
    vol.keyframe_cache(1, np.ascontiguousarray(last[1][..., :3]), last[0], synth.pose_inverse16(last[2]))
    return vol, ids, np.ones(len(ids), np.int32)


def measure(vol, ids, labels, warm, reps):
    host, dev, enq, counts = [], [], [], set()
    for r in range(warm + reps):
        for path in ("host", "device"):
            vol.generate_patches(ids, labels)
            vol.sync()
            if path == "host":
                t0 = time.perf_counter()
                n = vol.compensate_color()
                t1 = time.perf_counter()
                if r >= warm:
                    host.append(1e6 * (t1 - t0))
                counts.add(("host", n))
            else:
                t0 = time.perf_counter()
                rc = vol.L.tf_compensate_color_device(vol.h, None)
                t1 = time.perf_counter()
                vol.sync()
                t2 = time.perf_counter()
                assert rc == 0
                if r >= warm:
                    dev.append(1e6 * (t2 - t0))
                    enq.append(1e6 * (t1 - t0))
    g = vol.get_patches(ids)
    n_patches = int(((g["flags"] & 1) > 0).sum())
    n_vertices = int(np.diff(g["voff"])[(g["flags"] & 1) > 0].sum())
    med = lambda x: round(float(np.median(x)), 1) if x else None
    low = lambda x: round(float(np.min(x)), 1) if x else None
    return {"patches": n_patches, "vertices": n_vertices, "clusters": sorted(n for _, n in counts),
            "host_us": med(host), "host_us_min": low(host), "device_us": med(dev), "device_us_min": low(dev),
            "enqueue_us": med(enq), "reps": reps}


def kernel_times(scene, calls):
    """kernel microseconds per call of both paths from a child run under rocprofv3 --kernel-trace --stats"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--scenes", scene, "--reps", str(calls), "--warmup", "0"]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired:
            sys.exit("the profiled child ran into its time limit: nothing more is started on the GPU")
        if r.returncode != 0:  # (a fault, an abort or a kill among them: nothing more is started on the GPU)
            sys.exit("the profiled child ended with status %d: %s" % (r.returncode, (r.stdout + r.stderr)[-400:]))
        host, dev, per = 0.0, 0.0, {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                name = row.get("Name") or row.get("KernelName") or ""
                ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
                if "k_ccd_" in name:
                    dev += ns
                    short = name[name.index("k_ccd_"):].split("(")[0]
                    per[short] = round(ns / 1e3 / calls, 2)
                # (k_list_patches runs for tf_compensate_color and tf_draw_meshes only; the patch downloads of this run go
                # through k_patch_gather)
                elif "k_cc_" in name or "k_list_patches" in name:
                    host += ns
        if not dev:
            return {"error": "no kernel statistics found"}
        return {"host_kernels_us": round(host / 1e3 / calls, 2), "device_kernels_us": round(dev / 1e3 / calls, 2), "device_by_kernel_us": per}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default="wall,room")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if capi.lib().tf_device_count() <= 0:
        sys.exit("no HIP device: this tool measures the MI355X and has no CPU path")
    out = {}
    for scene in args.scenes.split(","):
        vol, ids, labels = {"wall": wall_scene, "room": room_scene}[scene]()
        try:
            out[scene] = measure(vol, ids, labels, args.warmup, args.reps)
        finally:
            vol.close()
        if args.profile:
            out[scene]["rocprofv3"] = kernel_times(scene, 5)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
