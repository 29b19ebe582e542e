"""Device time of the relocalisation retrieval (tf_reloc_index_add, tf_reloc_query) at 640x480.

64 frames of the S-room orbit (depth and RGBA, eight frames apart) are uploaded once and cached as keyframes from device
memory (tf_keyframe_cache_device, pixel stride 4); for the large index the same 64 image pairs are cached under 1024 ids.
The volume stays empty: retrieval does not read it.  Default parameters: 40 x 30 blocks of 16 x 16 pixels.  Reported:
  us_index_add_64            one tf_reloc_index_add of the 64 keyframes (a describe launch over 64 images and the totals),
                             HIP events on the handle's stream around R back-to-back calls after W warm-up calls.  Every
                             call begins by draining the stream for its staging area, so this is one call's device time.
  us_query_device[rows]      one tf_reloc_query_device against 64 and against 1024 rows, events around R calls: the
                             describe launch of one image, the totals, the score launch, the download of 12 bytes per row
  us_query_host_wall[rows]   one tf_reloc_query from host images, the host's clock: upload of 2.4 MB, the above, one wait
  what the calls returned: candidates, the best keyframe and its score for a query that is frame 3 of the 64
One JSON line.  Needs the GPU; run it under a time limit:

    timeout -k 10 600 python tools/reloc_time.py [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from texturefusion_amd import capi, synth  # noqa: E402
from raycast_time import Hip, timed  # noqa: E402


def _wall(fn, warm, reps):
    for _ in range(warm):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def run(hip, reps):
    cam = synth.Camera()
    stream = hip.stream()
    vol = capi.Volume(np.float32(0.005), cam, max_chunks=1 << 12, stream=stream, max_keyframes=1100)
    bufs = []
    try:
        frames = []
        for k in range(64):
            d, rgba, _, pose = synth.room_frame(8 * k, cam, with_quality=False)
            d_rgba, d_depth = hip.malloc(rgba.nbytes), hip.malloc(d.nbytes)
            hip.upload(d_rgba, rgba)
            hip.upload(d_depth, d)
            bufs += [d_rgba, d_depth]
            T = np.eye(4)
            T[:3] = np.asarray(pose, np.float64).reshape(3, 4)
            frames.append((d, rgba, d_rgba, d_depth, np.linalg.inv(T).astype(np.float32)))
        for kf_id in range(1024):
            _, _, d_rgba, d_depth, inv = frames[kf_id % 64]
            vol.keyframe_cache_device(kf_id, d_rgba, d_depth, 4, inv)
        vol.reloc_configure()
        ids64 = np.arange(64, dtype=np.int32)
        us_add = timed(hip, stream, lambda: vol.reloc_index_add(ids64), 3, reps)
        depth, rgba, q_rgba, q_depth, _ = frames[3]
        out = {"us_query_device": {}, "us_query_host_wall": {}, "candidates": {}, "best": {}}
        for rows in (64, 1024):
            vol.reloc_index_add(np.arange(rows, dtype=np.int32))
            assert vol.reloc_index_count() == rows
            out["us_query_device"][str(rows)] = round(timed(hip, stream, lambda: vol.reloc_query_device(q_depth, q_rgba, 4, cap=8), 3, reps), 1)
            out["us_query_host_wall"][str(rows)] = round(_wall(lambda: vol.reloc_query(depth, rgba, cap=8), 2, reps), 1)
            got = vol.reloc_query(depth, rgba, cap=8)
            out["candidates"][str(rows)] = got["n"]
            out["best"][str(rows)] = [int(got["kf_ids"][0]), float(got["scores"][0]), int(got["overlap"][0])] if got["n"] else None
        out.update({"scene": "room", "image": [cam.width, cam.height], "blocks": [40, 30], "us_index_add_64": round(us_add, 1), "reps": reps})
        return out
    finally:
        vol.close()
        for p in bufs:
            hip.h.hipFree(p)
        hip.h.hipStreamDestroy(stream)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    hip = Hip()
    if capi.lib().tf_device_count() <= 0:
        sys.exit("no HIP device: this tool measures the MI355X and has no CPU path")
    print(json.dumps(run(hip, args.reps)), flush=True)


if __name__ == "__main__":
    main()
