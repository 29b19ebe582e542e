"""Device time of the projective ICP (tf_align_frame_icp_device) on the S-room, with tf_align_frame_device as the yardstick.

S-room (640x480 @ 5 mm, 2^19-slot pool): one full orbit (the bench's pre-roll) is integrated, then one orbit depth image is
tracked from a pose moved by 80 mm and turned by 5 degrees; the model maps are raycast once on the device at that start.
Times are HIP events on the handle's stream around R back-to-back calls after W warm-up calls (enqueue only), or the
host's clock around the forms that wait.  Reported:
  us_per_evaluation[form][stride]  (a call of 8 steps - a call of none) / 8 at one level of that stride, eps 0: "icp" from the
                                   far start, "frame" = tf_align_frame_device from a start 1 cm and 0.5 degrees away (the far
                                   one is outside its capture range: it would stop at its first evaluation)
  us_raycast_vertex_normal         one tf_raycast_device writing the two maps the ICP reads
  us_icp_default_device            one tf_align_frame_icp_device call, default parameters, maps given
  us_icp_default_host_wall         one tf_align_frame_icp call: upload, raycast, the ICP, one wait
  us_track_frame_wall              one tf_track_frame call: the above, then tf_align_frame from the ICP's pose; two waits
  what the calls did: status, evaluations, valid pixels, distance from the integration pose, cond(A) of the ICP's last
  evaluation (a view of the plain yaw orbit sees one or two walls: the directions along a wall are not observed)
One JSON line.  Needs the GPU; run it under a time limit:

    timeout -k 10 900 python tools/align_icp_time.py [--orbit 200] [--reps 20]

--counter-run N times nothing: it issues N one-evaluation ICP calls per stride (1, 2, 4), then N one-evaluation
tf_align_frame_device calls per stride, and ends, for a run under a profiler (kernel durations of k_icp_rows, k_icp_solve
and k_align_rows).

--gate measures the normal-compatibility gate (tf_align_icp_set_gate, the library's default gate) beside the ungated
figures, in the same run: us_per_evaluation["icp_gated"][stride], timed right after the ungated figure of the same stride,
and "gated": what the default call and tf_track_frame did on this view with the gate set.  With --counter-run the N ICP
calls per stride are issued gated (k_gated_rows in place of k_icp_rows).

--pyramid measures the depth pyramid (tf_align_icp_set_pyramid, the library's default) beside the other figures, in the same
run, as "pyramid":
  us_pyramid_launch                one tf_align_icp_pyramid_depth_device building levels 1 and 2 (what the default schedule needs)
  us_raycast_level[s]              one raycast of the two maps at the camera of the level of stride s = 2, 4
  us_per_evaluation[s]             the evaluation a call with the setting on makes at the level of stride s: the level image,
                                   the level camera and the level maps handed to tf_align_frame_icp_device at stride 1 (the same
                                   rows launch, the same solve), (a call of 8 steps - a call of none) / 8 -- to be read against
                                   us_per_evaluation["icp"][s], the strided evaluation
  us_track_device_off / _on        one tf_track_frame_device call (raycasts, the ICP, the SDF stage, the finish; HIP events)
  us_icp_default_host_wall_on      one tf_align_frame_icp call with the setting on (us_icp_default_host_wall is the same, off)
  and what the default call did on this view with the setting on.

--color measures the colour ICP (tf_align_frame_icp_color_device, tf_align_icp_color.hip) beside the other figures, in the
same run, as "color" and us_per_evaluation["icp_color"][stride] (timed right after the plain figure of the same stride; the
two map launches of a call cancel in the difference):
  us_model_maps                    one tf_align_icp_color_model_maps_device (k_cicp_lum, k_cicp_grad and three copies)
  us_icp_color_default_device      one tf_align_frame_icp_color_device call, default parameters, maps given
  us_icp_color_default_host_wall   one tf_align_frame_icp_color call: uploads, raycast, the maps, the ICP, one wait
  and what the default call did on this view.  With --gate the gated colour evaluation is timed too ("icp_color_gated").
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
from align_time import _perturb  # noqa: E402
from raycast_time import Hip, timed  # noqa: E402


def _far(pose, metres, degrees):
    """pose moved by `metres` along (0.6, 0.53, 0.6) and turned by `degrees` about (0.6, -0.64, 0.48), about the camera centre"""
    t = np.array([0.6, 0.53, 0.6])
    w = np.array([0.6, -0.64, 0.48])
    t, w = metres * t / np.linalg.norm(t), np.radians(degrees) * w / np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    th = np.linalg.norm(w)
    E = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    P = np.asarray(pose, np.float64).reshape(3, 4).copy()
    P[:, :3] = E @ P[:, :3]
    P[:, 3] += t
    return P.astype(np.float32)


def _distance(a, b):
    a, b = np.asarray(a, np.float64).reshape(3, 4), np.asarray(b, np.float64).reshape(3, 4)
    R = a[:, :3] @ b[:, :3].T
    return [float(np.linalg.norm(a[:, 3] - b[:, 3])), float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))]


def _wall(fn, warm, reps):
    for _ in range(warm):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def _pyramid(hip, stream, vol, cam, depth, d_depth, far, truth, icp_default, reps, per_evaluation_on):
    """the --pyramid figures (this file's header); leaves the setting off and the raycast camera unset"""
    out = {"us_raycast_level": {}, "us_per_evaluation": {}}
    P = cam.width * cam.height
    d_l = [hip.malloc(4 * (P >> (2 * l))) for l in (1, 2)]
    bufs = list(d_l)
    pyr = capi.AlignIcpPyramid()
    build = lambda: vol.align_icp_pyramid_depth_device(d_depth, 2, pyr, d_l)
    out["us_pyramid_launch"] = round(timed(hip, stream, build, 3, reps), 2)
    build()
    for l, stride in ((1, 2), (2, 4)):
        c4, w, h = vol.align_icp_pyramid_camera(l)
        d_v, d_n = hip.malloc(12 * w * h), hip.malloc(12 * w * h)
        bufs += [d_v, d_n]
        vol.raycast_camera(synth.Camera(w, h, float(c4[0]), float(c4[1]), float(c4[2]), float(c4[3])))
        ray = lambda: vol.raycast_device(far, icp_default.ray_near, icp_default.ray_far, icp_default.ray_max_steps, d_normal=d_n, d_vertex=d_v)
        out["us_raycast_level"][str(stride)] = round(timed(hip, stream, ray, 3, reps), 2)
        ray()
        out["us_per_evaluation"][str(stride)] = per_evaluation_on(d_l[l - 1], d_v, d_n)
        vol.raycast_camera(None)
    cell = capi.DevicePose()
    cell.pose[:] = [float(x) for x in np.asarray(far, np.float32).reshape(12)]
    cell.valid = 1
    d_start, d_out, d_pose = hip.malloc(64), hip.malloc(256), hip.malloc(64)
    bufs += [d_start, d_out, d_pose]
    hip.upload(d_start, np.frombuffer(bytes(cell), np.uint8))
    sdf = capi.AlignParams()
    track = lambda: vol.track_frame_device(d_depth, d_start, icp_default, sdf, None, d_out, d_pose)
    out["us_track_device_off"] = round(timed(hip, stream, track, 3, reps), 1)
    vol.align_icp_set_pyramid(pyr)
    out["us_track_device_on"] = round(timed(hip, stream, track, 3, reps), 1)
    out["us_icp_default_host_wall_on"] = round(_wall(lambda: vol.align_frame_icp(depth, far, None, icp_default), 2, reps), 1)
    g = vol.align_frame_icp(depth, far, None, icp_default)
    log = vol.align_icp_log()
    trk = vol.track_frame(depth, far)
    vol.align_icp_set_pyramid(None)
    out.update({"icp_status": g["status"], "icp_evaluations": g["evaluations"],
                "icp_valid": [g["n_valid_first"], g["n_valid_last"], g["n_sampled"]],
                "icp_sampled_per_evaluation": [r["n_sampled"] for r in log],
                "icp_rms": [float(g["rms_first"]), float(g["rms_last"])], "icp_from_truth_m_rad": _distance(g["pose"], truth),
                "icp_cond_A_last": float(np.linalg.cond(log[-1]["A"])), "track_stage": trk["stage"],
                "track_from_truth_m_rad": _distance(trk["pose"], truth)})
    vol.sync()
    for p in bufs:
        hip.h.hipFree(p)
    return out


def run(hip, orbit, reps, counter_run=0, gate=False, pyramid=False, color=False):
    cam = synth.Camera()
    res = np.float32(0.005)
    pool = 1 << 19
    stream = hip.stream()
    vol = capi.Volume(res, cam, max_chunks=pool, max_list=1 << 18, mesh_blocks=pool // 4, stream=stream)
    try:
        first = orbit // 2
        frame = None
        for k in range(orbit):
            d, rgba, _, pose = synth.room_frame(k, cam, with_quality=False)
            vol.integrate_frame_host(d, rgba, pose.reshape(12), None, k)
            if k == first:
                frame = (d, pose, rgba)
        vol.update_meshes()  # the neighbour table: the sampler reads it
        vol.sync()
        n_chunks = int(vol.stats().n_chunks)
        P = cam.width * cam.height
        depth, truth, rgba = frame
        far = _far(truth, 0.080, 5.0)
        near = _perturb(truth, np.random.default_rng(0))
        d_depth, d_v, d_n = hip.malloc(4 * P), hip.malloc(12 * P), hip.malloc(12 * P)
        hip.upload(d_depth, depth)
        d_res = hip.malloc(C.sizeof(capi.AlignResult))
        bufs = [d_depth, d_v, d_n, d_res]
        icp_default = capi.AlignIcpParams()

        def raycast():
            vol.raycast_device(far, icp_default.ray_near, icp_default.ray_far, icp_default.ray_max_steps, d_normal=d_n, d_vertex=d_v)

        def icp_call(params):
            return lambda: vol.align_frame_icp_device(d_depth, far, d_v, d_n, far, params, d_res)

        def frame_call(params):
            return lambda: vol.align_frame_device(d_depth, near, params, d_res)

        def per_evaluation(stride):
            lv = dict(eps_t=0.0, eps_r=0.0)
            return round((timed(hip, stream, icp_call(capi.AlignIcpParams(levels=[(stride, 8)], **lv)), 3, reps) -
                          timed(hip, stream, icp_call(capi.AlignIcpParams(levels=[(stride, 0)], **lv)), 3, reps)) / 8, 2)

        d_rgba = d_cres = None
        if color:
            d_rgba, d_cres = hip.malloc(4 * P), hip.malloc(C.sizeof(capi.AlignColorResult))
            hip.upload(d_rgba, np.ascontiguousarray(rgba, np.uint8))
            bufs += [d_rgba, d_cres]

        def color_call(params):
            return lambda: vol.align_frame_icp_color_device(d_depth, d_rgba, far, d_v, d_n, far, params, d_cres)

        def per_evaluation_color(stride):
            lv = dict(eps_t=0.0, eps_r=0.0)
            return round((timed(hip, stream, color_call(capi.AlignIcpColorParams(levels=[(stride, 8)], **lv)), 3, reps) -
                          timed(hip, stream, color_call(capi.AlignIcpColorParams(levels=[(stride, 0)], **lv)), 3, reps)) / 8, 2)

        raycast()
        if counter_run:
            if gate:
                vol.align_icp_set_gate(capi.AlignIcpGate())
            for stride in (1, 2, 4):
                one = capi.AlignIcpParams(levels=[(stride, 0)])
                for _ in range(counter_run):
                    icp_call(one)()
            for stride in (1, 2, 4):
                one = capi.AlignParams(levels=[(stride, 0)])
                for _ in range(counter_run):
                    frame_call(one)()
            vol.sync()
            for p in bufs:
                hip.h.hipFree(p)
            return {"counter_run": counter_run, "n_chunks": n_chunks, "gate": bool(gate),
                    "launch_order": "icp at strides 1, 2, 4, then tf_align_frame_device at strides 1, 2, 4; N calls each"}
        per_eval = {"icp": {}, "frame": {}}
        for stride in (1, 2, 4):
            lv = dict(eps_t=0.0, eps_r=0.0)
            per_eval["icp"][str(stride)] = per_evaluation(stride)
            if color:
                per_eval.setdefault("icp_color", {})[str(stride)] = per_evaluation_color(stride)
            if gate:
                vol.align_icp_set_gate(capi.AlignIcpGate())
                per_eval.setdefault("icp_gated", {})[str(stride)] = per_evaluation(stride)
                if color:
                    per_eval.setdefault("icp_color_gated", {})[str(stride)] = per_evaluation_color(stride)
                vol.align_icp_set_gate(None)
            per_eval["frame"][str(stride)] = round((timed(hip, stream, frame_call(capi.AlignParams(levels=[(stride, 8)], **lv)), 3, reps) -
                                                    timed(hip, stream, frame_call(capi.AlignParams(levels=[(stride, 0)], **lv)), 3, reps)) / 8, 2)
        us_ray = timed(hip, stream, raycast, 3, reps)
        us_icp = timed(hip, stream, icp_call(icp_default), 3, reps)
        vol.sync()
        raw = np.empty(C.sizeof(capi.AlignResult), np.uint8)
        hip.download(d_res, raw)
        icp = vol.align_result(raw)
        last = vol.align_icp_log()[-1]
        us_host = _wall(lambda: vol.align_frame_icp(depth, far, None, icp_default), 2, reps)
        us_track = _wall(lambda: vol.track_frame(depth, far), 2, reps)
        trk = vol.track_frame(depth, far)
        alone = vol.align_frame(depth, far)
        gated = None
        if gate:
            vol.align_icp_set_gate(capi.AlignIcpGate())
            us_g = timed(hip, stream, icp_call(icp_default), 3, reps)
            vol.sync()
            hip.download(d_res, raw)
            g = vol.align_result(raw)
            g_last = vol.align_icp_log()[-1]
            g_trk = vol.track_frame(depth, far)
            vol.align_icp_set_gate(None)
            gated = {"us_icp_default_device": round(us_g, 1), "icp_status": g["status"], "icp_evaluations": g["evaluations"],
                     "icp_valid": [g["n_valid_first"], g["n_valid_last"], g["n_sampled"]],
                     "icp_rms": [float(g["rms_first"]), float(g["rms_last"])], "icp_from_truth_m_rad": _distance(g["pose"], truth),
                     "icp_cond_A_last": float(np.linalg.cond(g_last["A"])), "track_stage": g_trk["stage"],
                     "track_from_truth_m_rad": _distance(g_trk["pose"], truth)}
        col = None
        if color:
            cdef = capi.AlignIcpColorParams()
            d_m = [hip.malloc(4 * P) for _ in range(3)]
            bufs += d_m
            us_maps = timed(hip, stream, lambda: vol.align_icp_color_model_maps_device(d_v, d_n, far, cdef, *d_m), 3, reps)
            us_c = timed(hip, stream, color_call(cdef), 3, reps)
            vol.sync()
            craw = np.empty(C.sizeof(capi.AlignColorResult), np.uint8)
            hip.download(d_cres, craw)
            g = vol.align_color_result(craw)
            c_last = vol.align_icp_color_log()[-1]
            us_ch = _wall(lambda: vol.align_frame_icp_color(depth, rgba, far, None, cdef), 2, reps)
            col = {"us_model_maps": round(us_maps, 1), "us_icp_color_default_device": round(us_c, 1),
                   "us_icp_color_default_host_wall": round(us_ch, 1), "icp_status": g["status"],
                   "icp_evaluations": g["evaluations"], "icp_valid": [g["n_valid_first"], g["n_valid_last"], g["n_sampled"]],
                   "icp_photo": [g["n_photo_first"], g["n_photo_last"]],
                   "icp_rms_photo": [float(g["rms_photo_first"]), float(g["rms_photo_last"])],
                   "icp_from_truth_m_rad": _distance(g["pose"], truth),
                   "icp_cond_M_last": float(np.linalg.cond(c_last["A"] + float(np.float32(cdef.photo_weight)) ** 2 * c_last["Ac"]))}
        pyr = None
        if pyramid:
            lv = dict(eps_t=0.0, eps_r=0.0)

            def per_evaluation_on(d_img, d_lv, d_ln):
                call = lambda params: (lambda: vol.align_frame_icp_device(d_img, far, d_lv, d_ln, far, params, d_res))
                return round((timed(hip, stream, call(capi.AlignIcpParams(levels=[(1, 8)], **lv)), 3, reps) -
                              timed(hip, stream, call(capi.AlignIcpParams(levels=[(1, 0)], **lv)), 3, reps)) / 8, 2)

            pyr = _pyramid(hip, stream, vol, cam, depth, d_depth, far, truth, icp_default, reps, per_evaluation_on)
        for p in bufs:
            hip.h.hipFree(p)
        return {"gated": gated, "pyramid": pyr, "color": col, "scene": "room", "image": [cam.width, cam.height], "res_m": float(res), "orbit_frames": orbit, "frame": first,
                "n_chunks": n_chunks, "start": "80 mm / 5 deg", "us_per_evaluation": per_eval,
                "us_raycast_vertex_normal": round(us_ray, 1), "us_icp_default_device": round(us_icp, 1),
                "us_icp_default_host_wall": round(us_host, 1), "us_track_frame_wall": round(us_track, 1),
                "icp_status": icp["status"], "icp_evaluations": icp["evaluations"],
                "icp_valid": [icp["n_valid_first"], icp["n_valid_last"], icp["n_sampled"]],
                "icp_rms": [float(icp["rms_first"]), float(icp["rms_last"])], "icp_from_truth_m_rad": _distance(icp["pose"], truth),
                "icp_cond_A_last": float(np.linalg.cond(last["A"])),
                "track_stage": trk["stage"], "track_sdf_status": trk["sdf"]["status"],
                "track_sdf_evaluations": trk["sdf"]["evaluations"], "track_from_truth_m_rad": _distance(trk["pose"], truth),
                "align_frame_alone_status": alone["status"], "align_frame_alone_valid_first": alone["n_valid_first"],
                "align_frame_alone_from_truth_m_rad": _distance(alone["pose"], truth),
                "reps": reps}
    finally:
        vol.close()
        hip.h.hipStreamDestroy(stream)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--orbit", type=int, default=200, help="frames integrated before timing (the bench's pre-roll)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--counter-run", type=int, default=0, metavar="N",
                    help="no timing: N one-evaluation calls per stride of the ICP, then of tf_align_frame_device, for a profiler")
    ap.add_argument("--gate", action="store_true", help="also measure with the default normal-compatibility gate set")
    ap.add_argument("--pyramid", action="store_true", help="also measure the depth pyramid (tf_align_icp_set_pyramid)")
    ap.add_argument("--color", action="store_true", help="also measure the colour ICP (tf_align_frame_icp_color_device)")
    args = ap.parse_args()
    hip = Hip()
    if capi.lib().tf_device_count() <= 0:
        sys.exit("no HIP device: this tool measures the MI355X and has no CPU path")
    print(json.dumps(run(hip, args.orbit, args.reps, args.counter_run, args.gate, args.pyramid, args.color)), flush=True)


if __name__ == "__main__":
    main()
