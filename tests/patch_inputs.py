"""Input generators of the patch-border tests, shared by tests/test_patch_cpu.py (which counts, with the reference
alone, which branches of the projection every input set takes) and tests/test_gpu_patch_borders.py (which runs the
same sets through the device): the GPU tests cannot drift to inputs that were never counted.

numpy + texturefusion_amd.synth + tests/patch_ref.py only: no oracle, no GPU."""
import functools
import math

import numpy as np

from tests import patch_ref
from texturefusion_amd import synth

F = np.float32

# 640 x 480, 160 x 120, and an odd height with non-integer intrinsics (truncated, PinholeCamera.h:46-49; the width is a
# multiple of 8: the ABI's constraint)
CAMERAS = {
    "vga": synth.Camera(),
    "small": synth.Camera(160, 120, 131.25, 131.25, 79.5, 59.5, 0.01, 5.0),
    "odd": synth.Camera(328, 241, 260.4, 263.1, 163.8, 119.8, 0.01, 5.0),
}
RESOLUTIONS = (F(0.005), F(0.01))  # slots of 24 x 18 and 48 x 36 texels (Atlas.h:62-65)
# vertex counts that straddle the lane count and the one-sweep / two-sweep switch at 128; 2240 is the largest mesh a
# block of the mesh store's overflow pool holds; 0: tf_meshes_upload accepts an empty mesh
COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 2240)
KF_GENERAL, KF_AXIS, KF_HONEST = 3, 8, 11  # keyframe ids (labels)
EPS = 2.0 ** -9


def slot_size(res):
    return int(math.floor(float(F(4800.0) * F(res)))), int(math.floor(float(F(3600.0) * F(res))))


def keyframe_images(cam, seed):
    """rgb u8[H,W,3]: white noise (a tap that is off by one pixel shows in the first channel it touches);
    depth f32[H,W] in [1.0, 1.2); alpha (for the stride-4 form) non-zero noise."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rgb = rng.integers(0, 256, (cam.height, cam.width, 3), dtype=np.uint8)
    depth = (1.0 + 0.2 * rng.random((cam.height, cam.width))).astype(F)
    alpha = rng.integers(1, 256, (cam.height, cam.width, 1), dtype=np.uint8)
    return rgb, depth, alpha


def back_project(cam, pose, uvz):
    """World positions (f32) of image positions (u, v) -- in the units of CalculateTexCoords' cameraX / cameraY,
    i.e. including its + 0.5 -- at camera-frame depth z, through the camera-to-world pose.  Where f32 rounding
    actually puts them is what the census says, not this."""
    uvz = np.asarray(uvz, np.float64).reshape(-1, 3)
    fx, fy, cx, cy = int(cam.fx), int(cam.fy), int(cam.cx), int(cam.cy)
    z = uvz[:, 2]
    pc = np.stack([(uvz[:, 0] - 0.5 - cx) / fx * z, (uvz[:, 1] - 0.5 - cy) / fy * z, z], -1)
    P = np.asarray(pose, np.float64).reshape(3, 4)
    return (pc @ P[:, :3].T + P[:, 3]).astype(F)


def _edge_values(n_hi, rng, n):
    """positions around the far edge n_hi (W or H): integer, half-integer, just inside, on and beyond"""
    pool = np.array([n_hi - 2, n_hi - 1.5, n_hi - 1, n_hi - 1 + EPS, n_hi - 0.5, n_hi - EPS, n_hi, n_hi + EPS,
                     n_hi + 3, n_hi + 1000.25])
    return pool[rng.integers(0, len(pool), n)]


def _near_values(rng, n):
    pool = np.array([-1000.25, -3, -EPS, 0, EPS, 0.5, 1, 1.5])
    return pool[rng.integers(0, len(pool), n)]


def _cluster(rng, n, c, half, lo, hi):
    """n positions around c, a third of them on integers or half-integers"""
    p = c + (rng.random(n) * 2 - 1) * half
    snap = rng.integers(0, 3, n)
    p = np.where(snap == 0, np.round(p), np.where(snap == 1, np.floor(p) + 0.5, p))
    return np.clip(p, lo, hi)


THEMES = ("interior", "wide", "tall", "wide_tall", "right", "bottom", "left", "top", "corner_br", "corner_tl",
          "corner_tr", "corner_bl", "beyond_right", "beyond_bottom", "near_right", "behind", "whole", "plane_z0",
          "thr_color_lo", "thr_color_hi", "thr_depth_lo", "thr_depth_hi", "color_all", "depth_all")
HONEST_THEMES = ("interior", "wide", "tall", "wide_tall", "thr_color_lo", "thr_color_hi", "color_all")


def _positions(theme, n, cam, slot, rng):
    """-> (u, v, z) of the theme's n vertices"""
    W, H = cam.width, cam.height
    pw, ph = slot
    cu, cv = rng.uniform(0.3 * W, 0.7 * W), rng.uniform(0.3 * H, 0.7 * H)
    z = np.full(n, 1.1)
    small = (min(6.0, pw / 4), min(5.0, ph / 4))
    if theme in ("interior", "thr_color_lo", "thr_color_hi", "thr_depth_lo", "thr_depth_hi", "color_all", "depth_all",
                 "behind"):
        u, v = _cluster(rng, n, cu, small[0], 3, W - 4), _cluster(rng, n, cv, small[1], 3, H - 4)
        if theme == "behind":
            z[:] = -1.1  # the surface behind the keyframe camera: the same image position, negative distance
    elif theme == "wide":
        u, v = _cluster(rng, n, cu, 0.8 * pw, 3, W - 4), _cluster(rng, n, cv, small[1], 3, H - 4)
    elif theme == "tall":
        u, v = _cluster(rng, n, cu, small[0], 3, W - 4), _cluster(rng, n, cv, 0.8 * ph, 3, H - 4)
    elif theme == "wide_tall":
        u, v = _cluster(rng, n, cu, 0.8 * pw, 3, W - 4), _cluster(rng, n, cv, 0.8 * ph, 3, H - 4)
    elif theme == "right":
        u, v = _edge_values(W, rng, n), _cluster(rng, n, cv, small[1], 3, H - 4)
    elif theme == "bottom":
        u, v = _cluster(rng, n, cu, small[0], 3, W - 4), _edge_values(H, rng, n)
    elif theme == "left":
        u, v = _near_values(rng, n), _cluster(rng, n, cv, small[1], 3, H - 4)
    elif theme == "top":
        u, v = _cluster(rng, n, cu, small[0], 3, W - 4), _near_values(rng, n)
    elif theme == "corner_br":
        u, v = _edge_values(W, rng, n), _edge_values(H, rng, n)
    elif theme == "corner_tl":
        u, v = _near_values(rng, n), _near_values(rng, n)
    elif theme == "corner_tr":
        u, v = _edge_values(W, rng, n), _near_values(rng, n)
    elif theme == "corner_bl":
        u, v = _near_values(rng, n), _edge_values(H, rng, n)
    elif theme == "beyond_right":  # every vertex clamps to x == W: a ROI one pixel wide, every tap the next row's
        u, v = W + 1 + rng.random(n) * 50, _cluster(rng, n, cv, small[1], 3, H - 4)
    elif theme == "beyond_bottom":  # every vertex clamps to y == H: every tap past the image
        u, v = _cluster(rng, n, cu, small[0], 3, W - 4), H + 1 + rng.random(n) * 50
    elif theme == "near_right":  # min x within the last pixel: a ROI two pixels wide
        u, v = W - 0.75 + rng.random(n) * 0.5, _cluster(rng, n, cv, small[1], 3, H - 4)
        u[rng.integers(0, n)] = W - 0.5
    elif theme == "whole":  # vertices all over the image and beyond: the ROI is the image less one row and column
        u, v = rng.uniform(-20, W + 20, n), rng.uniform(-20, H + 20, n)
        z[rng.random(n) < 0.3] = 0.45
    else:
        raise KeyError(theme)
    return u, v, z


def interior_positions(n, cam, slot, rng, z=1.1):
    """-> f64[n, 3] (u, v, z): the "interior" theme's n image positions, all at the distance z"""
    u, v, _ = _positions("interior", n, cam, slot, rng)
    return np.stack([u, v, np.full(n, float(z))], -1)


def _plane_z0(n, rng):
    """Vertices in the plane z == 0 of the axis-aligned keyframe (v_l.z == 0 exactly, v_l.x and v_l.y != 0): the
    projection is +-inf in both coordinates and clamps to a corner."""
    sx = np.where(rng.random(n) < 0.5, -1.0, 1.0) * (0.1 + rng.random(n))
    sy = np.where(rng.random(n) < 0.5, -1.0, 1.0) * (0.1 + rng.random(n))
    return np.stack([sx, sy, np.zeros(n)], -1).astype(F)


def axis_pose():
    """camera-to-world of KF_AXIS: the identity -- T16 * (v, 1) is then exact, so v.z == 0 gives v_l.z == 0"""
    return synth.pose_identity()


def general_pose():
    return synth.pose_euler(0.3, -0.2, 0.1, (0.1, -0.05, 0.2))


def honest_pose():
    """KF_HONEST: KF_GENERAL's pose moved by a few millimetres -- what used to be interior stays interior"""
    return synth.pose_euler(0.3005, -0.2003, 0.1002, (0.101, -0.0505, 0.2008))


@functools.lru_cache(maxsize=None)
def hand_case(cam_name, res_index):
    """The hand-made meshes of one (camera, voxel size): dict(cam, slot, keyframes {id: (rgb, depth, alpha, pose)},
    meshes [dict(theme, kf, verts f32[n,3], colors f32[n,3])]).  Vertex sets are built by back-projecting chosen
    image positions at chosen depths through the keyframe's pose; mesh colours are derived from patch_ref's own
    texcolor so that the colour compare fires for none, all, or a count on either side of 0.3 * nv."""
    cam = CAMERAS[cam_name]
    res = RESOLUTIONS[res_index]
    slot = slot_size(res)
    seed = 1000 * sorted(CAMERAS).index(cam_name) + res_index
    rng = np.random.Generator(np.random.PCG64(77 + seed))
    kfs = {}
    for k, (kid, pose) in enumerate(((KF_GENERAL, general_pose()), (KF_AXIS, axis_pose()), (KF_HONEST, honest_pose()))):
        rgb, depth, alpha = keyframe_images(cam, 10 * seed + k)
        kfs[kid] = (rgb, depth, alpha, pose)
    # every count of COUNTS at least once, every theme at least six times
    plan = []
    extra = (5, 17, 40, 100, 150, 200, 300)
    pool = [c for c in COUNTS if c > 0] + list(extra)
    k = 0
    for theme in THEMES:
        for rep in range(6):
            plan.append((theme, pool[k % len(pool)]))
            k += 1
    plan.append(("interior", 0))
    if not any(n == 2240 and t in ("right", "whole") for t, n in plan):
        plan.append(("whole", 2240))  # the largest mesh, across the whole image: two sweeps, every branch
    meshes = []
    for mi, (theme, n) in enumerate(plan):
        kf = KF_AXIS if (theme == "plane_z0" or mi % 4 == 3) else KF_GENERAL
        rgb, depth, alpha, pose = kfs[kf]
        if n == 0:
            verts = np.zeros((0, 3), F)
        elif theme == "plane_z0":
            verts = _plane_z0(n, rng)
        else:
            u, v, z = _positions(theme, n, cam, slot, rng)
            if theme in ("thr_depth_lo", "thr_depth_hi", "depth_all"):  # a depth that disagrees with the keyframe's by 1 m
                k_fire = {"thr_depth_lo": int(0.3 * n), "thr_depth_hi": int(0.3 * n) + 1, "depth_all": n}[theme]
                z[rng.permutation(n)[:min(k_fire, n)]] = 2.1
            verts = back_project(cam, pose, np.stack([u, v, z], -1))
        colors = np.zeros((n, 3), F)
        if n:
            tcol = patch_ref.project(verts, colors, synth.pose_inverse16(pose), rgb, depth, cam)["texcolor"]
            colors = tcol.copy()  # the colour compare fires nowhere ...
            k_fire = {"thr_color_lo": int(0.3 * n), "thr_color_hi": int(0.3 * n) + 1, "color_all": n}.get(theme, 0)
            colors[rng.permutation(n)[:min(k_fire, n)]] += F(1.0)  # ... but here: |delta| = sqrt(3) > 0.6
        meshes.append(dict(theme=theme, kf=kf, verts=verts, colors=colors))
    return dict(cam=cam, res=res, slot=slot, keyframes=kfs, meshes=meshes)


def hand_case_keys():
    return [(c, r) for c in sorted(CAMERAS) for r in range(len(RESOLUTIONS))]


def nan_case(cam_name="small"):
    """Item 5: meshes whose projection is not a number, next to ordinary ones.  KF_AXIS (identity pose): the vertex
    (0, 0, 0) is the keyframe's centre, 0 / 0 in both coordinates; (x, 0, 0) is inf in x and 0 / 0 in y; a NaN
    coordinate in the vertex itself.  The NaN stands first, in the middle and last in the vertex list -- the three
    positions the reference's sequential fold tells apart.  -> (case dict like hand_case, indices of the NaN meshes)"""
    base = hand_case(cam_name, 0)
    cam = base["cam"]
    rng = np.random.Generator(np.random.PCG64(4242))
    rgb, depth, alpha, pose = base["keyframes"][KF_AXIS]
    meshes, bad = [], []
    for mi, n in enumerate((1, 3, 64, 65, 129, 200, 130, 40)):
        u, v, z = _positions("interior", n, cam, base["slot"], rng)
        verts = back_project(cam, pose, np.stack([u, v, z], -1))
        at = (0, n // 2, n - 1)[mi % 3]
        what = mi % 4
        if what == 0:
            verts[at] = (0, 0, 0)
        elif what == 1:
            verts[at] = (0.25, 0, 0)
        elif what == 2:
            verts[at] = (np.nan, 0.1, 1.0)
        else:
            verts[at] = (0.1, 0.2, np.nan)
        colors = rng.random((n, 3)).astype(F)
        bad.append(len(meshes))
        meshes.append(dict(theme="nan", kf=KF_AXIS, verts=verts, colors=colors))
        # an ordinary neighbour behind every NaN mesh
        meshes.append(dict(base["meshes"][7 * mi + 1]))
    return dict(base, meshes=meshes), bad


# ---- the fused per-frame flow with keyframe poses that are not the integration poses -------------------------------
# (entry point, pose_inv16 variant) per frame; the GPU test walks exactly this list
FUSED_PLAN = (
    # one call, n_ahead 0 (the first four frames only build up weight: the mesher emits nothing yet)
    ("stream0", "honest"), ("stream0", "honest"), ("stream0", "honest"), ("stream0", "honest"), ("stream0", "turn+"),
    ("stream0", "inside"),
    # one call, n_ahead 2: the last frame's stage stays pending and rides on the first host frame
    ("stream2", "turn-"), ("stream2", "shifted"), ("stream2", "away"), ("stream2", "inside"),
    ("host", "pitch"), ("host", "turn-"),
    ("host_tsdf", None),            # a TSDF-only frame: the pending stage goes out on its own
    ("texture_frame", "turn+"),     # tf_stream_frames_device + tf_texture_frame_device
    ("host", "honest"),             # (d): one more honest frame through the same handle
)
FUSED_CAM, FUSED_RES, FUSED_FIRST_ID = "small", F(0.01), 40


def variant_pose(pose, variant, centre_depth):
    """the camera-to-world pose whose inverse is handed over as pose_inv16"""
    P = np.asarray(pose, np.float64).reshape(3, 4).copy()
    yaw = math.atan2(P[0, 2], P[0, 0])
    t = P[:, 3].copy()
    if variant == "honest":
        return pose
    if variant in ("turn+", "turn-", "away"):  # turned about its own centre; 3.0 rad looks away from what it saw
        return synth.pose_yaw(yaw + {"turn+": 0.4, "turn-": -0.8, "away": 3.0}[variant], t)
    if variant == "pitch":
        return synth.pose_euler(yaw + 0.1, 0.5, 0.15, t)
    if variant == "inside":  # the camera's centre lies in the surface it looks at
        return synth.pose_yaw(yaw, t + P[:, 2] * centre_depth)
    if variant == "shifted":
        return synth.pose_yaw(yaw + 0.05, t + np.array([0.5, 0.2, 0.0]))
    raise KeyError(variant)


@functools.lru_cache(maxsize=None)
def fused_case():
    """-> dict(cam, res, frames [dict(how, variant, depth, rgba, pose, pose_inv16 | None, frame_id)]).  S-room at
    160 x 120 and 10 mm with two voxels of depth noise (a rough surface: meshes of more than 128 vertices, which the
    plain room never has) and per-pixel colour noise (a tap that is off by one pixel shows)."""
    cam = CAMERAS[FUSED_CAM]
    frames = []
    for k, (how, variant) in enumerate(FUSED_PLAN):
        d, rgba, q, pose = synth.room_frame(2 * k, cam, with_quality=False)
        rng = np.random.Generator(np.random.PCG64(500 + k))
        centre = float(d[cam.height // 2 - 3:cam.height // 2 + 3, cam.width // 2 - 3:cam.width // 2 + 3].max())
        d = np.where(d > 0, d + (rng.random(d.shape) - 0.5) * 4.0 * float(FUSED_RES), 0).astype(F)
        rgba = rgba.copy()
        rgba[..., :3] ^= rng.integers(0, 32, rgba[..., :3].shape, dtype=np.uint8)
        rgba[..., 3] = rng.integers(1, 256, rgba.shape[:2], dtype=np.uint8)  # (alpha != 0: the pixel's colour is valid)
        T = None if variant is None else synth.pose_inverse16(variant_pose(pose, variant, centre))
        frames.append(dict(how=how, variant=variant, depth=d, rgba=rgba, pose=pose, pose_inv16=T,
                           frame_id=FUSED_FIRST_ID + k, centre=centre))
    return dict(cam=cam, res=FUSED_RES, frames=frames)


def honest_meshes(case):
    """the meshes of a hand case that an ordinary keyframe sees whole: the round after the hostile one"""
    return [m for m in case["meshes"] if m["kf"] == KF_GENERAL and m["theme"] in HONEST_THEMES and len(m["verts"])]
