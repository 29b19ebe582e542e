"""The patch projection at and beyond the keyframe image's borders, without a GPU: the oracle's tfo_patch_project
against tests/patch_ref.py (a second statement of Patch::CalculateTexCoords / bilinear / bilinear_depth,
Structure/Patch.cpp:40-170), raw bits, on the very inputs tests/test_gpu_patch_borders.py feeds the device -- and the
CENSUS CONDITIONS that keep those GPU tests from being vacuous: for every input set the reference alone must show
every branch class (tap kinds 1-3, the four clamps, reads past the image, next-row reads, caution, wrong_mapping by
depth alone and by colour alone, the box clipped at each side, ROIs 1-2 pixels wide, wider / taller than the slot)
with at least 20 vertices or 5 patches.  These are conditions on the inputs, not measurements: a generator that is
weakened (the turned poses dropped, the border themes dropped) trips them, which the last tests here show.

Atlas::UpdateBuffer's copy / cv::resize (Structure/Atlas.cpp:71-91) at the ROI shapes these projections produce is
compared with a direct numpy statement (resize facts: tests/test_resize_properties.py)."""
import numpy as np
import pytest

from oracle import api as O
from tests import patch_inputs as PI
from tests import patch_ref as PR
from texturefusion_amd import synth

MIN_VERTICES, MIN_PATCHES = 20, 5
# |f32 - f64| of an unclamped image coordinate, in pixels, as a multiple of the image width: a rounding bound, O(W * 2^-23)
# per operation.  Measured maxima on these inputs: 1.48e-4 at W = 640, 7.6e-5 at W = 328, 3.9e-5 at W = 160 -- i.e.
# 2.3e-7 W, 2.3e-7 W, 2.4e-7 W; the bound is two-fold that.
F64_TOL_PER_W = 5e-7
CLAMP_MARGIN = 0.01  # pixels: vertices whose f64 position is closer than this to a clamp are not compared with f64


def _same(r, o):
    assert np.array_equal(r["texcoord"].view(np.uint32), o["texcoord"].view(np.uint32))
    assert np.array_equal(r["texcolor"].view(np.uint32), o["texcolor"].view(np.uint32))
    assert np.array_equal(r["bbox"], o["bbox"])
    assert r["flag"] == o["flag"] and r["n_caution"] == o["n_caution"] and r["wrong_mapping"] == o["wrong_mapping"]


def shortfalls(c, patch_classes=PR.PATCH_CLASSES):
    """the classes of a census that are below the condition"""
    return [k for k in PR.VERTEX_CLASSES if c[k] < MIN_VERTICES] + [k for k in patch_classes if c[k] < MIN_PATCHES]


def _project_case(case, meshes=None, kf_override=None):
    cam = case["cam"]
    out = []
    for m in (case["meshes"] if meshes is None else meshes):
        rgb, depth, alpha, pose = case["keyframes"][kf_override or m["kf"]]
        out.append((m, pose, PR.project(m["verts"], m["colors"], synth.pose_inverse16(pose), rgb, depth, cam)))
    return out


@pytest.mark.parametrize("key", PI.hand_case_keys(), ids=lambda k: "%s-%d" % k)
def test_hand_meshes_oracle_equals_reference_and_census(key):
    case = PI.hand_case(*key)
    cam, oc = case["cam"], O.camera_from(case["cam"])
    W, H = cam.width, cam.height
    got = _project_case(case)
    worst = 0.0
    for m, pose, r in got:
        rgb, depth, alpha, _ = case["keyframes"][m["kf"]]
        _same(r, O.patch_project(m["verts"], m["colors"], synth.pose_inverse16(pose), rgb, depth, oc))
        if len(m["verts"]):  # the f64 projection from the 3 x 4 pose: guards both against a shared misreading of T16
            a64, z64 = PR.project_f64(m["verts"], pose, cam)
            ok = ((z64 > 0.05) & (a64[:, 0] > CLAMP_MARGIN) & (a64[:, 0] < W - CLAMP_MARGIN) &
                  (a64[:, 1] > CLAMP_MARGIN) & (a64[:, 1] < H - CLAMP_MARGIN))
            if ok.any():
                worst = max(worst, float(np.abs(r["raw"].astype(np.float64)[ok] - a64[ok]).max()))
    print("largest |f32 - f64| texcoord difference: %.3g px at W = %d" % (worst, W))
    assert worst <= F64_TOL_PER_W * W
    c = PR.census([r for _, _, r in got], *case["slot"])
    print(key, c)
    assert shortfalls(c) == []
    assert c["interior"] >= MIN_VERTICES and c["no_box"] >= 1  # (no box: the empty mesh)
    assert sorted({len(m["verts"]) for m in case["meshes"]} & set(PI.COUNTS)) == sorted(PI.COUNTS)
    # the counts of the colour / depth compares land on both sides of 0.3 * nv, one apart
    for cmp_, flag, lo, hi in (("n_color", "by_color", "thr_color_lo", "thr_color_hi"),
                               ("n_depth", "by_depth", "thr_depth_lo", "thr_depth_hi")):
        below = [r for m, _, r in got if m["theme"] == lo]
        above = [r for m, _, r in got if m["theme"] == hi]
        assert len(below) >= MIN_PATCHES and len(above) >= MIN_PATCHES
        for r in below:
            n = len(r["kind"])
            assert r[cmp_] == int(0.3 * n) and not r[flag] and not r["wrong_mapping"]
        for r in above:
            n = len(r["kind"])
            assert r[cmp_] == int(0.3 * n) + 1 and r[flag] and r["wrong_mapping"]
    neither = [r for m, _, r in got if m["theme"] == "interior" and len(r["kind"])]
    assert all(not r["wrong_mapping"] for r in neither) and len(neither) >= MIN_PATCHES


@pytest.mark.parametrize("key", PI.hand_case_keys(), ids=lambda k: "%s-%d" % k)
def test_honest_round_is_honest(key):
    """The round that follows the hostile one in the GPU test (the interior meshes against KF_HONEST) takes none of the
    border branches -- it is the 'ordinary call' that shows nothing was left behind."""
    case = PI.hand_case(*key)
    meshes = PI.honest_meshes(case)
    assert len(meshes) >= 20
    got = _project_case(case, meshes, kf_override=PI.KF_HONEST)
    oc = O.camera_from(case["cam"])
    rgb, depth, alpha, pose = case["keyframes"][PI.KF_HONEST]
    for m, _, r in got:
        _same(r, O.patch_project(m["verts"], m["colors"], synth.pose_inverse16(pose), rgb, depth, oc))
        assert r["n_caution"] == 0 and (r["kind"] == 0).all() and not r["read_past"].any()


def test_known_answer_on_the_optical_axis():
    """One vertex on the optical axis lands at (int(cx) + 0.5, int(cy) + 0.5) before the box shift; the box is
    cv::Rect(x - 2, y - 2, 5, 5) truncated."""
    for cam in PI.CAMERAS.values():
        rgb, depth, alpha = PI.keyframe_images(cam, 1)
        pose = PI.general_pose()
        P = pose.astype(np.float64)
        v = (P[:, 3] + 1.25 * P[:, 2]).astype(np.float32).reshape(1, 3)
        col = np.zeros((1, 3), np.float32)
        for r in (PR.project(v, col, synth.pose_inverse16(pose), rgb, depth, cam),
                  O.patch_project(v, col, synth.pose_inverse16(pose), rgb, depth, O.camera_from(cam))):
            want = np.array([int(cam.cx) + 0.5, int(cam.cy) + 0.5])
            un = r["texcoord"][0].astype(np.float64) + r["bbox"][:2]
            assert np.abs(un - want).max() < 1e-3, (un, want)
            assert np.array_equal(r["bbox"], [int(cam.cx) - 2, int(cam.cy) - 2, 5, 5])
            assert r["flag"] == 0 and r["n_caution"] == 0
        # exactly, with the identity pose: x = y = 0 -> cx_i + 0.5
        v = np.array([[0.0, 0.0, 2.0]], np.float32)
        r = PR.project(v, col, synth.pose_inverse16(PI.axis_pose()), rgb, depth, cam)
        assert np.array_equal(r["raw"][0], np.float32([int(cam.cx) + 0.5, int(cam.cy) + 0.5]))


def _fused_census(case, plan_filter=lambda f: True):
    cam, res = case["cam"], case["res"]
    ov = O.Volume(res, O.camera_from(cam), O.default_integrator())
    oa = O.Atlas(res)
    per_frame, results = [], []
    for f in case["frames"]:
        if f["pose_inv16"] is None:
            ov.integrate_frame(f["depth"], f["rgba"], f["pose"])
            continue
        T = f["pose_inv16"] if plan_filter(f) else synth.pose_inverse16(f["pose"])
        ov.frame_textured(oa, f["depth"], f["rgba"], f["pose"], T, f["frame_id"])
        mine = []
        for cid in ov.list_meshes():  # later frames overwrite patches: the census is taken after EACH frame
            p = ov.get_patch(cid)
            if p is None or p["frameid"] != f["frame_id"]:
                continue
            m = ov.get_mesh(cid)
            r = PR.project(m["verts"], m["colors"], T, f["rgba"][..., :3], f["depth"], cam)
            assert np.array_equal(r["texcoord"].view(np.uint32), p["texcoord"].view(np.uint32)), cid
            assert np.array_equal(r["texcolor"].view(np.uint32), p["texcolor"].view(np.uint32)), cid
            assert np.array_equal(r["bbox"], p["bbox"]), cid
            assert (r["n_caution"] > 0) == bool(p["flags"] & 2) and r["wrong_mapping"] == bool(p["flags"] & 4), cid
            mine.append(r)
        per_frame.append((f, PR.census(mine, oa.pw, oa.ph)))
        results += mine
    return PR.census(results, oa.pw, oa.ph), per_frame


def test_fused_frames_oracle_equals_reference_and_census():
    """The fused per-frame unit with keyframe poses that are not the integration poses: every patch the oracle makes,
    frame by frame, equals patch_ref; over the run every class occurs, with at least 5 patches of more than 128
    vertices (the second sweep of the fused kernels)."""
    c, per_frame = _fused_census(PI.fused_case())
    for f, cf in per_frame:
        print(f["how"], f["variant"], {k: v for k, v in cf.items() if v})
    print("run", c)
    assert shortfalls(c) == []
    assert c["over_128"] >= MIN_PATCHES
    last = per_frame[-1]
    assert last[0]["variant"] == "honest" and last[1]["patches"] > 300


def test_census_conditions_trip_on_weakened_generators():
    """Drop the border themes of the hand-made meshes, or the turned poses of the fused run: the conditions fail."""
    case = PI.hand_case("small", 0)
    honest = [r for _, _, r in _project_case(case, PI.honest_meshes(case), kf_override=PI.KF_HONEST)]
    missing = shortfalls(PR.census(honest, *case["slot"]))
    assert {"kind1", "kind2", "kind3", "clamp_l", "clamp_r", "clamp_t", "clamp_b", "read_past", "next_row", "caution",
            "clip_right", "roi_1_2_wide"} <= set(missing)
    c, _ = _fused_census(PI.fused_case(), plan_filter=lambda f: False)  # every pose_inv16 the integration pose's
    missing = shortfalls(c)
    assert {"kind2", "clamp_r", "next_row", "clip_right", "roi_1_2_wide"} <= set(missing), missing


# ---- not a number -----------------------------------------------------------------------------------
def test_nan_projection_is_defined_and_the_oracle_follows_it():
    """A projected coordinate that is NaN counts as outside the image: caution, clamped to 0 -- so the box no longer
    depends on where the NaN stands in the vertex list.  The oracle and patch_ref agree bit for bit; moving the NaN
    vertex to another position of the list changes nothing but the order of the per-vertex outputs."""
    case, bad = PI.nan_case()
    cam, oc = case["cam"], O.camera_from(case["cam"])
    for i in bad:
        m = case["meshes"][i]
        rgb, depth, alpha, pose = case["keyframes"][m["kf"]]
        T = synth.pose_inverse16(pose)
        r = PR.project(m["verts"], m["colors"], T, rgb, depth, cam)
        _same(r, O.patch_project(m["verts"], m["colors"], T, rgb, depth, oc))
        assert r["flag"] == -1 and r["n_caution"] >= 1
        assert np.isfinite(r["texcoord"]).all() and np.isfinite(r["texcolor"]).all()
        assert (r["raw"].min(axis=0) == 0).any()  # the NaN coordinate went to 0
        perm = np.roll(np.arange(len(m["verts"])), 1)
        r2 = O.patch_project(m["verts"][perm], m["colors"][perm], T, rgb, depth, oc)
        assert np.array_equal(r2["bbox"], r["bbox"]) and r2["wrong_mapping"] == r["wrong_mapping"]
        assert np.array_equal(r2["texcoord"].view(np.uint32), r["texcoord"][perm].view(np.uint32))


# ---- Atlas::UpdateBuffer at the ROI shapes the projections produce ----------------------------------------------------
def _resize_ref(src, dw, dh):
    """cv::resize(src, dst, dst.size()), CV_8UC3, INTER_LINEAR: coordinates (d + 0.5) * scale - 0.5, 11-bit coefficients,
    horizontal pass in int32, vertical pass ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2 >> 2."""
    sh, sw = src.shape[:2]
    f32 = np.float32

    def axis(n_dst, n_src, clamp_coeff):
        scale = 1.0 / (float(n_dst) / n_src)
        f = ((np.arange(n_dst) + 0.5) * scale - 0.5).astype(f32)
        s = np.floor(f).astype(np.int64)
        f = (f - s.astype(f32)).astype(f32)
        if clamp_coeff:  # x: the coefficient is reset at the borders
            f = np.where((s < 0) | (s >= n_src - 1), f32(0), f)
            s0 = np.clip(s, 0, n_src - 1)
            s1 = np.minimum(s0 + 1, n_src - 1)
        else:  # y: indices clamped, coefficients kept
            s0 = np.clip(s, 0, n_src - 1)
            s1 = np.clip(s + 1, 0, n_src - 1)
        c0 = np.rint(((f32(1) - f) * f32(2048)).astype(np.float64)).astype(np.int64)
        c1 = np.rint((f * f32(2048)).astype(np.float64)).astype(np.int64)
        return s0, s1, c0, c1

    x0, x1, a0, a1 = axis(dw, sw, True)
    y0, y1, b0, b1 = axis(dh, sh, False)
    S = src.astype(np.int64)
    h0 = S[y0][:, x0] * a0[None, :, None] + S[y0][:, x1] * a1[None, :, None]
    h1 = S[y1][:, x0] * a0[None, :, None] + S[y1][:, x1] * a1[None, :, None]
    val = (((b0[:, None, None] * (h0 >> 4)) >> 16) + ((b1[:, None, None] * (h1 >> 4)) >> 16) + 2) >> 2
    return np.clip(val, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("res_index", [0, 1])
def test_blit_at_the_roi_shapes_of_border_patches(res_index):
    res = PI.RESOLUTIONS[res_index]
    cam = PI.CAMERAS["odd"]
    W, H = cam.width, cam.height
    img = PI.keyframe_images(cam, 5)[0]
    a = O.Atlas(res, 1920, 720)
    pw, ph = a.pw, a.ph
    assert (pw, ph) == PI.slot_size(res)
    shapes = [(1, 1), (1, 7), (9, 1), (1, ph + 3), (pw + 5, 1), (W - 1, H - 1), (pw, ph), (pw + 1, ph), (pw, ph + 1),
              (2, ph), (pw, 2), (W - 1, 1), (1, H - 1)]
    for cols, rows in shapes:
        for bx, by in ((0, 0), (W - 1 - cols, H - 1 - rows)):  # against the first and against the last row / column
            ok, t = a.alloc()
            assert ok == 0
            r, ratio = a.blit(t, img, [bx, by, cols, rows])
            assert r == 0
            x, y = t % 1920, t // 1920
            slot = a.buffer()[y:y + ph, x:x + pw]
            src = img[by:by + rows, bx:bx + cols]
            want_ratio = (np.float32(pw) / np.float32(cols) if cols > pw else np.float32(1),
                          np.float32(ph) / np.float32(rows) if rows > ph else np.float32(1))
            assert ratio[0] == want_ratio[0] and ratio[1] == want_ratio[1], (cols, rows)
            if cols > pw or rows > ph:  # cv::resize into the FULL slot
                assert np.array_equal(slot, _resize_ref(src, pw, ph)), (cols, rows, bx, by)
            else:  # copyTo at the slot's origin; the rest of the slot is untouched
                assert np.array_equal(slot[:rows, :cols], src), (cols, rows, bx, by)
                rest = slot.copy()
                rest[:rows, :cols] = 0
                assert not rest.any()
    a.close()
