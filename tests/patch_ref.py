"""A second, independent statement of the patch projection -- Patch::CalculateTexCoords with Patch::bilinear,
Patch::bilinear_depth and the bounding box (Structure/Patch.cpp:40-170) -- in numpy, written from the reference's
behaviour and vectorised over the vertices of one patch.  Every operation is rounded to f32 in the reference's order:

  * T_g_l * (v, 1) accumulates column by column (:52-53);
  * the intrinsics are int-truncated (PinholeCamera.h:46-49) and the `+ 0.5` is a double addition (:55-56);
  * `> 0.6`, `> 0.7` and `> 0.3 * n` compare in double (:88-96);
  * bilinear's fourth tap is c2 again (:125-128), cv::Mat::at is unchecked pointer arithmetic (x == W is the next
    row's first pixel), a read past the last pixel -- undefined in the reference -- is 0 as in the oracle and the device;
  * the box is cv::Rect(float...) truncated and intersected with (0, 0, W - 1, H - 1) (:98-99), from a min / max that is
    a plain sequential fold (:66-69), then subtracted from the texcoords (:100-102).

Not a number ("undefined in the reference, defined here"): a projected coordinate that is NaN -- 0 / 0
for a vertex at the keyframe's centre, a NaN in the pose or the vertex -- counts as outside the image: the patch is
flagged caution and the coordinate is clamped to 0, like a negative one.  (In the reference NaN passes every clamp,
the fold's result depends on where the NaN stands in the vertex list, and floor(NaN) -> int is INT_MIN on x86.)

`project` returns what oracle.api.patch_project returns plus a census of the branches every vertex and the patch took;
`project_f64` is a plain double projection from the 3 x 4 camera-to-world pose (not from T16): it guards both f32
restatements against a shared misreading of the matrix layout."""
import numpy as np

F = np.float32


def _cam(cam):
    W, H = int(cam.width), int(cam.height)
    return W, H, F(int(cam.fx)), F(int(cam.fy)), F(int(cam.cx)), F(int(cam.cy))


def _fetch(flat, idx, n_pix):
    """flat[idx] with 0 outside [0, n_pix); flat is [n_pix] or [n_pix, 3]"""
    ok = (idx >= 0) & (idx < n_pix)
    got = flat[np.where(ok, idx, 0)].astype(F)
    return np.where(ok.reshape(ok.shape + (1,) * (got.ndim - 1)), got, F(0)), ok


def project(verts, colors, T16, rgb, depth, cam):
    W, H, fxi, fyi, cxi, cyi = _cam(cam)
    V = np.ascontiguousarray(verts, F).reshape(-1, 3)
    M = np.ascontiguousarray(colors, F).reshape(-1, 3)
    T = np.ascontiguousarray(T16, F).reshape(4, 4)
    n = len(V)
    rgbf = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    dflat = np.ascontiguousarray(depth, F).reshape(-1)
    assert len(rgbf) == W * H and len(dflat) == W * H
    with np.errstate(all="ignore"):
        vl = []
        for r in range(3):
            s = T[r, 0] * V[:, 0]
            s = s + T[r, 1] * V[:, 1]
            s = s + T[r, 2] * V[:, 2]
            s = s + T[r, 3] * F(1)
            vl.append(s.astype(F))
        dist = vl[2]
        x = (vl[0] / vl[2]).astype(F)
        y = (vl[1] / vl[2]).astype(F)
        a = ((x * fxi + cxi).astype(F).astype(np.float64) + 0.5).astype(F)
        b = ((y * fyi + cyi).astype(F).astype(np.float64) + 0.5).astype(F)
        Wf, Hf = F(W), F(H)
        caution_v = ~((a >= 0) & (a < Wf) & (b >= 0) & (b < Hf))  # (NaN: outside)
        clamp_l = ~(a >= 0)
        a = np.where(clamp_l, F(0), a)
        clamp_r = a >= Wf
        a = np.where(clamp_r, Wf, a)
        clamp_t = ~(b >= 0)
        b = np.where(clamp_t, F(0), b)
        clamp_b = b >= Hf
        b = np.where(clamp_b, Hf, b)
    raw = np.stack([a, b], -1).astype(F)
    # ---- the taps
    xi = np.floor(a).astype(np.int64)
    yi = np.floor(b).astype(np.int64)
    kind = np.where((xi < W - 1) & (yi < H - 1), 0,
                    np.where((xi < W - 1) & (yi == H - 1), 1, np.where((xi == W - 1) & (yi < H - 1), 2, 3)))
    i1 = yi * W + xi
    i2 = np.where(kind == 2, i1 + W, i1 + 1)  # (y, x + 1), or (y + 1, x) in the last column
    i3 = i1 + W  # (y + 1, x)
    use2 = kind != 3
    use3 = kind == 0
    ax = (xi + 1).astype(F) - a
    bx = a - xi.astype(F)
    ay = (yi + 1).astype(F) - b
    by = b - yi.astype(F)

    def blend(flat):
        c1, ok1 = _fetch(flat, i1, W * H)
        c2, ok2 = _fetch(flat, i2, W * H)
        c3, ok3 = _fetch(flat, i3, W * H)
        sh = (n,) + (1,) * (c1.ndim - 1)
        Ax, Bx, Ay, By, K = ax.reshape(sh), bx.reshape(sh), ay.reshape(sh), by.reshape(sh), kind.reshape(sh)
        t = (c1 * Ax) * Ay
        t = t + (c2 * Bx) * Ay
        t = t + (c3 * Ax) * By
        t = t + (c2 * Bx) * By
        r1 = c1 * Ax + c2 * Bx
        r2 = c1 * Ay + c2 * By
        out = np.where(K == 0, t, np.where(K == 1, r1, np.where(K == 2, r2, c1))).astype(F)
        return out, (ok1, ok2, ok3)

    with np.errstate(all="ignore"):
        col, oks = blend(rgbf)
        texcolor = (col / F(255)).astype(F)
        dpt, _ = blend(dflat)
        e = texcolor - M
        nrm = np.sqrt(e[:, 0] * e[:, 0] + (e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])).astype(F)
        cc = nrm.astype(np.float64) > 0.6
        dc = np.abs(dist - dpt).astype(np.float64) > 0.7
    past = ~oks[0] | (use2 & ~oks[1]) | (use3 & ~oks[2])
    # a tap whose column lies outside [0, W) but whose linear index is a pixel: the neighbouring row's
    next_row = oks[0] & ((xi >= W) | (xi < 0))
    n_color, n_depth = int(cc.sum()), int(dc.sum())
    by_depth = float(n_depth) > 0.3 * float(n)
    by_color = float(n_color) > 0.3 * float(n)
    # ---- the box: a sequential fold, as the reference does it
    minX, maxX, minY, maxY = F(W), F(0), F(H), F(0)
    for i in range(n):
        cX, cY = raw[i, 0], raw[i, 1]
        minX = minX if minX < cX else cX
        maxX = maxX if maxX > cX else cX
        minY = minY if minY < cY else cY
        maxY = maxY if maxY > cY else cY
    bbox = np.zeros(4, np.int32)
    clip = dict(left=False, right=False, top=False, bottom=False)
    no_box = not (maxX >= minX and maxY >= minY)
    texcoord = raw.copy()
    if not no_box:
        bx0, by0 = int(F(minX - F(2))), int(F(minY - F(2)))
        bw, bh = int(F(F(maxX - minX) + F(5))), int(F(F(maxY - minY) + F(5)))
        x1, y1 = max(bx0, 0), max(by0, 0)
        x2, y2 = min(bx0 + bw, W - 1), min(by0 + bh, H - 1)
        clip = dict(left=bx0 < 0, top=by0 < 0, right=bx0 + bw > W - 1, bottom=by0 + bh > H - 1)
        w, h = x2 - x1, y2 - y1
        if w <= 0 or h <= 0:
            x1 = y1 = w = h = 0
        bbox[:] = (x1, y1, w, h)
        texcoord[:, 0] = raw[:, 0] - F(x1)
        texcoord[:, 1] = raw[:, 1] - F(y1)
    n_caution = int(caution_v.sum())
    return dict(flag=-1 if n_caution else 0, texcoord=texcoord.astype(F), texcolor=texcolor, bbox=bbox,
                wrong_mapping=bool(by_depth or by_color), n_caution=n_caution,
                # ---- census, per vertex
                raw=raw, kind=kind, clamp_l=clamp_l, clamp_r=clamp_r, clamp_t=clamp_t, clamp_b=clamp_b,
                read_past=past, next_row=next_row, color_cmp=cc, depth_cmp=dc,
                # ---- census, per patch
                n_color=n_color, n_depth=n_depth, by_depth=by_depth, by_color=by_color, clip=clip, no_box=no_box)


def project_f64(verts, pose, cam):
    """Unclamped image coordinates (before the box shift) and camera-frame depth in double, from the 3 x 4
    camera-to-world pose: p = R^T (v - t)."""
    W, H, fxi, fyi, cxi, cyi = _cam(cam)
    P = np.asarray(pose, np.float64).reshape(3, 4)
    V = np.asarray(verts, np.float64).reshape(-1, 3)
    p = (V - P[:, 3]) @ P[:, :3]
    with np.errstate(all="ignore"):
        a = p[:, 0] / p[:, 2] * float(fxi) + float(cxi) + 0.5
        b = p[:, 1] / p[:, 2] * float(fyi) + float(cyi) + 0.5
    return np.stack([a, b], -1), p[:, 2]


VERTEX_CLASSES = ("kind1", "kind2", "kind3", "clamp_l", "clamp_r", "clamp_t", "clamp_b", "read_past", "next_row")
PATCH_CLASSES = ("caution", "by_depth_alone", "by_color_alone", "clip_left", "clip_right", "clip_top", "clip_bottom",
                 "roi_1_2_wide", "roi_wider", "roi_taller", "roi_wider_and_taller", "over_128")


def census(results, pw, ph):
    """Branch counts over a list of `project` results: vertices per vertex class, patches per patch class.
    pw x ph is the atlas slot (Atlas.h:62-65)."""
    c = {k: 0 for k in VERTEX_CLASSES + PATCH_CLASSES + ("interior", "no_box", "vertices", "patches")}
    for r in results:
        c["patches"] += 1
        c["vertices"] += len(r["kind"])
        c["interior"] += int((r["kind"] == 0).sum())
        for k in (1, 2, 3):
            c["kind%d" % k] += int((r["kind"] == k).sum())
        for k in ("clamp_l", "clamp_r", "clamp_t", "clamp_b", "read_past", "next_row"):
            c[k] += int(r[k].sum())
        cols, rows = int(r["bbox"][2]), int(r["bbox"][3])
        c["caution"] += r["n_caution"] > 0
        c["by_depth_alone"] += r["by_depth"] and not r["by_color"]
        c["by_color_alone"] += r["by_color"] and not r["by_depth"]
        for side in ("left", "right", "top", "bottom"):
            c["clip_" + side] += bool(r["clip"][side])
        c["no_box"] += bool(r["no_box"])
        c["roi_1_2_wide"] += 1 <= cols <= 2 and rows > 0
        c["roi_wider"] += cols > pw and 0 < rows <= ph
        c["roi_taller"] += rows > ph and 0 < cols <= pw
        c["roi_wider_and_taller"] += cols > pw and rows > ph
        c["over_128"] += len(r["kind"]) > 128
    return {k: int(v) for k, v in c.items()}
