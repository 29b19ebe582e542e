"""numpy float32 restatement of tf_ray.hip (a helper of the raycast tests, not a test module).

k_query: GetSDF / GetWeight / GetSDFAndGradient / trilinear SDF / trilinear colour, operation for operation in f32 (the
library is built with -ffp-contract=off, so the device results are reproduced bit for bit).  k_raycast, all four maps
(RefVolume.raycast_maps): the march (chunk DDA over absent chunks, voxel steps where the sampler is invalid,
max(voxel, 0.75 sdf) where it is valid, linear refinement at the first + -> - crossing) over the same samples, the vertex
o + thit * d, the normal from six taps of the trilinear SDF (central, or one-sided and doubled, or none), the trilinear
colour at the hit, and a per-pixel trace of the branches a ray took.  raycast_depth is its depth map.

The volume is a set of chunks: ids [n, 3] int32 with sdf / weight [n, 512] f32 and colour [n, 2048] u16 (R, G, B, count
per voxel), as Volume.get_chunks (HIP) or oracle.api.Volume.get_chunk return them.
"""
import numpy as np

from texturefusion_amd import synth

F = np.float32
STEP_K = F(0.75)
GAP = F(4.0)
VOX_LIMIT = F(8388607.0)
CHUNK_LIMIT = F(1048576.0)
END_HIT, END_BACK, END_FAR, END_STEPS, END_CHUNK = 1, 2, 3, 4, 5  # trace["end"] of raycast_maps
# One rule of the march or of the normal changed at a time, for tests/test_raycast_cpu.py alone: the hand-built cases of
# tests/ray_inputs.py must tell every one of these from the kernel's rule.
#   gap_lt            t - pt < gap instead of <=            hit_lt           s < 0 closes a crossing instead of s <= 0
#   far_lt            t < far instead of <=                 no_back          no - -> + break
#   no_eps            the chunk jump lands on the chunk's face, without eps
#   one_sided_1       the one-sided difference not doubled  one_sided_sign   and with the wrong sign
#   reset_on_invalid  an invalid sample forgets the last valid one
_FLIPS = ("gap_lt", "hit_lt", "far_lt", "no_back", "no_eps", "one_sided_1", "one_sided_sign", "reset_on_invalid")


def _floor_in(a, lim):
    f = np.floor(a)
    with np.errstate(invalid="ignore"):
        ok = (f > -lim) & (f < lim)
    return np.where(ok, f, F(0)).astype(np.int64), ok


def _lerp(a, b, t):
    return a + t * (b - a)


def _tri8(c, fx, fy, fz):
    e0, e1 = _lerp(c[0], c[1], fx), _lerp(c[2], c[3], fx)
    e2, e3 = _lerp(c[4], c[5], fx), _lerp(c[6], c[7], fx)
    return _lerp(_lerp(e0, e1, fy), _lerp(e2, e3, fy), fz)


class RefVolume:
    def __init__(self, ids, sdf, weight, color, res):
        self.res = F(res)
        ids = np.asarray(ids, np.int64).reshape(-1, 3)
        self.sdf = np.asarray(sdf, np.float32).reshape(-1, 512)
        self.w = np.asarray(weight, np.float32).reshape(-1, 512)
        self.col = np.asarray(color, np.uint16).reshape(-1, 512, 4)
        # one unused row behind the chunks: absent lookups index row 0 and are masked (an empty volume has none else)
        self.sdf = np.concatenate([self.sdf, np.zeros((1, 512), np.float32)])
        self.w = np.concatenate([self.w, np.zeros((1, 512), np.float32)])
        self.col = np.concatenate([self.col, np.zeros((1, 512, 4), np.uint16)])
        keys = self._key(ids[:, 0], ids[:, 1], ids[:, 2])
        self.order = np.argsort(keys, kind="stable")
        self.keys = keys[self.order]

    @staticmethod
    def from_volume(vol, ids, res):
        """chunks of a HIP capi.Volume (get_chunks) or an oracle Volume (get_chunk one by one)"""
        ids = np.asarray(ids, np.int32).reshape(-1, 3)
        if hasattr(vol, "get_chunks"):
            s, w, c = vol.get_chunks(ids) if len(ids) else (np.zeros((0, 512), np.float32),) * 2 + (np.zeros((0, 2048), np.uint16),)
        else:
            got = [vol.get_chunk(cid) for cid in ids]
            s = np.array([g[0] for g in got], np.float32).reshape(-1, 512)
            w = np.array([g[1] for g in got], np.float32).reshape(-1, 512)
            c = np.array([g[2] for g in got], np.uint16).reshape(-1, 2048)
        return RefVolume(ids, s, w, c, res)

    @staticmethod
    def _key(x, y, z):
        b = 1 << 20
        return ((x + b) << 42) | ((y + b) << 21) | (z + b)

    def slot(self, x, y, z):
        """index of chunk (x, y, z) in the arrays, -1 where absent"""
        x, y, z = (np.asarray(a, np.int64) for a in (x, y, z))
        b = 1 << 20
        inr = (x >= -b) & (x < b) & (y >= -b) & (y < b) & (z >= -b) & (z < b)
        k = self._key(np.where(inr, x, 0), np.where(inr, y, 0), np.where(inr, z, 0))
        if len(self.keys) == 0:
            return np.full(k.shape, -1, np.int64)
        i = np.minimum(np.searchsorted(self.keys, k), len(self.keys) - 1)
        hit = inr & (self.keys[i] == k)
        return np.where(hit, self.order[i], -1)

    # ---- k_query ----------------------------------------------------------------------------------------------
    def point_voxel(self, p):
        res = self.res
        rc, ir = F(1) / (F(8) * res), F(1) / res
        c, okc = zip(*(_floor_in(p[:, a] * rc, CHUNK_LIMIT) for a in range(3)))
        ok = okc[0] & okc[1] & okc[2]
        s = np.where(ok, self.slot(*c), -1)
        v = []
        for a in range(3):
            rel = p[:, a] - (8 * c[a]).astype(np.float32) * res
            va, oka = _floor_in(rel * ir, CHUNK_LIMIT)
            v.append(va)
            ok &= oka
        vid = (v[2] * 8 + v[1]) * 8 + v[0]
        ok &= (s >= 0) & (vid >= 0) & (vid < 512)
        return np.where(ok, s, -1), np.where(ok, vid, 0)

    def gradient(self, p):
        res = self.res
        half, ir, rc = res / F(2), F(1) / res, F(1) / (res * F(8))
        n = len(p)
        ok = np.ones(n, bool)
        cid, vid = [], []
        for a in range(3):
            q = np.floor(p[:, a] / res) * res + half
            vg, o1 = _floor_in(q * ir, VOX_LIMIT)
            cc, o2 = _floor_in(q * rc, CHUNK_LIMIT)
            vv = vg - cc * 8
            ok &= o1 & o2 & (vv >= 0) & (vv <= 7)
            cid.append(cc)
            vid.append(np.where(ok, vv, 0))
        centre = np.where(ok, self.slot(*cid), -1)
        ok &= centre >= 0
        d = np.zeros((6, n), np.float32)
        for k in range(6):
            a, s = k >> 1, (1 if k & 1 else -1)
            nb = list(vid)
            nb[a] = (vid[a] + s) & 7
            cross = vid[a] == (0 if s < 0 else 7)
            c2 = list(cid)
            c2[a] = cid[a] + s
            sl = np.where(cross, self.slot(*c2), centre)
            ok &= sl >= 0
            val = self.sdf[np.maximum(sl, 0), (nb[2] * 8 + nb[1]) * 8 + nb[0]]
            ok &= val < F(1)
            d[k] = val
        g = np.stack([d[1] - d[0], d[3] - d[2], d[5] - d[4]], 1)
        return np.where(ok[:, None], g, F(0)), ok

    def trilinear(self, p, want_rgb=True):
        """(sdf [n], sdf valid [n], rgb [n, 3] u8, rgb valid [n])"""
        ir = F(1) / self.res
        n = len(p)
        g = [p[:, a] * ir - F(0.5) for a in range(3)]
        ok = np.ones(n, bool)
        i, f = [], []
        for a in range(3):
            ia, oka = _floor_in(g[a], VOX_LIMIT)
            ok &= oka
            i.append(ia)
            f.append(g[a] - np.floor(g[a]))
        c = np.zeros((8, n), np.float32)
        cnt = np.zeros((8, n, 4), np.float32)
        okc = ok.copy()
        inr = ok.copy()  # (the corners are looked up wherever the coordinates are in range: colour validity does not
        for k in range(8):  # depend on the corners' weights -- a colour-only voxel, weight 0, count > 0, counts as coloured)
            vx, vy, vz = i[0] + (k & 1), i[1] + ((k >> 1) & 1), i[2] + ((k >> 2) & 1)
            sl = np.where(inr, self.slot(vx >> 3, vy >> 3, vz >> 3), -1)
            vi = ((vz & 7) * 8 + (vy & 7)) * 8 + (vx & 7)
            s0 = np.maximum(sl, 0)
            ok_k = sl >= 0
            c[k] = np.where(ok_k, self.sdf[s0, vi], F(0))
            okc &= ok_k & (self.col[s0, vi, 3] > 0)
            ok &= ok_k & (self.w[s0, vi] > F(0))
            cnt[k] = self.col[s0, vi].astype(np.float32)
        sdf = np.where(ok, _tri8(c, *f), F(0))
        rgb = np.zeros((n, 3), np.uint8)
        if want_rgb:
            with np.errstate(divide="ignore", invalid="ignore"):
                for ch in range(3):
                    m = cnt[:, :, ch] / cnt[:, :, 3]
                    v = np.minimum(F(255), np.floor(_tri8(m, *f) + F(0.5)))
                    rgb[:, ch] = np.where(okc, v, F(0)).astype(np.uint8)
        return sdf, ok, rgb, okc

    def query(self, points):
        """all five outputs of k_query, as tf_query_points writes them (0 where invalid)"""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = len(p)
        flags = np.zeros(n, np.uint32)
        s, vid = self.point_voxel(p)
        has = s >= 0
        w = np.where(has, self.w[np.maximum(s, 0), vid], F(0))
        sd = self.sdf[np.maximum(s, 0), vid]
        ok_sdf = has & (w.astype(np.float64) > 1e-12)
        flags |= np.where(ok_sdf, 1, 0).astype(np.uint32) | np.where(has, 2, 0).astype(np.uint32)
        grad, okg = self.gradient(p)
        flags |= np.where(okg, 4, 0).astype(np.uint32)
        st, okt, rgb, okc = self.trilinear(p)
        flags |= np.where(okt, 8, 0).astype(np.uint32) | np.where(okc, 16, 0).astype(np.uint32)
        return {"flags": flags, "sdf": np.where(ok_sdf, sd, F(0)), "weight": w, "grad": grad, "sdf_tri": st, "rgb": rgb}

    # ---- k_raycast: the march and the four maps -----------------------------------------------------------------
    def raycast_depth(self, pose, fx, fy, cx, cy, W, H, near, far, max_steps):
        """camera-frame depth [H, W] (0 = miss); fx .. cy as given to tf_set_camera (truncated here)"""
        return self.raycast_maps(pose, fx, fy, cx, cy, W, H, near, far, max_steps)["depth"]

    def raycast_maps(self, pose, fx, fy, cx, cy, W, H, near, far, max_steps, _flip=None):
        """raycast_body, all four maps: 'depth' [H, W] f32 (0 = miss), 'vertex' [3, H, W] f32, 'normal' [3, H, W] f32,
        'rgba' [H, W, 4] u8, and 'trace', a dict of small integers per pixel ([H, W] unless noted) that says which way
        a ray went:
          end      how the march ended: END_HIT, END_BACK (- -> +), END_FAR (t > far), END_STEPS (the step cap),
                   END_CHUNK (a chunk coordinate out of range)
          steps    samples taken (loop iterations entered)
          jumps    absent-chunk jumps;  invalid  steps over an invalid sample;  gap  valid samples whose pairing the
                   kRayGap rule refused
          m        [3, H, W] the normal's validity bits per axis (bit 0: minus tap, bit 1: plus tap), -1 on a miss
          t_end    f32: t when the march ended (on a hit or a back break, the t of the sample that ended it)
        fx .. cy as given to tf_raycast_camera (truncated here).  _flip: see _FLIPS."""
        assert _flip is None or _flip in _FLIPS
        res = self.res
        ir, cs, rc, eps, gap = F(1) / res, F(8) * res, F(1) / (F(8) * res), res * F(0.015625), GAP * res
        fxi, fyi, cxs, cys = F(int(fx)), F(int(fy)), F(int(cx)) + F(0.5), F(int(cy)) + F(0.5)
        P = np.asarray(pose, np.float32).reshape(3, 4)
        yy, xx = np.mgrid[0:H, 0:W]
        dcx = (xx.reshape(-1).astype(np.float32) - cxs) / fxi
        dcy = (yy.reshape(-1).astype(np.float32) - cys) / fyi
        d = [(P[r, 0] * dcx + P[r, 1] * dcy) + P[r, 2] for r in range(3)]
        o = [P[r, 3] for r in range(3)]
        n = W * H
        t = np.full(n, F(near), np.float32)
        pt = np.zeros(n, np.float32)
        ps = np.zeros(n, np.float32)
        pok = np.zeros(n, bool)
        thit = np.full(n, F(-1), np.float32)
        live = np.ones(n, bool)
        end = np.full(n, END_STEPS, np.int8)
        steps, jumps, invalid, gaps = (np.zeros(n, np.int32) for _ in range(4))
        for _ in range(int(max_steps)):
            in_far = (t < F(far)) if _flip == "far_lt" else (t <= F(far))
            end[live & ~in_far] = END_FAR
            live &= in_far
            idx = np.nonzero(live)[0]
            if len(idx) == 0:
                break
            steps[idx] += 1
            tt = t[idx]
            dd = [a[idx] for a in d]
            x = [o[a] + tt * dd[a] for a in range(3)]
            cc, okc = zip(*(_floor_in(x[a] * rc, CHUNK_LIMIT) for a in range(3)))
            inr = okc[0] & okc[1] & okc[2]
            live[idx[~inr]] = False
            end[idx[~inr]] = END_CHUNK
            absent = inr & (self.slot(*cc) < 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                tx = []
                for a in range(3):
                    hi = ((cc[a] + 1).astype(np.float32) * cs - o[a]) / dd[a]
                    lo = (cc[a].astype(np.float32) * cs - o[a]) / dd[a]
                    tx.append(np.where(dd[a] > 0, hi, np.where(dd[a] < 0, lo, np.float32(np.inf))))
            tn = np.maximum(np.minimum(np.minimum(tx[0], tx[1]), tx[2]), tt)
            if _flip != "no_eps":
                tn = tn + eps
            s, oks, _, _ = self.trilinear(np.stack(x, 1), want_rgb=False)
            present = inr & ~absent
            inval = present & ~oks
            val = present & oks
            p_s, p_t = ps[idx], pt[idx]
            near_enough = (tt - p_t < gap) if _flip == "gap_lt" else (tt - p_t <= gap)
            p_ok = pok[idx] & near_enough
            hit = val & p_ok & (p_s > 0) & ((s < 0) if _flip == "hit_lt" else (s <= 0))
            back = val & p_ok & (p_s <= 0) & (s > 0) & ~hit
            if _flip == "no_back":
                back[:] = False
            with np.errstate(divide="ignore", invalid="ignore"):
                th = p_t + (tt - p_t) * (p_s / (p_s - s))
            thit[idx[hit]] = th[hit]
            live[idx[hit | back]] = False
            end[idx[hit]] = END_HIT
            end[idx[back]] = END_BACK
            jumps[idx[absent]] += 1
            invalid[idx[inval]] += 1
            gaps[idx[val & pok[idx] & ~near_enough]] += 1
            go = val & ~hit & ~back
            newt = tt.copy()
            newt[absent] = tn[absent]
            newt[inval] = tt[inval] + res
            newt[go] = tt[go] + np.maximum(res, STEP_K * s[go])
            t[idx] = newt
            keep = np.zeros(len(idx), bool) if _flip == "reset_on_invalid" else pok[idx]
            pok[idx] = np.where(go, True, np.where(absent, False, np.where(inval, keep, p_ok)))
            pt[idx[go]] = tt[go]
            ps[idx[go]] = s[go]
        hit = thit >= 0
        hidx = np.nonzero(hit)[0]
        h = [(o[a] + thit * d[a])[hidx] for a in range(3)]
        vertex = np.zeros((3, n), np.float32)
        normal = np.zeros((3, n), np.float32)
        rgba = np.zeros((n, 4), np.uint8)
        m = np.full((3, n), -1, np.int8)
        if len(hidx):
            for a in range(3):
                vertex[a, hidx] = h[a]
            # the six taps: one voxel each way through the trilinear SDF (an invalid tap reads 0)
            g, ok = [], np.ones(len(hidx), bool)
            for a in range(3):
                tap = []
                for sg in (-res, res):
                    p = [h[b] + (sg if b == a else F(0)) for b in range(3)]
                    tap.append(self.trilinear(np.stack(p, 1), want_rgb=False)[:2])
                (sm, okm), (sp, okp) = tap
                ma = okm.astype(np.int8) + 2 * okp.astype(np.int8)
                m[a, hidx] = ma
                k2 = F(1) if _flip == "one_sided_1" else F(2)
                if _flip == "one_sided_sign":
                    k2 = -k2
                g.append(np.where(ma == 3, sp - sm, np.where(ma == 2, k2 * sp, -k2 * sm)).astype(np.float32))
                ok &= ma != 0
            ln = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            ok &= ln > 0
            with np.errstate(divide="ignore", invalid="ignore"):
                for a in range(3):
                    normal[a, hidx] = np.where(ok, g[a] / ln, F(0))
            _, _, rgb, okc = self.trilinear(np.stack(h, 1))
            rgba[hidx, :3] = np.where(okc[:, None], rgb, 0)
            rgba[hidx, 3] = 255
        img = lambda a: a.reshape(H, W)
        trace = {"end": img(end), "steps": img(steps), "jumps": img(jumps), "invalid": img(invalid), "gap": img(gaps),
                 "m": m.reshape(3, H, W), "t_end": img(t.copy())}
        return {"depth": img(np.where(hit, thit, F(0))), "vertex": vertex.reshape(3, H, W), "normal": normal.reshape(3, H, W),
                "rgba": rgba.reshape(H, W, 4), "trace": trace}


# ---- the S-wall scene of the raycast tests --------------------------------------------------------------------------
WALL_Z = 1.22  # mid-chunk (chunk z = 30 spans 1.20 .. 1.24 m at 5 mm): chunks hold both sides of the surface


def wall_poses():
    """S-wall from five poses: the same fronto-parallel plane, the camera shifted sideways so that the image borders of
    the middle pose are seen by the others"""
    return [synth.pose_yaw(0.0, t) for t in ((0.0, 0.0, 0.0), (0.08, 0.0, 0.0), (-0.08, 0.0, 0.0), (0.0, 0.08, 0.0),
                                              (0.0, -0.08, 0.0))]


def wall_frames(cam):
    out = []
    for k, pose in enumerate(wall_poses()):
        depth, rgba, _, _ = synth.wall_frame(WALL_Z - float(pose[2, 3]), cam, seed=k)
        out.append((depth, rgba, pose))
    return out
