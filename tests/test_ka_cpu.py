"""The hand-built K-A cases (tests/ka_inputs.py) on the CPU: the numpy restatement (tests/ka_ref.py) equals both oracle
kernels (scalar and AVX2) bit for bit on every case, and -- from the restatement's intermediates -- every case hits the
edge it names, with a count of at least one per edge.  tests/test_gpu_ka_edges.py then only has to compare the device
with the oracle on the same cases.

A stored NaN equals a stored NaN whatever its sign and payload, in case G only; test_no_nan_outside_g shows on the oracle
alone that no other case stores one, so that exception cannot hide anything elsewhere."""
import numpy as np
import pytest

from oracle import api as O
from tests import ka_inputs as KI
from tests import ka_ref as KR

F = np.float32
MODES = ((False, False), (True, False), (True, True))  # (colour, quality)


def oracle_volume(c, kernel=0):
    ov = O.Volume(c.res, O.camera_from(c.cam), O.Integrator(*c.ig))
    ov.set_kernel(kernel)
    for i, cid in enumerate(c.ids):
        ov.set_chunk(cid, *c.chunk(i))
    return ov


def oracle_run(c, kernel, flag, colour, quality, frames=(0,)):
    """-> (needs u8[n], quality f32[n] of the last frame, [(sdf, weight, colour)] per chunk)"""
    ov = oracle_volume(c, kernel)
    needs = np.zeros(len(c.ids), np.uint8)
    for f in frames:
        q = ov.integrate(c.depths[f], c.rgba if colour else None, c.quality if quality else None, c.poses[f], c.ids, needs, flag, -1)
    out = [ov.get_chunk(cid) for cid in c.ids]
    ov.close()
    return needs, q.copy(), out


def ref_run(c, i, flag, colour, quality, frame=0):
    s, w, col = c.chunk(i)
    return KR.voxel_update(c.depths[frame], c.rgba if colour else None, c.quality if quality else None, c.cam_tuple(), c.ig,
                           c.poses[frame], flag, c.ids[i], c.res, s, w, col)


@pytest.mark.parametrize("kernel", [0, 1], ids=["scalar", "avx2"])
@pytest.mark.parametrize("name", KI.ALL)
def test_restatement_equals_oracle(name, kernel):
    if kernel == 1:
        assert O.lib().tfo_have_avx2(), "the AVX2 row kernel is part of the comparison"
    c = KI.cases()[name]
    nan_ok = name in KI.NAN_ALLOWED
    for flag in (1, 0):
        for colour, quality in MODES:
            needs, oq, chunks = oracle_run(c, kernel, flag, colour, quality)
            for i in range(len(c.ids)):
                r = ref_run(c, i, flag, colour, quality)
                what = "%s chunk %d flag %d colour %d quality %d" % (name, i, flag, colour, quality)
                assert bool(needs[i]) == r["updated"], what
                assert KR.same_floats(chunks[i][0], r["sdf"], nan_ok), what + ": sdf"
                assert KR.same_floats(chunks[i][1], r["weight"], nan_ok), what + ": weight"
                assert np.array_equal(chunks[i][2], r["color"]), what + ": colour"
                if colour:
                    assert F(oq[i]).view(np.uint32) == r["quality"].view(np.uint32), what + ": quality sum"
        if len(c.poses) > 1:  # the depth-only group: the single-frame function applied n times
            frames = range(len(c.poses))
            needs, _, chunks = oracle_run(c, kernel, flag, False, False, frames)
            for i in range(len(c.ids)):
                s, w, _ = c.chunk(i)
                gs, gw, upd, _ = KR.depth_group(c.depths, c.cam_tuple(), c.ig, c.poses, flag, c.ids[i], c.res, s, w)
                assert bool(needs[i]) == upd
                assert KR.same_floats(chunks[i][0], gs) and KR.same_floats(chunks[i][1], gw), "%s group chunk %d flag %d" % (name, i, flag)


@pytest.mark.parametrize("name", [n for n in KI.ALL if n not in KI.NAN_ALLOWED])
def test_no_nan_outside_g(name):
    c = KI.cases()[name]
    for flag in (1, 0):
        _, q, chunks = oracle_run(c, 0, flag, True, True, range(len(c.poses)))
        assert not np.isnan(q).any()
        for s, w, _ in chunks:
            assert not np.isnan(s).any() and not np.isnan(w).any()
    g = KI.cases()["G"]
    assert any(np.isnan(s).any() for s, _, _ in oracle_run(g, 0, 1, False, False)[2]), "case G is there to store NaNs"


def _geo(name, flag=1, colour=True, quality=True, frame=0):
    c = KI.cases()[name]
    return c, [ref_run(c, i, flag, colour, quality, frame) for i in range(len(c.ids))]


def test_case_a_borders():
    c, g = _geo("A")
    g2 = _geo("A2")[1]
    for axis, n, gg in (("X", KI.W, g), ("Y", KI.H, g2)):  # (A's rows share one Y, A2's one X)
        for val in (-1, 0, 1, n - 2, n - 1, n):
            assert sum(int((x[axis][x["live"]] == val).sum()) for x in gg) >= 1, "%s == %d in a processed row" % (axis, val)
    for axis, n, gg in (("Y", KI.H, g), ("X", KI.W, g2)):  # ... and the other coordinate decides which row stalls
        for val in (-1, 0, 1, n - 2, n - 1, n):
            assert sum(int((x[axis] == val).sum()) for x in gg) >= 1, "%s == %d" % (axis, val)
    assert any(0 < x["rows"] < 64 for x in g2) and any(x["rows"] == 0 for x in g2) and any(x["valid"].all() for x in g2)
    assert any(x["rows"] == 0 and x["valid"][1:].any() for x in g), "row 0 invalid, later rows valid"
    assert any(0 < x["rows"] < 64 for x in g), "a stall in the middle"
    assert any(x["valid"].all() for x in g), "a fully valid chunk"
    for x in g:
        if x["rows"] == 0:
            assert not x["updated"] and x["quality"] == 0
    # the sentinel is assigned after rows have added and before other rows add; the additions show in the float
    hit = 0
    for x in g:
        oob_rows = np.flatnonzero(x["oob"].any(axis=1))
        add_rows = np.flatnonzero(x["upd"].any(axis=1))
        if len(oob_rows) and len(add_rows) and add_rows[0] < oob_rows[-1] < add_rows[-1]:
            assert x["quality"] != KR.QOOB and x["quality"] < F(-9e10)
            hit += 1
    assert hit >= 1


@pytest.mark.parametrize("name", ["B", "B2"])
def test_case_b_ties(name):
    c, g = _geo(name)
    k = KR.constants(c.cam_tuple(), c.res)
    if name == "B2":
        assert (k["fxi"], k["fyi"]) == (52, 51) and (k["cxs"], k["cys"]) == (31.5, 23.5) and c.cam.fx != 52 and c.cam.cx != 31
        return
    for ax, coord in (("u", "X"), ("v", "Y")):
        for parity in (0, 1):
            n = 0
            for x in g:
                t = x[ax][x["live"] & x["valid"]]
                fl = np.floor(t)
                tie = (t - fl == F(0.5)) & (fl.astype(np.int64) % 2 == parity)
                n += int(tie.sum())
                r = x[coord][x["live"] & x["valid"]][tie]
                assert np.array_equal(r, (fl[tie] + (1 if parity else 0)).astype(np.int32)), "ties go to the even integer"
            assert n >= 8, "ties at %s integers in %s" % ("odd" if parity else "even", ax)
    assert sum(int((x["pz"] == F(0.25)).sum()) for x in g) >= 64, "p.z is a power of two in slice 0"


def test_case_c_at_and_behind_the_camera():
    c, g = _geo("C1")
    x = g[0]
    assert x["px"][0, 0] == 0 and x["py"][0, 0] == 0 and x["pz"][0, 0] == 0, "a voxel centre on the camera centre"
    assert np.isnan(x["u"][0, 0]) and x["X"][0, 0] == KR.INT_MIN
    assert (x["pz"][:8] == 0).all(), "a whole slice with p.z == 0"
    assert sum(int((y["valid"] & y["live"] & (y["pz"] < 0)).sum()) for y in g) >= 1, "negative p.z that projects into the image"
    c2, g2 = _geo("C2")
    assert sum(int(((y["pz"] == 0) & y["live"]).sum()) for y in g2) >= 1, "p.z == 0 lanes in processed rows"
    assert any(y["updated"] for y in g) and any(y["updated"] for y in g2)
    x = _geo("C3")[1][0]  # one processed row whose only off-image lane is the 0 / 0 one: the sentinel hangs on its class
    assert x["rows"] == 1 and x["oob"][0].tolist() == [True] + [False] * 7 and x["pz"][0, 0] == 0 and x["px"][0, 0] == 0
    assert x["valid"][0, 1:].all() and x["upd"][0].any() and x["quality"] < F(-9e10)


def test_case_d_both_sides_of_the_guard():
    band = KI.D_BAND
    assert F(32.0) * KI.RES8 == band
    nearest = []
    for name, sign, step in (("D_eq", 1, 0), ("D_pos_above", 1, 1), ("D_pos_below", 1, -1), ("D_neg_eq", -1, 0),
                             ("D_neg_above", -1, 1), ("D_neg_below", -1, -1)):
        c, g = _geo(name)
        assert g[0]["o"][2] == F(sign) * KI.ulps(band, step), name
        assert KI.guard_safe(g[0]["o"], c.res) == (step > 0), name      # `>`: equality is outside the fast path
        assert g[0]["rows"] == 64
        sides = [KI.guard_safe(x["o"], c.res) for x in g]
        assert any(sides) and not all(sides), "neighbouring chunks on either side"
        if sign > 0:
            assert g[0]["updated"]
            assert any(x["updated"] for x, s in zip(g, sides) if s) and any(x["updated"] for x, s in zip(g, sides) if not s)
        else:
            assert sum(int((x["valid"] & x["live"] & (x["pz"] < 0)).sum()) for x in g) >= 512, "mirrored projections"
        nearest += [float(np.abs(x["pz"][x["live"]]).min()) / float(c.res) for x, s in zip(g, sides) if s and x["rows"]]
    # how close to the camera plane the fast path comes, in voxels (tests/ka_inputs.py says why not closer)
    assert min(nearest) < 25.0
    under = KI.ulps(KI.TWO20, -1)
    for ax, nm in enumerate("xyz"):
        c, g = _geo("D_%s_under" % nm)
        assert any(abs(x["o"][ax]) == under and KI.guard_safe(x["o"], c.res) for x in g), nm
        assert not any(x["updated"] for x in g)
        c, g = _geo("D_%s_over" % nm)
        assert any(abs(x["o"][ax]) == F(KI.TWO20) and not KI.guard_safe(x["o"], c.res) for x in g), nm
        assert not any(x["updated"] for x in g)


def test_case_e_thresholds():
    c, g = _geo("E")
    near, far = F(c.cam.near), F(c.cam.far)

    def at(tgt, step):
        i, k = c.named["%s%+d" % (tgt, step)]
        return g[i], k

    for step in (-1, 0, 1):
        x, k = at("near", step)
        assert x["d"].flat[k] == KI.ulps(near, step) and bool(x["F"].flat[k]) == (step > 0), "d == near: only above it"
        x, k = at("far", step)
        assert x["d"].flat[k] == KI.ulps(far, step) and bool(x["F"].flat[k]) == (step < 0)
        x, k = at("lower", step)
        assert x["sd"].flat[k] == KI.ulps(KR.LOWER, step) and bool(x["F"].flat[k]) == (step > 0)
        x, k = at("upper", step)
        assert x["sd"].flat[k] == KI.ulps(x["upper"], step) and bool(x["F"].flat[k]) == (step < 0)
        x, k = at("thr_pos", step)
        assert x["sd"].flat[k] == KI.ulps(x["thr_col"], step) and bool(x["upd"].flat[k]) == (step < 0)
        x, k = at("thr_neg", step)
        assert x["sd"].flat[k] == KI.ulps(-x["thr_col"], step) and bool(x["upd"].flat[k]) == (step > 0)
    assert len(c.named) == 18


def test_case_f_keep_threshold():
    c, g1 = _geo("F", flag=1)
    _, g0 = _geo("F", flag=0)
    half_up = KI.ulps(0.5, 1)
    for i in range(len(c.ids)):
        w = c.chunk(i)[1].reshape(64, 8)
        x1, x0 = g1[i], g0[i]
        eq = x1["F"] & (x1["nwt"] == F(0.5))
        assert eq.sum() >= 1 and (x1["weight"].reshape(64, 8)[eq] == 0).all() and (x1["sdf"].reshape(64, 8)[eq] == 999).all()
        up = x1["F"] & (x1["nwt"] == half_up)
        assert up.sum() >= 1 and (x1["weight"].reshape(64, 8)[up] == half_up).all()
        wD = -x0["wD"]
        assert (x0["F"] & (w == wD) & (x0["nwt"] == 0)).sum() >= 1, "flag 0: w == wD goes to 0"
        assert (x0["F"] & (w == 0) & ~np.signbit(w)).sum() >= 1 and (x0["F"] & (w == 0) & np.signbit(w)).sum() >= 1, "w == +0 and -0"
        just = x0["F"] & (x0["nwt"] > F(0.5)) & (w == c.named["w%d" % i][4])
        assert just.sum() >= 1 and (x0["weight"].reshape(64, 8)[just] > 0.5).all(), "flag 0: the first weight that survives"
        assert (x0["F"] & (w == c.named["w%d" % i][7]) & ~(x0["nwt"] > F(0.5))).sum() >= 1, "flag 0: w - wD == 0.5 is reset"


def test_case_g_extreme_states():
    c, g = _geo("G")
    n = dict(inf_s=0, nan_s=0, inf_w=0, nan_w=0, overflow=0, sub_s=0, sub_w=0, sub_prod=0, neg_w=0, nan_out=0, inf_out=0)
    tiny = np.finfo(F).tiny
    with np.errstate(all="ignore"):
        for i, x in enumerate(g):
            s, w, _ = c.chunk(i)
            wr = np.repeat(x["row_tsdf"], 8)
            prod = (s * w).astype(F)
            n["inf_s"] += int((wr & np.isinf(s)).sum()); n["nan_s"] += int((wr & np.isnan(s)).sum())
            n["inf_w"] += int((wr & np.isinf(w)).sum()); n["nan_w"] += int((wr & np.isnan(w)).sum())
            n["overflow"] += int((wr & np.isinf(prod) & np.isfinite(s) & np.isfinite(w)).sum())
            n["sub_s"] += int((wr & (s != 0) & (np.abs(s) < tiny)).sum()); n["sub_w"] += int((wr & (w != 0) & (np.abs(w) < tiny)).sum())
            n["sub_prod"] += int((wr & (prod != 0) & (np.abs(prod) < tiny) & (np.abs(s) >= tiny) & (np.abs(w) >= tiny)).sum())
            n["neg_w"] += int((wr & (w < 0) & np.isfinite(w)).sum())
            n["nan_out"] += int(np.isnan(x["sdf"]).sum()); n["inf_out"] += int(np.isinf(x["sdf"]).sum() + np.isinf(x["weight"]).sum())
    assert all(v >= 1 for v in n.values()), n


def test_case_h_packed_colour():
    c, g1 = _geo("H", flag=1)
    _, g0 = _geo("H", flag=0)
    pix = c.rgba.reshape(-1, 4)
    carry = borrow = 0
    seen = set()
    lazy200 = untouched = 0
    for i in range(len(c.ids)):
        col = c.chunk(i)[2].reshape(64, 8, 4).astype(np.int64)
        x = g1[i]
        upd = x["upd"]
        assert np.array_equal(upd, g0[i]["upd"])
        assert (pix[x["idx"][upd]][:, :3] == 255).all()
        for lo, hi in ((0, 1), (2, 3)):  # the two dwords {r, g} and {b, count}
            inp = np.where(upd, pix[x["idx"]][..., lo], 0)
            carry += int((upd & (col[..., lo] + inp > 65535) & (col[..., hi] != 0)).sum())
            borrow += int((upd & (col[..., lo] - inp < 0) & (col[..., hi] != 0)).sum())
        alpha = pix[x["idx"]][..., 3]
        for cnt, a in zip(col[..., 3][upd], alpha[upd]):
            seen.add((int(cnt), int(a)))
        rc = np.repeat(x["row_color"][:, None], 8, axis=1)
        lazy200 += int((rc & ~upd & (col[..., 3] == 200)).sum())
        dead = ~x["row_color"]
        untouched += int(dead.sum())
        for gg in (x, g0[i]):
            assert np.array_equal(gg["color"].reshape(64, 8, 4)[dead], c.chunk(i)[2].reshape(64, 8, 4)[dead])
        out = x["color"].reshape(64, 8, 4)
        assert (out[..., 3][rc & ~upd & (col[..., 3] == 200)] == 50).all(), "a count above 120 is halved in a lane that is not updated"
    assert carry >= 1 and borrow >= 1, "a low half that wraps next to a non-zero high half, adding and subtracting"
    for cnt in (119, 120, 121):
        for a in (0, 1, 255):
            assert (cnt, a) in seen, (cnt, a)
    assert any(k[0] == 0x8000 for k in seen) and any(k[0] == 0xFFFF for k in seen)
    assert lazy200 >= 1 and untouched >= 1


def _quality_in_order(c, x, lanes, tree=False):
    q = c.quality.reshape(-1)
    total = F(0)
    for r in range(x["rows"]):
        if x["oob"][r].any():
            total = KR.QOOB
        if not x["upd"][r].any():
            continue
        v = [q[x["idx"][r, l]] if x["upd"][r, l] else F(0) for l in lanes]
        if tree:
            s = F(F(F(v[0] + v[1]) + F(v[2] + v[3])) + F(F(v[4] + v[5]) + F(v[6] + v[7])))
        else:
            s = F(0)
            for t in v:
                s = F(s + t)
        total = F(total + s)
    return total


def test_case_i_quality_order():
    c, g = _geo("I")
    differs = dict(reversed=0, tree=0, rows_first=0)
    sentinel_mid = 0
    for x in g:
        if not x["upd"].any():
            continue
        assert _quality_in_order(c, x, range(8)).view(np.uint32) == x["quality"].view(np.uint32)
        differs["reversed"] += int(_quality_in_order(c, x, range(7, -1, -1)) != x["quality"])
        differs["tree"] += int(_quality_in_order(c, x, range(8), tree=True) != x["quality"])
        # one running sum over every lane of every row, instead of a sum per row added to the total
        q = c.quality.reshape(-1)
        flat = F(0)
        for r in range(x["rows"]):
            if x["oob"][r].any():
                flat = KR.QOOB
            for l in range(8):
                if x["upd"][r, l]:
                    flat = F(flat + q[x["idx"][r, l]])
        differs["rows_first"] += int(flat != x["quality"])
        oob_rows, add_rows = np.flatnonzero(x["oob"].any(axis=1)), np.flatnonzero(x["upd"].any(axis=1))
        if len(oob_rows) and add_rows[0] < oob_rows[-1] < add_rows[-1] and x["quality"] != KR.QOOB:
            sentinel_mid += 1
    assert all(v >= 1 for v in differs.values()), differs
    assert sentinel_mid >= 1


def test_case_j_groups():
    cs = KI.cases()
    assert [len(cs[n].poses) for n in KI.GROUPS] == [1, 2, 6]
    c = cs["J6"]
    rows = np.array([[ref_run(c, i, 1, False, False, f)["rows"] for f in range(6)] for i in range(len(c.ids))])
    assert sum(len(set(r)) > 1 for r in rows) >= 2, "the frames stall at different rows: %s" % rows.tolist()
    assert ((rows > 0) & (rows < 64)).any() and (rows == 0).any() and (rows == 64).any()
    s, w, _ = c.chunk(0)
    _, _, _, per = KR.depth_group(c.depths, c.cam_tuple(), c.ig, c.poses, 1, c.ids[0], c.res, s, w)
    reset_then_rebuilt = (w != 0) & (per[0]["weight"] == 0) & (per[1]["weight"] > 0.5)
    assert reset_then_rebuilt.sum() >= 1
    _, _, _, per0 = KR.depth_group(c.depths, c.cam_tuple(), c.ig, c.poses, 0, c.ids[0], c.res, s, w)
    assert ((w > 0.5) & (per0[0]["weight"] == 0)).sum() >= 1, "flag 0: a weight taken below the threshold"


def test_fused_selection_finds_the_preset_chunks():
    """tests/test_gpu_ka_edges.py runs E - H through the fused frame: the oracle's selection must reach the preset chunks"""
    for name, least in (("E", 8), ("F", 3), ("G", 3), ("H", 3)):
        c = KI.cases()[name]
        ov = oracle_volume(c)
        ov.integrate_frame(c.depths[0], c.rgba, c.poses[0])
        changed = 0
        for i, cid in enumerate(c.ids):
            s, w, col = ov.get_chunk(cid)
            s0, w0, c0 = c.chunk(i)
            changed += int(not (KR.same_floats(s, s0, True) and KR.same_floats(w, w0, True)))
        ov.close()
        assert changed >= least, (name, changed)
