"""Chisel::CompensateColor with nothing crossing to the host (tf_compensate_color_device, texturefusion_amd/csrc/tf_cc.hip)
and the keyframe tail that enqueues it (TF_TAIL_COMPENSATE_COLOR): against the oracle, against the host-solved path
tf_compensate_color, against itself (two runs give the same bits), at its edges (no patch, one cluster, a cluster that
learns nothing, more clusters than a wave has lanes), in front of DrawMeshes and behind the tail.

Tolerance: TOL of tests/test_gpu_atlas.py (2e-5 absolute on labs in [0, 1], stated in tests/test_color_compensate.py) --
the bound tf_compensate_color is held to; the device path sums in f64 in chunk order where the oracle sums in f32 in
order and the host path in f32 trees, the solve is the same f64 text.  Flags, frame ids and counts are exact."""
import functools

import numpy as np
import pytest

from oracle import api as O
from texturefusion_amd import capi, synth
from tests import texmap_inputs as I
from tests.cc_ref import labs_exact_sums
from tests.test_gpu_atlas import TOL, _cache, _compare_patches, _integrate, _keyframe
from tests.util import RES5, make_pair

pytestmark = pytest.mark.gpu
ADJ, WRONG, HAS = 16, 4, 1


@functools.lru_cache(maxsize=1)
def _wall():
    """the scene of test_compensate_color_and_draw_meshes: six wall frames at 1.2 m; keyframes 2, 5 (darkened) and 7 (depth
    pushed back: every patch maps wrongly)"""
    cam = synth.Camera()
    frames = []
    for k in range(6):
        d, rgba, q, pose = synth.wall_frame(1.2, cam, seed=k)
        rgba = synth._hash_colour(np.stack(np.meshgrid(np.arange(cam.width) * 0.01, np.arange(cam.height) * 0.01), -1)[..., [0, 1, 1]], 5)
        frames.append((d, rgba, pose))
    dark = (frames[1][0], (frames[1][1].astype(np.float32) * 0.7).astype(np.uint8), frames[1][2])
    far = (np.where(frames[2][0] > 0, frames[2][0] + 1.0, 0).astype(np.float32), frames[2][1], frames[2][2])  # depth test fails
    kfs = {2: _keyframe(frames[0]), 5: _keyframe(dark), 7: _keyframe(far)}
    return cam, frames, kfs


def _labels3(n):
    return np.array([(2, 5, 7)[i % 3] for i in range(n)], np.int32)


def _gpu_scene(labels_of=_labels3, **kw):
    """the scene on a device volume alone, behind GeneratePatches + UpdateAtlas"""
    cam, frames, kfs = _wall()
    gv = capi.Volume(RES5, cam, max_chunks=1 << 15, **kw)
    for depth, rgba, pose in frames:
        gv.frame_upload(depth, rgba, None)
        gv.integrate_frame(pose, True)
    gv.update_meshes()
    ids = gv.compress_meshes()
    _cache(gv, kfs)
    gv.generate_patches(ids, labels_of(len(ids)))
    gv.update_atlas(ids)
    return gv, ids


def _against_exact_sums(gv, ids, before, after, what):
    """labs the device wrote between two downloads against tests/cc_ref.py fed the device's own patches and mesh colours;
    returns the largest difference"""
    voff, ioff, V, N, Cc, I_, adj, simp = gv.get_meshes(ids)
    assert np.array_equal(voff, before["voff"])
    has = (before["flags"] & HAS) > 0
    want, adj = labs_exact_sums(before["frameid"], (before["flags"] & WRONG) > 0, ((before["flags"] & ADJ) > 0) | ~has,
                                voff, before["texcolor"], Cc)
    assert np.array_equal(adj[has], (after["flags"][has] & ADJ) > 0), what
    wrote = ~np.isnan(want)
    assert wrote.any(), what
    err = float(np.abs(after["labs"][wrote] - want[wrote]).max())
    print("%s: device labs vs exact-sum restatement, max abs %.3g over %d values" % (what, err, wrote.sum()))
    assert err <= TOL, what
    return err


def _unadjusted(g):
    return int(((g["flags"] & HAS) > 0).sum() - ((g["flags"] & ADJ) > 0).sum())


def test_three_clusters_against_the_oracle(gpu_required):
    cam, frames, kfs = _wall()
    ov, gv, cam, ig = make_pair(RES5, cam, max_chunks=1 << 15)
    ids = _integrate(ov, gv, frames)
    oa = O.Atlas(RES5)
    _cache(gv, kfs)
    labels = _labels3(len(ids))
    ov.generate_patches(oa, ids, labels, kfs)
    gv.generate_patches(ids, labels)
    g = gv.get_patches(ids)
    assert _unadjusted(g) > 256, "the list and rank kernels were meant to span several workgroups"
    assert (g["flags"] & WRONG).any() and not (g["flags"] & WRONG).all()
    assert ov.compensate_color() == 3
    assert gv.compensate_color_device() == 3
    g1 = _compare_patches(ov, gv, ids, "after the device CompensateColor", labs=True)
    assert (g1["flags"] & ADJ).any()
    _against_exact_sums(gv, ids, g, g1, "three clusters")
    # a second call finds the cluster of the "far" keyframe only (nothing was learnt: has_adjusted stayed clear) and
    # touches no labs
    assert ov.compensate_color() == 1
    assert gv.compensate_color_device() == 1
    g2 = gv.get_patches(ids)
    assert np.array_equal(g2["flags"], g1["flags"])
    assert np.array_equal(g2["labs"].view(np.uint32), g1["labs"].view(np.uint32))
    gv.close()


def test_against_the_host_path(gpu_required):
    ga, ids = _gpu_scene()
    gb, ids_b = _gpu_scene()
    assert np.array_equal(ids, ids_b)
    assert ga.compensate_color() == 3
    assert gb.compensate_color_device() == 3
    a, b = ga.get_patches(ids), gb.get_patches(ids)
    assert np.array_equal(a["flags"], b["flags"]) and np.array_equal(a["frameid"], b["frameid"])
    learnt = np.repeat(((a["flags"] & ADJ) > 0) & ((a["flags"] & WRONG) == 0), np.diff(a["voff"]))
    assert learnt.sum() > 1000
    err = np.abs(a["labs"][learnt] - b["labs"][learnt]).max()
    print("device path vs host path: max |labs| difference %.3g over %d vertices" % (err, learnt.sum()))
    assert err <= TOL
    ga.close()
    gb.close()


def test_two_runs_give_the_same_bits(gpu_required):
    out = []
    for _ in range(2):
        gv, ids = _gpu_scene()
        assert gv.compensate_color_device() == 3
        g = gv.get_patches(ids)
        out.append((ids.copy(), g["flags"].copy(), g["labs"].view(np.uint32).copy()))
        gv.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert (out[0][1] & ADJ).any()
    assert np.array_equal(out[0][2], out[1][2])


def test_edges_no_patch_one_cluster_all_wrong(gpu_required):
    cam, frames, kfs = _wall()
    fresh = capi.Volume(RES5, cam, max_chunks=1 << 12)
    assert fresh.compensate_color_device() == 0  # nothing integrated at all
    fresh.close()
    ov, gv, cam, ig = make_pair(RES5, cam, max_chunks=1 << 15)
    ids = _integrate(ov, gv, frames)
    assert gv.compensate_color_device() == 0  # meshes, no patch
    oa = O.Atlas(RES5)
    _cache(gv, kfs)
    # one cluster: every label names keyframe 5
    labels = np.full(len(ids), 5, np.int32)
    ov.generate_patches(oa, ids, labels, kfs)
    gv.generate_patches(ids, labels)
    before = gv.get_patches(ids)
    assert ov.compensate_color() == 1
    assert gv.compensate_color_device() == 1
    # flags and everything integer against the oracle; labs against the reference's statements with exact sums
    # (tests/cc_ref.py): one cluster holds all 74 936 vertices of the scene, and over that many the oracle's own f32
    # in-order sums are 3.8e-5 from the exact evaluation -- outside TOL by themselves (figures in tests/cc_ref.py)
    g = _compare_patches(ov, gv, ids, "one cluster")
    _against_exact_sums(gv, ids, before, g, "one cluster")
    has = (g["flags"] & HAS) > 0
    assert has.any() and ((g["flags"][has] & ADJ) > 0).all()
    assert gv.compensate_color_device() == 0  # everything is adjusted now
    # a cluster that is entirely wrongly mapped: counted, has_adjusted clear, labs untouched
    labels = np.full(len(ids), 7, np.int32)
    ov.generate_patches(oa, ids, labels, kfs)
    gv.generate_patches(ids, labels)
    before = gv.get_patches(ids)
    has = (before["flags"] & HAS) > 0
    assert has.any() and ((before["flags"][has] & WRONG) > 0).all()
    assert ov.compensate_color() == 1
    assert gv.compensate_color_device() == 1
    after = _compare_patches(ov, gv, ids, "all wrong")
    assert ((after["flags"] & ADJ) == 0).all()
    assert np.array_equal(after["flags"], before["flags"])
    assert np.array_equal(after["labs"].view(np.uint32), before["labs"].view(np.uint32))
    assert gv.compensate_color_device() == 1  # ... and again: the cluster stays unadjusted
    gv.close()


def test_65_clusters(gpu_required):
    """one more cluster than a wave has lanes: 65 cached keyframes, scaled copies of one frame, labels i % 65"""
    cam, frames, _ = _wall()
    ov, gv, cam, ig = make_pair(RES5, cam, max_chunks=1 << 15, max_keyframes=80)
    ids = _integrate(ov, gv, frames)
    oa = O.Atlas(RES5)
    rgb, depth, T = _keyframe(frames[0])
    kfs = {100 + k: (np.ascontiguousarray((rgb.astype(np.float32) * (0.5 + 0.5 * k / 64.0)).astype(np.uint8)), depth, T) for k in range(65)}
    _cache(gv, kfs)
    labels = (100 + np.arange(len(ids)) % 65).astype(np.int32)
    ov.generate_patches(oa, ids, labels, kfs)
    gv.generate_patches(ids, labels)
    # every cluster keeps at least two vertices: the reference's N - 1 divisor stays non-zero
    nvert = {}
    for cid in ids:
        o = ov.get_patch(cid)
        if (o["flags"] & HAS) and not (o["flags"] & WRONG):
            nvert[o["frameid"]] = nvert.get(o["frameid"], 0) + len(o["texcoord"])
    assert len(nvert) == 65 and min(nvert.values()) >= 2, sorted(nvert.values())[:3]
    assert ov.compensate_color() == 65
    assert gv.compensate_color_device() == 65
    g = _compare_patches(ov, gv, ids, "65 clusters", labs=True)
    has = (g["flags"] & HAS) > 0
    assert ((g["flags"][has] & ADJ) > 0).all()
    gv.close()


def test_draw_meshes_behind_the_device_path(gpu_required):
    gv, ids = _gpu_scene()
    assert gv.compensate_color_device() == 3
    gV, gI = gv.draw_meshes()
    assert len(gI) > 0
    voff, ioff, V, N, Cc, I_, adj, simp = gv.get_meshes(ids)
    p = gv.get_patches(ids)
    complete = ((np.diff(voff) > 0) & (simp > 0) & ((p["flags"] & 8) > 0) & (p["frameid"] >= 0)).astype(np.uint8)
    wrong = ((p["flags"] & WRONG) > 0).astype(np.uint8)
    labs_valid = (((p["flags"] & ADJ) > 0) & (wrong == 0)).astype(np.uint8)
    assert labs_valid.any()
    rV, rI = O.pack_vertices(complete, wrong, labs_valid, p["texloc"], p["ratio"], 13824, 13824, voff, V, Cc, N,
                             p["texcoord"], p["texcolor"], p["labs"], ioff, I_)
    assert np.array_equal(rV.view(np.uint32), gV.view(np.uint32)) and np.array_equal(rI, gI)
    assert (gV[:, 5] != 0).any()  # the colour deltas of the compensated patches are in the stream
    gv.close()


def _tail_plan(in_tail):
    """keyframes 4, 7, 9 and 12 (keyframe 4 moved) of tests/texmap_inputs.py through the one-call tail: CompensateColor
    either inside it (TF_TAIL_COMPENSATE_COLOR) or as tf_compensate_color behind it.  Returns per step (ids, patches, hot
    atlas rows, flags of the step's patches right behind the tail)."""
    gv = capi.Volume(I.RES8, I.CAM, max_chunks=1 << 15)
    if in_tail:
        plain = gv.texture_tail
        gv.texture_tail = lambda *a, **kw: plain(*a, compensate_color=True, **kw)
    run = I.Run(gv, unit=True, tail=True, extra=False)
    out = []
    try:
        for i in range(4):
            o = run.step(i)
            behind = gv.get_patches(o["ids"])["flags"].copy()
            if not in_tail:
                gv.compensate_color()
            labels, hot = run.patches(o["ids"])
            w = run.oa.buffer().shape[1]
            g = gv.get_patches(o["ids"])
            out.append((o["ids"], g, gv.atlas_rows(hot[0] // w, hot[1] // w, w), behind))
        # an unknown flag is refused and the handle keeps working
        rc = gv.L.tf_texture_tail_device(gv.h, I.STEPS[3][0], None, 0, 16, 0)
        assert rc == capi.TF_ERR_INVALID
        gv.sync()
        assert len(gv.get_patches(out[-1][0])["flags"]) == len(out[-1][0])
    finally:
        run.close()
        gv.close()
    return out


def test_tail_with_compensation(gpu_required):
    a, b = _tail_plan(True), _tail_plan(False)
    n_adjusted = 0
    for step, ((ia, ga, ra, fa), (ib, gb, rb, fb)) in enumerate(zip(a, b)):
        assert np.array_equal(ia, ib) and len(ia) > 0
        # a tail without the flag leaves has_adjusted clear on the patches it generated; with it, not
        has = (fb & HAS) > 0
        assert has.any() and ((fb[has] & ADJ) == 0).all(), step
        assert ((fa[has] & ADJ) > 0).any(), step
        assert np.array_equal(ga["flags"], gb["flags"]) and np.array_equal(ga["frameid"], gb["frameid"]), step
        assert np.array_equal(ga["voff"], gb["voff"])
        learnt = np.repeat(((ga["flags"] & ADJ) > 0) & ((ga["flags"] & WRONG) == 0), np.diff(ga["voff"]))
        n_adjusted += int(learnt.sum())
        if learnt.any():
            assert np.abs(ga["labs"][learnt] - gb["labs"][learnt]).max() <= TOL, step
        assert np.array_equal(ra, rb), "hot atlas rows of step %d" % step
    assert n_adjusted > 1000
