"""Relocalisation on the MI355X (tf_reloc.hip): descriptors of cached keyframes and of host frames against the restatement bit
for bit (both pixel strides, 4 x 4 and 1 x 1 blocks, every kind of bad depth, the half-valid threshold), scores and ranking
bit for bit (5 keyframes, 65 with ties, a query of holes, an empty index), the index's calls, tf_relocalise found and not
found, invalid arguments, the read-only guarantee and the C++ mirror.  Everything runs on the hand-built corner at 160 x 120
or smaller; the scene is tests/reloc_inputs.py's, checked without a GPU by tests/test_reloc_cpu.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import align_inputs as I
from tests import align_ref as R
from tests import reloc_inputs as QI
from tests import reloc_ref as Q
from tests.util import HipBuffer, sorted_ids
from texturefusion_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (I.CAM.height, I.CAM.width)
KF0, FAR0 = 10, 20  # ids of the scene's keyframes and of the far ones
f32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))


@pytest.fixture(scope="module")
def frames():
    """{kf_id: (depth, rgb, pose)} of the scene's keyframes and the far ones: rendered once, shared, left unchanged"""
    out = {KF0 + k: QI.frame(p) + (p,) for k, p in enumerate(QI.keyframe_poses())}
    out.update({FAR0 + k: QI.frame(p) + (p,) for k, p in enumerate(QI.far_poses())})
    return out


@pytest.fixture(scope="module")
def hand(gpu_required, frames):
    """the hand-built corner, uploaded chunk by chunk, and every keyframe cached with its pose"""
    gv = capi.Volume(I.HAND_RES, I.CAM, max_chunks=1 << 10, max_keyframes=96)
    ids, s, w, c = I.hand_corner()
    for k in range(len(ids)):
        gv.set_chunk(ids[k], s[k], w[k], c[k])
    for kf_id, (depth, rgb, pose) in frames.items():
        gv.keyframe_cache(kf_id, rgb, depth, QI.pose_inv16(pose))
    gv.sync()
    yield gv
    gv.close()


@pytest.fixture(scope="module")
def rows(frames):
    p = Q.params()
    return p, {kf_id: Q.describe(f[0], f[1], p) for kf_id, f in frames.items()}


def _same(got, want):
    assert got[0].dtype == np.uint32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def _same_ranking(got, want):
    assert got["n"] == len(want) == len(got["kf_ids"])
    assert list(got["kf_ids"]) == [w[0] for w in want]
    assert got["scores"].tobytes() == b"".join(struct.pack("<d", w[1]) for w in want)
    assert list(got["overlap"]) == [w[2] for w in want]


def _bad_depths(depth, seed):
    """the frame with every kind of bad depth sprinkled in, block 0 exactly half valid and block 1 one pixel short of it"""
    rng = np.random.default_rng(seed)
    d = depth.copy()
    for val in (np.nan, np.inf, -np.inf, 0.0, 7.0, -1.0, 0.04, 0.05, 5.0):
        d[rng.random(d.shape) < 0.03] = val
    d[0:4, 0:8] = 1.0
    d[2:4, 0:4] = np.nan   # block 0: 8 of 16
    d[2:4, 4:8] = np.nan
    d[1, 7] = -np.inf      # block 1: 7 of 16
    return d


# ---- 1. descriptors -------------------------------------------------------------------------------------------------------
def test_keyframe_rows_equal_the_restatement(hand, frames, rows):
    gv = hand
    p, want = rows
    gv.reloc_configure()
    gv.reloc_index_add(sorted(frames))
    assert gv.reloc_index_count() == len(frames)
    for kf_id in frames:
        _same(gv.reloc_descriptor(kf_id), want[kf_id])


@pytest.mark.parametrize("stride", [3, 4])
def test_host_frame_descriptors_equal_the_restatement(hand, stride):
    gv = hand
    p = Q.params()
    gv.reloc_configure()
    depth, rgb = QI.frame(QI.query_pose(1, 1))
    bad = _bad_depths(depth, 3)
    want = Q.describe(bad, rgb, p)
    assert want[1][0] == 1000 and want[1][1] == -1 and (want[1] < 0).sum() > 20 and (want[1] >= 0).sum() > 600
    image = rgb if stride == 3 else QI.rgba(rgb, 77)
    _same(gv.reloc_describe(bad, image), want)
    _same(gv.reloc_describe(depth, image), Q.describe(depth, rgb, p))
    # the same through the keyframe table: a caller-owned device image of that stride
    bufs = [HipBuffer(image.nbytes).from_host(image), HipBuffer(bad.nbytes).from_host(bad)]
    try:
        gv.keyframe_cache_device(50 + stride, bufs[0].ptr, bufs[1].ptr, stride, QI.pose_inv16(QI.query_pose(1, 1)))
        gv.reloc_index_add([50 + stride])
        _same(gv.reloc_descriptor(50 + stride), want)
        gv.reloc_index_remove([50 + stride])
        gv.keyframe_release(50 + stride)
    finally:
        for b in bufs:
            b.free()
    # another grid and range: 8 x 12 blocks of 20 x 10 pixels
    p2 = Q.params(tiny_w=8, tiny_h=12, min_depth=0.2, max_depth=0.45, min_overlap=10)
    gv.reloc_configure(capi.RelocParams(tiny_w=8, tiny_h=12, min_depth=0.2, max_depth=0.45, min_overlap=10))
    want2 = Q.describe(bad, rgb, p2)
    assert (want2[1] >= 0).sum() > 10 and (want2[1] < 0).sum() > 10
    _same(gv.reloc_describe(bad, image), want2)


def test_one_pixel_blocks_on_a_40_x_30_camera(gpu_required):
    cam = synth.Camera(40, 30, 33.0, 33.0, 19.5, 14.5)
    gv = capi.Volume(I.HAND_RES, cam, max_chunks=1 << 10)
    try:
        with pytest.raises(capi.TFError) as e:  # a grid that does not divide the camera
            gv.reloc_configure(capi.RelocParams(tiny_w=7, tiny_h=30))
        assert e.value.code == capi.TF_ERR_INVALID
        with pytest.raises(capi.TFError):
            gv.reloc_index_count()  # nothing was configured
        p = Q.params(min_overlap=100)
        gv.reloc_configure(capi.RelocParams(min_overlap=100))
        rng = np.random.default_rng(11)
        kf = {}
        for kf_id in (1, 2, 3):
            depth = _bad_depths(rng.uniform(0.04, 5.2, (30, 40)).astype(np.float32), kf_id)
            rgb = rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)
            kf[kf_id] = Q.describe(depth, rgb, p)
            gv.keyframe_cache(kf_id, rgb, depth, np.eye(4, dtype=np.float32))
        gv.reloc_index_add([3, 1, 2])
        for kf_id, want in kf.items():
            _same(gv.reloc_descriptor(kf_id), want)
        depth = _bad_depths(rng.uniform(0.04, 5.2, (30, 40)).astype(np.float32), 9)
        rgb = rng.integers(0, 256, (30, 40, 4), dtype=np.uint8)
        q = Q.describe(depth, rgb, p)
        _same(gv.reloc_describe(depth, rgb), q)
        want = Q.rank(q, kf, p, (30, 40))
        assert len(want) == 3
        _same_ranking(gv.reloc_query(depth, rgb), want)
        gv.set_camera(synth.Camera(48, 30, 33.0, 33.0, 19.5, 14.5))  # the configuration was another camera's
        with pytest.raises(capi.TFError) as e:
            gv.reloc_index_add([1])
        assert e.value.code == capi.TF_ERR_INVALID
    finally:
        gv.close()


# ---- 2. scores and ranking ------------------------------------------------------------------------------------------------
def test_ranking_of_five_keyframes_equals_the_restatement(hand, frames, rows):
    gv = hand
    p, want = rows
    five = {k: v for k, v in want.items() if k < FAR0}
    gv.reloc_configure()
    gv.reloc_index_add(sorted(five, reverse=True))
    for k, rung in ((0, 0), (2, 1), (4, 1)):
        depth, rgb = QI.frame(QI.query_pose(k, rung))
        ranked = Q.rank(Q.describe(depth, rgb, p), five, p, SHAPE)
        assert ranked[0][0] == KF0 + k and len(ranked) == 5
        got = gv.reloc_query(depth, rgb)
        _same_ranking(got, ranked)
        short = gv.reloc_query(depth, QI.rgba(rgb), cap=2)  # fewer than there are: the best two, n says how many there are
        assert short["n"] == 5 and list(short["kf_ids"]) == [r[0] for r in ranked[:2]]
        bufs = [HipBuffer(depth.nbytes).from_host(depth), HipBuffer(rgb.nbytes).from_host(rgb)]
        try:
            _same_ranking(gv.reloc_query_device(bufs[0].ptr, bufs[1].ptr, 3), ranked)
        finally:
            for b in bufs:
                b.free()


def test_ranking_of_65_keyframes_with_ties_and_a_query_of_holes(hand, frames, rows):
    gv = hand
    p, want = rows
    gv.reloc_configure()
    dup = {}
    bufs = []
    try:
        for k in range(5):  # the five keyframes' images on the device, each cached under 13 ids
            depth, rgb, pose = frames[KF0 + k]
            image = QI.rgba(rgb)
            bufs += [HipBuffer(image.nbytes).from_host(image), HipBuffer(depth.nbytes).from_host(depth)]
            for c in range(13):
                kf_id = 100 + 5 * c + k
                gv.keyframe_cache_device(kf_id, bufs[-2].ptr, bufs[-1].ptr, 4, QI.pose_inv16(pose))
                dup[kf_id] = want[KF0 + k]
        gv.reloc_index_add(sorted(dup, reverse=True))
        assert gv.reloc_index_count() == 65
        depth, rgb = QI.frame(QI.query_pose(3, 1))
        ranked = Q.rank(Q.describe(depth, rgb, p), dup, p, SHAPE)
        assert len(ranked) == 65 and [r[0] for r in ranked[:13]] == [100 + 5 * c + 3 for c in range(13)]
        _same_ranking(gv.reloc_query(depth, rgb), ranked)
        # all holes: no block of the query is valid, every score is +inf, nobody is a candidate
        holes = np.zeros_like(depth)
        assert Q.rank(Q.describe(holes, rgb, p), dup, p, SHAPE) == []
        got = gv.reloc_query(holes, rgb)
        assert got["n"] == 0 and len(got["kf_ids"]) == 0
        res = gv.relocalise(holes, rgb)
        assert res["status"] == capi.TF_RELOC_NO_CANDIDATE and res["n_tried"] == 0 and res["kf_id"] == -1 and res["rank"] == -1
        assert not res["pose"].any()
        # an empty index
        gv.reloc_index_clear()
        assert gv.reloc_index_count() == 0 and gv.reloc_query(depth, rgb)["n"] == 0
        assert gv.relocalise(depth, rgb)["status"] == capi.TF_RELOC_NO_CANDIDATE
    finally:
        gv.reloc_index_clear()
        for kf_id in dup:
            gv.keyframe_release(kf_id)
        for b in bufs:
            b.free()


# ---- 3. the index ---------------------------------------------------------------------------------------------------------
def test_index_calls(hand, frames, rows):
    gv = hand
    p, want = rows
    gv.reloc_configure()
    gv.reloc_index_add([KF0, KF0 + 1, KF0 + 2, KF0 + 1])  # named twice: one row
    assert gv.reloc_index_count() == 3
    depth, rgb = QI.frame(QI.query_pose(1, 0))
    q = Q.describe(depth, rgb, p)
    three = {k: want[k] for k in (KF0, KF0 + 1, KF0 + 2)}
    _same_ranking(gv.reloc_query(depth, rgb), Q.rank(q, three, p, SHAPE))
    # an id that is not cached: refused, the index as it was
    with pytest.raises(capi.TFError) as e:
        gv.reloc_index_add([KF0 + 3, 999])
    assert e.value.code == capi.TF_ERR_INVALID and gv.reloc_index_count() == 3
    with pytest.raises(capi.TFError):
        gv.reloc_descriptor(KF0 + 3)
    _same_ranking(gv.reloc_query(depth, rgb), Q.rank(q, three, p, SHAPE))
    # a keyframe cached again keeps its row until it is added again, then the row is replaced
    other = frames[KF0 + 4]
    gv.keyframe_cache(KF0 + 1, other[1], other[0])
    _same(gv.reloc_descriptor(KF0 + 1), want[KF0 + 1])
    gv.reloc_index_add([KF0 + 1])
    assert gv.reloc_index_count() == 3
    _same(gv.reloc_descriptor(KF0 + 1), want[KF0 + 4])
    three[KF0 + 1] = want[KF0 + 4]
    _same_ranking(gv.reloc_query(depth, rgb), Q.rank(q, three, p, SHAPE))
    gv.keyframe_cache(KF0 + 1, frames[KF0 + 1][1], frames[KF0 + 1][0])  # as the fixture left it
    gv.reloc_index_add([KF0 + 1])
    three[KF0 + 1] = want[KF0 + 1]
    # remove: the first row goes, the last one moves into its place
    gv.reloc_index_remove([KF0, 12345])
    assert gv.reloc_index_count() == 2
    del three[KF0]
    _same_ranking(gv.reloc_query(depth, rgb), Q.rank(q, three, p, SHAPE))
    _same(gv.reloc_descriptor(KF0 + 2), want[KF0 + 2])
    # a keyframe without a pose, and one released since, are passed over by a query
    gv.keyframe_cache(60, frames[KF0][1], frames[KF0][0])
    gv.keyframe_cache(61, frames[KF0 + 3][1], frames[KF0 + 3][0], QI.pose_inv16(frames[KF0 + 3][2]))
    gv.reloc_index_add([60, 61])
    assert gv.reloc_index_count() == 4
    three[61] = want[KF0 + 3]
    _same_ranking(gv.reloc_query(depth, rgb), Q.rank(q, three, p, SHAPE))
    gv.keyframe_set_pose(60, QI.pose_inv16(frames[KF0][2]))
    three[60] = want[KF0]
    _same_ranking(gv.reloc_query(depth, rgb), Q.rank(q, three, p, SHAPE))
    gv.keyframe_release(61)
    del three[61]
    assert gv.reloc_index_count() == 4
    _same_ranking(gv.reloc_query(depth, rgb), Q.rank(q, three, p, SHAPE))
    gv.keyframe_release(60)
    gv.reloc_index_clear()
    assert gv.reloc_index_count() == 0


# ---- 4. tf_relocalise -----------------------------------------------------------------------------------------------------
def _snapshot(gv):
    ids = sorted_ids(gv.list_chunks())
    s, w, c = gv.get_chunks(ids)
    return (bytes(gv.stats()), sorted_ids(gv.dirty()).tobytes(), ids.tobytes(), s.tobytes(), w.tobytes(), c.tobytes(),
            gv.check_summaries(), gv.check_neighbours().tobytes(), gv.model_stream_stats())


def test_relocalise_finds_the_pose_from_no_pose_at_all(hand, frames, rows):
    gv = hand
    p, want = rows
    j = 3
    truth = QI.query_pose(j, 1)  # the 80 mm / 5 deg rung off keyframe j
    depth, rgb = QI.frame(truth)
    sp = capi.AlignParams(**I.SCENE_PARAMS)
    before = _snapshot(gv)
    gv.reloc_configure()
    gv.reloc_index_add(sorted(frames))  # the far keyframes too
    rows_before = [gv.reloc_descriptor(k) for k in sorted(frames)]
    res = gv.relocalise(depth, rgb, capi.RelocaliseParams(sdf=sp))
    ranked = Q.rank(Q.describe(depth, rgb, p), want, p, SHAPE)
    fixed = gv.align_frame(depth, truth, sp)  # the SDF stage owns the fixed point
    dt, dr = R.pose_distance(res["pose"], fixed["pose"])
    print("relocalise: status %d, keyframe %d at rank %d, %d tried, score %.1f; %.3g m and %.3g rad from tf_align_frame's end from the "
          "true pose, %.3g m from the true pose" % (res["status"], res["kf_id"], res["rank"], res["n_tried"], res["tries"][0]["score"],
                                                    dt, dr, R.pose_distance(res["pose"], truth)[0]))
    assert res["status"] == capi.TF_RELOC_FOUND and res["kf_id"] == KF0 + j and res["rank"] == 0 and res["n_tried"] == 1
    t = res["tries"][0]
    assert (t["kf_id"], t["overlap"]) == (ranked[0][0], ranked[0][2]) and struct.pack("<d", t["score"]) == struct.pack("<d", ranked[0][1])
    assert t["track"]["stage"] == 2 and np.array_equal(res["pose"], t["track"]["pose"])
    assert dt <= I.FIXED_TOL_T and dr <= I.FIXED_TOL_R
    # the try is tf_track_frame from the keyframe's pose, bit for bit
    pose_k = QI.rigid_inverse(QI.pose_inv16(frames[KF0 + j][2]))
    direct = capi.TrackResult()
    assert gv.L.tf_track_frame(gv.h, f32p(depth), f32p(np.ascontiguousarray(pose_k)), C.byref(capi.AlignIcpParams()), C.byref(sp),
                               C.byref(direct)) == capi.TF_OK
    assert t["raw"] == bytes(direct)
    # with a pixel stride of 4, and again: the same answer
    again = gv.relocalise(depth, QI.rgba(rgb), capi.RelocaliseParams(sdf=sp))
    assert again["tries"][0]["raw"] == t["raw"] and again["status"] == capi.TF_RELOC_FOUND
    # nothing was written: the volume and the index are as they were
    assert _snapshot(gv) == before
    for k, was in zip(sorted(frames), rows_before):
        _same(gv.reloc_descriptor(k), was)


def test_relocalise_does_not_accept_a_start_from_far_keyframes(hand, frames, rows):
    """only the far keyframes in the index, more than a metre off: candidates, tried in rank order, none accepted
    (tests/test_reloc_cpu.py shows the tracker restated failing from them)"""
    gv = hand
    p, want = rows
    far = {k: v for k, v in want.items() if k >= FAR0}
    depth, rgb = QI.frame(QI.query_pose(3, 1))
    before = _snapshot(gv)
    gv.reloc_configure()
    gv.reloc_index_add(sorted(far))
    ranked = Q.rank(Q.describe(depth, rgb, p), far, p, SHAPE)
    assert len(ranked) == 2
    res = gv.relocalise(depth, rgb, capi.RelocaliseParams(max_tries=2))
    print("far keyframes:", [(t["kf_id"], round(t["score"], 1), t["track"]["stage"], t["track"]["icp"]["status"]) for t in res["tries"]])
    assert res["status"] == capi.TF_RELOC_NOT_FOUND and res["n_tried"] == 2 and res["rank"] == -1
    assert [t["kf_id"] for t in res["tries"]] == [r[0] for r in ranked] and res["kf_id"] == ranked[0][0]
    assert np.array_equal(res["pose"], QI.rigid_inverse(QI.pose_inv16(frames[ranked[0][0]][2])))
    assert all(t["track"]["stage"] < 2 for t in res["tries"])
    one = gv.relocalise(depth, rgb, capi.RelocaliseParams(max_tries=1))
    assert one["status"] == capi.TF_RELOC_NOT_FOUND and one["n_tried"] == 1
    assert _snapshot(gv) == before


def test_invalid_arguments_launch_nothing(hand, frames):
    gv = hand
    L = gv.L
    INV = capi.TF_ERR_INVALID
    depth, rgb = QI.frame(QI.query_pose(0, 0))
    gv.reloc_configure()
    gv.reloc_index_add([KF0])
    res = capi.RelocaliseResult()
    C.memset(C.byref(res), 0x5A, C.sizeof(res))
    preset = bytes(res)
    gv.align_frame_icp(depth, frames[KF0][2])
    log = gv.align_icp_log()

    def call(params, d=depth, c=rgb, stride=3, out=res):
        return L.tf_relocalise(gv.h, None if d is None else f32p(d), None if c is None else u8p(c), stride,
                               None if params is None else C.byref(params), None if out is None else C.byref(out))

    good = capi.RelocaliseParams()
    for kw in (dict(max_tries=0), dict(max_tries=9), dict(min_stage=0), dict(min_stage=3), dict(min_valid_fraction=-0.1),
               dict(min_valid_fraction=1.5), dict(min_valid_fraction=np.nan), dict(max_rms=-1.0), dict(max_rms=np.nan)):
        assert call(capi.RelocaliseParams(**kw)) == INV, kw
    for icp in (capi.AlignIcpParams(n_levels=0), capi.AlignIcpParams(max_distance=np.nan), capi.AlignIcpParams(ray_max_steps=0)):
        assert call(capi.RelocaliseParams(icp=icp)) == INV
    for sdf in (capi.AlignParams(n_levels=5), capi.AlignParams(huber=-1.0), capi.AlignParams(iters=[60, 30, 0, 0])):
        assert call(capi.RelocaliseParams(sdf=sdf)) == INV
    assert call(good, stride=2) == INV and call(good, d=None) == INV and call(good, c=None) == INV
    assert call(None) == INV and call(good, out=None) == INV
    gv.raycast_camera(synth.Camera(13, 9, 11.0, 11.0, 6.5, 4.5))  # the tracker would read the frame at this size
    try:
        assert call(good) == INV
    finally:
        gv.raycast_camera(None)
    for bad in (dict(tiny_w=0), dict(tiny_w=3), dict(tiny_h=7), dict(max_depth=61.0), dict(min_depth=2.0, max_depth=1.0),
                dict(grey_weight=-1.0), dict(depth_weight=np.nan), dict(min_overlap=-1)):
        with pytest.raises(capi.TFError) as e:
            gv.reloc_configure(capi.RelocParams(**bad))
        assert e.value.code == INV, bad
    assert gv.reloc_index_count() == 1  # a refused configuration leaves the index alone
    assert bytes(res) == preset and gv.align_icp_log()[-1]["pose"].tobytes() == log[-1]["pose"].tobytes() and len(gv.align_icp_log()) == len(log)
    assert call(good) == capi.TF_OK and res.status == capi.TF_RELOC_FOUND


# ---- 5. the C++ mirror ----------------------------------------------------------------------------------------------------
def test_host_mirror_reloc(gpu_required, tmp_path):
    exe = str(tmp_path / "mirror_reloc")
    src = os.path.join(ROOT, "tests", "cpp_reloc", "mirror_reloc.cpp")
    lib = os.path.join(ROOT, "texturefusion_amd")
    subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", src,
                    "-o", exe, "-L" + lib, "-ltexfusion_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                    "-lamdhip64"], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mirror ok" in r.stdout, r.stdout + r.stderr
