"""Frame pre-processing on the device (tf_pre_*, texturefusion_amd/csrc/tf_pre.hip) on the hand-built cases of
tests/pre_inputs.py, every output image against the oracle bit for bit: thresholds fed their boundary values,
projections off the image, behind the camera and onto V.z == 0, non-finite and denormal readings, image sizes whose
grid tail is partial, the loader's weight 0, and in-place chains of up to 297 rounds -- more than the 256 the pass
once gave up at (the 16x300 case returned "did not settle" by the code of that version).
tests/test_pre_cpu.py shows on the CPU that each case sits on the edge it is named after.

The device binds its camera through tf_set_camera, which takes widths that are multiples of 8 only; the cases at other
widths exist between the two CPU statements, and here it is checked that the device refuses such a camera."""
import numpy as np
import pytest

from oracle import api as O
from texturefusion_amd import capi
from tests import pre_inputs as I
from tests import pre_ref as R
from tests.util import RES5, HipBuffer

pytestmark = pytest.mark.gpu


def _on_device(cases):
    return [c for c in cases if c.cam.width % 8 == 0]


def _ids(cases):
    return [c.name for c in cases]


NORMAL_MAP = _on_device(I.normal_map_cases())
DEPTH_NORMAL = _on_device(I.refine_depth_normal_cases())
COLOR_VALID = _on_device(I.color_valid_cases())
COLOR_QUALITY = _on_device(I.color_quality_cases())
NEWFRAME = _on_device(I.refine_newframe_cases())
KEYFRAME = _on_device(I.refine_keyframe_cases())
FRAME_DEPTH = I.frame_depth_cases()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


class _Device:
    """one capi.Volume per camera, kept for the module; buffers freed per test"""

    def __init__(self):
        self.volumes, self.buffers = {}, []

    def volume(self, cam):
        key = (cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy)
        if key not in self.volumes:
            self.volumes[key] = capi.Volume(RES5, cam, max_chunks=1 << 10, max_list=1 << 10, max_coarse=1 << 12)
        return self.volumes[key]

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        self.buffers.append(HipBuffer(arr.nbytes).from_host(arr))
        return self.buffers[-1]

    def get(self, buf, like):
        return buf.to_host().view(like.dtype).reshape(like.shape).copy()

    def free(self):
        for b in self.buffers:
            b.free()
        self.buffers = []


@pytest.fixture(scope="module")
def _device(gpu_required):
    dev = _Device()
    yield dev
    dev.free()
    for v in dev.volumes.values():
        v.close()


@pytest.fixture
def dev(_device):
    yield _device
    _device.free()


@pytest.mark.parametrize("case", NORMAL_MAP, ids=_ids(NORMAL_MAP))
def test_normal_map(dev, case):
    gv = dev.volume(case.cam)
    want = O.pre_normal_map(case.depth, case.cam)
    bd, bn = dev.put(case.depth), dev.put(np.full_like(want, 7.0))  # every pixel is written, the border as 0
    gv.pre_normal_map(bd.ptr, bn.ptr)
    gv.sync()
    assert _same(dev.get(bn, want), want)
    assert _same(dev.get(bd, case.depth), case.depth)


@pytest.mark.parametrize("case", DEPTH_NORMAL, ids=_ids(DEPTH_NORMAL))
def test_refine_depth_normal(dev, case):
    gv = dev.volume(case.cam)
    n_o, d_o = O.pre_refine_depth_normal(case.normal, case.depth, case.cam)
    bn, bd = dev.put(case.normal), dev.put(case.depth)
    gv.pre_refine_depth_normal(bn.ptr, bd.ptr)
    gv.sync()
    assert _same(dev.get(bn, n_o), n_o) and _same(dev.get(bd, d_o), d_o)


@pytest.mark.parametrize("case", COLOR_VALID, ids=_ids(COLOR_VALID))
def test_color_valid(dev, case):
    gv = dev.volume(case.cam)
    f_o = O.pre_color_valid(case.normal, case.cam)
    bn, bf = dev.put(case.normal), dev.put(np.full_like(f_o, 9))
    gv.pre_color_valid(bn.ptr, bf.ptr)
    gv.sync()
    assert np.array_equal(dev.get(bf, f_o), f_o)


@pytest.mark.parametrize("case", COLOR_QUALITY, ids=_ids(COLOR_QUALITY))
def test_color_quality(dev, case):
    gv = dev.volume(case.cam)
    q_o = O.pre_color_quality(case.depth, case.normal, case.rgb, case.cam)
    bd, bn, brgb, bq = dev.put(case.depth), dev.put(case.normal), dev.put(case.rgb), dev.put(np.full_like(q_o, 7.0))
    gv.pre_color_quality(bd.ptr, bn.ptr, brgb.ptr, bq.ptr)
    gv.sync()
    assert _same(dev.get(bq, q_o), q_o)


@pytest.mark.parametrize("case", NEWFRAME, ids=_ids(NEWFRAME))
def test_refine_newframe(dev, case):
    gv = dev.volume(case.cam)
    want = O.pre_refine_newframe(case.depth_ref, case.depth_new, case.cam, case.T)
    br, bn = dev.put(case.depth_ref), dev.put(case.depth_new)
    gv.pre_refine_newframe(br.ptr, bn.ptr, case.T)
    gv.sync()
    assert _same(dev.get(bn, want), want)
    assert _same(dev.get(br, case.depth_ref), case.depth_ref)


@pytest.mark.parametrize("case", KEYFRAME, ids=_ids(KEYFRAME))
def test_refine_keyframe(dev, case):
    """the sequential in-place result, however long the chain: the device runs at least as many rounds as the Jacobi
    form of the restatement needs, and may run more (it queues rounds in batches)"""
    gv = dev.volume(case.cam)
    args = (case.depth_ref, case.weight, case.depth_new, case.cam, case.T)
    d_o, w_o = O.pre_refine_keyframe(*args)
    needed = R.refine_keyframe_jacobi(*args)[2]
    bd, bw, bn = dev.put(case.depth_ref), dev.put(case.weight), dev.put(case.depth_new)
    rounds = gv.pre_refine_keyframe(bd.ptr, bw.ptr, bn.ptr, case.T)
    assert _same(dev.get(bd, d_o), d_o), rounds
    assert _same(dev.get(bw, w_o), w_o), rounds
    assert _same(dev.get(bn, case.depth_new), case.depth_new)
    assert rounds >= needed, (rounds, needed)


@pytest.mark.parametrize("case", FRAME_DEPTH, ids=_ids(FRAME_DEPTH))
def test_frame_depth(dev, case):
    H, W = case.z.shape
    gv = dev.volume(I.room_cam(W, H))
    z_o, r_o = O.pre_frame_depth(case.z, case.maximum_depth, case.depth_scale, case.d)
    bz, br = dev.put(case.z), dev.put(np.full_like(r_o, 7.0))
    gv.pre_frame_depth(bz.ptr, br.ptr, case.maximum_depth, case.depth_scale, case.d)
    gv.sync()
    assert _same(dev.get(br, r_o), r_o)
    assert np.array_equal(dev.get(bz, z_o), z_o)


def _refused(call):
    with pytest.raises(capi.TFError) as e:
        call()
    assert e.value.code == capi.TF_ERR_INVALID, e.value


def test_argument_checks_leave_the_images_alone(dev):
    cam = I.room_cam(24, 13)
    gv = dev.volume(cam)
    rng = np.random.default_rng(1)
    d = rng.random((13, 24)).astype(np.float32) + 1
    n = rng.normal(size=(3, 13, 24)).astype(np.float32)
    z = rng.integers(500, 3000, (13, 24)).astype(np.uint16)
    rgb = rng.integers(0, 256, (13, 24, 3), dtype=np.uint8)
    flag = np.full((13, 24), 9, np.uint8)
    bd, bd2, bw, bn, bz, brgb, bf = (dev.put(a) for a in (d, d + 1, d + 2, n, z, rgb, flag))
    for bad_d in I.FRAME_DEPTH_REJECTED_D:  # radius 8, and the radius 15 a non-positive d takes from sigma_space = 10
        _refused(lambda: gv.pre_frame_depth(bz.ptr, bd.ptr, 4.0, 1000.0, bad_d))
    _refused(lambda: gv.pre_frame_depth(bz.ptr, bd.ptr, 4.0, 0.0, 9))
    _refused(lambda: gv.pre_frame_depth(None, bd.ptr, 4.0, 1000.0, 9))
    _refused(lambda: gv.pre_normal_map(bd.ptr, None))
    _refused(lambda: gv.pre_normal_map(None, bn.ptr))
    _refused(lambda: gv.pre_refine_depth_normal(bn.ptr, None))
    _refused(lambda: gv.pre_color_valid(None, bf.ptr))
    _refused(lambda: gv.pre_color_quality(bd.ptr, bn.ptr, None, bd2.ptr))
    _refused(lambda: gv.pre_refine_newframe(None, bd.ptr, I.I34))
    _refused(lambda: gv.pre_refine_newframe(bd.ptr, None, I.I34))
    _refused(lambda: gv.pre_refine_keyframe(bd.ptr, bw.ptr, None, I.I34))
    _refused(lambda: gv.pre_refine_keyframe(bd.ptr, None, bd2.ptr, I.I34))
    _refused(lambda: gv.pre_refine_keyframe(None, bw.ptr, bd2.ptr, I.I34))
    gv.sync()
    for buf, arr in ((bd, d), (bd2, d + 1), (bw, d + 2), (bn, n), (bz, z), (brgb, rgb), (bf, flag)):
        assert np.array_equal(dev.get(buf, arr).view(np.uint8), np.ascontiguousarray(arr).view(np.uint8))
    # d = 1 is radius 1, the smallest filter
    z_o, r_o = O.pre_frame_depth(z, 4.0, 1000.0, 1)
    gv.pre_frame_depth(bz.ptr, bd.ptr, 4.0, 1000.0, 1)
    gv.sync()
    assert _same(dev.get(bd, r_o), r_o) and np.array_equal(dev.get(bz, z_o), z_o)


@pytest.mark.parametrize("width", [1, 2, 11, 12, 19, 20, 21, 27])
def test_widths_without_whole_groups_are_refused(dev, width):
    """tf_set_camera takes multiples of 8 only, so no pass ever sees another width: a refused camera leaves the
    handle on the one it had, and the two refinement passes check the width themselves as well"""
    cam = I.room_cam(24, 13)
    gv = dev.volume(cam)
    assert gv.L.tf_set_camera(gv.h, 128.0, 128.0, 5.0, 2.0, width, 5, 0.01, 5.0) == capi.TF_ERR_INVALID
    case = I.keyframe_exact(24, 13)
    d_o, w_o = O.pre_refine_keyframe(case.depth_ref, case.weight, case.depth_new, cam, case.T)
    bd, bw, bn = dev.put(case.depth_ref), dev.put(case.weight), dev.put(case.depth_new)
    gv.pre_refine_keyframe(bd.ptr, bw.ptr, bn.ptr, case.T)
    assert _same(dev.get(bd, d_o), d_o) and _same(dev.get(bw, w_o), w_o)
