"""Every place tf_integrate_frame_host / _rgb can take a frame from, mixed in one stream: plain arrays (staged), the
pinned slot of tf_host_frame_buffers (composed in place: no staging copy), registered caller buffers (uploaded in place,
waiting and asynchronous), RGB + valid flags from each of these.  Bit for bit against the oracle's per-frame unit, with
the deferral on and off, with flushes in between, and what tf_host_frame_times counts.  A 160x120 camera at 10 mm voxels:
16 frames give ~500 meshes and every case takes a few seconds."""
import functools

import numpy as np
import pytest

from oracle import api as O
from texturefusion_amd import capi, synth
from tests.util import sorted_ids
from tests.test_gpu_textured_soak import compare_with_oracle

pytestmark = pytest.mark.gpu

CAM = synth.Camera(160, 120, 131.25, 131.25, 79.5, 59.5, 0.01, 5.0)
RES = np.float32(0.01)
NPIX = CAM.width * CAM.height
N_FRAMES = 16
FLAGGED = (4, 6, 7)  # sources (frame index mod 8) that pass valid flags: their frames get holes
FLUSH_AFTER = (9, 10, 12, 15)


@functools.lru_cache(maxsize=None)
def _frames():
    """the 16 frames as the oracle gets them: (depth, rgba, pose, pose_inv16); frames of the flagged sources with holes
    punched into the RGBA like test_host_frames_as_rgb_and_valid_flags does (scaled from 640x480 to this image)"""
    out = []
    for k in range(N_FRAMES):
        depth, rgba, _, pose = synth.room_frame(k, CAM, with_quality=False, wobble=0.03)
        assert rgba[..., 3].all()
        if k % 8 in FLAGGED:
            rgba = rgba.copy()
            rgba[10 + 2 * k:50, 25:75 + 3 * k] = 0  # colorValidFlag == 0: the staging loop zeroes all four bytes
            rgba[::5, ::3] = 0
        out.append((depth, rgba, pose, synth.pose_inverse16(pose)))
    return out


def _oracle(lo, hi, flush_after=()):
    ov = O.Volume(RES, O.camera_from(CAM), O.default_integrator())
    oa = O.Atlas(RES)
    chunks = {}
    for k in range(lo, hi):
        d, c, pose, pinv = _frames()[k]
        ov.frame_textured(oa, d, c, pose, pinv, 10 + k)
        if k in flush_after:
            chunks[k] = sorted_ids(ov.list_chunks())
    return ov, oa, chunks


@functools.lru_cache(maxsize=None)
def _oracle_all():
    """the oracle after all 16 frames: computed once, only read by the tests"""
    return _oracle(0, N_FRAMES)


def _rgb_and_flags(rgba):
    valid = np.ascontiguousarray(rgba[..., 3])
    rgb = np.ascontiguousarray(rgba[..., :3]).copy()
    rgb[valid == 0] = 77  # (whatever the camera delivered where the flag says invalid)
    return rgb, valid


def _own_pages(shape, dtype):
    """an array on pages of its own: images this small come out of the heap, where two arrays share a page -- and a page is
    locked once (tf_host_register wants ranges that do not overlap)"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.empty(((n + 4095) & ~4095) + 4096, np.uint8)
    at = -raw.ctypes.data % 4096
    return raw[at:at + n].view(dtype).reshape(shape)


class _Feeder:
    """hands frame k to the volume through source k % 8; caller buffers are scribbled over as soon as they are the caller's
    again (right after a waiting call; after the fence for the asynchronous ring)"""

    def __init__(self, gv):
        self.gv = gv
        f32 = lambda: _own_pages((CAM.height, CAM.width), np.float32)
        u8 = lambda *shape: _own_pages((CAM.height, CAM.width) + shape, np.uint8)
        self.pair = (f32(), u8(4))                        # source 2
        self.ring = [(f32(), u8(4)), (f32(), u8(4))]      # source 3
        self.ring_next = 0
        self.rgb_bufs = (f32(), u8(3), u8())              # source 6
        self.registered = list(self.pair) + [b for p in self.ring for b in p] + list(self.rgb_bufs)
        for b in self.registered:
            gv.host_register(b)

    def feed(self, k):
        gv = self.gv
        depth, rgba, pose, pinv = _frames()[k]
        pose = pose.reshape(12)
        src = k % 8
        if src == 0:    # plain arrays: staged
            d, c = depth.copy(), rgba.copy()
            gv.integrate_frame_host(d, c, pose, pinv, 10 + k)
            d[...] = 123.0; c[...] = 200
        elif src == 1:  # composed in the pinned slot and passed as its views: nothing to copy
            d, c = gv.host_frame_buffers()
            d[...] = depth; c[...] = rgba
            gv.integrate_frame_host(d, c, pose, pinv, 10 + k)
        elif src == 2:  # one registered pair, a call that waits for its upload
            d, c = self.pair
            d[...] = depth; c[...] = rgba
            gv.integrate_frame_host(d, c, pose, pinv, 10 + k)
            d[...] = 123.0; c[...] = 200
        elif src == 3:  # a ring of two registered pairs, calls that do not wait: a fence before each refill
            gv.host_frame_set_async(True)
            d, c = self.ring[self.ring_next]
            self.ring_next ^= 1
            gv.host_frame_fence()
            d[...] = depth; c[...] = rgba
            gv.integrate_frame_host(d, c, pose, pinv, 10 + k)
            gv.host_frame_set_async(False)
        elif src in (4, 5):  # RGB staged, with flags / without (every pixel valid)
            rgb, valid = _rgb_and_flags(rgba)
            assert valid.all() == (src == 5)
            d = depth.copy()
            gv.integrate_frame_host_rgb(d, rgb, valid if src == 4 else None, pose, pinv, 10 + k)
            d[...] = 123.0; rgb[...] = 200; valid[...] = 1
        elif src == 6:  # RGB and flags out of registered buffers
            d, rgb, valid = self.rgb_bufs
            d[...] = depth
            rgb[...], valid[...] = _rgb_and_flags(rgba)
            gv.integrate_frame_host_rgb(d, rgb, valid, pose, pinv, 10 + k)
            d[...] = 123.0; rgb[...] = 200; valid[...] = 1
        else:           # RGB composed in the slot: at the start of the colour view, the flags at byte 3 npix of it
            d, c = gv.host_frame_buffers()
            flat = c.reshape(-1)
            rgb, valid = flat[:3 * NPIX], flat[3 * NPIX:]
            d[...] = depth
            rgb[...], valid[...] = (a.reshape(-1) for a in _rgb_and_flags(rgba))
            gv.integrate_frame_host_rgb(d, rgb, valid, pose, pinv, 10 + k)

    def finish(self):
        """fence + scribble over the asynchronous ring, sync; the volume then holds every frame"""
        self.gv.host_frame_fence()
        for d, c in self.ring:
            d[...] = 7.0; c[...] = 9
        self.gv.sync()

    def close(self):
        for b in self.registered:
            self.gv.host_unregister(b)
        self.gv.close()


def _volume(defer):
    gv = capi.Volume(RES, CAM, max_chunks=1 << 16)
    gv.host_frame_set_deferral(defer)
    assert gv.host_frame_deferral()[0] == (4 if defer else 0)
    return gv


@pytest.mark.parametrize("defer", [True, False], ids=["deferral", "no_deferral"])
def test_every_source_in_one_stream(gpu_required, defer):
    """frames cycle twice through the eight sources; with the deferral on, the final sync flushes four pending frames"""
    ov, oa, _ = _oracle_all()
    fd = _Feeder(_volume(defer))
    for k in range(N_FRAMES):
        fd.feed(k)
    fd.finish()
    assert compare_with_oracle(ov, oa, fd.gv, stride=1) > 300
    fd.close()


def test_flushes_while_the_sources_change(gpu_required):
    """the second cycle on a fresh pair of volumes, a flushing entry point (tf_list_chunks) after frames 9, 10, 12 and 15:
    2, 1, 2 and 3 frames are pending at those flushes (4: the final sync of the test above), each from another source"""
    ov, oa, chunks = _oracle(8, N_FRAMES, FLUSH_AFTER)
    fd = _Feeder(_volume(True))
    for k in range(8, N_FRAMES):
        fd.feed(k)
        if k in FLUSH_AFTER:
            assert np.array_equal(chunks[k], sorted_ids(fd.gv.list_chunks())), k
    fd.finish()
    assert compare_with_oracle(ov, oa, fd.gv, stride=1) > 0
    fd.close()


def test_what_the_trace_counts(gpu_required):
    """tf_host_frame_times' call count (bench.py divides its phase times by it): launches a host-frame call made for its
    oldest pending frame -- N calls less the frames still deferred at the end; the flush of those does not count"""
    gv = _volume(True)
    n = 9
    for k in range(n):
        depth, rgba, pose, pinv = _frames()[k]
        gv.integrate_frame_host(depth, rgba, pose.reshape(12), pinv, 10 + k)
    gv.sync()
    assert gv.host_frame_times(reset=True)["calls"] == n - gv.host_frame_deferral()[0]
    assert gv.host_frame_times()["calls"] == 0
    gv.close()
