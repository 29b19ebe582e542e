"""Texturing from a device pose without a GPU: devpose_inverse16 (tf_devpose.h) as the host runs it against its restatement
(tests/pose_inverse_ref.py), bit for bit; the restatement against tf_reloc.hip's rigid_inverse; the three new symbols; and
the register / private-memory figures of k_patch_posed beside k_patch<true, true, true> from the same compile, and of the
launch that computes the inverse (k_pose_consts: a second lane of it writes the PoseInverse block)."""
import os
import subprocess

import numpy as np
import pytest

from tests import pose_consts_ref as PR
from tests import pose_inverse_ref as IR
from tests.test_devpose_cpu import GRANULE, HIPCC, ROOT, _one, _usage

NAMES = ("tf_integrate_frame_textured_posed_device", "tf_track_texture_device", "tf_pose_inverse_download")


def _hex(a):
    return " ".join("%08x" % w for w in np.asarray(a, np.float32).view(np.uint32))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_restatement_equals_devpose_inverse16(tmp_path):
    exe = str(tmp_path / "inverse_print")
    # tf_devpose.h names device intrinsics next to the function: the HIP compiler's host pass, no device code, no GPU
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off",
           os.path.join(ROOT, "tests", "cpp_devpose", "inverse_print.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    poses = PR.poses()
    assert sorted(poses) == ["generic", "identity", "odd"]
    r = subprocess.run([exe], input="".join(_hex(p) + "\n" for p in poses.values()), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 3
    for (name, p), line in zip(poses.items(), lines):
        got = np.array([int(t, 16) for t in line.split()], np.uint32)
        want = IR.inverse16(p).view(np.uint32)
        assert got.shape == (16,) and np.array_equal(got, want), (name, np.flatnonzero(got != want))
    # what the cases exercise: a translation that is a sum of three non-zero products, and one that stays denormal
    g = IR.inverse16(poses["generic"])
    assert np.all(g[[3, 7, 11]] != 0) and np.array_equal(g[12:], np.array([0, 0, 0, 1], np.float32))
    odd = IR.inverse16(poses["odd"])
    assert 0 < np.abs(odd[[3, 7, 11]]).max() < 1.2e-38
    eye = IR.inverse16(poses["identity"])
    assert np.array_equal(eye.reshape(4, 4), np.eye(4, dtype=np.float32))  # (the translation is -0.0: equal to 0, not the same bits)
    assert np.signbit(eye[[3, 7, 11]]).all()


def test_rigid_inverse_returns_the_rotation_exactly():
    for name, p in PR.poses().items():
        back = IR.rigid_inverse12(IR.inverse16(p))
        rot = [0, 1, 2, 4, 5, 6, 8, 9, 10]
        assert np.array_equal(back[rot].view(np.uint32), np.asarray(p, np.float32)[rot].view(np.uint32)), name
    # the generic pose is a rotation to f32 accuracy, so the translation comes back to within a few ulps of its size
    p = PR.poses()["generic"]
    back = IR.rigid_inverse12(IR.inverse16(p))
    assert np.abs(back[[3, 7, 11]] - p[[3, 7, 11]]).max() < 1e-5


def test_symbols_are_declared_and_exported():
    from texturefusion_amd import capi
    L = capi.lib()
    for n in NAMES:
        assert n in capi.SYMBOLS, n
        fn = getattr(L, n)  # AttributeError: not exported
        assert fn.argtypes is not None and len(fn.argtypes) >= 4, n
    assert len(L.tf_integrate_frame_textured_posed_device.argtypes) == 5
    assert len(L.tf_track_texture_device.argtypes) == 10
    import ctypes as C
    assert C.sizeof(capi.PoseInverse) == 80
    for m in ("integrate_frame_textured_posed_device", "track_texture_device", "pose_inverse_download"):
        assert callable(getattr(capi.Volume, m))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_posed_patch_stage_costs_no_more_than_the_host_pose_one():
    usage = _usage("tf_atlas.hip")
    t, h = _one(usage, "k_patch_posed"), _one(usage, "k_patchILb1ELb1ELb1EE")
    print("k_patch_posed", t, "k_patch<true, true, true>", h)
    assert t["ScratchSize"] == 0, "k_patch_posed uses %d B/lane of private memory" % t["ScratchSize"]
    granules = lambda v: (v["VGPRs"] + GRANULE - 1) // GRANULE
    assert granules(t) <= granules(h), "k_patch_posed: %d VGPRs, k_patch<true, true, true>: %d" % (t["VGPRs"], h["VGPRs"])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_inverse_launch_owns_no_private_memory():
    k = _one(_usage("tf_devpose.hip"), "k_pose_consts")  # the inverse is a second lane's work in this launch
    print("k_pose_consts", k)
    assert k["ScratchSize"] == 0 and k["VGPRs"] <= 64
