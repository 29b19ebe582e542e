"""np.float32 restatement of the pose-dependent part of make_select_consts (texturefusion_amd/csrc/tf_host_math.h), which
k_pose_consts (tf_devpose.hip) computes on the device from a pose cell: every multiply and every add rounded to f32 on
its own, sums taken left to right.  A helper, not a test module: tests/test_devpose_cpu.py holds it to the host function,
tests/test_gpu_devpose.py holds the device to it, both bit for bit."""
import math

import numpy as np

from texturefusion_amd import synth

F = np.float32
FIELDS = ("rot", "tc", "r0", "r1", "r2", "coarse", "fine", "pose")  # in the struct's order, flattened row-major
WORDS = 9 + 3 + 9 + 48 + 12


def step_of(res):
    """stepSize: 1 above 10 mm, else 4 (the comparison is made in double)"""
    return 1 if float(F(res)) > 0.01 else 4


def consts(pose, res):
    """pose: 12 f32 (row-major 3 x 4), res: f32 -> dict of f32 arrays"""
    p = np.asarray(pose, F).reshape(12)
    res = F(res)
    fstep = F(step_of(res))
    rot = np.empty((3, 3), F)
    for i in range(3):
        for j in range(3):
            rot[i, j] = p[4 * j + i]
    tc, r0, r1, r2 = (np.empty(3, F) for _ in range(4))
    with np.errstate(all="ignore"):
        for i in range(3):
            s = F(rot[i, 0] * p[3])
            s = F(s + F(rot[i, 1] * p[7]))
            s = F(s + F(rot[i, 2] * p[11]))
            tc[i] = s
            r0[i] = F(F(rot[i, 0] * F(8.0)) * res)
            r1[i] = F(F(rot[i, 1] * F(8.0)) * res)
            r2[i] = F(F(rot[i, 2] * F(8.0)) * res)
        half = F(res * F(0.5))
        coarse, fine = np.empty((3, 8), F), np.empty((3, 8), F)
        for x in range(2):
            for y in range(2):
                for z in range(2):
                    cur = (F(x * 8), F(y * 8), F(z * 8))
                    k = x + y * 2 + z * 4
                    for a in range(3):
                        d = F(rot[a, 0] * cur[0])
                        d = F(d + F(rot[a, 1] * cur[1]))
                        d = F(d + F(rot[a, 2] * cur[2]))
                        coarse[a, k] = F(F(F(d * res) * fstep) + half)
                        fine[a, k] = F(F(F(d * res) * F(1.0)) + half)
    return dict(rot=rot, tc=tc, r0=r0, r1=r1, r2=r2, coarse=coarse, fine=fine, pose=p.copy())


def words(c):
    """the fields as one u32 array in the struct's order"""
    return np.concatenate([np.asarray(c[k], F).reshape(-1) for k in FIELDS]).view(np.uint32)


def poses():
    """name -> 12 f32: the identity, a generic rotation, one with negative zeros and denormal translation entries"""
    eye = np.eye(3, 4, dtype=F).reshape(12)
    generic = np.asarray(synth.pose_euler(math.radians(37.0), math.radians(-21.0), math.radians(8.0), (0.31, -1.27, 2.05)),
                         F).reshape(12)
    odd = np.asarray(synth.pose_euler(math.radians(-90.0), 0.0, math.radians(180.0), (0.0, 0.0, 0.0)), F).reshape(12).copy()
    odd[np.abs(odd) < 1e-6] = F(-0.0)                       # the small entries of a quarter turn as negative zeros
    odd[3], odd[7], odd[11] = F(1e-40), F(-3e-42), F(-0.0)  # denormals and a negative zero in the translation
    assert np.signbit(odd[odd == 0]).all() and 0 < abs(float(odd[3])) < 1.2e-38
    return {"identity": eye, "generic": generic, "odd": odd}


RESOLUTIONS = (F(0.005), F(0.02))  # both branches of the step rule
