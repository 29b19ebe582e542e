"""np.float32 / np.float64 restatement of devpose_inverse16 (texturefusion_amd/csrc/tf_devpose.h): the rigid inverse a
frame tracked on the device is textured with.  The rotation is copied; a translation entry is the f32 of the negated sum of
three f64 products of f32 values -- each exact, 48 bits at the most -- added left to right.  A helper, not a test module:
tests/test_devpose_textured_cpu.py holds it to the host function, tests/test_gpu_devpose_textured.py holds the device to it,
both bit for bit.  synth.pose_inverse16 goes through a BLAS product whose summation order is not fixed: it is not this."""
import numpy as np

F, D = np.float32, np.float64


def inverse16(pose):
    """pose: 12 f32 (row-major 3 x 4) -> T: 16 f32 (row-major 4 x 4)"""
    p = np.asarray(pose, F).reshape(12)
    T = np.zeros(16, F)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                T[4 * r + c] = p[4 * c + r]
            t = D(D(p[r]) * D(p[3])) + D(D(p[4 + r]) * D(p[7]))
            t = D(t + D(D(p[8 + r]) * D(p[11])))
            T[4 * r + 3] = F(-t)
    T[15] = F(1.0)
    return T


def rigid_inverse12(T):
    """tf_reloc.hip's rigid_inverse: the arithmetic above run the other way, a 4 x 4 back to a 3 x 4"""
    T = np.asarray(T, F).reshape(16)
    p = np.zeros(12, F)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                p[4 * r + c] = T[4 * c + r]
            t = D(D(T[r]) * D(T[3])) + D(D(T[4 + r]) * D(T[7]))
            t = D(t + D(D(T[8 + r]) * D(T[11])))
            p[4 * r + 3] = F(-t)
    return p
