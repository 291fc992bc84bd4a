"""The contract of albedo demodulation (include/mi_denoise.h, section a4k) in NumPy float32, written from the header:

    d_c = fmaxf(A_c, floor)     c in {R, G, B};  A read as a guide texel (uint8 code c -> the correctly rounded c / 255)
    demodulate   I_c = C_c / d_c     one IEEE division, C widened (uint8 -> c / 255 correctly rounded, float16 exactly);  float32 out
    modulate     O_c = I_c * d_c     one multiplication;  out in float32, or packed by the rules of mid_pack_u8 / mid_pack_f16
    alpha passes through.

Every operation is ONE float32 operation of NumPy, so the results are the bits the kernels must give (the library is built with
-ffp-contract=off and without fast-math).  np.fmax, not np.maximum: a NaN albedo gives floor, as fmaxf does.
"""
import numpy as np

import np_atrous_joint


def widen(a):
    """A frame or an albedo plane as float32, by the widening of the a-trous checkers (np_atrous_joint.widen: uint8 codes c / 255 in
    float64, floats as they are) rounded to float32: for all 256 codes that is the correctly rounded quotient, which
    tests/test_albedo_checker.py checks in exact arithmetic; float16 and float32 values widen exactly."""
    return np_atrous_joint.widen(a).astype(np.float32)


def pack_u8(x):
    """mid_pack_u8: (unsigned char)(255.0f * v), truncation; 0 where v <= -1 or NaN, 255 where v >= 256."""
    with np.errstate(all="ignore"):
        v = np.float32(255.0) * np.asarray(x, np.float32)
        out = np.zeros(v.shape, np.uint8)
        ok = v > np.float32(-1.0)
        hi = ok & (v >= np.float32(256.0))
        mid = ok & ~hi
        out[hi] = 255
        out[mid] = np.trunc(v[mid]).astype(np.int32).astype(np.uint8)
    return out


def pack_f16(x):
    """mid_pack_f16: round to nearest even, overflow to +-Inf, NaN stays NaN."""
    with np.errstate(all="ignore"):
        return np.asarray(x, np.float32).astype(np.float16)


def divisor(albedo, floor):
    return np.fmax(widen(albedo)[..., :3], np.float32(floor))


def demodulate(frame, albedo, floor=1e-3):
    c = widen(frame)
    out = c.copy()
    with np.errstate(all="ignore"):
        out[..., :3] = c[..., :3] / divisor(albedo, floor)
    return out


def modulate(illum, albedo, floor=1e-3, out_dtype=np.float32):
    i = np.asarray(illum)
    assert i.dtype == np.float32
    out = i.copy()
    with np.errstate(all="ignore"):
        out[..., :3] = i[..., :3] * divisor(albedo, floor)
    dt = np.dtype(out_dtype)
    return out if dt == np.float32 else pack_u8(out) if dt == np.uint8 else pack_f16(out)
