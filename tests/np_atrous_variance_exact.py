"""Exact integer answers of one variance-guided a-trous pass (include/mi_denoise.h, section a4i), after np_atrous_exact.py.

Guide planes of two values at sigma 0.02 make a layer weight 1 or 0.  The frame is GREY: r = g = b, an integer 0 .. 15 (distinct
rgb integers can have nearly equal luminance; equal greys give dl = 0 exactly, different ones |dl| of about 1 or more), alpha a
random integer.  The variance plane holds integers 0 .. 15, sigmaLum = 2^-20 and epsilon = 2^-10: the denominator of the
luminance term stays below 1e-3, the exponent of unequal greys beyond -1400, so 2^arg is exactly 0 for them and exactly 1 for
equal ones.  Then w is K(o) or 0 and

    sum w C = num / 256,   sum w = den / 256,   sum w^2 V = numv / 65536

are integers over 256 or 65536 below 2^24, exact in fp32 in any order, and so is (sum w)^2 = den^2 / 65536.  C and V of the pass
are one correctly rounded fp32 quotient each.  The grey of a texel is 3 + b0 + 2 b1 + 4 b2 of three more label planes of
np_atrous_exact.label_bits' kind, so that equal greys are as frequent as equal labels.
"""
import functools

import numpy as np

import np_atrous_exact as ex

SIGMA = ex.SIGMA
SIGMA_LUM, EPSILON = 2.0 ** -20, 2.0 ** -10
FRAME, WIDE = ex.FRAME, ex.WIDE
LAYERS = ex.LAYERS
WIDE_LAYERS, WIDE_PASSES = ex.WIDE_LAYERS, ex.WIDE_PASSES


def grey_frame(shape, L, dtype=np.float32, seed=1):
    h, w = shape
    b = ex.label_bits(shape, 3 * L + 3, 0, seed + 100)[3 * L:]
    grey = 3 + b[0] + 2 * b[1] + 4 * b[2]
    fr = np.empty((h, w, 4), dtype)
    fr[..., 0] = fr[..., 1] = fr[..., 2] = grey
    fr[..., 3] = np.random.default_rng([seed, 7, 0]).integers(0, 16, (h, w))
    return fr


def variance_plane(shape, seed=3):
    return np.random.default_rng([seed, 11]).integers(0, 16, shape).astype(np.float32)


def inputs(shape, L, fdt=np.float32, gdt=np.float32):
    """(frame, variance, layers): the same integers and the same pattern in every dtype, hence one answer."""
    return grey_frame(shape, L, fdt), variance_plane(shape), ex.colour_layers(shape, L, gdt)


@functools.lru_cache(maxsize=None)
def predicate(shape, L):
    fr, _, ly = inputs(shape, L)
    return ex.equal_on(ly, fr)


def sums(C, V, same, step, reverse=False):
    """(num [h, w, 4], den [h, w], numv [h, w], accepted, offered) as int64."""
    Ci, Vi = ex._ints(C), ex._ints(V)
    h, w = Vi.shape
    num, den, numv = np.zeros((h, w, 4), np.int64), np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    accepted = offered = 0
    for j, i, p, q in ex._taps(h, w, step, reverse):
        ok = same(p, q)
        kk = ex.K1[i + 2] * ex.K1[j + 2]
        num[p] += kk * ok[..., None] * Ci[q]
        den[p] += kk * ok
        numv[p] += kk * kk * ok * Vi[q]
        if (j, i) != (0, 0):
            accepted += int(ok.sum())
            offered += ok.size
    return num, den, numv, accepted, offered


def variance_quotient(numv, den):
    """float32(numv / 65536) / (float32(den / 256) * float32(den / 256)): the product and both operands exact, one IEEE division."""
    assert 0 <= numv.min() and numv.max() < 2 ** 24 and 0 < den.min() and den.max() <= 256
    n = (numv / 65536.0).astype(np.float32)
    d = (den / 256.0).astype(np.float32)
    dd = d * d
    assert np.array_equal(n.astype(np.float64) * 65536, numv) and np.array_equal(dd.astype(np.float64) * 65536, den * den)
    return n / dd


def exact_pass(C, V, same, step, reverse=False):
    """(C', V') float32 of one pass at `step` over the integer level C and the integer variance plane V."""
    num, den, numv, _, _ = sums(C, V, same, step, reverse)
    return ex.quotient(num, den), variance_quotient(numv, den)


@functools.lru_cache(maxsize=None)
def answer(shape, L, step):
    fr, v, _ = inputs(shape, L)
    return exact_pass(fr, v, predicate(shape, L), step)
