"""Inputs of the variance-guided a-trous tests (include/mi_denoise.h, section a4i), shared by the CPU test that holds them to
their conditions (test_atrous_variance_args.py) and the GPU tests that assert on them (test_gpu_atrous_variance.py).

Frames: a smooth HDR base times Gamma(4, 0.25) noise (conftest.synth_hdr), values up to about 8.  Guide layers: smooth patterns
in [0, 1] plus noise, so that the same layer exists as float32, float16 and -- quantised -- uint8.  Sigmas 0.3 / 0.5 / 0.4.
"""
import functools

import numpy as np

import np_atrous_variance as chk
from conftest import synth_hdr

SHAPE = (131, 261)                                     # rows x columns: the 261 x 131 frame
SIGMAS = (0.3, 0.5, 0.4)
N_FRAMES = 3


def sigmas_of(L):
    return [SIGMAS[l % 3] for l in range(L)]


@functools.lru_cache(maxsize=None)
def _frame32(shape, f):
    fr = synth_hdr(np.random.default_rng(100 + f), shape[0], shape[1])
    fr.setflags(write=False)
    return fr


def frame_of(shape, f=0, dtype=np.float32):
    """Frame f as float32, as the float16 it rounds to, or as uint8 of frame / 8."""
    fr = _frame32(shape, f)
    if np.dtype(dtype) == np.uint8:
        return np.clip(fr * (255.0 / 8.0), 0, 255).astype(np.uint8)
    return fr.astype(dtype)


@functools.lru_cache(maxsize=None)
def _layer64(shape, f, l):
    h, w = shape
    rng = np.random.default_rng([7, f, l])
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a, b, c = 0.05 + 0.02 * l, 0.07 + 0.01 * l, 0.03 + 0.015 * l
    g = np.stack([0.5 + 0.35 * np.sin(xx * a + 0.3 * f), 0.5 + 0.35 * np.cos(yy * b + 0.2 * l), 0.5 + 0.35 * np.sin((xx + yy) * c + f)], -1)
    g = np.clip(g + rng.normal(0, 0.06, (h, w, 3)), 0, 1)
    out = np.concatenate([g, rng.random((h, w, 1))], -1)
    out.setflags(write=False)
    return out


def layers_of(shape, L, dtype=np.float32, f=0):
    if np.dtype(dtype) == np.uint8:
        return [np.round(_layer64(shape, f, l) * 255).astype(np.uint8) for l in range(L)]
    return [_layer64(shape, f, l).astype(dtype) for l in range(L)]


@functools.lru_cache(maxsize=None)
def v0_of(shape, L, fdt, gdt, k, t=1):
    """float32(V_0) of frame t by the float64 checker: the var_in of a case, the same plane for the checker and the GPU."""
    frames = [frame_of(shape, f, fdt) for f in range(N_FRAMES)]
    layers = [layers_of(shape, L, gdt, f) for f in range(N_FRAMES)]
    v = chk.moments(frames, layers, sigmas_of(L), k=k, t=t)[0].astype(np.float32)
    v.setflags(write=False)
    return v


# (L, frame dtype, guide dtype, passes, sigma_lum, epsilon, k of the moments): what test_gpu_atrous_variance.py asserts on
F32, F16, U8 = np.float32, np.float16, np.uint8
CASES = (
    [(3, F32, F32, n, 4.0, 1e-3, n % 2) for n in range(1, 9)] +
    [(1, F32, U8, 5, 1.0, 1e-2, 0), (2, F16, F16, 5, 0.25, 1e-3, 1), (4, U8, F32, 5, 4.0, 1e-3, 0), (4, F32, F16, 3, 1.0, 1e-4, 1),
     (5, F16, U8, 5, 4.0, 1e-2, 0), (5, F32, F32, 8, 1.0, 1e-3, 1), (16, F32, F32, 5, 4.0, 1e-3, 0), (16, U8, U8, 2, 0.25, 1e-2, 1)]
)


def case_id(c):
    L, fdt, gdt, n, sl, eps, k = c
    return f"L{L}-{np.dtype(fdt).name}-{np.dtype(gdt).name}-p{n}-s{sl:g}-e{eps:g}-k{k}"


def case_inputs(c):
    """(frame, var_in, layers, sigmas) of a case."""
    L, fdt, gdt, n, sl, eps, k = c
    return frame_of(SHAPE, 1, fdt), v0_of(SHAPE, L, fdt, gdt, k), layers_of(SHAPE, L, gdt, 1), sigmas_of(L)


@functools.lru_cache(maxsize=None)
def case_reference(c):
    """(C, V) of the float64 checker, and the same with every level rounded to fp32 after each pass."""
    L, fdt, gdt, n, sl, eps, k = c
    fr, v0, ly, sg = case_inputs(c)
    return (chk.atrous_variance(fr, v0, ly, sg, passes=n, sigma_lum=sl, epsilon=eps),
            chk.atrous_variance(fr, v0, ly, sg, passes=n, sigma_lum=sl, epsilon=eps, round32=True))
