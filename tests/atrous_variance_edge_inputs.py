"""Inputs of the edge tests of the variance-guided a-trous filter (include/mi_denoise.h, section a4i), shared by the CPU test that
holds them to their conditions (test_atrous_variance_edge_inputs.py) and the GPU tests that assert on them
(test_gpu_atrous_variance_edges.py).  Frames, layers, V_0 and sigmas are atrous_variance_inputs.py's; shapes are (rows, columns).

A case is (shape, L, frame dtype, guide dtype, first_pass, n_passes, sigma_lum, epsilon); var_in is v0_of(shape, L, fdt, gdt, 0).

    TINY      frames narrower than a wave, shorter than the step, shorter than a comb chunk, 1 x 1, and frames with a seam at
              x = 64 and one to three columns beyond it; 1 .. 16 layers; pass ranges that reach steps 1 .. 128
    SWEEP     every height 1 .. 40 at width 67, one pass at steps 1 .. 8: every chunk count of both comb chunk sizes
    TALL      tall narrow frames, one pass at steps 8 .. 128: whole residue classes without a row, several chunks per class
    SCALED    the 40 x 129 frame times 1/64, 16 and 1024 with V_0 and epsilon to match
    NONFINITE NaN, +Inf, -Inf colour texels and NaN, +Inf, -1 variance texels on the seam column and at the corners
"""
import functools

import numpy as np

import atrous_variance_inputs as avi
import np_atrous_variance as chk

F32, F16, U8 = np.float32, np.float16, np.uint8
DT = (F32, F16, U8)
LUM = ((4.0, 1e-3), (0.25, 1e-2))                       # (sigma_lum, epsilon)

# ---- 1. tiny and seam frames ---------------------------------------------------------------------------------------------------------
TINY_SHAPES = [(1, 1), (1, 64), (2, 65), (5, 7), (7, 3), (64, 1), (17, 65), (33, 66), (40, 129), (9, 200)]
TINY_LAYERS = (1, 2, 3, 4, 5, 16)
PASS_RANGES = ((0, 1), (0, 5), (3, 3), (6, 2), (0, 8))   # (first_pass, n_passes): steps 1; 1..16; 8..32; 64, 128; 1..128


def tiny_cases(shape):
    """The 30 cases of a shape; the frame dtype, the guide dtype and (sigma_lum, epsilon) rotate over the table."""
    si = TINY_SHAPES.index(shape)
    out = []
    for li, L in enumerate(TINY_LAYERS):
        for pi, (first, n) in enumerate(PASS_RANGES):
            r = si + len(PASS_RANGES) * li + pi
            sl, eps = LUM[(r + li) % 2]
            out.append((shape, L, DT[r % 3], DT[(r // 3) % 3], first, n, sl, eps))
    return out


TINY = [c for s in TINY_SHAPES for c in tiny_cases(s)]

# ---- 2. every chunk count ------------------------------------------------------------------------------------------------------------
SWEEP_WIDTH = 67                                        # a seam at x = 64 with three columns beyond
SWEEP_HEIGHTS = tuple(range(1, 41))
SWEEP_LAYERS = (1, 4, 5)                                # two rows per wave, one row per wave, global taps
SWEEP_FIRST = (0, 1, 2, 3)
TALL_SHAPES = [(130, 5), (257, 5), (300, 3)]
TALL_LAYERS = (1, 2, 4, 5)
TALL_FIRST = (3, 4, 5, 6, 7)


def one_pass_case(shape, L, first):
    return (shape, L, F32, F32, first, 1, 4.0, 1e-3)


SWEEP = [one_pass_case((h, SWEEP_WIDTH), L, first) for L in SWEEP_LAYERS for first in SWEEP_FIRST for h in SWEEP_HEIGHTS]
TALL = [one_pass_case(s, L, first) for s in TALL_SHAPES for L in TALL_LAYERS for first in TALL_FIRST]


def case_id(c):
    shape, L, fdt, gdt, first, n, sl, eps = c
    return f"{shape[0]}x{shape[1]}-L{L}-{np.dtype(fdt).name}-{np.dtype(gdt).name}-p{first}+{n}-s{sl:g}-e{eps:g}"


def case_inputs(c):
    """(frame, var_in, layers, sigmas) of a case."""
    shape, L, fdt, gdt = c[:4]
    return avi.frame_of(shape, 1, fdt), avi.v0_of(shape, L, fdt, gdt, 0), avi.layers_of(shape, L, gdt, 1), avi.sigmas_of(L)


@functools.lru_cache(maxsize=None)
def case_reference(c, round32=False):
    """(C, V) of the float64 checker; round32: with every level rounded to fp32 after each pass."""
    fr, v0, ly, sg = case_inputs(c)
    return chk.atrous_variance(fr, v0, ly, sg, passes=c[5], first_pass=c[4], sigma_lum=c[6], epsilon=c[7], round32=round32)


def posedness(ref, ref32):
    """test_the_inputs_of_the_gpu_test_are_well_posed's measure: how far rounding the levels to fp32 moves the float64 formula."""
    (C, V), (C32, V32) = ref, ref32
    return (float(np.max(np.abs(C - C32) / np.maximum(1.0, np.abs(C)))), float(np.max(np.abs(V - V32) / np.maximum(1.0, np.abs(V)))))


# ---- 3. value range ------------------------------------------------------------------------------------------------------------------
RANGE_SHAPE = (40, 129)
SCALES = (1.0 / 64.0, 16.0, 1024.0)
SCALED_SIGMA_LUM = (0.25, 4.0, 16.0)
SCALED_LAYERS = (2, 4, 5)
SCALED_RANGES = ((0, 5), (0, 1), (5, 3))
SCALED = [(s, L, sl, first, n) for s in SCALES for L in SCALED_LAYERS for sl in SCALED_SIGMA_LUM for first, n in SCALED_RANGES]


def scaled_frames(scale, dtype=np.float32, alpha_too=False):
    """The three frames of RANGE_SHAPE with rgb times `scale` (a power of two: exact) and alpha left alone, or scaled too."""
    out = []
    for f in range(avi.N_FRAMES):
        fr = avi.frame_of(RANGE_SHAPE, f, dtype).copy()
        fr[..., :4 if alpha_too else 3] *= dtype(scale)
        out.append(fr)
    return out


@functools.lru_cache(maxsize=None)
def scaled_v0(scale, L):
    """float32 of the checker's moments (k = 0, t = 1) of the scaled frames: the var_in of a scaled case."""
    layers = [avi.layers_of(RANGE_SHAPE, L, np.float32, f) for f in range(avi.N_FRAMES)]
    v = chk.moments(scaled_frames(scale), layers, avi.sigmas_of(L), k=0, t=1)[0].astype(np.float32)
    v.setflags(write=False)
    return v


def scaled_id(c):
    s, L, sl, first, n = c
    return f"x{s:g}-L{L}-s{sl:g}-p{first}+{n}"


def scaled_inputs(c):
    """(frame, var_in, layers, sigmas, epsilon) of a scaled case; epsilon = 1e-3 * scale."""
    s, L = c[:2]
    return scaled_frames(s)[1], scaled_v0(s, L), avi.layers_of(RANGE_SHAPE, L, np.float32, 1), avi.sigmas_of(L), 1e-3 * s


@functools.lru_cache(maxsize=None)
def scaled_reference(c, round32=False):
    fr, v0, ly, sg, eps = scaled_inputs(c)
    return chk.atrous_variance(fr, v0, ly, sg, passes=c[4], first_pass=c[3], sigma_lum=c[2], epsilon=eps, round32=round32)


# ---- 4. non-finite texels ------------------------------------------------------------------------------------------------------------
NF_SHAPE = (40, 129)
NF_LAYERS = (3, 5)
NF_RANGES = ((0, 1), (0, 2), (2, 1), (5, 1))
NAN, INF = float("nan"), float("inf")
# (row, column, channel, value): one texel of each kind on the seam column x = 64 and one at a frame corner
NF_COLOUR = [(6, 64, 1, NAN), (20, 64, 0, INF), (33, 64, 2, -INF), (0, 0, 2, NAN), (39, 128, 1, INF), (0, 128, 0, -INF)]
NF_VARIANCE = [(13, 64, NAN), (27, 64, INF), (38, 64, -1.0), (0, 0, NAN), (0, 128, INF), (39, 0, -1.0)]
NONFINITE = [(L, first, n) for L in NF_LAYERS for first, n in NF_RANGES]


def nonfinite_id(c):
    return f"L{c[0]}-p{c[1]}+{c[2]}"


def nonfinite_inputs(c):
    """(frame, var_in, layers, sigmas): the finite inputs of NF_SHAPE with the twelve texels above replaced."""
    L = c[0]
    fr = avi.frame_of(NF_SHAPE, 1).copy()
    v0 = avi.v0_of(NF_SHAPE, L, F32, F32, 0).copy()
    for y, x, ch, val in NF_COLOUR:
        fr[y, x, ch] = val
    for y, x, val in NF_VARIANCE:
        v0[y, x] = val
    return fr, v0, avi.layers_of(NF_SHAPE, L, F32, 1), avi.sigmas_of(L)


@functools.lru_cache(maxsize=None)
def nonfinite_reference(c):
    fr, v0, ly, sg = nonfinite_inputs(c)
    return chk.atrous_variance(fr, v0, ly, sg, passes=c[2], first_pass=c[1], sigma_lum=4.0, epsilon=1e-3)
