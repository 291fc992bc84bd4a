"""Exact integer answers of one a-trous pass (include/mi_denoise.h, sections a4g and a4h), and the inputs that have them.

The method.  A frame holds small integers.  Every guide plane takes two values, and sigma is 0.02: two texels either agree in every
plane, and the tap's weight is K(o) 2^0 = K(o) exactly, or differ by at least 1 = 50 sigma somewhere, and 2^arg is exactly 0 (in
fp32 and in float64 alike).  With k1 = (1, 4, 6, 4, 1), K(o) = k1[i] k1[j] / 256, so

    sum_o w C(q) = num / 256,   sum_o w = den / 256,   num = sum k1[i] k1[j] [accepted] C(q),   den = sum k1[i] k1[j] [accepted]

are integers over 256, far below 2^24: fp32 holds every partial sum exactly, in any order of accumulation.  The result of the
pass is therefore the correctly rounded fp32 quotient float32(num / 256) / float32(den / 256), the same bits in every kernel.
Nothing here is shared with np_atrous_joint.py: no exponential, no sigma, no floating-point sum.

A predicate says which taps are accepted.  It gets two index tuples (slices) of equal extent, the centres p and the taps q, and
returns a bool array; `equal_on` builds "agree in every given plane" from the arrays themselves.
"""
import functools

import numpy as np

K1 = np.array([1, 4, 6, 4, 1], np.int64)
SIGMA = 0.02                                   # of every layer, and colorSigma of the colour family
LOW_HIGH = ((0.0, 1.0), (0.25, 3.0))           # the two values of a float guide plane; plane 3 l + c takes pair (3 l + c) mod 2


def _ints(C):
    C = np.asarray(C)
    Ci = C.astype(np.int64)
    assert np.array_equal(Ci, C), "levels must hold integers"
    return Ci


def _taps(h, w, step, reverse):
    taps = [(j, i) for j in range(-2, 3) for i in range(-2, 3)]
    for j, i in (reversed(taps) if reverse else taps):
        dy, dx = j * step, i * step
        y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
        if y0 < y1 and x0 < x1:
            yield j, i, (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def pass_sums(C, same, step, reverse=False):
    """(num [h, w, 4], den [h, w], accepted, offered): the int64 sums of one pass, and how many in-image non-centre taps the
    predicate accepted out of how many there are."""
    Ci = _ints(C)
    h, w = Ci.shape[:2]
    num, den = np.zeros((h, w, 4), np.int64), np.zeros((h, w), np.int64)
    accepted = offered = 0
    for j, i, p, q in _taps(h, w, step, reverse):
        ok = same(p, q)
        kk = K1[i + 2] * K1[j + 2]
        num[p] += kk * ok[..., None] * Ci[q]
        den[p] += kk * ok
        if (j, i) != (0, 0):
            accepted += int(ok.sum())
            offered += ok.size
    return num, den, accepted, offered


def quotient(num, den):
    """float32(num / 256) / float32(den / 256): one IEEE fp32 division per channel, both operands exact."""
    assert 0 <= num.min() and num.max() < 2 ** 24 and 0 < den.min() and den.max() < 2 ** 24
    n = (num / 256.0).astype(np.float32)
    d = (den / 256.0).astype(np.float32)
    assert np.array_equal(n.astype(np.float64) * 256, num) and np.array_equal(d.astype(np.float64) * 256, den)
    return n / d[..., None]


def exact_pass(C, same, step, reverse=False):
    """The float32 result [h, w, 4] of one pass at `step` over the integer level C [h, w, 4]."""
    num, den, _, _ = pass_sums(C, same, step, reverse)
    return quotient(num, den)


def temporal_sums(frames, accepted, t, k, reverse=False):
    """pass_sums over the window of output t; accepted(f, p, q): centres p of frame t against taps q of frame f."""
    n = len(frames)
    lo, hi = max(0, t - k), min(n - 1, t + k)
    h, w = np.asarray(frames[t]).shape[:2]
    num, den = np.zeros((h, w, 4), np.int64), np.zeros((h, w), np.int64)
    acc = off = 0
    window = range(lo, hi + 1)
    for f in (reversed(window) if reverse else window):
        Ci = _ints(frames[f])
        for j, i, p, q in _taps(h, w, 1, reverse):
            ok = accepted(f, p, q)
            kk = K1[i + 2] * K1[j + 2]
            num[p] += kk * ok[..., None] * Ci[q]
            den[p] += kk * ok
            if (f, j, i) != (t, 0, 0):
                acc += int(ok.sum())
                off += ok.size
    return num, den, acc, off


def exact_temporal_pass(frames, accepted, t, k, reverse=False):
    """The float32 result of pass 0 of output t over the frames t - k .. t + k."""
    num, den, _, _ = temporal_sums(frames, accepted, t, k, reverse)
    return quotient(num, den)


# ---- predicates ----------------------------------------------------------------------------------------------------------------------
def _keys(stacks):
    """One integer per texel, equal for two texels (of any of the stacks) exactly where every plane agrees."""
    flat = np.concatenate([s.reshape(-1, s.shape[-1]) for s in stacks])
    inv, radix = np.zeros(len(flat), np.int64), 1
    for m in range(flat.shape[1]):                                  # mixed radix over the planes: a plane's digit is the rank of its value
        vals, digit = np.unique(flat[:, m], return_inverse=True)
        inv = inv * len(vals) + digit.reshape(-1)
        radix *= len(vals)
    assert radix < 2 ** 62
    out, at = [], 0
    for s in stacks:
        out.append(inv[at:at + s.shape[0] * s.shape[1]].reshape(s.shape[:2]))
        at += s.shape[0] * s.shape[1]
    return out


def _planes(layers, colour):
    parts = [np.asarray(l)[..., :3].astype(np.float64) for l in layers]
    if colour is not None:
        parts.append(np.asarray(colour)[..., :3].astype(np.float64))
    return np.concatenate(parts, -1)


def equal_on(layers, colour=None):
    """same(p, q) of one frame: the x, y, z planes of every layer agree, and with `colour` its r, g, b too (never its alpha)."""
    (key,) = _keys([_planes(layers, colour)])
    return lambda p, q: key[p] == key[q]


def equal_across(layers, t, colours=None):
    """accepted(f, p, q) of a sequence for output t; layers: [frame][layer], colours: the frames or None."""
    keys = _keys([_planes(layers[f], None if colours is None else colours[f]) for f in range(len(layers))])
    return lambda f, p, q: keys[t][p] == keys[f][q]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def int_frame(shape, seed=1, dtype=np.float32):
    """Integers 0 .. 15 in every channel: exact in float32 and in float16."""
    return np.random.default_rng(seed).integers(0, 16, shape + (4,)).astype(dtype)


@functools.lru_cache(maxsize=None)
def label_bits(shape, planes, frame=0, seed=5):
    """bool [planes, h, w].  Plane m is low except for one block and some isolated texels, both of its own size, place and seed:
    an isolated texel accepts no tap but itself at any step, a block decides by where the tap lands.  Their number shrinks with
    the number of planes of the input set, so that the share of accepted taps stays away from 0 and from 1 for 3 planes and for
    48.  Frame f sees the pattern moved by (f, 2 f) texels (down, right)."""
    h, w = shape
    pad = 16
    H, W = h + 2 * pad, w + 2 * pad
    out = np.zeros((planes, h, w), bool)
    for m in range(planes):
        rng = np.random.default_rng([seed, planes, m])
        canvas = np.zeros((H, W), bool)
        side = 0.55 * np.sqrt(h * w / planes)                       # the blocks of all planes cover about 0.3 of the frame
        bh = int(np.clip(round(side * (0.7 + 0.15 * (m % 5))), 1, h))
        bw = int(np.clip(round(side * (1.3 - 0.15 * (m % 5))), 1, w))
        by, bx = pad + rng.integers(0, h - bh + 1), pad + rng.integers(0, w - bw + 1)
        canvas[by:by + bh, bx:bx + bw] = True
        n_iso = max(2, int(round(0.1 * h * w / planes)))            # about 0.1 of the texels are isolated in some plane
        canvas[rng.integers(0, H, n_iso), rng.integers(0, W, n_iso)] ^= True
        out[m] = canvas[pad - frame:pad - frame + h, pad - 2 * frame:pad - 2 * frame + w]
    out.setflags(write=False)
    return out


def label_layers(shape, L, dtype, frame=0, seed=5):
    """L guide layers [h, w, 4] of `dtype` with label_bits' planes: 0 / 255 as uint8, LOW_HIGH's pairs as float16 / float32.  Alpha
    holds finite values of every size; no filter may look at it."""
    return layers_from_bits(label_bits(shape, 3 * L, frame, seed), dtype, frame, seed)


def colour_frame(shape, L, seed=1, dtype=np.float32, frame=0):
    """The colour family's frame: rgb small integers, constant but for blocks and isolated texels (three more planes of
    label_bits' kind, drawn together with the 3 L label planes), alpha random 0 .. 15 per texel."""
    h, w = shape
    b = label_bits(shape, 3 * L + 3, frame, seed + 100)[3 * L:]
    fr = np.empty((h, w, 4), dtype)
    for c, (lo, hi) in enumerate(((3, 9), (5, 2), (1, 12))):
        fr[..., c] = np.where(b[c], hi, lo)
    fr[..., 3] = np.random.default_rng([seed, 7, frame]).integers(0, 16, (h, w))
    return fr


def colour_layers(shape, L, dtype, frame=0, seed=1):
    """The colour family's layers: the first 3 L of its 3 L + 3 planes."""
    return layers_from_bits(label_bits(shape, 3 * L + 3, frame, seed + 100)[:3 * L], dtype, frame, seed + 100)


def layers_from_bits(bitsv, dtype, frame=0, seed=5):
    """Guide layers [h, w, 4] of `dtype` from bool planes [3 L, h, w]."""
    L = bitsv.shape[0] // 3
    h, w = bitsv.shape[1:]
    rng = np.random.default_rng([seed, 99, frame])
    out = []
    for l in range(L):
        g = np.empty((h, w, 4), dtype)
        for c in range(3):
            if np.dtype(dtype) == np.uint8:
                g[..., c] = np.where(bitsv[3 * l + c], 255, 0)
            else:
                lo, hi = LOW_HIGH[(3 * l + c) % 2]
                g[..., c] = np.where(bitsv[3 * l + c], hi, lo)
        if np.dtype(dtype) == np.uint8:
            g[..., 3] = rng.integers(0, 256, (h, w))
        else:
            g[..., 3] = rng.choice(np.array([-60000.0, -7.5, 0.0, 0.3, 1.0, 1000.0, 65000.0]), (h, w))
        out.append(g)
    return out


# ---- the input sets of tests/test_gpu_atrous_exact.py (test_atrous_exact_reference.py holds every one of them to its conditions) -------
FRAME = (261, 131)                             # rows x columns: a second row-comb chunk at steps 16 and 32, three tile columns
SMALL = ((1, 1), (5, 7), (33, 130))
SMALL_PASSES = (0, 1, 3)                       # steps 1, 2 and 8
WIDE = (259, 258)                              # the smallest kind of frame in which all 25 taps of step 128 lie inside the image somewhere
WIDE_PASSES = (6, 7)                           # steps 64 and 128
WIDE_LAYERS = (3, 5)                           # global taps below and above four layers
LAYERS = (1, 2, 3, 4, 5, 16)
COLOUR_LAYERS = (1, 4, 5)
T_SHAPES = ((35, 130), (21, 70))
T_FRAMES = 4
T_K = (1, 2)


def single_inputs(shape, L, colour=False, fdt=np.float32, gdt=np.float32):
    """(frame, layers) of one single-frame input set in the given frame and guide dtypes: the same integers and the same
    pattern in every dtype, hence one answer."""
    if colour:
        return colour_frame(shape, L, dtype=fdt), colour_layers(shape, L, gdt)
    return int_frame(shape, dtype=fdt), label_layers(shape, L, gdt)


@functools.lru_cache(maxsize=None)
def single_predicate(shape, L, colour=False):
    fr, ly = single_inputs(shape, L, colour)
    return equal_on(ly, fr if colour else None)


@functools.lru_cache(maxsize=None)
def single_answer(shape, L, colour, step):
    return exact_pass(single_inputs(shape, L, colour)[0], single_predicate(shape, L, colour), step)


def temporal_inputs(shape, L, fdt=np.float32, gdt=np.float32):
    """(frames, layers[frame][layer]) of one sequence: T_FRAMES frames of their own integers, the label pattern moving with the frame."""
    return ([int_frame(shape, seed=20 + f, dtype=fdt) for f in range(T_FRAMES)],
            [label_layers(shape, L, gdt, frame=f) for f in range(T_FRAMES)])


@functools.lru_cache(maxsize=None)
def temporal_answer(shape, L, t, k):
    fr, ly = temporal_inputs(shape, L)
    return exact_temporal_pass(fr, equal_across(ly, t), t, k)
