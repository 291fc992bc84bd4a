"""Test-only float64 evaluation of the joint (cross) bilateral filter (mid_bilateral_joint), written from the formula in
include/mi_denoise.h, section a4e:

    w(p, f, o) = exp(-0.5 |o|^2 / ss^2) * prod_l exp(-0.5 |G[t][l](p) - G[f][l](p+o)|^2_rgb / sigma_l^2)
    out_t(p)   = sum_{f, o} w * In_f(p+o) / sum_{f, o} w          (magenta (1,0,1,1) where the denominator is 0)

f = max(0,t-k) .. min(n-1,t+k), o = (i, j) with |i|, |j| <= R, out-of-image texels vec4(0) in frames and guides.  It shares no
code with the kernels (fp32 LDS planes, exp2 with folded scales, one FMA chain): zero-padded images, one shifted slice per tap,
one exp per layer, NumPy float64.  IEEE all the way: exp(-inf) = 0, Inf - Inf = NaN, and a NaN weight poisons its pixel.
pair_sums is the tap loop of one neighbour frame, which joint_sums adds over a window; tests whose cases share (output, neighbour)
pairs call it directly, with planes of their own appended to the frame's channels.
"""
import math

import numpy as np

MAGENTA = np.array([1.0, 0.0, 1.0, 1.0])


def decode(a):
    """A frame or guide as the float32 texels the filter reads: uint8 -> c/255 (the correctly rounded fp32 quotient), float16
    widened, float32 as it is."""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a.astype(np.float32) / np.float32(255.0)
    return a.astype(np.float32)


def _pad(a, c, R):
    h, w = a.shape[:2]
    out = np.zeros((h + 2 * R, w + 2 * R, c), np.float64)
    out[R:R + h, R:R + w] = decode(a)[..., :c]
    return out


def _planes(a):
    """[h, w, 3] -> [3, h, w], one contiguous plane per channel: |difference|^2 is then three whole-plane products."""
    return np.ascontiguousarray(np.moveaxis(a, -1, 0))


def pair_sums(image, target_layers, layers, R, sigma_s, sigmas, into=None):
    """(num [h,w,C], den [h,w]), float64: the taps of ONE neighbour frame.  image: that frame, [h,w,C] with any C >= 1 -- the weights
    do not depend on it, so a caller may append planes of its own to the frame's four channels and get their sums from the same
    taps; target_layers: the output frame's L guide layers (the centres); layers: the neighbour's.  into: (num, den) to add to in
    place, so that joint_sums adds every tap of a window in one running sum."""
    C = np.asarray(image).shape[-1]
    h, w = np.asarray(image).shape[:2]
    L = len(target_layers)
    assert len(sigmas) == L == len(layers)
    num, den = (np.zeros((h, w, C)), np.zeros((h, w))) if into is None else into
    gt = [_planes(decode(g)[..., :3].astype(np.float64)) for g in target_layers]
    im = _pad(image, C, R)
    gn = [_planes(_pad(g, 3, R)) for g in layers]
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(-R, R + 1):
            for i in range(-R, R + 1):
                wt = np.full((h, w), math.exp(-0.5 * (i * i + j * j) / float(sigma_s) ** 2))
                for l in range(L):
                    d = gt[l] - gn[l][:, R + j:R + j + h, R + i:R + i + w]
                    d *= d
                    wt = wt * np.exp(-0.5 * (d[0] + d[1] + d[2]) / float(sigmas[l]) ** 2)
                num += im[R + j:R + j + h, R + i:R + i + w] * wt[..., None]
                den += wt
    return num, den


def joint_sums(frames, layers, t, k, R, sigma_s, sigmas):
    """(num [h,w,4], den [h,w]) of output t, float64."""
    n = len(frames)
    h, w = np.asarray(frames[0]).shape[:2]
    assert len(sigmas) == len(layers[t])
    into = np.zeros((h, w, 4)), np.zeros((h, w))
    for f in range(max(0, t - k), min(n - 1, t + k) + 1):
        pair_sums(np.asarray(frames[f])[..., :4], layers[t], layers[f], R, sigma_s, sigmas, into)
    return into


def bilateral_joint(frames, layers, sigmas, k, R, sigma_s, first=0, count=None):
    """Outputs [first, first+count) as float64 [h,w,4] arrays.  layers: one list of L guide layers per frame (uint8, float16 or
    float32); sigmas: L values."""
    n = len(frames)
    count = n - first if count is None else count
    outs = []
    for t in range(first, first + count):
        num, den = joint_sums(frames, layers, t, k, R, sigma_s, sigmas)
        with np.errstate(invalid="ignore", divide="ignore"):
            out = num / den[..., None]
        out[den == 0] = MAGENTA
        outs.append(out)
    return outs
