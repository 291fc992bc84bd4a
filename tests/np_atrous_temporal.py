"""float64 checker of the a-trous filter over neighbouring frames, written from include/mi_denoise.h, section a4h (not from the
kernels):

    pass 0 (step 1) of output t, window lo = max(0, t - k) .. hi = min(n - 1, t + k), q = p + o, o = (i, j), |i|, |j| <= 2:
    w(p, f, o) = K(o) prod_l exp(-.5 |G[t][l](p) - G[f][l](q)|^2_rgb / sigma_l^2) [exp(-.5 |C[t](p) - C[f](q)|^2_rgb / colorSigma^2)]
    C_1(p)     = sum_f sum_o w C[f](q) / sum_f sum_o w        over the taps whose q lies inside the image
    passes 1 .. N-1: np_atrous_joint.atrous_joint on C_1 with frame t's layers, first_pass = 1

The sums of pass 0 run in np_atrous_joint.one_pass's order inside a frame, frames ascending, so that a window of one frame gives
np_atrous_joint.atrous_joint's float64 values exactly.
"""
import numpy as np

import np_atrous_joint as single


def temporal_pass(frames, layers, sigmas, t, k, color_sigma=0.0):
    """C_1 of output t as float64 [h, w, 4].  frames: n arrays [h, w, 4]; layers: n lists of L arrays [h, w, 4]."""
    n = len(frames)
    lo, hi = max(0, t - k), min(n - 1, t + k)
    Ct = single.widen(frames[t])
    h, w = Ct.shape[:2]
    assert len(layers[t]) == len(sigmas) >= 1
    Gt = np.concatenate([single.widen(g)[..., :3] / float(s) for g, s in zip(layers[t], sigmas)], -1)
    num, den = np.zeros((h, w, 4)), np.zeros((h, w))
    with np.errstate(all="ignore"):
        for f in range(lo, hi + 1):
            Cf = single.widen(frames[f])
            Gf = np.concatenate([single.widen(g)[..., :3] / float(s) for g, s in zip(layers[f], sigmas)], -1)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    y0, y1, x0, x1 = max(0, -j), min(h, h - j), max(0, -i), min(w, w - i)
                    if y0 >= y1 or x0 >= x1:
                        continue                                    # every such tap lies outside the image
                    p = (slice(y0, y1), slice(x0, x1))
                    q = (slice(y0 + j, y1 + j), slice(x0 + i, x1 + i))
                    arg = -0.5 * ((Gt[p] - Gf[q]) ** 2).sum(-1)
                    if color_sigma > 0:
                        arg = arg - 0.5 * ((Ct[p][..., :3] - Cf[q][..., :3]) ** 2).sum(-1) / float(color_sigma) ** 2
                    wt = single.K1[i + 2] * single.K1[j + 2] * np.exp(arg)
                    num[p] += wt[..., None] * Cf[q]
                    den[p] += wt
        return num / den[..., None]


def atrous_joint_temporal(frames, layers, sigmas, k, passes=5, color_sigma=0.0, first=0, count=None):
    """The float64 outputs [first, first + count), each [h, w, 4]."""
    n = len(frames)
    count = n - first if count is None else count
    out = []
    for t in range(first, first + count):
        level = temporal_pass(frames, layers, sigmas, t, k, color_sigma)
        if passes > 1:
            level = single.atrous_joint(level, layers[t], sigmas, passes=passes - 1, first_pass=1, color_sigma=color_sigma)
        out.append(level)
    return out
