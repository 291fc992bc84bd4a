"""float64 checker of the variance-guided a-trous filter, written from include/mi_denoise.h, section a4i (not from the kernels).

    l(C) = 0.2126 r + 0.7152 g + 0.0722 b        (the header's fp32 constants, widened)

(1) moments of output frame t over the frames f = max(0, t - k) .. min(n - 1, t + k), a 7 x 7 neighbourhood in each, q = p + o:
    w  = prod_l exp(-.5 |G[t][l](p) - G[f][l](q)|^2_rgb / sigma_l^2),   d = l(C[f](q)) - l(C[t](p)),   in-image taps only
    W  = sum w,  m = sum w d / W,  M2 = sum w d^2 / W,  V_0 = max(0, M2 - m^2)

(2) pass i, step s = 2^i, over the level C_i and the variance plane V_i, q = p + s o, |i|, |j| <= 2:
    vt(p) = 3 x 3 Gaussian (1, 2, 1)^2 / 16 of V_i at step 1 over the in-image taps, normalized by the weights met
    w     = K(o) prod_l exp(-.5 |G_l(p) - G_l(q)|^2 / sigma_l^2) [sigma_lum > 0:  exp(-|l(C_i(p)) - l(C_i(q))| / (sigma_lum sqrt(vt(p)) + epsilon))]
    C_{i+1} = sum w C_i(q) / sum w,    V_{i+1} = sum w^2 V_i(q) / (sum w)^2

round32=True rounds every level and variance plane to fp32 after each pass: the difference to the plain float64 run says how
far the rounding of the levels alone moves the result of the formula, that is how well-posed an input is for an fp32 filter.
"""
import numpy as np

from np_atrous_joint import K1, widen

LR, LG, LB = (float(np.float32(c)) for c in (0.2126, 0.7152, 0.0722))


def lum(C):
    return LR * C[..., 0] + LG * C[..., 1] + LB * C[..., 2]


def _shifted(h, w, dy, dx):
    """(p, q): index tuples of the centres whose tap p + (dy, dx) lies inside the image, and of those taps; None if there are none."""
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def _scaled(layers, sigmas):
    return np.concatenate([widen(g)[..., :3] / float(s) for g, s in zip(layers, sigmas)], -1)


def moments(frames, layers, sigmas, k=0, t=0):
    """(V_0, M2), float64 [h, w] each.  layers[f][l]."""
    n = len(frames)
    lo, hi = max(0, t - k), min(n - 1, t + k)
    Lt = lum(widen(frames[t]))
    Gt = _scaled(layers[t], sigmas)
    h, w = Lt.shape
    W, s1, s2 = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
    with np.errstate(all="ignore"):
        for f in range(lo, hi + 1):
            Lf = lum(widen(frames[f]))
            Gf = _scaled(layers[f], sigmas)
            for j in range(-3, 4):
                for i in range(-3, 4):
                    pq = _shifted(h, w, j, i)
                    if pq is None:
                        continue
                    p, q = pq
                    wt = np.exp(-0.5 * ((Gt[p] - Gf[q]) ** 2).sum(-1))
                    d = Lf[q] - Lt[p]
                    W[p] += wt
                    s1[p] += wt * d
                    s2[p] += wt * d * d
        m, M2 = s1 / W, s2 / W
        v = M2 - m * m
        return np.where(v < 0, 0.0, v), M2


def smooth_variance(V):
    """vt: the 3 x 3 Gaussian of V over the in-image taps."""
    h, w = V.shape
    num, den = np.zeros((h, w)), np.zeros((h, w))
    g = (0.25, 0.5, 0.25)
    for j in range(-1, 2):
        for i in range(-1, 2):
            pq = _shifted(h, w, j, i)
            if pq is None:
                continue
            p, q = pq
            num[p] += g[j + 1] * g[i + 1] * V[q]
            den[p] += g[j + 1] * g[i + 1]
    return num / den


def one_pass(C, V, Gs, step, sigma_lum, epsilon):
    """One pass at `step`: (C', V').  Gs: every layer in units of its own sigma, concatenated [h, w, 3 L]."""
    h, w = V.shape
    num, den, nv = np.zeros((h, w, 4)), np.zeros((h, w)), np.zeros((h, w))
    with np.errstate(all="ignore"):
        if sigma_lum > 0:
            Lc = lum(C)
            inv = 1.0 / (float(sigma_lum) * np.sqrt(smooth_variance(V)) + float(epsilon))
        for j in range(-2, 3):
            for i in range(-2, 3):
                pq = _shifted(h, w, j * step, i * step)
                if pq is None:
                    continue                                        # every such tap lies outside the image
                p, q = pq
                arg = -0.5 * ((Gs[p] - Gs[q]) ** 2).sum(-1)
                if sigma_lum > 0:
                    arg = arg - np.abs(Lc[p] - Lc[q]) * inv[p]
                wt = K1[i + 2] * K1[j + 2] * np.exp(arg)
                num[p] += wt[..., None] * C[q]
                den[p] += wt
                nv[p] += wt * wt * V[q]
        return num / den[..., None], nv / (den * den)


def atrous_variance(frame, variance, layers, sigmas, passes=5, first_pass=0, sigma_lum=4.0, epsilon=1e-3, round32=False, levels=None):
    """(C, V) in float64 after passes first_pass .. first_pass + passes - 1.  levels: a list that receives (C, V) after every pass."""
    C = widen(frame)
    V = np.asarray(variance, np.float64)
    assert len(layers) == len(sigmas) >= 1
    Gs = _scaled(layers, sigmas)
    for i in range(first_pass, first_pass + passes):
        C, V = one_pass(C, V, Gs, 2 ** i, float(sigma_lum), float(epsilon))
        if round32:
            C, V = C.astype(np.float32).astype(np.float64), V.astype(np.float32).astype(np.float64)
        if levels is not None:
            levels.append((C, V))
    return C, V
