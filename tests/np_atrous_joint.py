"""float64 checker of the edge-avoiding a-trous filter, written from include/mi_denoise.h, section a4g (not from the kernels):

    C_0 = the frame widened (RGBA8 texels c / 255);  k1 = (1, 4, 6, 4, 1) / 16,  K(o) = k1[i + 2] k1[j + 2]
    pass i, step s = 2^i, q = p + s o, o = (i, j), |i|, |j| <= 2:
    w(p, o)    = K(o) prod_l exp(-.5 |G_l(p) - G_l(q)|^2_rgb / sigma_l^2) [exp(-.5 |C_i(p) - C_i(q)|^2_rgb / (colorSigma 2^-i)^2)]
    C_{i+1}(p) = sum_o w C_i(q) / sum_o w          over the taps whose q lies inside the image (the others are skipped)

Non-finite texels follow IEEE arithmetic, as NumPy's float64 does: the NaN mask of the result is the filter's.
"""
import numpy as np

K1 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0


def widen(a):
    a = np.asarray(a)
    return a.astype(np.float64) / 255.0 if a.dtype == np.uint8 else a.astype(np.float64)


def one_pass(C, G, sigmas, step, color_sigma):
    """One pass at `step` over the float64 level C [h, w, 4] with the float64 guides G (each [h, w, 3]); color_sigma: this pass's
    own colour sigma, 0 = no colour term."""
    h, w = C.shape[:2]
    num, den = np.zeros((h, w, 4)), np.zeros((h, w))
    Gs = np.concatenate([g / float(s) for g, s in zip(G, sigmas)], -1)      # every layer in units of its own sigma
    with np.errstate(all="ignore"):
        for j in range(-2, 3):
            for i in range(-2, 3):
                dy, dx = j * step, i * step
                y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
                if y0 >= y1 or x0 >= x1:
                    continue                                        # every such tap lies outside the image
                p = (slice(y0, y1), slice(x0, x1))
                q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                arg = -0.5 * ((Gs[p] - Gs[q]) ** 2).sum(-1)          # sum_l |G_l(p) - G_l(q)|^2 / sigma_l^2, all layers at once
                if color_sigma > 0:
                    arg = arg - 0.5 * ((C[p][..., :3] - C[q][..., :3]) ** 2).sum(-1) / float(color_sigma) ** 2
                wt = K1[i + 2] * K1[j + 2] * np.exp(arg)
                num[p] += wt[..., None] * C[q]
                den[p] += wt
        return num / den[..., None]


def atrous_joint(frame, layers, sigmas, passes=5, first_pass=0, color_sigma=0.0):
    """The float64 result [h, w, 4] of passes first_pass .. first_pass + passes - 1."""
    C = widen(frame)
    G = [widen(l)[..., :3] for l in layers]
    assert len(G) == len(sigmas) >= 1
    for i in range(first_pass, first_pass + passes):
        C = one_pass(C, G, sigmas, 2 ** i, float(color_sigma) * 2.0 ** -i if color_sigma > 0 else 0.0)
    return C


def reach_mask(seeds, passes, first_pass=0):
    """Pixels whose result can depend on a seed texel: the seeds dilated by the 5 x 5 stencil of every pass (bool [h, w])."""
    m = np.asarray(seeds, bool).copy()
    h, w = m.shape
    for i in range(first_pass, first_pass + passes):
        s, out = 2 ** i, m.copy()
        for j in range(-2, 3):
            for k in range(-2, 3):
                dy, dx = j * s, k * s
                y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
                if y0 < y1 and x0 < x1:
                    out[y0:y1, x0:x1] |= m[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        m = out
    return m
