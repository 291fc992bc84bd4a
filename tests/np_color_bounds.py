"""The contract of the neighbourhood colour box (include/mi_denoise.h, section a4m) in NumPy float64, written from the header:

    C = the texel widened (uint8 -> the correctly rounded c / 255, float16 exactly)
    valid q of p: the q of the (2 radius + 1)^2 window, centre INCLUDED, inside the image, whose R, G and B are all finite; n of them
    n == 0:   lo_rgb = -inf, hi_rgb = +inf
    else, per channel:  mu = (sum v) / n, rounded to float32;  var = (sum (v - mu)^2) / n;  sigma = sqrt(var)
              lo = mu - gamma sigma;  hi = mu + gamma sigma
    lo.w = hi.w = n

Validity and widening are taken as the kernel takes them (on the float32 values); gamma is the float32 the kernel reads.  The sums,
the deviations, the square root and the two products are float64.  color_bounds returns float64 planes and, on request, the scale
|mu| + gamma sigma of the GPU tests' tolerance.
"""
import numpy as np

from np_albedo import widen


def _windows(P, radius, h, w):
    return [P[radius + j:radius + j + h, radius + i:radius + i + w] for j in range(-radius, radius + 1) for i in range(-radius, radius + 1)]


def color_bounds(frame, radius=1, gamma=1.0, scale=None):
    """(lo, hi): float64 (h, w, 4).  scale: a dict that receives "scale", the float64 (h, w, 3) plane |mu| + gamma sigma (0 where
    n == 0), and "n"."""
    assert radius in (1, 2)
    C = widen(frame)
    h, w = C.shape[:2]
    g = float(np.float32(gamma))
    valid = np.isfinite(C[..., :3]).all(-1)
    V = np.zeros((h + 2 * radius, w + 2 * radius, 3))
    M = np.zeros((h + 2 * radius, w + 2 * radius))
    V[radius:radius + h, radius:radius + w] = np.where(valid[..., None], C[..., :3], np.float32(0)).astype(np.float64)
    M[radius:radius + h, radius:radius + w] = valid
    n = sum(_windows(M, radius, h, w))
    nn = np.maximum(n, 1)[..., None]
    mu = (sum(_windows(V, radius, h, w)) / nn).astype(np.float32).astype(np.float64)
    var = sum(m[..., None] * (v - mu) ** 2 for v, m in zip(_windows(V, radius, h, w), _windows(M, radius, h, w))) / nn
    sigma = np.sqrt(var)
    lo, hi = np.empty((h, w, 4)), np.empty((h, w, 4))
    none = (n == 0)[..., None]
    lo[..., :3] = np.where(none, -np.inf, mu - g * sigma)
    hi[..., :3] = np.where(none, np.inf, mu + g * sigma)
    lo[..., 3] = hi[..., 3] = n
    if scale is not None:
        scale["scale"] = np.where(none, 0.0, np.abs(mu) + g * sigma)
        scale["n"] = n
    return lo, hi


def color_bounds_loop(frame, radius=1, gamma=1.0):
    """The same, one pixel at a time with nothing vectorised: what test_color_bounds_checker.py holds color_bounds to."""
    C = widen(frame)
    h, w = C.shape[:2]
    g = float(np.float32(gamma))
    lo, hi = np.empty((h, w, 4)), np.empty((h, w, 4))
    for y in range(h):
        for x in range(w):
            vs = []
            for j in range(-radius, radius + 1):
                for i in range(-radius, radius + 1):
                    qy, qx = y + j, x + i
                    if 0 <= qy < h and 0 <= qx < w and all(abs(float(c)) < np.inf for c in C[qy, qx, :3]):
                        vs.append([float(c) for c in C[qy, qx, :3]])
            n = len(vs)
            lo[y, x, 3] = hi[y, x, 3] = n
            for c in range(3):
                if n == 0:
                    lo[y, x, c], hi[y, x, c] = -np.inf, np.inf
                    continue
                mu = float(np.float32(sum(v[c] for v in vs) / n))
                sigma = (sum((v[c] - mu) ** 2 for v in vs) / n) ** 0.5
                lo[y, x, c], hi[y, x, c] = mu - g * sigma, mu + g * sigma
    return lo, hi
