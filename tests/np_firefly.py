"""The contract of the firefly clamp (include/mi_denoise.h, section a4l) in NumPy float32, written from the header:

    C = the texel widened (uint8 -> the correctly rounded c / 255, float16 exactly);  l() = lum32, a4i's FMA chain bit-true
    valid neighbours of p: the q != p of the (2 radius + 1)^2 window inside the image with l(C(q)) finite; n of them
    n == 0:                out = C
    m = the min(rank, n)-th largest valid neighbour luminance (a multiset);  T = fmaxf(gain * m, floor)
    lc = l(C(p)) finite:   lc <= T: out = C;   lc > T: out_rgb = C_rgb * (T / lc)
    lc not finite:         out_rgb = (T, T, T)
    alpha passes through.

The selection is exact (a sort of float32 values); gain * m, T / lc and C_c * s are ONE float32 operation of NumPy each, so the
results are the bits the kernel must give (the library is built with -ffp-contract=off and without fast-math).
"""
import numpy as np

from np_albedo import widen
from np_temporal_accumulate_exact import lum32

F32 = np.float32


def neighbour_luminances(L, radius):
    """(h, w, (2 radius + 1)^2 - 1) float32: the luminance of every neighbour, -inf where it is outside the image or not finite."""
    h, w = L.shape
    P = np.full((h + 2 * radius, w + 2 * radius), -np.inf, np.float32)
    P[radius:radius + h, radius:radius + w] = np.where(np.isfinite(L), L, F32(-np.inf))
    taps = [P[radius + j:radius + j + h, radius + i:radius + i + w] for j in range(-radius, radius + 1) for i in range(-radius, radius + 1) if (i, j) != (0, 0)]
    return np.stack(taps, -1)


def firefly_clamp(frame, radius=1, rank=1, gain=1.0, floor=0.0, counts=None):
    """float32 (h, w, 4).  counts: a dict that receives the numbers of clamped, repaired and untouched pixels."""
    assert radius in (1, 2) and 1 <= rank <= 4
    C = widen(frame)
    with np.errstate(all="ignore"):
        L = lum32(C)
        nb = -np.sort(-neighbour_luminances(L, radius), axis=-1)         # descending; -inf last
        n = (nb > -np.inf).sum(-1)
        k = np.clip(np.minimum(rank, n) - 1, 0, None)
        m = np.take_along_axis(nb, k[..., None], -1)[..., 0]
        T = np.fmax(F32(gain) * m, F32(floor))
        have = n > 0
        fin = np.isfinite(L)
        clamp = have & fin & (L > T)
        repair = have & ~fin
        s = T / np.where(clamp, L, F32(1))
        out = C.copy()
        out[..., :3] = np.where(clamp[..., None], C[..., :3] * s[..., None], out[..., :3])
        out[..., :3] = np.where(repair[..., None], T[..., None], out[..., :3])
    if counts is not None:
        counts.update(clamped=int(clamp.sum()), repaired=int(repair.sum()), untouched=int((~clamp & ~repair).sum()), pixels=int(L.size))
    return out
