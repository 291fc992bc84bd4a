"""The contract of the image quality metrics (include/mi_denoise.h, section a4n) in NumPy float64, written from the header:

    C = the texel widened (uint8 -> the correctly rounded c / 255, float16 exactly), then float64;  VALID(p): R, G, B of a(p) and b(p) finite
    pointwise, over VALID pixels, d_c = a_c - b_c:  n_valid, n_invalid, sum d_c^2, sum |d_c|, max |d_c|, sum d_c^2 / (b_c^2 + eps)
    SSIM on l() = lum32 (a4i's FMA chain in float32, bit-true), widened:  window |i|, |j| <= 5, taps inside the image and VALID,
        w = g_|i| g_|j|, g_k = exp(-k^2 / 4.5);  W = sum w;  mu_a = sum w la / W;  S_aa = sum w la^2 / W - mu_a^2;  S_ab = sum w la lb / W - mu_a mu_b
        ssim = (2 mu_a mu_b + C1)(2 S_ab + C2) / ((mu_a^2 + mu_b^2 + C1)(S_aa + S_bb + C2)),  C1 = (0.01 peak)^2, C2 = (0.03 peak)^2

Luminance is taken in float32 the kernel's way; everything after that is float64 with plain 2-D window sums (121 shifted planes added
in row-major order).  peak and eps are rounded to float32 first, as the C struct holds them.
"""
import math

import numpy as np

from np_albedo import widen
from np_temporal_accumulate_exact import lum32

R = 5
G = np.array([math.exp(-k * k / 4.5) for k in range(R + 1)])          # the six constants MID_METRICS_G0 .. G5
N_SUMS = 16
I_VALID, I_INVALID, I_SQ, I_ABS, I_MAX, I_REL, I_SSIM = 0, 1, 2, 5, 8, 9, 12


def _shifted(P, j, i, h, w):
    return P[R + j:R + j + h, R + i:R + i + w]


def window_sums(planes, weight_ok):
    """sum over the 11 x 11 window of w(q) * plane(q) for every plane, w = 0 where weight_ok is False or q is outside the image."""
    h, w = weight_ok.shape
    pad = [np.zeros((h + 2 * R, w + 2 * R)) for _ in planes]
    for P, x in zip(pad, planes):
        P[R:R + h, R:R + w] = np.where(weight_ok, x, 0.0)
    out = [np.zeros((h, w)) for _ in planes]
    for j in range(-R, R + 1):
        for i in range(-R, R + 1):
            g = G[abs(i)] * G[abs(j)]
            for o, P in zip(out, pad):
                o += g * _shifted(P, j, i, h, w)
    return out


def window_max(x, weight_ok):
    h, w = weight_ok.shape
    P = np.zeros((h + 2 * R, w + 2 * R))
    P[R:R + h, R:R + w] = np.where(weight_ok, x, 0.0)
    out = np.zeros((h, w))
    for j in range(-R, R + 1):
        for i in range(-R, R + 1):
            out = np.maximum(out, _shifted(P, j, i, h, w))
    return out


def image_metrics(a, b, peak=1.0, eps=1e-2, ssim=True):
    """A dict: `sums` (16 float64, the header's order), `valid` (h, w) bool, the derived values under the names of
    mid_image_metrics_result and, with ssim, `map` (float64 (h, w), NaN where the pixel is not valid), `s_ab` (the covariance, likewise)
    and `M` (float64 (h, w): the largest |l| of both images over the pixel's window -- the scale of the rounding error of its moments)."""
    A32, B32 = widen(a), widen(b)
    assert A32.shape == B32.shape and A32.ndim == 3 and A32.shape[2] == 4
    peak, eps = float(np.float32(peak)), float(np.float32(eps))
    A, B = A32[..., :3].astype(np.float64), B32[..., :3].astype(np.float64)
    valid = np.isfinite(A).all(-1) & np.isfinite(B).all(-1)
    sums = np.zeros(N_SUMS)
    sums[I_VALID], sums[I_INVALID] = valid.sum(), (~valid).sum()
    with np.errstate(all="ignore"):
        d = np.where(valid[..., None], A - B, 0.0)
        for c in range(3):
            dc, bc = d[..., c][valid], B[..., c][valid]
            sums[I_SQ + c] = math.fsum(dc * dc)
            sums[I_ABS + c] = math.fsum(np.abs(dc))
            sums[I_REL + c] = math.fsum(dc * dc / (bc * bc + eps))
        sums[I_MAX] = np.abs(d).max() if valid.any() else 0.0
    out = {"valid": valid}
    if ssim:
        with np.errstate(all="ignore"):
            la, lb = lum32(A32).astype(np.float64), lum32(B32).astype(np.float64)
            W, sa, sb, saa, sbb, sab = window_sums([np.ones_like(la), la, lb, la * la, lb * lb, la * lb], valid)
            Wd = np.where(valid, W, 1.0)
            mu_a, mu_b = sa / Wd, sb / Wd
            s_aa, s_bb, s_ab = saa / Wd - mu_a * mu_a, sbb / Wd - mu_b * mu_b, sab / Wd - mu_a * mu_b
            c1, c2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
            m = (2 * mu_a * mu_b + c1) * (2 * s_ab + c2) / ((mu_a * mu_a + mu_b * mu_b + c1) * (s_aa + s_bb + c2))
            out["map"] = np.where(valid, m, np.nan)
            out["s_ab"] = np.where(valid, s_ab, np.nan)
            out["M"] = window_max(np.maximum(np.abs(la), np.abs(lb)), valid)
        sums[I_SSIM] = math.fsum(m[valid])
    out["sums"] = sums
    out.update(derive(sums, peak, ssim))
    return out


def derive(sums, peak=1.0, ssim=True):
    """mid_image_metrics_derive, restated."""
    n, nan = sums[I_VALID], float("nan")
    peak = float(np.float32(peak))
    r = {"n_valid": float(n), "n_invalid": float(sums[I_INVALID]), "max_abs": float(sums[I_MAX])}
    if n == 0:
        r.update(mse=nan, mse_r=nan, mse_g=nan, mse_b=nan, mae=nan, psnr=nan, relmse=nan, ssim=nan)
        return r
    r["mse"] = (sums[I_SQ] + sums[I_SQ + 1] + sums[I_SQ + 2]) / (3.0 * n)
    r["mse_r"], r["mse_g"], r["mse_b"] = sums[I_SQ] / n, sums[I_SQ + 1] / n, sums[I_SQ + 2] / n
    r["mae"] = (sums[I_ABS] + sums[I_ABS + 1] + sums[I_ABS + 2]) / (3.0 * n)
    r["psnr"] = math.inf if r["mse"] == 0 else 10.0 * math.log10(peak * peak / r["mse"])
    r["relmse"] = (sums[I_REL] + sums[I_REL + 1] + sums[I_REL + 2]) / (3.0 * n)
    r["ssim"] = sums[I_SSIM] / n if ssim else nan
    return r


# ---- the tolerances of the GPU tests, as the header's precision statement derives them -------------------------------------------
def sum_rtol(n):
    """Every sum: all terms are >= 0 and each carries at most three roundings; the factor 8 is slack for the tree."""
    return (n + 8) * 2.0 ** -53 * 8


def ssim_atol(M, peak):
    """ssim(p): the rounding of a 121-term binary64 moment is about 1.5e-14 M^2, against a denominator >= C2 = 9e-4 peak^2."""
    return 1e-12 + 1e-10 * (np.asarray(M) / float(np.float32(peak))) ** 2
