"""The contract of the median and the layer-weighted median (include/mi_denoise.h, section a4p) in NumPy float64, sort-based:

    C = the texel widened (uint8 -> the correctly rounded c / 255, float16 exactly); the taps q: the (2 radius + 1)^2 window, cut at the image
    w(q) = 1 without layers; else 2^arg, arg = -sum_l sum_xyz (G_l(p) sc_l - G_l(q) sc_l)^2 -- the guide values scaled in float32 as the
           kernel scales them (the fp32 product g * sc_l, sc_l = float32(sqrt(.5 log2 e) / sigma_l)), everything after that in float64;
           0 where that is not finite, and 0 below the float32 normal range (arg < -126)
    per channel c:  V = taps with C_c(q) finite and w(q) > 0;  W = sum_V w;  S_<=(v), S_<(v) = the sums over C_c(q) <= v, < v
    out_c = the smallest value of V with 2 S_<=(v) >= W;  V empty: C_c(p);  alpha passes through.

median() returns the output, and per pixel and channel the margin min(S_<=(v*) - W/2, W/2 - S_<(v*)) / W of the answer v* (inf where V
is empty) and whether every weight of the window is exactly 0 or 1 (then the fp32 sums are exact integers and so is the answer).
accept() holds a result to the acceptance rule of the header's precision clause.
"""
import numpy as np

from np_albedo import widen

F32 = np.float32
DELTA = 2.0 ** -16
LOG2E = 1.4426950408889634


def tap_stack(P, radius, fill):
    """(h, w, (2 radius + 1)^2): every tap of every pixel, rows top to bottom, a row left to right; `fill` outside the image."""
    h, w = P.shape
    Q = np.full((h + 2 * radius, w + 2 * radius), fill, P.dtype)
    Q[radius:radius + h, radius:radius + w] = P
    return np.stack([Q[j:j + h, i:i + w] for j in range(2 * radius + 1) for i in range(2 * radius + 1)], -1)


def scale_of(sigma):
    return F32(np.sqrt(0.5 * LOG2E) / np.float64(F32(sigma)))


def tap_args(layers, sigmas, radius, shape):
    """(h, w, T) float64: the exponent of every tap, NaN outside the image."""
    h, w = shape
    T = (2 * radius + 1) ** 2
    arg = np.zeros((h, w, T))
    with np.errstate(all="ignore"):
        for lyr, sigma in zip(layers, sigmas):
            gs = (widen(lyr)[..., :3] * scale_of(sigma)).astype(F32)          # the fp32 product, as the tile holds it
            for c in range(3):
                taps = tap_stack(gs[..., c], radius, F32(np.nan)).astype(np.float64)
                d = gs[..., c].astype(np.float64)[..., None] - taps
                arg -= d * d
    return arg


def tap_weights(layers, sigmas, radius, shape):
    """(h, w, T) float64: w(q); 0 outside the image."""
    h, w = shape
    if not layers:
        return np.isfinite(tap_stack(np.zeros((h, w)), radius, np.nan)).astype(np.float64)
    arg = tap_args(layers, sigmas, radius, shape)
    with np.errstate(all="ignore"):
        wt = np.exp2(arg)
    wt[~np.isfinite(wt) | ~(arg >= -126.0)] = 0.0
    return wt


def median(frame, layers=None, sigmas=None, radius=1):
    """(out float32 (h, w, 4), margin float64 (h, w, 3), exact bool (h, w, 3))."""
    C = widen(frame)
    h, w = C.shape[:2]
    wt = tap_weights(list(layers or []), list(sigmas or []), radius, (h, w))
    T = wt.shape[-1]
    out = C.copy()
    margin = np.full((h, w, 3), np.inf)
    exact = np.zeros((h, w, 3), bool)
    for c in range(3):
        vals = tap_stack(C[..., c], radius, F32(np.nan)).astype(np.float64)
        valid = np.isfinite(vals) & (wt > 0)
        ww = np.where(valid, wt, 0.0)
        vv = np.where(valid, vals, np.inf)
        order = np.argsort(vv, axis=-1, kind="stable")
        sv, sw = np.take_along_axis(vv, order, -1), np.take_along_axis(ww, order, -1)
        cs = np.cumsum(sw, -1)
        W = cs[..., -1]
        s_le, s_lt = cs.copy(), np.zeros_like(cs)
        for i in range(T - 2, -1, -1):
            s_le[..., i] = np.where(sv[..., i] == sv[..., i + 1], s_le[..., i + 1], cs[..., i])
        for i in range(1, T):
            s_lt[..., i] = np.where(sv[..., i] == sv[..., i - 1], s_lt[..., i - 1], cs[..., i - 1])
        ok = np.isfinite(sv) & (2.0 * s_le >= W[..., None])
        idx = np.argmax(ok, -1)[..., None]
        have = W > 0
        best = np.take_along_axis(sv, idx, -1)[..., 0]
        out[..., c] = np.where(have, best, C[..., c].astype(np.float64)).astype(F32)
        with np.errstate(all="ignore"):
            m = np.minimum(np.take_along_axis(s_le, idx, -1)[..., 0] - W / 2, W / 2 - np.take_along_axis(s_lt, idx, -1)[..., 0]) / W
        margin[..., c] = np.where(have, m, np.inf)
        exact[..., c] = ((ww == 0) | (ww == 1)).all(-1)
    return out, margin, exact


def same_values(a, b):
    """Element-wise: equal as values (+0 == -0), or both NaN."""
    a, b = np.asarray(a), np.asarray(b)
    with np.errstate(invalid="ignore"):
        return (a == b) | (np.isnan(a) & np.isnan(b))


def accept(got, frame, layers=None, sigmas=None, radius=1, delta=DELTA, ref=None):
    """The acceptance rule of section a4p for a float32 result `got`.  Returns a dict: `bad` (h, w, 3) bool -- pixel-channels that break
    it --, `near` the share of pixel-channels that were NOT held to the bits (margin <= delta and not exact), `worst` the smallest margin
    among those held to the bits by the margin rule, and `alpha_ok`.  ref: median(...)'s triple, to share it between tests."""
    out, margin, exact = ref if ref is not None else median(frame, layers, sigmas, radius)
    C = widen(frame)
    h, w = C.shape[:2]
    strict = exact | (margin > delta)
    bad = strict & ~same_values(got[..., :3], out[..., :3])
    if (~strict).any():
        wt = tap_weights(list(layers or []), list(sigmas or []), radius, (h, w))
        for c in range(3):
            loose = ~strict[..., c]
            if not loose.any():
                continue
            vals = tap_stack(C[..., c], radius, F32(np.nan)).astype(np.float64)[loose]
            wl = wt[loose]
            valid = np.isfinite(vals) & (wl > 0)
            ww = np.where(valid, wl, 0.0)
            g = got[..., c][loose].astype(np.float64)[:, None]
            is_tap = (valid & (vals == g)).any(-1)
            W = ww.sum(-1)
            s_le = np.where(valid & (vals <= g), ww, 0.0).sum(-1)
            s_lt = np.where(valid & (vals < g), ww, 0.0).sum(-1)
            good = is_tap & (s_lt <= (0.5 + delta) * W) & (s_le >= (0.5 - delta) * W)
            b = np.zeros((h, w), bool)
            b[loose] = ~good
            bad[..., c] |= b
    by_margin = strict & ~exact & np.isfinite(margin)
    return {"bad": bad, "near": float((~strict).mean()), "worst": float(margin[by_margin].min()) if by_margin.any() else np.inf,
            "alpha_ok": bool(same_values(got[..., 3], C[..., 3]).all())}
