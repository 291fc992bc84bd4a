"""float64 checker of the recursive temporal accumulation, written from include/mi_denoise.h, section a4j (not from the kernel).

The previous position and its split are taken exactly as the header states them, in fp32, so that both sides take the same taps:

    ppx = fp32(x + mx),  x0 = floor(ppx),  fx = ppx - x0 (exact);  likewise y
    taps only where ppx > -1, ppx < width, ppy > -1, ppy < height (false for NaN and Inf)
    the four taps q = (x0 + a, y0 + b), b then a, bw = (a ? fx : 1 - fx) (b ? fy : 1 - fy); outside the image or bw == 0: skipped

Everything after that is float64:

    w  = bw prod_l exp(-.5 |Gcur_l(p) - Gprev_l(q)|^2_rgb / sigma_l^2)
    S  = sum w,  hc = sum w Hc(q),  h1, h2, hn = sum w Hs(q).{x, y, z};   S > 0: hc, h1, h2 /= S (hn is NOT divided), else 0
    N' = fmin(historyMax, hn + 1),  a = fmax(1 / N', alpha),  am = fmax(1 / N', alphaMoments)
    colour = hc + a (C - hc),  m1' = h1 + am (l - h1),  m2' = h2 + am (l^2 - h2),  state = (m1', m2', N', 0)
    Vt = max(0, m2' - m1'^2);  variance = Vs given ? Vs + fmin(1, (N' - 1) / (historyFull - 1)) (Vt - Vs) : Vt

alpha, alphaMoments, historyMax and historyFull are the fp32 values the parameter block holds.
"""
import numpy as np

from np_atrous_joint import widen
from np_atrous_variance import lum


def tap_geometry(h, w, motion):
    """The fp32 part: (ok, x0, y0, fx, fy) -- ok bool [h, w]; x0, y0 int64 (0 where not ok); fx, fy float32."""
    yy, xx = np.mgrid[0:h, 0:w]
    if motion is None:
        ppx, ppy = xx.astype(np.float32), yy.astype(np.float32)
    else:
        m = np.asarray(motion, np.float32)
        with np.errstate(all="ignore"):
            ppx = xx.astype(np.float32) + m[..., 0]
            ppy = yy.astype(np.float32) + m[..., 1]
    assert ppx.dtype == np.float32 and ppy.dtype == np.float32
    with np.errstate(invalid="ignore"):
        ok = (ppx > np.float32(-1)) & (ppx < np.float32(w)) & (ppy > np.float32(-1)) & (ppy < np.float32(h))
    ppx, ppy = np.where(ok, ppx, np.float32(0)), np.where(ok, ppy, np.float32(0))
    fx0, fy0 = np.floor(ppx), np.floor(ppy)
    fx, fy = ppx - fx0, ppy - fy0
    assert fx.dtype == np.float32
    return ok, fx0.astype(np.int64), fy0.astype(np.int64), fx, fy


def temporal_accumulate(frame, layers, prev_layers, sigmas, hist=None, motion=None, var_spatial=None, alpha=0.2, alpha_moments=0.2,
                        history_max=32, history_full=4):
    """dict of float64 arrays: colour [h, w, 4], state [h, w, 4], variance [h, w], S [h, w] (the weight the history met)."""
    C = widen(frame)
    h, w = C.shape[:2]
    l = lum(C)
    alpha, alpha_moments, history_max, history_full = (float(np.float32(v)) for v in (alpha, alpha_moments, history_max, history_full))
    assert len(layers) == len(prev_layers) == len(sigmas)
    S, hc, hs = np.zeros((h, w)), np.zeros((h, w, 4)), np.zeros((h, w, 3))
    with np.errstate(all="ignore"):
        if hist is not None:
            Hc, Hs = np.asarray(hist[0], np.float64), np.asarray(hist[1], np.float64)
            Gc = [widen(g)[..., :3] / float(np.float32(s)) for g, s in zip(layers, sigmas)]
            Gp = [widen(g)[..., :3] / float(np.float32(s)) for g, s in zip(prev_layers, sigmas)]
            ok, x0, y0, fx, fy = tap_geometry(h, w, motion)
            for b in (0, 1):
                for a in (0, 1):
                    wx32, wy32 = (fx if a else np.float32(1) - fx), (fy if b else np.float32(1) - fy)
                    bw32 = wx32 * wy32                                  # which taps are skipped is an fp32 statement
                    qx, qy = x0 + a, y0 + b
                    take = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h) & (bw32 != 0)
                    bw = (fx.astype(np.float64) if a else 1.0 - fx.astype(np.float64)) * (fy.astype(np.float64) if b else 1.0 - fy.astype(np.float64))
                    py, px = np.nonzero(take)
                    ty, tx = qy[take], qx[take]
                    arg = np.zeros(py.size)
                    for gc, gp in zip(Gc, Gp):
                        arg -= 0.5 * ((gc[py, px] - gp[ty, tx]) ** 2).sum(-1)
                    wt = bw[take] * np.exp(arg)
                    S[py, px] += wt
                    hc[py, px] += wt[:, None] * Hc[ty, tx]
                    hs[py, px] += wt[:, None] * Hs[ty, tx, :3]
        pos = S > 0
        Sd = np.where(pos, S, 1.0)
        hc = np.where(pos[..., None], hc / Sd[..., None], 0.0)
        h1, h2, hn = np.where(pos, hs[..., 0] / Sd, 0.0), np.where(pos, hs[..., 1] / Sd, 0.0), hs[..., 2]
        N = np.fmin(history_max, hn + 1.0)
        al, am = np.fmax(1.0 / N, alpha), np.fmax(1.0 / N, alpha_moments)
        colour = hc + al[..., None] * (C - hc)
        m1 = h1 + am * (l - h1)
        m2 = h2 + am * (l * l - h2)
        v = m2 - m1 * m1
        Vt = np.where(v < 0, 0.0, v)
        if var_spatial is not None:
            Vs = np.asarray(var_spatial, np.float64)
            tt = np.fmin(1.0, (N - 1.0) / (history_full - 1.0))
            var = Vs + tt * (Vt - Vs)
        else:
            var = Vt
    return {"colour": colour, "state": np.stack([m1, m2, N, np.zeros_like(N)], -1), "variance": var, "S": S}
