"""float64 checker of the accumulation with a clip box (include/mi_denoise.h, section a4m: mid_temporal_accumulate_clip), written
from the header.  It WRAPS tests/np_temporal_accumulate.py, which it imports and does not restate: that checker is called three
times, and only the clip itself -- step 2 of the issue, four lines -- is evaluated here.

    1. the normalised history sums hc, h1, h2 (and S).  The wrapped checker is called with an all-zero frame, alpha = alphaMoments
       = 0, historyMax = 1e30 and the history's N plane replaced by 1e300: N' is then 1e30 wherever a tap is taken, both blend
       factors are 1e-30, and colour = hc (1 - 1e-30), m1' = h1 (1 - 1e-30), m2' = h2 (1 - 1e-30) -- hc, h1, h2 to the last bit
       of a float64.  Where no tap is taken N' = 1, both factors are 1 and the three are the frame's zeros, which is what a4j's
       step 4 makes of them.
    2. the unnormalised hn.  The wrapped checker is called with the true history and historyMax = 1e30: hn = N' - 1.
    3. the clip, in float64, the clip planes taken as the fp32 values given, where S > 0:
           hc' = hc < lo ? lo : (hc > hi ? hi : hc);  d = l(hc') - l(hc);  h1' = h1 + d;  h2' = h2 + d (2 h1 + d)
    4. steps 5 - 8 of a4j on hc', h1', h2', hn.  The wrapped checker is called with the true frame and parameters, NO layers, NO
       motion, and (hc', (h1', h2', hn, 0)) as its history: every pixel then takes the one tap q = p with weight exactly 1, so its
       normalised sums are the planes given and its hn is the hn given.  (A pixel that had S == 0 arrives with all-zero sums, as in
       step 4 of a4j.)

clip_lo == clip_hi == None is the wrapped checker itself, once.
"""
import numpy as np

from np_atrous_variance import lum
from np_temporal_accumulate import temporal_accumulate as unclipped


def temporal_accumulate_clip(frame, layers, prev_layers, sigmas, hist=None, motion=None, var_spatial=None, alpha=0.2, alpha_moments=0.2,
                             history_max=32, history_full=4, clip_lo=None, clip_hi=None):
    """The wrapped checker's dict, and "clipped": bool [h, w, 3], the channels the clip moved."""
    kw = dict(var_spatial=var_spatial, alpha=alpha, alpha_moments=alpha_moments, history_max=history_max, history_full=history_full)
    if clip_lo is None and clip_hi is None or hist is None:
        assert (clip_lo is None) == (clip_hi is None)
        out = unclipped(frame, layers, prev_layers, sigmas, hist=hist, motion=motion, **kw)
        out["clipped"] = np.zeros(out["colour"].shape[:2] + (3,), bool)
        return out
    lo, hi = (np.asarray(a, np.float32).astype(np.float64)[..., :3] for a in (clip_lo, clip_hi))
    Hc, Hs = np.asarray(hist[0], np.float64), np.asarray(hist[1], np.float64)
    zero = np.zeros(Hc.shape, np.float32)
    long = Hs.copy()
    long[..., 2] = 1e300
    sums = unclipped(zero, layers, prev_layers, sigmas, hist=(Hc, long), motion=motion, alpha=0.0, alpha_moments=0.0, history_max=1e30)
    S = sums["S"]
    hc, h1, h2 = sums["colour"], sums["state"][..., 0], sums["state"][..., 1]
    hn = unclipped(zero, layers, prev_layers, sigmas, hist=(Hc, Hs), motion=motion, alpha=0.0, alpha_moments=0.0, history_max=1e30)["state"][..., 2] - 1.0
    with np.errstate(invalid="ignore"):
        rgb = hc[..., :3]
        cl = np.where(rgb < lo, lo, np.where(rgb > hi, hi, rgb))                # a NaN hc stays NaN; a NaN bound clips nothing
        cl = np.where((S > 0)[..., None], cl, rgb)
        d = lum(cl) - lum(rgb)
    hc2 = np.concatenate([cl, hc[..., 3:]], -1)
    st2 = np.stack([h1 + d, h2 + d * (2.0 * h1 + d), hn, np.zeros_like(hn)], -1)
    out = unclipped(frame, [], [], [], hist=(hc2, st2), motion=None, **kw)
    out["S"] = S
    out["clipped"] = cl != rgb
    return out
