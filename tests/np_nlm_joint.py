"""float64 NumPy restatement of joint layer-guided non-local means (mid_nlm_joint), written from the contract in
include/mi_denoise.h (section a4f), not from the kernel.  Sequence of n frames with L RGBA8 layers each, texels c/255, out-of-image
texels 0 in frames and guides:

    d_l(p,f,s) = sum_{q in [patch)^2} |G[t][l](p+q) - G[f][l](p+s+q)|^2_rgb
    w(p,f,s)   = exp(-sum_l d_l(p,f,s) / h_l^2)
    out_t(p)   = sum_{f,s} w * In_f(p+s) / sum_f (0.001 + sum_s w)        (magenta where the denominator is 0)

f = max(0,t-k) .. min(n-1,t+k).  Each d_l is a box sum of per-texel squared byte differences taken exactly in integers
(np_nlm_layers._box) and then scaled by 1/(255^2 h_l^2): the checker itself adds no rounding to d."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from np_nlm_layers import _as_f64, _box
from np_nlm_layers_temporal import _pad_guide, normalize


def _offsets(xp, tps, gps, scales, offs, h, w, P, plo, PW):
    num = np.zeros((h, w, 4))
    den = np.zeros((h, w))
    y0 = x0 = P + plo
    for sy, sx in offs:
        arg = np.zeros((h, w))
        for tp, gp, scale in zip(tps, gps, scales):
            a = tp[:, y0:y0 + h + PW - 1, x0:x0 + w + PW - 1]                          # the TARGET guide: never shifted
            b = gp[:, y0 + sy:y0 + sy + h + PW - 1, x0 + sx:x0 + sx + w + PW - 1]      # the NEIGHBOUR guide at p + s + q
            d = a - b
            arg += _box((d * d).sum(0), PW, h, w) * scale                              # exact integers, then one scale per layer
        wt = np.exp(arg)
        num += xp[P + sy:P + sy + h, P + sx:P + sx + w] * wt[..., None]
        den += wt
    return num, den


def pair_sums(target_layers, neighbour_layers, neighbour_in, hs, search, patch, threads=8):
    """(num [h, w, 4], den [h, w]) float64 of ONE neighbour frame, its 0.001 included."""
    x = _as_f64(neighbour_in)
    h, w, _ = x.shape
    slo, shi = search
    plo, phi = patch
    PW = phi - plo
    P = max(-plo, phi) + max(-slo, shi) + 1
    xp = np.pad(x, ((P, P), (P, P), (0, 0)))
    tps = [_pad_guide(g, P, h, w) for g in target_layers]
    gps = [_pad_guide(g, P, h, w) for g in neighbour_layers]
    scales = [-1.0 / (255.0 * 255.0) / (float(hl) ** 2) for hl in hs]
    offs = [(sy, sx) for sy in range(slo, shi) for sx in range(slo, shi)]
    n_t = max(1, min(threads, len(offs)))
    with ThreadPoolExecutor(n_t) as ex:
        parts = list(ex.map(lambda i: _offsets(xp, tps, gps, scales, offs[i::n_t], h, w, P, plo, PW), range(n_t)))
    num = np.zeros((h, w, 4))
    den = np.full((h, w), 0.001)                                   # nonlocal.comp:32-33, once per neighbour frame
    for pn, pd in parts:
        num += pn
        den += pd
    return num, den


def nlm_joint(frames, layers, hs, k, search, patch, first=0, count=None):
    """Outputs [first, first+count) as a list of [h, w, 4] float64; frames: n images, layers: n lists of L RGBA8 guides, hs: L
    values of h."""
    n = len(frames)
    assert len(layers) == n and all(len(ls) == len(hs) >= 1 for ls in layers)
    count = n - first if count is None else count
    h, w = np.asarray(frames[0]).shape[:2]
    outs = []
    for t in range(first, first + count):
        num = np.zeros((h, w, 4))
        den = np.zeros((h, w))
        for f in range(max(0, t - k), min(n - 1, t + k) + 1):
            pn, pd = pair_sums(layers[t], layers[f], frames[f], hs, search, patch)
            num += pn
            den += pd
        outs.append(normalize(num, den))
    return outs


# ---- the hand-derived known answer -----------------------------------------------------------------------------------------------
# Frame of constant colour C; layer 0 is 64 left of column EX and 192 from it on, layer 1 is 64 above row EY and 192 from it on;
# h_l = 0.02 for both, so one mismatching texel in a patch scales to 2^-(128^2 * 3 * log2(e) / (255^2 * 0.02^2)) < 2^-600, exactly 0 in
# fp32 and 1e-800 = 0 in float64; the out-of-image 0 matches neither value.  A window pixel then weighs 1 if its whole patch lies in
# the pixel's own quadrant and inside the image, else 0: out = C * n / (0.001 + n).
KA_W, KA_H, KA_EX, KA_EY, KA_HS = 61, 70, 30, 35, (0.02, 0.02)
KA_C = np.array([0.25, 0.5, 0.75, 1.0])


def known_answer_inputs():
    g0 = np.full((KA_H, KA_W, 4), 64, np.uint8)
    g0[:, KA_EX:, :3] = 192
    g1 = np.full((KA_H, KA_W, 4), 64, np.uint8)
    g1[KA_EY:, :, :3] = 192
    frame = np.broadcast_to(KA_C, (KA_H, KA_W, 4)).astype(np.float32).copy()
    return frame, [g0, g1]


def cnt(edge, size, coord, reach=10, margin=0):
    """Per axis: positions x' in [coord - reach, coord + reach] that lie in coord's own half (left of `edge` / from it on) and at
    least `margin` texels from the edge and from the border (margin = 3: a 7-wide patch around x' stays inside the half)."""
    lo = np.where(coord < edge, margin, edge + margin)
    hi = np.where(coord < edge, edge - 1 - margin, size - 1 - margin)
    return np.minimum(coord + reach, hi) - np.maximum(coord - reach, lo) + 1


def known_answer(patch):
    """(want [h, w, 4] float64, mask of the pixels it holds at) for search [-10, 11) and patch [0, 1) or [-3, 4)."""
    yy, xx = np.mgrid[0:KA_H, 0:KA_W]
    if tuple(patch) == (0, 1):
        n = cnt(KA_EX, KA_W, xx) * cnt(KA_EY, KA_H, yy)
        ok = np.ones((KA_H, KA_W), bool)
    else:
        assert tuple(patch) == (-3, 4)
        n = cnt(KA_EX, KA_W, xx, margin=3) * cnt(KA_EY, KA_H, yy, margin=3)
        # pixels whose own patch touches neither an edge nor the border (else the target patch matches nothing, or partly)
        ok = (np.abs(xx - KA_EX + 0.5) > 3.5) & (np.abs(yy - KA_EY + 0.5) > 3.5) & (xx >= 3) & (xx <= KA_W - 4) & (yy >= 3) & (yy <= KA_H - 4)
    return KA_C * (n / (0.001 + n))[..., None], ok, n
