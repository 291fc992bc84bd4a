"""float64 NumPy restatement of layer-guided non-local means over neighbouring frames (mid_nlm_layers_pair_accum /
mid_nlm_layers_temporal), written from the contract in include/mi_denoise.h, not from the kernel.  One accumulate dispatch with a
target guide Gt, a neighbour guide Gn (RGBA8, texels c/255) and a neighbour colour image In, out-of-image texels 0 everywhere, is

    d(p,s) = sum_{q in [patch)^2} |Gt(p+q) - Gn(p+s+q)|^2_rgb,   w = exp(-d / h^2)
    num[p] += w * In(p+s)   (all four channels),   den[p] += w,   plus 0.001 once per dispatch,

and output t of a sequence with L layers per frame is: zero sums; for each neighbour f = max(0,t-k) .. min(n-1,t+k) and inside it
each layer l = 0..L-1 one dispatch with Gt = layer[t][l], Gn = layer[f][l], In = frame[f]; then num / den (magenta where den ==
0).  The patch distance of each search offset is a box sum of per-texel squared byte differences taken exactly in integers
(np_nlm_layers._box), then scaled by 1/255^2: the checker itself adds no rounding to d."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from np_nlm_layers import _as_f64, _box


def _pad_guide(g, P, h, w):
    g = np.asarray(g)
    assert g.dtype == np.uint8 and g.shape == (h, w, 4), "guide layers are RGBA8 of the image's size"
    return np.pad(np.moveaxis(g[..., :3], -1, 0).astype(np.int32), ((0, 0), (P, P), (P, P)))


def _offsets(xp, tp, gp, offs, h, w, P, plo, PW, scale):
    num = np.zeros((h, w, 4))
    den = np.zeros((h, w))
    y0 = x0 = P + plo                                              # texel p + q for p = (0,0), q = (plo, plo)
    a = tp[:, y0:y0 + h + PW - 1, x0:x0 + w + PW - 1]              # the TARGET guide: never shifted
    for sy, sx in offs:
        b = gp[:, y0 + sy:y0 + sy + h + PW - 1, x0 + sx:x0 + sx + w + PW - 1]   # the NEIGHBOUR guide at p + s + q
        d = a - b
        D = (d * d).sum(0)                                         # exact integers
        wt = np.exp(_box(D, PW, h, w) * scale)
        num += xp[P + sy:P + sy + h, P + sx:P + sx + w] * wt[..., None]
        den += wt
    return num, den


def pair_sums(target_layer, neighbour_layer, neighbour_in, hparam, search, patch, threads=8):
    """(num [h, w, 4], den [h, w]) float64 of ONE dispatch, its 0.001 included.  The search offsets are shared out over `threads`
    threads; their partial sums are added at the end."""
    x = _as_f64(neighbour_in)
    h, w, _ = x.shape
    slo, shi = search
    plo, phi = patch
    PW = phi - plo
    P = max(-plo, phi) + max(-slo, shi) + 1
    xp = np.pad(x, ((P, P), (P, P), (0, 0)))
    tp, gp = _pad_guide(target_layer, P, h, w), _pad_guide(neighbour_layer, P, h, w)
    scale = -1.0 / (255.0 * 255.0) / (float(hparam) ** 2)
    offs = [(sy, sx) for sy in range(slo, shi) for sx in range(slo, shi)]
    n_t = max(1, min(threads, len(offs)))
    with ThreadPoolExecutor(n_t) as ex:
        parts = list(ex.map(lambda i: _offsets(xp, tp, gp, offs[i::n_t], h, w, P, plo, PW, scale), range(n_t)))
    num = np.zeros((h, w, 4))
    den = np.full((h, w), 0.001)                                   # nonlocal.comp:32-33, once per dispatch
    for pn, pd in parts:
        num += pn
        den += pd
    return num, den


def normalize(num, den):
    h, w = den.shape
    out = np.empty((h, w, 4))
    out[:] = (1.0, 0.0, 1.0, 1.0)
    nz = den != 0
    out[nz] = num[nz] / den[nz][:, None]
    return out


def nlm_layers_temporal(frames, layers, k, hparam, search, patch, first=0, count=None, n_layers=None, cache=None):
    """Outputs [first, first+count) as a list of [h, w, 4] float64; frames: n images, layers: n lists of L RGBA8 guides (n_layers:
    only the first n_layers of each list).  cache: a dict the caller keeps for ONE set of frames, layers and parameters; the sums of
    the dispatch (t, f, l) do not depend on k, first, count or the sequence's length and are then worked out once."""
    n = len(frames)
    assert len(layers) == n
    count = n - first if count is None else count
    h, w = np.asarray(frames[0]).shape[:2]
    outs = []
    for t in range(first, first + count):
        num = np.zeros((h, w, 4))
        den = np.zeros((h, w))
        for f in range(max(0, t - k), min(n - 1, t + k) + 1):
            for l in range(len(layers[t]) if n_layers is None else n_layers):
                if cache is not None and (t, f, l) in cache:
                    pn, pd = cache[(t, f, l)]
                else:
                    pn, pd = pair_sums(layers[t][l], layers[f][l], frames[f], hparam, search, patch)
                    if cache is not None:
                        cache[(t, f, l)] = (pn, pd)
                num += pn
                den += pd
        outs.append(normalize(num, den))
    return outs
