"""float64 NumPy restatement of layer-guided non-local means (mid_nlm_layers_accum / mid_nlm_layers), written from the contract in
include/mi_denoise.h, not from the kernel: one accumulate dispatch for guide layer G (RGBA8, texels c/255, out-of-image texels 0) is

    d(p,s) = sum_{q in [patch)^2} |G(p+q) - G(p+s+q)|^2_rgb,   w = exp(-d / h^2)
    num[p] += w * I(p+s)   (all four channels, out-of-image texels 0),   den[p] += w,   plus 0.001 once per dispatch,

and the fused call is L dispatches into zero sums followed by num / den (magenta where den == 0).  The patch distance of each
search offset is a box sum of the per-texel squared byte differences, taken exactly in integers (an integral image), then scaled
by 1/255^2: the checker itself adds no rounding to d."""
import numpy as np


def _as_f64(img):
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img.astype(np.float64) / 255.0
    return img.astype(np.float64)


def _box(D, PW, h, w):
    """PW x PW box sums of the (h+PW-1, w+PW-1) integer image D at the h x w top-left corners, exactly (integral sums along each axis)."""
    c = np.zeros((D.shape[0], w + PW), np.int64)
    np.cumsum(D, axis=1, out=c[:, 1:])
    hb = c[:, PW:] - c[:, :w]
    r = np.zeros((h + PW, w), np.int64)
    np.cumsum(hb, axis=0, out=r[1:])
    return r[PW:] - r[:h]


def _offsets(xp, gp, offs, h, w, P, plo, PW, scale):
    num = np.zeros((h, w, 4))
    den = np.zeros((h, w))
    y0 = x0 = P + plo                                              # texel p + q for p = (0,0), q = (plo, plo)
    a = gp[:, y0:y0 + h + PW - 1, x0:x0 + w + PW - 1]
    for sy, sx in offs:
        b = gp[:, y0 + sy:y0 + sy + h + PW - 1, x0 + sx:x0 + sx + w + PW - 1]
        d = a - b
        D = (d * d).sum(0)                                         # exact integers
        wt = np.exp(_box(D, PW, h, w) * scale)
        num += xp[P + sy:P + sy + h, P + sx:P + sx + w] * wt[..., None]
        den += wt
    return num, den


def nlm_layers_sums(img, layers, hparam, search, patch, threads=8):
    """(num [h, w, 4], den [h, w]) float64 of len(layers) accumulate dispatches into zero sums.  The search offsets are shared out
    over `threads` threads (NumPy releases the GIL in its array loops); their partial sums are added at the end."""
    from concurrent.futures import ThreadPoolExecutor
    x = _as_f64(img)
    h, w, _ = x.shape
    slo, shi = search
    plo, phi = patch
    PW = phi - plo
    P = max(-plo, phi) + max(-slo, shi) + 1
    xp = np.pad(x, ((P, P), (P, P), (0, 0)))
    scale = -1.0 / (255.0 * 255.0) / (float(hparam) ** 2)
    offs = [(sy, sx) for sy in range(slo, shi) for sx in range(slo, shi)]
    num = np.zeros((h, w, 4))
    den = np.zeros((h, w))
    for g in layers:
        g = np.asarray(g)
        assert g.dtype == np.uint8 and g.shape == (h, w, 4), "guide layers are RGBA8 of the image's size"
        gp = np.pad(np.moveaxis(g[..., :3], -1, 0).astype(np.int32), ((0, 0), (P, P), (P, P)))
        den += 0.001                                               # nonlocal.comp:32-33, once per dispatch
        n_t = max(1, min(threads, len(offs)))
        with ThreadPoolExecutor(n_t) as ex:
            parts = list(ex.map(lambda i: _offsets(xp, gp, offs[i::n_t], h, w, P, plo, PW, scale), range(n_t)))
        for pn, pd in parts:
            num += pn
            den += pd
    return num, den


def nlm_layers(img, layers, hparam, search, patch):
    """The fused call: [h, w, 4] float64, magenta (1, 0, 1, 1) where the weight sum is 0 (no layers)."""
    num, den = nlm_layers_sums(img, layers, hparam, search, patch)
    h, w = den.shape
    out = np.empty((h, w, 4))
    out[:] = (1.0, 0.0, 1.0, 1.0)
    nz = den != 0
    out[nz] = num[nz] / den[nz][:, None]
    return out
