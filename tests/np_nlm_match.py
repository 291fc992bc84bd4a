"""Exact known answers of non-local means for 0/1-weight frames: frames built so that every weight a kernel computes is exactly
0.0 or exactly 1.0, and every sum of weighted colours is exact in fp32.  Written from the contract in include/mi_denoise.h (the one
tests/np_reference.py states), not from the kernels.

Why the weights are exact.  The kernels compute w = exp2(-d * log2(e) / h^2) for the patch distance
d(p,s) = sum_{q in patch} |T(p+q) - Nb(p+s+q)|^2_rgb.  A patch that matches texel for texel has d = 0 exactly, also after the strip
kernels scale the colours by sk = sqrt(log2 e)/h (equal texels scale equally), so w = exp2(0) = 1.  Every texel of the frames here
comes from a palette whose entries differ by at least 0.5 in some channel and lie at least 0.5 from (0,0,0), the out-of-image texel;
with h = EXACT_H the exponent of a patch that differs in one texel is at most -0.25 * 4096 = -1024, far below the smallest fp32
subnormal 2^-149, so w = 0.  EXACT_H makes sk = 64.0f exactly: the scaled palette colours (32, 64, 96) and their sums over the
matching offsets stay exact.  RGBA8 frames use the bytes {64, 192} (the nearest pair is 64/255 apart: exponent below -258).

So one accumulate dispatch adds, at pixel p:
    normWeight  += 0.001 + n(p)                          n(p) = the number of search offsets whose patch matches
    weightColor += sum over those offsets of Nb(p+s)     = n(p) * T(p) in rgb (a matching patch contains its centre)
and alpha, which enters no distance, sums the neighbour's alpha over exactly the matching offsets: with small integer alpha codes
that sum is exact and names which offsets were visited and matched.

The reference decides matches with integers only: per search offset a "differs" mask over the zero-padded frames, its patch box
by an integral image, match = box == 0.  Search and patch ranges may differ between the axes (((ylo, yhi), (xlo, xhi))) so that
tests can state what a kernel that is off by one row or one column would produce.

WIDE_CASES are the windows of tests/test_gpu_nlm_wide_windows.py -- both sides of every boundary between the kernels that serve a
search window (mid_nlm_accum's dispatch, 160 KB of LDS) -- and case_pair / case_frames the frames it runs them on, so that the CPU
tests can show, on the very same frames, that an off-by-one kernel would fail them."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

LOG2E = 1.4426950408889634
EXACT_H = float(np.float32(math.sqrt(LOG2E) / 64.0))    # filteringParameter with sk = 64.0f, inv_sk = 2^-6, kexp = -4096.0f
PALETTE_F = np.array([(r, g, b) for r in (0.5, 1.0, 1.5) for g in (0.5, 1.0, 1.5) for b in (0.5, 1.0, 1.5)], np.float32)
PALETTE_U8 = np.array([(r, g, b) for r in (64, 192) for g in (64, 192) for b in (64, 192)], np.uint8)
MAGENTA = np.array([1.0, 0.0, 1.0, 1.0])


def sym(sw):
    """The search range of width sw centred on 0 as the ABI's half-open ranges are: [-(sw // 2), sw - sw // 2)."""
    return (-(sw // 2), sw - sw // 2)


P7, P5, P3, P9, P1, P16 = (-3, 4), (-2, 3), (-1, 2), (-4, 5), (0, 1), (-8, 8)
# (search, patch, the kernel the dispatch picks, run the temporal test too).  Strip kernels: "4w" (4 waves x 8-row strips), "4w>80K"
# (the same with a tile of more than 80 KB: one workgroup per CU), "8w" (8 waves x 8-row strips, 64-row tile), "4row" (4 waves x
# 4-row strips: patches of 10x10 and up); "generic": nlm_generic_kernel, one thread per pixel (temporal only at small patches: it
# does S^2 P^2 work per pixel and frame)
WIDE_CASES = [
    (sym(22), P7, "4w", True), (sym(23), P7, "8w", True), (sym(35), P7, "8w", True), (sym(36), P7, "4w>80K", True),
    (sym(43), P7, "4w>80K", True), (sym(52), P7, "4w>80K", True), (sym(53), P7, "generic", True), (sym(64), P7, "generic", True),
    (sym(23), P5, "4w", True), (sym(24), P5, "8w", True), (sym(36), P5, "8w", True), (sym(37), P5, "4w>80K", True),
    (sym(53), P5, "4w>80K", True), (sym(54), P5, "generic", True),
    (sym(25), P3, "4w", True), (sym(26), P3, "8w", True), (sym(37), P3, "8w", True), (sym(38), P3, "4w>80K", True),
    (sym(54), P3, "4w>80K", True), (sym(55), P3, "generic", True),
    (sym(50), P9, "4w>80K", True), (sym(51), P9, "generic", False),
    (sym(55), P1, "4w>80K", True), (sym(56), P1, "generic", True),
    (sym(56), P16, "4row", True), (sym(57), P16, "generic", False), (sym(64), P16, "generic", False),
    ((-40, 24), P7, "generic", True),          # lopsided search range
    (sym(64), (-1, 3), "generic", True),       # lopsided patch
]
CASE_SHAPE = (100, 130)                         # frames: > 1 tile in both directions for every strip kernel, ragged


def case_id(case):
    (slo, shi), (plo, phi), kern, _ = case
    return f"s{slo}_{shi}-p{plo}_{phi}-{kern}"


def kernel_scales(hparam):
    """(sk, inv_sk, kexp) as the library derives them from filteringParameter (fp32 results of float64 expressions)."""
    hp = float(np.float32(hparam))
    sk = np.float32(math.sqrt(LOG2E) / hp)
    return sk, np.float32(1.0 / float(sk)), np.float32(-LOG2E / (hp * hp))


def axes(r):
    """(lo, hi) for both axes, or ((ylo, yhi), (xlo, xhi)) -> ((ylo, yhi), (xlo, xhi))."""
    if np.ndim(r[0]) == 0:
        return (int(r[0]), int(r[1])), (int(r[0]), int(r[1]))
    return (int(r[0][0]), int(r[0][1])), (int(r[1][0]), int(r[1][1]))


def _codes(frames):
    """One int32 code per texel rgb, equal codes <=> equal rgb, over all `frames` jointly, and the code of (0,0,0), the
    out-of-image texel."""
    flat = [np.asarray(f)[..., :3].reshape(-1, 3) for f in frames]
    allv = np.concatenate([np.zeros((1, 3), flat[0].dtype)] + flat)
    if allv.dtype == np.float16:
        allv = allv.astype(np.float32)
    _, inv = np.unique(allv, axis=0, return_inverse=True)
    inv = inv.reshape(-1).astype(np.int32)
    out, at = [], 1
    for f in frames:
        h, w = f.shape[:2]
        out.append(inv[at:at + h * w].reshape(h, w))
        at += h * w
    return out, int(inv[0])


def _rows(a, npd, cp, P, y0, x0, h, w, ph, pw, sys_, sxlo, sxhi):
    """Sums over the search rows sys_, every search column of a row at once (a sliding window over the padded neighbour)."""
    num = np.zeros((h, w, 4))
    count = np.zeros((h, w), np.int64)
    nsx = sxhi - sxlo
    for sy in sys_:
        rows = npd[y0 + sy:y0 + sy + h + ph - 1, x0 + sxlo:x0 + sxhi - 1 + w + pw - 1]
        b = sliding_window_view(rows, w + pw - 1, axis=1)                      # [h+ph-1, nsx, w+pw-1]
        c = np.zeros((b.shape[0], nsx, w + pw), np.int32)
        np.cumsum(b != a[:, None, :], axis=2, out=c[:, :, 1:])
        hb = c[:, :, pw:] - c[:, :, :w]                                        # texels that differ in each patch row [h+ph-1, nsx, w]
        r = np.zeros((h + ph, nsx, w), np.int32)
        np.cumsum(hb, axis=0, out=r[1:])
        m = (r[ph:] - r[:h]) == 0                                              # [h, nsx, w]: the whole patch matches
        if not m.any():
            continue
        count += m.sum(1)
        crow = cp[P + sy:P + sy + h, P + sxlo:P + sxhi - 1 + w]               # [h, nsx + w - 1, 4]
        cw = sliding_window_view(crow, w, axis=1)                              # [h, nsx, 4, w]
        num += np.einsum("hscw,hsw->hwc", cw, m.astype(np.float64))
    return num, count


def match_sums(target, nb, search, patch, colour=None, threads=8):
    """One accumulate dispatch of a 0/1-weight frame pair, exactly: (num [h, w, 4] float64, count [h, w] int64).
    num = sum of colour(p+s) over the matching offsets s (colour = nb unless given: layer-guided NLM matches on its guide and sums
    the input image; out-of-image colours are 0), count = the number of matching offsets.  Texels match when their rgb are
    equal; RGBA8 frames compare bytes, which is the same thing.  The search rows are shared out over `threads` threads."""
    (sylo, syhi), (sxlo, sxhi) = axes(search)
    (pylo, pyhi), (pxlo, pxhi) = axes(patch)
    target, nb = np.asarray(target), np.asarray(nb)
    h, w = target.shape[:2]
    col = nb if colour is None else np.asarray(colour)
    col = col.astype(np.float64) / 255.0 if col.dtype == np.uint8 else col.astype(np.float64)
    (ct, cn), zero = _codes([target, nb])
    P = max(abs(v) for v in (sylo, syhi, sxlo, sxhi)) + max(abs(v) for v in (pylo, pyhi, pxlo, pxhi)) + 1
    tp = np.pad(ct, P, constant_values=zero)
    npd = np.pad(cn, P, constant_values=zero)
    cp = np.pad(col, ((P, P), (P, P), (0, 0)))
    ph, pw = pyhi - pylo, pxhi - pxlo
    y0, x0 = P + pylo, P + pxlo                                   # texel p + q for p = (0, 0), q = (pylo, pxlo)
    a = tp[y0:y0 + h + ph - 1, x0:x0 + w + pw - 1]
    sys_ = list(range(sylo, syhi))
    n_t = max(1, min(threads, len(sys_)))
    with ThreadPoolExecutor(n_t) as ex:
        parts = list(ex.map(lambda i: _rows(a, npd, cp, P, y0, x0, h, w, ph, pw, sys_[i::n_t], sxlo, sxhi), range(n_t)))
    return sum(p[0] for p in parts), sum(p[1] for p in parts)


def temporal_sums(frames, t, k, search, patch, cache=None):
    """Output frame t of the fused temporal call, as sums: neighbour frames clipped to the sequence.  Returns (num [h, w, 4]
    float64, the per-frame match counts [n, h, w]).  cache: a dict (t, f) -> match_sums, shared between calls."""
    cache = {} if cache is None else cache
    lo, hi = max(0, t - k), min(len(frames) - 1, t + k)
    num, counts = 0.0, []
    for f in range(lo, hi + 1):
        if (t, f) not in cache:
            cache[(t, f)] = match_sums(frames[t], frames[f], search, patch)
        n, c = cache[(t, f)]
        num = num + n
        counts.append(c)
    return num, np.stack(counts)


def fp32_norm(counts):
    """The normWeight the kernels form in fp32 for weights that are 1.0 or 0.0: per neighbour frame 0.001f, then + 1.0f once per
    matching offset (equal terms: the order does not matter), then the frames' totals added in frame order.
    counts: [n_frames, h, w] integers.  Returns [h, w] float32."""
    counts = np.asarray(counts, np.int64)
    tot = np.zeros(counts.shape[1:], np.float32)
    for c in counts:
        acc = np.full(c.shape, np.float32(0.001), np.float32)
        for i in range(int(c.max()) if c.size else 0):
            acc = np.where(c > i, acc + np.float32(1.0), acc).astype(np.float32)
        tot = (tot + acc).astype(np.float32)
    return tot


def normalized_fp32(num, counts):
    """The fused output as the kernels form it: fp32(num) / fp32_norm(counts), magenta where the norm is 0; float32 [h, w, 4]."""
    den = fp32_norm(counts)
    n32 = np.asarray(num, np.float32)
    out = np.empty(n32.shape, np.float32)
    out[:] = MAGENTA
    nz = den != 0
    out[nz] = n32[nz] / den[nz][:, None]
    return out


def pattern_frame(rng, h, w, search, palette=PALETTE_F):
    """A 0/1-weight frame [h, w, 4] for the search range (lo, hi), every texel a palette colour (float32, or RGBA8 for a uint8
    palette):
      * columns [0, w/2): periodic with period p1 in both axes, p1 the smallest divisor >= 2 of the first search offset |lo|;
        columns [w/2, w): period p2, the smallest divisor >= 2 of the last offset hi - 1 -- so that patches match in the first and
        in the last search row and column (the colours of one period drawn at random from the palette);
      * a constant block at the foot of the seam, where every offset matches whose patch stays inside it;
      * sparse single-texel defects (another palette colour), so that some offsets fail on one patch edge row or column only.
    Alpha: random integer codes 1..1023 (float frames: exact sums), or 0 / 255 (RGBA8: the exact values 0.0 / 1.0)."""
    lo, hi = int(search[0]), int(search[1])

    def period(v):
        v = abs(v)
        return next(d for d in range(2, v + 1) if v % d == 0) if v >= 2 else 2

    idx = np.empty((h, w), np.int64)
    for (c0, c1), p in (((0, w // 2), period(lo)), ((w // 2, w), period(hi - 1))):
        cell = rng.integers(0, len(palette), (p, p))
        yy, xx = np.mgrid[0:h, c0:c1]
        idx[:, c0:c1] = cell[yy % p, xx % p]
    idx[h - h // 4:, w // 2 - w // 8:w // 2 + w // 8] = rng.integers(0, len(palette))
    nd = max(1, h * w // 400)
    ys, xs = rng.integers(0, h, nd), rng.integers(0, w, nd)
    idx[ys, xs] = (idx[ys, xs] + rng.integers(1, len(palette), nd)) % len(palette)
    return _with_alpha(rng, palette[idx])


def _with_alpha(rng, rgb):
    h, w = rgb.shape[:2]
    u8 = rgb.dtype == np.uint8
    out = np.empty((h, w, 4), np.uint8 if u8 else np.float32)
    out[..., :3] = rgb
    out[..., 3] = 255 * rng.integers(0, 2, (h, w)) if u8 else rng.integers(1, 1024, (h, w))
    return out


def with_defects(rng, frame, n, palette=None):
    """A copy of `frame` with n more single-texel defects (another colour of the palette) and fresh alpha codes."""
    palette = (PALETTE_U8 if frame.dtype == np.uint8 else PALETTE_F) if palette is None else palette
    rgb = np.array(frame[..., :3], copy=True)
    h, w = rgb.shape[:2]
    for y, x in zip(rng.integers(0, h, n), rng.integers(0, w, n)):
        choices = [c for c in palette if not np.array_equal(c, rgb[y, x])]
        rgb[y, x] = choices[rng.integers(0, len(choices))]
    return _with_alpha(rng, rgb)


def _seed(case, salt):
    (slo, shi), (plo, phi) = case[0], case[1]
    return (slo + 64) * 1000003 + (shi + 64) * 10007 + (plo + 16) * 101 + (phi + 16) + 7919 * salt


def case_pair(case, u8=False):
    """(target, neighbour) of the accumulate test of a WIDE_CASES entry: float32 (alpha codes 1..1023), or RGBA8."""
    rng = np.random.default_rng(_seed(case, 1 if u8 else 0))
    t = pattern_frame(rng, *CASE_SHAPE, case[0], PALETTE_U8 if u8 else PALETTE_F)
    return t, with_defects(rng, t, CASE_SHAPE[0] * CASE_SHAPE[1] // 400)


def case_frames(case, n=5):
    """The n float32 frames of the temporal test of a WIDE_CASES entry: one pattern, each frame with defects of its own."""
    rng = np.random.default_rng(_seed(case, 2))
    base = pattern_frame(rng, *CASE_SHAPE, case[0])
    return [with_defects(rng, base, CASE_SHAPE[0] * CASE_SHAPE[1] // 400) for _ in range(n)]


def off_by_one(search, patch):
    """The windows of kernels that are off by one, as (name, search, patch): the search window one row or column shorter at either
    end; the patch one shorter (a 1x1 patch: one longer) at either end of either axis; and the patch mirrored in one axis,
    [1 - phi, 1 - plo) -- for a patch that is not symmetric about 0, what a kernel produces that takes one axis's extent the wrong
    way round (as transposing a lopsided patch's row and column roles does to one of them)."""
    (slo, shi), (plo, phi) = (int(search[0]), int(search[1])), (int(patch[0]), int(patch[1]))
    s, p = (slo, shi), (plo, phi)
    out = [("search first row", ((slo + 1, shi), s), p), ("search last row", ((slo, shi - 1), s), p),
           ("search first column", (s, (slo + 1, shi)), p), ("search last column", (s, (slo, shi - 1)), p)]
    other = [(plo + 1, phi), (plo, phi - 1)] if phi - plo > 1 else [(plo - 1, phi), (plo, phi + 1)]
    for q, end in zip(other, ("first", "last")):
        out.append((f"patch {end} row", s, (q, p)))
        out.append((f"patch {end} column", s, (p, q)))
    mirror = (1 - phi, 1 - plo)
    if mirror != p:
        out.append(("patch mirrored in rows", s, (mirror, p)))
        out.append(("patch mirrored in columns", s, (p, mirror)))
    return out
