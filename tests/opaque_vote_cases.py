"""Cases for the opaque-tile vote of the tuned kernels (tests/test_opaque_vote_cases.py on the CPU, tests/test_gpu_opaque_vote.py on the GPU).

Every tuned kernel stages a colour tile in LDS with fill_tile, and-s "every texel this thread stored has alpha == 1.0f" into a flag,
lets the workgroup vote on it and, on a yes, runs a tap loop without the alpha accumulator (bilateral: acc.w = accw; NLM:
normWeight = 0.001 + weightColor.w).  A vote that wrongly says "opaque" is invisible unless a frame has ONE odd texel in an otherwise
opaque tile, at the slot the faulty fill would miss.  This module restates the geometry of every such colour tile, derives the odd
texel's image positions from it, builds flat frames in which a far halo tap still weighs enough to be seen, and holds the comparison.

Tile geometry (origin relative to the tile's first output pixel; LW x LH slots; threads that fill it):

  bilateral, radius R, shape BilShape<R, P, NW>   origin (-R, -R)            LW = 64 + 2R        LH = NW*P + 2R       NW*64 threads
  NLM strip, search [SLO,SHI), patch [PLO,PHI)    origin (PLO+SLO, PLO+SLO)  LW = 64 + SW - 1    LH = 32 + PW-1 + SW-1  256 (HALF: 512)
  layer-guided NLM (colour tile: centres only)    origin (PLO+SLO, SLO)      LW = 64 + SW - 1    LHC = 64 + SW - 1    kLNW*64 = 512

A bilateral output reads the alpha of every slot of its tile.  An NLM output reads alpha only at its centre texels p + s: the strip
kernel's tile carries NL = -PLO columns and rows on the left / top and NR = PHI-1 on the right / bottom that enter patch distances
only, and the layer-guided colour tile carries those columns (the lanes without a finished patch sum read them) but no such rows.
A slot whose alpha no valid output of its own tile reads is replaced by the nearest slot that is read (POSITIONS' `note`).
"""
import zlib
from collections import namedtuple

import numpy as np

BIL_SHAPES = {4: (2, 8), 8: (2, 8), 10: (2, 16), 20: (1, 8)}             # R: (P, NW) of bilateral_shapes.hpp
NLM_WINDOWS = {"ref": ((-7, 7), (-3, 3)), "bench": ((-10, 11), (-3, 4))}  # the tuned windows: (search, patch), half-open
NLM_LAYERS_SHAPE = (8, 8)                                                 # kLR, kLNW of nlm_layers.hip / nlm_layers_temporal.hip
NLM_STRIP_SHAPES = {"whole": (8, 4), "half": (4, 8)}                      # rows per wave, waves: nlm_strip.hpp and its HALF shape
NLM_SMALL_ROUNDS = 7                                                      # kNlmSmallRounds

BIL_TOL, NLM_TOL = 1e-5, 2e-5

# ox, oy: tile origin relative to the first output pixel; out_w x out_h: the tile's outputs; reach = (lo, hi): output p reads the ALPHA of
# p + o for lo <= o <= hi on both axes; cols / rows: the slot columns / rows whose alpha some valid output of the tile reads
# pad: columns / rows the frame needs beyond the LDS tile, so that every pixel that sees a texel of the tile, and its patch, is in the frame
# (an NLM pixel whose patch leaves the frame weighs its neighbours by e^-(a patch row of 0.5^2 / h^2): it sees the texel, but not measurably)
Tile = namedtuple("Tile", "name ox oy lw lh threads out_w out_h reach cols rows pad")


def bil_tile(R):
    P, NW = BIL_SHAPES[R]
    lw, lh = 64 + 2 * R, NW * P + 2 * R
    return Tile(f"bilateral r={R}", -R, -R, lw, lh, NW * 64, 64, NW * P, (-R, R), (0, lw - 1), (0, lh - 1), (3, 1))


def nlm_strip_tile(window, shape="whole"):
    (slo, shi), (plo, phi) = NLM_WINDOWS[window]
    rows, waves = NLM_STRIP_SHAPES[shape]
    assert rows * waves == 32, "both shapes work on the same 32-row tile"
    sw, pw, nl, nr = shi - slo, phi - plo, -plo, phi - 1
    lw, lh = 64 + sw - 1, 32 + pw - 1 + sw - 1
    return Tile(f"nlm strip {window} {shape}", plo + slo, plo + slo, lw, lh, waves * 64, 64 - (pw - 1), 32, (slo, shi - 1),
                (nl, lw - 1 - nr), (nl, lh - 1 - nr), (-slo, -slo))


def nlm_layers_tile(window):
    (slo, shi), (plo, phi) = NLM_WINDOWS[window]
    rows, waves = NLM_LAYERS_SHAPE
    sw, pw, nl, nr = shi - slo, phi - plo, -plo, phi - 1
    lw, lh = 64 + sw - 1, rows * waves + sw - 1
    return Tile(f"nlm layers {window}", plo + slo, slo, lw, lh, waves * 64, 64 - (pw - 1), rows * waves, (slo, shi - 1),
                (nl, lw - 1 - nr), (0, lh - 1), (-slo, -slo + nr))


def interior_tile(t):
    """(a, b, X0, Y0): the first tile with a left and an upper neighbour whose whole LDS tile lies inside a frame of frame_size(t)."""
    a = max(1, -(t.ox // t.out_w))
    b = max(1, -(t.oy // t.out_h))
    return a, b, a * t.out_w, b * t.out_h


def frame_size(t):
    """(h, w): the smallest frame with three tile columns in which interior_tile(t)'s LDS tile and its pad are inside (no multiple of the tile)."""
    _, _, X0, Y0 = interior_tile(t)
    w = max(X0 + t.ox + t.lw + t.pad[0], 2 * t.out_w + 5)
    h = Y0 + t.oy + t.lh + t.pad[1]
    return h, w


def tile_outputs(t, a, b, h, w):
    """The slices (rows, columns) of tile (a, b)'s outputs in an h x w frame."""
    return slice(b * t.out_h, min((b + 1) * t.out_h, h)), slice(a * t.out_w, min((a + 1) * t.out_w, w))


Position = namedtuple("Position", "name xy slot note")


def positions(t):
    """The odd texel's image positions (x, y) for interior_tile(t), duplicates removed (the first name wins)."""
    _, _, X0, Y0 = interior_tile(t)
    n, trip = t.lw * t.lh, 4 * t.threads
    wanted = [("slot 0", 0), ("slot n-1", n - 1), ("first slot of the last trip", ((n - 1) // trip) * trip),
              ("slot LW-1", t.lw - 1), ("slot n-LW", n - t.lw)]
    out, seen = [], set()
    for name, s in wanted:
        ty, tx = divmod(s, t.lw)
        cx, cy = min(max(tx, t.cols[0]), t.cols[1]), min(max(ty, t.rows[0]), t.rows[1])
        note = "" if (cx, cy) == (tx, ty) else f"slot {s} = ({tx}, {ty}) feeds no alpha of this tile: nearest read slot ({cx}, {cy})"
        xy = (X0 + t.ox + cx, Y0 + t.oy + cy)
        if xy not in seen:
            seen.add(xy)
            out.append(Position(name, xy, cy * t.lw + cx, note))
    for name, xy in (("middle of the outputs", (X0 + t.out_w // 2, Y0 + t.out_h // 2)), ("junction of four tiles", (X0, Y0))):
        if xy not in seen:
            seen.add(xy)
            out.append(Position(name, xy, (xy[1] - Y0 - t.oy) * t.lw + xy[0] - X0 - t.ox, ""))
    return out


def case_table():
    """[(tile name, frame h x w, interior tile, position name, (x, y), note)]: the table LABNOTES carries."""
    rows = []
    tiles = [bil_tile(R) for R in BIL_SHAPES] + [nlm_strip_tile(wd, s) for wd in NLM_WINDOWS for s in NLM_STRIP_SHAPES] + \
            [nlm_layers_tile(wd) for wd in NLM_WINDOWS]
    for t in tiles:
        a, b, _, _ = interior_tile(t)
        for p in positions(t):
            rows.append((t.name, frame_size(t), (a, b), p.name, p.xy, p.note))
    return rows


# ---- which pixels see a texel -----------------------------------------------------------------------------------------------------
def window_mask(h, w, texels, reach, linear=False):
    """[h, w] bool: the pixels p that read the alpha of one of `texels` = [(x, y)].  2-D addressing: p + o == texel for an offset o
    in reach^2.  linear: the flat index of p plus dx + dy * w is the texel's (bialteral_linear.comp: columns wrap into the next row)."""
    lo, hi = reach
    m = np.zeros((h, w), bool)
    for qx, qy in texels:
        if linear:
            flat = m.reshape(-1)
            for dy in range(lo, hi + 1):
                p0, p1 = qy * w + qx - dy * w - hi, qy * w + qx - dy * w - lo
                flat[max(p0, 0):max(min(p1 + 1, h * w), 0)] = True
        else:
            m[max(qy - hi, 0):max(qy - lo + 1, 0), max(qx - hi, 0):max(qx - lo + 1, 0)] = True
    return m


def interior_mask(h, w, reach, linear=False):
    """[h, w] bool: the pixels whose whole window is inside the frame (no out-of-image texel, whose alpha is 0, under any tap)."""
    lo, hi = reach
    m = np.zeros((h, w), bool)
    if linear:
        flat = m.reshape(-1)
        flat[max(-(lo + lo * w), 0):h * w - (hi + hi * w)] = True
    else:
        m[-lo:h - hi, -lo:w - hi] = True
    return m


def check_alpha(got, ref, texels, reach, tol, linear=False, exact_outside=True):
    """The comparison of one case; got, ref: [h, w, 4].  Returns (worst alpha error inside the windows, smallest |ref alpha - 1| there).

    * On the reference alone, first: |ref.alpha - 1| >= 5 * tol at EVERY pixel whose window holds an odd texel -- a wrong vote yields the
      opaque form's alpha there (exactly 1.0 in the bilateral kernels), so a case whose true alpha is that close to 1 would be blind.
    * |got.alpha - ref.alpha| < tol at every such pixel.
    * Interior pixels outside every window are exactly 1.0 in `got`, and 1.0 to float64 rounding in `ref` (exact_outside=False for the NLM kernels: their norm carries
      nonlocal.comp's 0.001, so an opaque frame's alpha is sum / (0.001 + sum), not 1; those pixels are then left to the caller's
      four-channel comparison)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    h, w = ref.shape[:2]
    assert got.shape == ref.shape == (h, w, 4)
    win = window_mask(h, w, texels, reach, linear)
    assert win.any(), "no pixel sees the odd texel"
    dev = np.abs(ref[..., 3][win] - 1.0)
    assert dev.min() >= 5 * tol, f"blind case: the reference's alpha is within {dev.min():.3g} of 1 inside the window (5 x tol = {5 * tol:.3g})"
    err = np.abs(got[..., 3][win] - ref[..., 3][win])
    assert err.max() < tol, f"alpha off by {err.max():.3g} inside the odd texel's window (tol {tol:.3g}); worst pixel (y, x) = " \
                            f"{tuple(np.argwhere(win)[err.argmax()])}, got {got[..., 3][win][err.argmax()]!r}"
    if exact_outside:
        out = interior_mask(h, w, reach, linear) & ~win
        assert out.any()
        # (the float64 reference: to 1e-12 -- on a GPU the checkers' index_add_ adds a window's pairs in any order, so their alpha sum and
        # weight sum, equal term by term, may round apart in the last bits)
        assert np.all(np.abs(ref[..., 3][out] - 1.0) <= 1e-12), "reference: an interior pixel outside every window is not 1.0"
        assert np.all(got[..., 3][out] == 1.0), f"{int((got[..., 3][out] != 1.0).sum())} interior pixels outside every window are not exactly 1.0"
    return float(err.max()), float(dev.min())


# ---- frames -------------------------------------------------------------------------------------------------------------------------
# Flat frames 0.5 + N(0, 0.02) and guides of 128 +- 2 codes: with sigma_c = 0.1 and sigma_s = R (bilateral), h = 0.5 (NLM) the range and
# patch weights stay near 1, so a far halo tap still weighs about 1 / (window area) and the reference's alpha leaves 1 by more than
# 5 x tol.  (The suite's other generators -- 0.3-amplitude ramps, sigma_s = R / 2.5 -- drive those weights to nothing.)
SIGMA_C, HPARAM = 0.1, 0.5
ODD_ALPHA = {np.dtype(np.uint8): 0, np.dtype(np.float16): -3.0, np.dtype(np.float32): -3.0}   # RGBA8: code 0; float frames: an HDR alpha far from 1


def sigma_s(R):
    """sigma_s = R; 2R at R = 20, where one RGBA8 texel (alpha code 0) among five neighbour frames would otherwise move the far corner's
    alpha by 5.3e-5, too near 5 x tol."""
    return float(R) if R < 20 else 2.0 * R


def flat_frame(rng, h, w, dtype):
    rgb = 0.5 + rng.normal(0.0, 0.02, (h, w, 3))
    f = np.concatenate([rgb, np.ones((h, w, 1))], -1)
    if np.dtype(dtype) == np.uint8:
        return np.round(f * 255).astype(np.uint8)
    return f.astype(dtype)


def flat_guide(rng, h, w):
    g = rng.integers(126, 131, (h, w, 4)).astype(np.uint8)
    g[..., 3] = 255
    return g


def base_frames(t, dtype, n=5, size=None):
    """(n frames, n lists of two guide layers) for tile t: the same draws for every dtype, so that the CPU file's observability figures are
    worked out on the frames the GPU file runs."""
    rng = np.random.default_rng(zlib.crc32(t.name.encode()))
    h, w = frame_size(t) if size is None else size
    frames = [flat_frame(rng, h, w, dtype) for _ in range(n)]
    return frames, [[flat_guide(rng, h, w) for _ in range(2)] for _ in range(n)]


def bil_positions(R, linear):
    """The single-frame bilateral positions; the linear layout adds (w-1, y), a texel that enters the left-border tile of the next row only
    through the row wrap (away from the first and last rows those tiles are fully opaque in this layout)."""
    t = bil_tile(R)
    ps = positions(t)
    if linear:
        _, w = frame_size(t)
        _, _, _, Y0 = interior_tile(t)
        ps = ps + [Position("row wrap", (w - 1, Y0 + 2), -1, "tile (0, b) holds it at column R-1, one row down")]
    return ps


def strip_positions(window):
    """The positions of the whole-strip shape and of the HALF shape together (their last fill trips may start at different slots)."""
    return list({p.xy: p for s in ("half", "whole") for p in positions(nlm_strip_tile(window, s))}.values())


def with_odd(frame, xy, alpha=None):
    out = frame.copy()
    out[xy[1], xy[0], 3] = ODD_ALPHA[frame.dtype] if alpha is None else alpha
    return out


def decode(a):
    """The float32 texels the kernels read from a frame or a guide."""
    a = np.asarray(a)
    return a.astype(np.float32) / np.float32(255.0) if a.dtype == np.uint8 else a.astype(np.float32)


# One odd frame f_odd in a sequence of n frames at window half-width k: (n, k, f_odd).  Per output t the odd frame is
#   (3, 1, 1): t = 0 the last neighbour (window clipped), 1 the target, 2 the first (clipped)
#   (5, 1, 2): t = 1 the last, 2 the target, 3 the first; 0 and 4 do not see it at all
#   (5, 2, 2): t = 0 the last (clipped), 1 and 3 a middle one (clipped), 2 the target, 4 the first (clipped)
#   (3, 2, 0): the first neighbour of every output (every window is the whole sequence), the target of 0
#   (3, 2, 2): the last neighbour of every output, the target of 2
SEQUENCES = [(3, 1, 1), (5, 1, 2), (5, 2, 2), (3, 2, 0), (3, 2, 2)]
# The NLM families' float64 checkers cost a fifth of a second per (target, neighbour) pair on a CPU, so they run two sequences per window
# that between them hold every placement, three and five frames, k = 1 and 2 and clipped windows; (3, 2, 1): the odd frame is a middle
# neighbour of outputs 0 and 2 and the target of 1.
NLM_SEQUENCES = {"ref": [(3, 1, 1), (5, 2, 2)], "bench": [(3, 1, 1), (3, 2, 1)]}


def seq_positions(t, i):
    """The three odd-texel positions sequence i of SEQUENCES runs at: slot 0, slot n-1 (the two a vote carried over from the previous
    neighbour shows at) and one of the others in turn."""
    ps = positions(t)
    assert ps[0].name == "slot 0" and ps[1].name == "slot n-1"
    return [ps[0], ps[1], ps[2 + i % (len(ps) - 2)]]


def placement(n, k, f_odd, t):
    lo, hi = max(0, t - k), min(n - 1, t + k)
    if not lo <= f_odd <= hi:
        return "unseen"
    if f_odd == t:
        return "target"
    return "first" if f_odd == lo else "last" if f_odd == hi else "middle"


# ---- the NLM dispatcher's arithmetic (nlm.hip: dispatch_ranges, nlm_small.hip: nlm_dispatch_small / tail_split) ---------------------
def nlm_tile_workgroups(w, h, patch_w, frames):
    return -(-w // (64 - (patch_w - 1))) * -(-h // 32) * frames


def nlm_launch_shape(w, h, patch_w, frames, cu_count, k=0):
    """What a tuned-window launch of `frames` outputs runs as: dict(copy = 'small' | 'long', whole = workgroups in whole strips,
    half = workgroups in the HALF tail shape)."""
    nwg = nlm_tile_workgroups(w, h, patch_w, frames)
    slots = 2 * cu_count
    if k > 0 or nwg > NLM_SMALL_ROUNDS * slots:
        return dict(copy="long", whole=nwg, half=0)
    rem = nwg % slots
    if 0 < rem <= cu_count:
        return dict(copy="small", whole=nwg - rem, half=rem)
    return dict(copy="small", whole=nwg, half=0)
