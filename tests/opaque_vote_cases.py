"""Cases for the opaque-tile vote of the tuned kernels (tests/test_opaque_vote_cases.py on the CPU, tests/test_gpu_opaque_vote.py and
tests/test_gpu_bilateral_joint_vote.py on the GPU).

Every tuned kernel stages a colour tile in LDS with fill_tile, and-s "every texel this thread stored has alpha == 1.0f" into a flag,
lets the workgroup vote on it and, on a yes, runs a tap loop without the alpha accumulator (bilateral: acc.w = accw; NLM:
normWeight = 0.001 + weightColor.w).  A vote that wrongly says "opaque" is invisible unless a frame has ONE odd texel in an otherwise
opaque tile, at the slot the faulty fill would miss.  This module restates the geometry of every such colour tile, derives the odd
texel's image positions from it, builds flat frames in which a far halo tap still weighs enough to be seen, and holds the comparison.

Tile geometry (origin relative to the tile's first output pixel; LW x LH slots; threads that fill it):

  bilateral, radius R, shape BilShape<R, P, NW>   origin (-R, -R)            LW = 64 + 2R        LH = NW*P + 2R       NW*64 threads
  joint bilateral (bilateral_joint.hip)           the bilateral's colour tile, with up to four guide tiles of three float planes beside it
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


# ---- the joint (cross) bilateral (bilateral_joint.hip) -------------------------------------------------------------------------------
# Its colour tile is the bilateral's, bil_tile(R); the tuned kernels hold one opaque tap loop per layer count they can keep in LDS.
# The vote goes through the first word of the guide tiles -- layer 0's x of slot 0, which thread 0 keeps in a register (`held`) and
# stores once the vote is read -- so "slot 0" also proves that word: a wrong value there changes the weight of the one tap of output
# (X0, Y0) that reads the odd texel (test_opaque_vote_cases.py asserts the size of that change on the reference).
JOINT_LDS_MAX = 160 * 1024                                 # bytes of LDS a workgroup may have on the MI355X
JOINT_TILED_LAYERS = 4                                     # kJointTiledLayers
BIL_RT_SHAPE = (2, 8)                                      # kBilRtP, kBilRtNW: the run-time-radius kernels' 16-row tile
JOINT_LAYERS = {4: (1, 2, 3, 4), 8: (1, 2, 3, 4), 10: (1,), 20: (1,)}      # R: the layer counts its tuned kernel runs tiled
JOINT_SEQUENCES = {4: (0, 1, 2, 3, 4), 8: (0, 1, 2, 3, 4), 10: (0, 2), 20: (0,)}   # R: indices into SEQUENCES, RGBA32F frames
JOINT_U8_SEQUENCES = {4: (0,), 8: (0,), 10: (), 20: ()}                    # the same, RGBA8 frames
JOINT_SIGMAS = (0.1, 0.15, 0.2, 0.12)                      # one per layer


def joint_lds_bytes(radius, n_layers):
    """bilateral_joint.hip's joint_lds_bytes at the radius's tile: a float4 colour tile and n_layers guide tiles of three floats."""
    P, NW = BIL_SHAPES.get(radius, BIL_RT_SHAPE)
    return (64 + 2 * radius) * (NW * P + 2 * radius) * (16 + 12 * n_layers)


def joint_class(radius, n_layers, lds_max=JOINT_LDS_MAX):
    """'tuned', 'run-time radius' or 'per pixel': dispatch_joint / launch_joint_tiled / joint_tiled restated.  One layer: the LDS test of
    the layered form's two float4 tiles; a tuned radius never falls back to the run-time-radius kernel."""
    P, NW = BIL_SHAPES.get(radius, BIL_RT_SHAPE)
    texels = (64 + 2 * radius) * (NW * P + 2 * radius)
    fits = n_layers <= JOINT_TILED_LAYERS and (texels * 32 if n_layers == 1 else joint_lds_bytes(radius, n_layers)) <= lds_max
    if radius in BIL_SHAPES:
        max_l = max(l for l in range(1, JOINT_TILED_LAYERS + 1) if l == 1 or joint_lds_bytes(radius, l) <= 160 * 1024)   # joint_max_layers
        return "tuned" if fits and n_layers <= max_l else "per pixel"
    return "run-time radius" if fits else "per pixel"


def odd_value(dtype):
    """The odd texel's alpha as the kernels decode it."""
    return float(decode(np.array([ODD_ALPHA[np.dtype(dtype)]], dtype))[0])


def joint_layers(t, n=5):
    """n lists of four RGBA8 guide layers for tile t: base_frames' two, whose draws stay what they are, and two more flat guides from
    a generator of their own."""
    _, layers = base_frames(t, np.uint8, n)
    rng = np.random.default_rng(zlib.crc32((t.name + ": joint layers 2 and 3").encode()))
    h, w = frame_size(t)
    return [ls + [flat_guide(rng, h, w) for _ in range(2)] for ls in layers]


_JOINT_REFS = {}


def joint_refs(R, L):
    """{(frame dtype, sequence index): (positions, [per output t: {position name: ref [h, w, 4] float64}])} of np_bilateral_joint for
    the joint cases of radius R with L layers: RGBA32F frames in JOINT_SEQUENCES[R], RGBA8 frames in JOINT_U8_SEQUENCES[R], guides
    joint_layers(bil_tile(R))[f][:L] with JOINT_SIGMAS[:L] (RGBA8; as float32 c / 255 they decode to the same texels).

    The weights depend on neither the frames nor their alpha, and every sequence draws on the same five frames, so each pair
    (output t, neighbour f) is worked out ONCE by np_bilateral_joint.pair_sums -- the loop bilateral_joint itself is made of -- on an
    image that carries, beside frame f's rgb in both formats, one alpha plane per case in which f is the odd frame."""
    if (R, L) in _JOINT_REFS:
        return _JOINT_REFS[(R, L)]
    import np_bilateral_joint as chk
    t = bil_tile(R)
    h, w = frame_size(t)
    f32, u8 = np.dtype(np.float32), np.dtype(np.uint8)
    rgb = {dt: [decode(f)[..., :3] for f in base_frames(t, dt)[0]] for dt in (f32, u8)}
    layers = [ls[:L] for ls in joint_layers(t)]
    runs = [(f32, i) for i in JOINT_SEQUENCES[R]] + [(u8, i) for i in JOINT_U8_SEQUENCES[R]]
    col = {dt: slice(3 * c, 3 * c + 3) for c, dt in enumerate((f32, u8))}
    planes = [{} for _ in range(5)]                                      # per frame: (dtype, position name) -> channel
    for dt, i in runs:
        for p in seq_positions(t, i):
            planes[SEQUENCES[i][2]].setdefault((dt, p.name), (p, 6 + len(planes[SEQUENCES[i][2]])))
    pairs = {}

    def pair(t_out, f):
        if (t_out, f) not in pairs:
            img = np.ones((h, w, 6 + len(planes[f])), np.float32)
            img[..., col[f32]], img[..., col[u8]] = rgb[f32][f], rgb[u8][f]
            for (dt, _), (p, c) in planes[f].items():
                img[p.xy[1], p.xy[0], c] = odd_value(dt)
            pairs[(t_out, f)] = chk.pair_sums(img, layers[t_out], layers[f], R, sigma_s(R), JOINT_SIGMAS[:L])
        return pairs[(t_out, f)]
    out = {}
    for dt, i in runs:
        n, k, f_odd = SEQUENCES[i]
        group = seq_positions(t, i)
        refs = []
        for t_out in range(n):
            win = range(max(0, t_out - k), min(n - 1, t_out + k) + 1)
            den = sum(pair(t_out, f)[1] for f in win)
            colour = sum(pair(t_out, f)[0][..., col[dt]] for f in win)
            refs.append({})
            for p in group:
                # a frame without an odd texel adds its weights to the alpha sum (alpha 1.0 under every tap), the odd frame its plane's sums
                alpha = sum(pair(t_out, f)[0][..., planes[f][(dt, p.name)][1]] if f == f_odd else pair(t_out, f)[1] for f in win)
                refs[-1][p.name] = np.concatenate([colour, alpha[..., None]], -1) / den[..., None]
        out[(dt, i)] = (group, refs)
    _JOINT_REFS[(R, L)] = out
    return out


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
