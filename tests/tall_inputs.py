"""The input recipe of the tall-frame GPU tests (tests/test_gpu_tall_frames.py) and of the later-tile tests
(tests/test_gpu_later_tiles.py), held to its conditions on the CPU by tests/test_tall_inputs_args.py -- no kernel takes part.

A tall frame, its guide layers, motion vectors and history planes repeat a pattern of PERIOD = 37 rows: row y holds pattern row
y % 37, tiled in y only.  A SMALL frame of hs rows is tiled from the same pattern, with

    hs >= 37 + 2 r   and   hs = H (mod 37)                                                         (small_height)

for a stencil that reaches r rows.  Then every row y of the tall frame has the inputs of one row of the small frame (row_map):

    y < r            row y                  the same rows above it, the same image edge
    y >= H - r       row hs - (H - y)       the same distance to the bottom edge and, hs = H (mod 37), the same phase
    otherwise        row r + (y - r) % 37   the same phase, r rows of the same phases above and below, no edge within reach

so the whole tall output is compared with the small frame's output indexed by row_map, no row left out.  A block index that wrapped
at 65536 would store row y + 4 * 65536 (or 16 * 65536) over row y: 262144 % 37 = 36 and 1048576 % 37 = 33, so the phases differ and the
patterns below have no two equal rows.

Heights: H4 = 262149 gives ceil(H4 / 4) = 65538 workgroups in y to the kernels of four rows per workgroup, H16 = 1048593 the same
number to those of sixteen.
"""
import numpy as np

import atrous_variance_inputs as avi
import median_inputs as mi
import np_atrous_exact as ax
import np_atrous_variance
import np_atrous_variance_exact as vex
import np_temporal_accumulate_exact as tae
from np_temporal_accumulate_clip_exact import clip_planes

PERIOD = 37
H4, H16 = 262149, 1048593
GRID_Y = 65538
WIDTHS = (3, 65)

ACCUM_REACH = 4             # motion of up to 3 rows, and the bilinear tap one row further
ATROUS_REACH = 2            # one pass at step 1
ACCUM_LAYERS = 2
ACCUM_PARAMS = dict(alpha=0.1, alpha_moments=0.05, history_max=8)


def cdiv(a, b):
    return -(-a // b)


def small_height(H, r):
    """The smallest hs >= PERIOD + 2 r with hs = H (mod PERIOD)."""
    hs = PERIOD + 2 * r
    return hs + (H - hs) % PERIOD


def tile_rows(pattern, h):
    """h rows that repeat the pattern's PERIOD rows."""
    pattern = np.asarray(pattern)
    assert pattern.shape[0] == PERIOD
    return np.concatenate([pattern] * cdiv(h, PERIOD))[:h].copy()


def row_map(H, r, hs):
    """int64 [H]: the row of the small frame whose inputs tall row y has (module docstring)."""
    assert hs >= PERIOD + 2 * r and hs % PERIOD == H % PERIOD and H >= hs
    y = np.arange(H, dtype=np.int64)
    return np.where(y < r, y, np.where(y >= H - r, hs - (H - y), r + (y - r) % PERIOD))


def interior_repeats(out, r):
    """The property the GPU tests lean on: rows r .. rows - r of a checker's output repeat with period 37, to the last bit."""
    out = np.ascontiguousarray(out)
    body = out[r:out.shape[0] - r]
    u = body.view({8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[body.dtype.itemsize])
    return body.shape[0] > PERIOD and np.array_equal(u[PERIOD:], u[:-PERIOD])


def distinct_rows(pattern):
    """No two of the pattern's rows are equal: an aliased row shows."""
    p = np.ascontiguousarray(pattern).reshape(PERIOD, -1)
    return len({row.tobytes() for row in p}) == PERIOD


# ---- the recursive accumulation: np_temporal_accumulate_exact's construction, one period of it ---------------------------------------
def accumulate_patterns(w, seed=3):
    """dict of [37, w, ...] patterns: frame, history colour and state, motion (integers and halves up to +-3 in x and in y: it crosses
    rows), ACCUM_LAYERS label layers of this frame and of the previous one, the clip box."""
    shape = (PERIOD, w)
    hc, hs = tae.history(shape, seed)
    lo, hi = clip_planes(shape, seed)
    return dict(frame=tae.grey_frame(shape, seed), hist_colour=hc, hist_state=hs, motion=tae.motion(shape, seed),
                layers=tae.label_layers(shape, ACCUM_LAYERS, 1), prev_layers=tae.label_layers(shape, ACCUM_LAYERS, 0), clip_lo=lo, clip_hi=hi)


def tiled(patterns, h):
    """The patterns (arrays, or lists of arrays) as frames of h rows."""
    return {k: [tile_rows(a, h) for a in v] if isinstance(v, list) else tile_rows(v, h) for k, v in patterns.items()}


def accumulate_answer(t, clip):
    """(colour, state, Vt) of the frames t = tiled(accumulate_patterns(w), hs): bit-true (np_temporal_accumulate_clip_exact.py)."""
    from np_temporal_accumulate_clip_exact import temporal_accumulate_clip_exact
    p = ACCUM_PARAMS
    out = temporal_accumulate_clip_exact(t["frame"], t["layers"], t["prev_layers"], (t["hist_colour"], t["hist_state"]), t["motion"], p["alpha"],
                                         p["alpha_moments"], p["history_max"], t["clip_lo"] if clip else None, t["clip_hi"] if clip else None)
    return out[:3]


# ---- one a-trous pass at step 1: np_atrous_exact's construction ----------------------------------------------------------------------
def atrous_patterns(w, L):
    """Integer frame and L label layers (float32) of one period."""
    shape = (PERIOD, w)
    return dict(frame=ax.int_frame(shape, seed=4), layers=ax.label_layers(shape, L, np.float32))


def atrous_answer(t):
    """The exact float32 result of pass 0 over the frames t = tiled(atrous_patterns(w, L), hs), and the share of taps accepted."""
    same = ax.equal_on(t["layers"])
    num, den, accepted, offered = ax.pass_sums(t["frame"], same, 1)
    return ax.quotient(num, den), accepted / max(offered, 1)


# ---- one variance-guided pass at step 1: np_atrous_variance_exact's construction ------------------------------------------------------
def variance_patterns(w, L):
    shape = (PERIOD, w)
    return dict(frame=vex.grey_frame(shape, L), variance=vex.variance_plane(shape), layers=ax.colour_layers(shape, L, np.float32))


def variance_answer(t):
    """(C', V') exact, and the share of taps accepted."""
    num, den, numv, accepted, offered = vex.sums(t["frame"], t["variance"], ax.equal_on(t["layers"], t["frame"]), 1)
    return (ax.quotient(num, den), vex.variance_quotient(numv, den)), accepted / max(offered, 1)


# ---- the temporal pass of the a-trous filter over three frames, output 1: np_atrous_exact's construction ------------------------------
TEMPORAL_FRAMES, TEMPORAL_K, TEMPORAL_T = 3, 1, 1


def temporal_patterns(w, L):
    """frame0 .. frame2 and layers0 .. layers2: integer frames of their own, the label pattern moving with the frame."""
    shape = (PERIOD, w)
    out = {}
    for f in range(TEMPORAL_FRAMES):
        out[f"frame{f}"] = ax.int_frame(shape, seed=20 + f)
        out[f"layers{f}"] = ax.label_layers(shape, L, np.float32, frame=f)
    return out


def temporal_answer(t):
    frames = [t[f"frame{f}"] for f in range(TEMPORAL_FRAMES)]
    layers = [t[f"layers{f}"] for f in range(TEMPORAL_FRAMES)]
    num, den, accepted, offered = ax.temporal_sums(frames, ax.equal_across(layers, TEMPORAL_T), TEMPORAL_T, TEMPORAL_K)
    return ax.quotient(num, den), accepted / max(offered, 1)


# ---- the luminance moments over three frames, output 1: atrous_variance_inputs' frames and layers, one period of them -----------------
MOMENTS_REACH = 3           # the 7 x 7 neighbourhood


def moments_patterns(w, L):
    shape = (PERIOD, w)
    out = {}
    for f in range(TEMPORAL_FRAMES):
        out[f"frame{f}"] = np.array(avi.frame_of(shape, f, np.float32))
        out[f"layers{f}"] = [np.array(l) for l in avi.layers_of(shape, L, np.float32, f)]
    return out


def moments_reference(t, L):
    """(V_0, M2) of the float64 checker for output 1 of the frames t."""
    frames = [t[f"frame{f}"] for f in range(TEMPORAL_FRAMES)]
    layers = [t[f"layers{f}"] for f in range(TEMPORAL_FRAMES)]
    return np_atrous_variance.moments(frames, layers, avi.sigmas_of(L), k=TEMPORAL_K, t=TEMPORAL_T)


# ---- the median: median_inputs' exact scene, one period of it -------------------------------------------------------------------------
def median_patterns(w, seed=2):
    """Frame of integers / 8 with NaN, +-Inf and fireflies, and a float32 guide of integer levels (weights 0 or 1 at mi.EXACT_SIGMA)."""
    frame, guide = mi.exact_scene(PERIOD, w, seed=seed)
    return dict(frame=frame, guide=guide)


def tie_frame(h, w, seed=0):
    """A finite float32 frame (h, w, 4) with many tied values: a smooth pattern of period 37 in y, rounded to sixteenths."""
    rng = np.random.default_rng(seed)
    pat = np.round(rng.random((PERIOD, w, 4)) * 4 * 16) / 16
    yy, xx = np.mgrid[0:PERIOD, 0:w]
    pat[..., :3] += (np.round(np.sin(xx * 0.21 + yy * 0.4) * 16) / 16)[..., None]
    return tile_rows(pat.astype(np.float32), h)


# ---- the bilateral filters: a noisy frame and two uint8 guide layers of one period ------------------------------------------------------
BILATERAL_GENERIC_RADIUS = 18      # the layer modes leave the LDS-tiled kernels above radius 17 (csrc/bilateral.hip, dispatch_radius)
BILATERAL_TUNED_RADIUS = 8
BILATERAL_SIGMAS = (2.0, 0.2)      # spatial, colour


BILATERAL_JOINT_LAYERS, BILATERAL_JOINT_RADIUS = 5, 1      # more than four layers run one thread per pixel at every radius (csrc/bilateral_joint.hip)


def bilateral_patterns(w, seed=6, n_layers=2):
    """Frame: smooth colour with gamma noise, alpha 1.  Layers: smooth uint8 ramps with +-3 codes of noise, so that at colour
    sigma 0.2 many weights are neither 0 nor 1."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:PERIOD, 0:w].astype(np.float64)
    base = np.stack([0.5 + 0.4 * np.sin(xx * 0.7 + yy * 0.3), 0.5 + 0.4 * np.cos(yy * 0.5), (xx + yy) % 11 / 11.0], -1)
    frame = np.concatenate([base * rng.gamma(16.0, 1 / 16.0, (PERIOD, w, 1)), np.ones((PERIOD, w, 1))], -1).astype(np.float32)
    layers = []
    for i in range(n_layers):
        ramp = np.stack([(xx * (9 + i) + yy * 5) % 256, (yy * 7 + 31 * i) % 256, (xx + yy) * 3 % 256, np.full((PERIOD, w), 255.0)], -1)
        ramp[..., :3] += rng.integers(-3, 4, (PERIOD, w, 3))
        layers.append(np.clip(ramp, 0, 255).astype(np.uint8))
    return dict(frame=frame, layers=layers)


def bilateral_pair_patterns(w):
    """Two frames with two layers each: bilateral_patterns' and the same with the pattern's rows in reverse order."""
    a = bilateral_patterns(w)
    return dict(frame0=a["frame"], layers0=a["layers"], frame1=np.ascontiguousarray(a["frame"][::-1]),
                layers1=[np.ascontiguousarray(l[::-1]) for l in a["layers"]])


# ---- the geometry of a capped grid that strides over tiles ----------------------------------------------------------------------------
def later_tiles_height(cap, tiles_x, tile_h=16):
    """Rows of the smallest frame of tiles_x tile columns with at least 2 cap + 3 tiles."""
    return tile_h * cdiv(2 * cap + 3, tiles_x)


def rounds_of(tiles, grid):
    """How many tiles the busiest workgroup takes when `grid` workgroups stride over `tiles` tiles."""
    return cdiv(tiles, grid)
