"""Kernel and host-to-host rates of the variance-guided a-trous filter on one MI355X (development aid; writes
profiles/r20_atrous_variance.txt when given --out).  1080p, one lease, variants interleaved round by round; a figure is the event
time (mid_timer) of REPS back-to-back calls / REPS, median over the rounds, with the spread over the rounds beside it.

1. One variance pass per step (mid_atrous_variance, one pass, first_pass = i, sigmaLum 4) against the mid_atrous_joint pass at the
   same step with the colour term on.  L = 1 .. 4 and 16; RGBA32F frames, RGBA8 guides.
   Expectation from the code: the tap reads go from 4 + 3 L to 5 + 3 L words, nine centre loads and one sqrt and division per
   pixel are added: about (5 + 3 L) / (4 + 3 L) x plus a few percent.
2. The moments (mid_atrous_moments) at k = 0 and 2, L = 1 .. 4: time per (frame, tap) against mid_bilateral_joint at radius 3 (the
   same 49 taps per frame, with a colour sum).
3. The whole filter -- moments at k = 2 plus five passes -- against five passes of mid_atrous_joint, three layers.
4. Host to host over 64 RGBA8 frames with 4 RGBA8 layers, page-locked, overlap = 1: mid_sequence_atrous_variance at k = 2 (five
   passes) against mid_sequence_atrous_joint_temporal at k = 2."""
import argparse
import ctypes
import statistics
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

import image_denoising_filter_amd as mid  # noqa: E402
from image_denoising_filter_amd._lib import lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--frames", type=int, default=64)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: {lib.mid_last_error().decode()}")


W, H, NF, LRES = 1920, 1080, 5, 4                  # five frames (k = 2), four distinct layers per frame (layer l of L = 16 is layer l mod 4)
NPIX = W * H
SIGMAS = [0.2, 0.3, 0.15, 0.25]
ctx = mid.Context(0)
say(f"device {ctx.name}; 1080p RGBA32F frames, RGBA8 guides; sigmas {SIGMAS} (repeated); {args.rounds} rounds x {args.reps} calls per figure")
rng = np.random.default_rng(20)
yy, xx = np.mgrid[0:H, 0:W]


def guide(f, i):
    return np.clip(np.stack([(xx + 2 * f) * (i % 4 + 1) % 256, yy * 2 % 256, (xx + yy + f) // 2 % 256, np.full_like(xx, 255)], -1)
                   + rng.integers(-3, 4, (H, W, 4)), 0, 255).astype(np.uint8)


g8 = [[guide(f, i) for i in range(LRES)] for f in range(NF)]
f32 = [np.concatenate([rng.random((H, W, 3), dtype=np.float32), np.ones((H, W, 1), np.float32)], 2) for _ in range(NF)]
d_fr = [ctx.upload(f) for f in f32]
d_g = [[ctx.upload(g) for g in gs] for gs in g8]
d_out, d_scr = ctx.alloc(NPIX * 16), ctx.alloc(2 * NPIX * 20)
d_v0, d_v1 = ctx.upload(rng.random((H, W), dtype=np.float32) * np.float32(0.1)), ctx.alloc(NPIX * 4)
timer = ctypes.c_void_p()
ok(lib.mid_timer_create(ctx.handle, ctypes.byref(timer)), "mid_timer_create")
F32 = mid.FMT_RGBA32F


def sig(L):
    return (ctypes.c_float * L)(*[SIGMAS[l % 4] for l in range(L)])


def window(k):
    return range(2 - k, 2 + k + 1)


def tables(L, k):
    return ((ctypes.c_void_p * (2 * k + 1))(*[d_fr[f].ptr for f in window(k)]),
            (ctypes.c_void_p * ((2 * k + 1) * L))(*[d_g[f][l % LRES].ptr for f in window(k) for l in range(L)]))


def call_joint(L, first, passes, cs):
    p = mid.AtrousParams(W, H, first, passes, cs, F32)
    tbl, sg = (ctypes.c_void_p * L)(*[d_g[2][l % LRES].ptr for l in range(L)]), sig(L)
    return lambda: ok(lib.mid_atrous_joint(ctx.handle, ctypes.byref(p), sg, d_fr[2].ptr, tbl, L, d_out.ptr, F32, d_scr.ptr, None), "mid_atrous_joint")


def call_variance(L, first, passes):
    p = mid.AtrousVarianceParams(W, H, first, passes, 4.0, 1e-3, F32)
    tbl, sg = (ctypes.c_void_p * L)(*[d_g[2][l % LRES].ptr for l in range(L)]), sig(L)
    return lambda: ok(lib.mid_atrous_variance(ctx.handle, ctypes.byref(p), sg, d_fr[2].ptr, d_v0.ptr, tbl, L, d_out.ptr, F32, d_v1.ptr, d_scr.ptr, None),
                      "mid_atrous_variance")


def call_moments(L, k, into):
    p = mid.AtrousMomentsParams(W, H, F32)
    (fr, tbl), sg = tables(L, k), sig(L)
    return lambda: ok(lib.mid_atrous_moments(ctx.handle, ctypes.byref(p), sg, fr, tbl, L, 2 * k + 1, k, k, into.ptr, None), "mid_atrous_moments")


def call_bilateral(L, k, radius):
    p = mid.BilateralParams(W, H, 2.0, 0.2, radius, mid.LAYOUT_TEXTURE, F32)
    (fr, tbl), sg = tables(L, k), sig(L)
    ou = (ctypes.c_void_p * 1)(d_out.ptr)
    return lambda: ok(lib.mid_bilateral_joint(ctx.handle, ctypes.byref(p), sg, fr, tbl, L, 2 * k + 1, k, k, 1, ou, F32, None), "mid_bilateral_joint")


def timed(fn, reps=args.reps):
    fn()
    ok(lib.mid_timer_tick(timer, None), "tick")
    for _ in range(reps):
        fn()
    ok(lib.mid_timer_tock(timer, None), "tock")
    ms = ctypes.c_float()
    ok(lib.mid_timer_ms(timer, ctypes.byref(ms)), "ms")
    return ms.value / reps


LS = (1, 2, 3, 4, 16)
calls = {}
for L in LS:
    for i in range(8):
        calls[("joint", L, i)] = call_joint(L, i, 1, 1.0)
        calls[("variance", L, i)] = call_variance(L, i, 1)
for L in (1, 2, 3, 4):
    for k in (0, 2):
        calls[("moments", L, k)] = call_moments(L, k, d_v1)
        calls[("bilateral r3", L, k)] = call_bilateral(L, k, 3)
whole_m, whole_v = call_moments(3, 2, d_v0), call_variance(3, 0, 5)
calls[("whole", 3, 0)] = lambda: (whole_m(), whole_v())
calls[("five joint", 3, 0)] = call_joint(3, 0, 5, 1.0)
res = {key: [] for key in calls}
for _ in range(args.rounds):
    for key, fn in calls.items():
        res[key].append(timed(fn))
med = {key: statistics.median(v) for key, v in res.items()}


def fig(key):
    return f"{med[key]:7.4f} ({min(res[key]):.4f}-{max(res[key]):.4f})"


say("\n1. one variance pass against the mid_atrous_joint pass (colorSigma 1) at the same step; kernel ms per call (spread), ratio, and the")
say("   ratio of the tap words (5 + 3 L) / (4 + 3 L):")
for L in LS:
    say(f"  L = {L}: tap words x {(5 + 3 * L) / (4 + 3 * L):.3f}")
    for i in range(8):
        r = med[("variance", L, i)] / med[("joint", L, i)]
        say(f"    step {2 ** i:3}   joint {fig(('joint', L, i))}   variance {fig(('variance', L, i))}   x {r:.3f}")

say("\n2. the moments against mid_bilateral_joint at radius 3 (49 taps per frame each); kernel ms per call, ns per (Mpixel-frame, tap) in brackets:")
for L in (1, 2, 3, 4):
    for k in (0, 2):
        m, b = med[("moments", L, k)], med[("bilateral r3", L, k)]
        per = 1e6 / (NPIX / 1e6 * (2 * k + 1) * 49)
        say(f"  L = {L} k = {k}: moments {fig(('moments', L, k))} [{m * per:.1f}]   bilateral r = 3 {fig(('bilateral r3', L, k))} [{b * per:.1f}]   x {m / b:.3f}")

say("\n3. the whole filter (moments at k = 2, then five variance passes) against five passes of mid_atrous_joint (colorSigma 1), three layers:")
say(f"  whole {fig(('whole', 3, 0))}   five joint passes {fig(('five joint', 3, 0))}   x {med[('whole', 3, 0)] / med[('five joint', 3, 0)]:.3f}   "
    f"(moments at k = 2 alone: {fig(('moments', 3, 2))})")
for d in (*d_fr, d_out, d_scr, d_v0, d_v1, *[x for ds in d_g for x in ds]):
    d.free()

# ---- 4. host to host ----
n, L, NSRC = args.frames, 4, 4
say(f"\n4. host to host, {n} x 1080p RGBA8 in and out, {L} RGBA8 layers per frame, pinned, overlap = 1, five passes, k = 2")
src = [np.roll((f32[0] * 255).astype(np.uint8), 7 * i, 1) for i in range(NSRC)]
pin_in, pin_out, pin_l = mid.PinnedFrames(ctx, src), mid.PinnedFrames(ctx, n, NPIX * 4), mid.PinnedFrames(ctx, g8[0])
hin = [pin_in.ptrs[i % NSRC] for i in range(n)]
hl = [pin_l.ptrs[j] for i in range(n) for j in range(L)]
KINDS = ("a-trous over neighbouring frames", "variance-guided a-trous")
stats = {kind: ([], []) for kind in KINDS}
for _ in range(args.rounds):
    for kind, (walls, spans) in stats.items():
        if kind == KINDS[0]:
            t = ctx.sequence_atrous_joint_temporal_pinned(hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, hl, L, SIGMAS, 2, 0, n, 5, 0.0, True, np.uint8)
        else:
            t = ctx.sequence_atrous_variance_pinned(hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, hl, L, SIGMAS, 2, 0, n, 5, 4.0, 1e-3, True, np.uint8)
        _, o = ctx.pipe_last_timeline()
        walls.append(t[0])
        spans.append(max(x[2] for x in o) - min(x[1] for x in o))
rate = {}
for kind, (walls, spans) in stats.items():
    wall = statistics.median(walls)
    rate[kind] = n * NPIX / wall / 1e3
    say(f"  {kind:34}: {wall:8.2f} ms wall ({min(walls):.2f}-{max(walls):.2f}), {rate[kind]:7.1f} Mpixel/s, {wall / n:.3f} ms per frame; "
        f"compute stage spans {statistics.median(spans) / wall:.3f} of the wall time")
say(f"  variance-guided / over neighbouring frames {rate[KINDS[1]] / rate[KINDS[0]]:.3f}")
for bb in (pin_in, pin_out, pin_l):
    bb.free()
lib.mid_timer_destroy(timer)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
