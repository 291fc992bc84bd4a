"""Kernel and host-to-host rates of the a-trous filter over neighbouring frames on one MI355X (development aid; writes
profiles/r19_atrous_temporal.txt when given --out).  1080p, one lease, variants interleaved round by round; a figure is the event
time (mid_timer) of REPS back-to-back calls / REPS, median over the rounds, with the spread over the rounds beside it.

1. The temporal pass (mid_atrous_joint_temporal, one pass, the middle output of 2k + 1 frames) against (2k + 1) x the step-1 pass
   of mid_atrous_joint on one of those frames.  k = 1, 2; L = 1 .. 4 and 16; RGBA8 and RGBA32F guides; RGBA32F frames.
   Expectation (DESIGN 3.7's "one more loop"): 1.0 - 1.1 x per neighbour.
2. Five passes at k = 2 with three layers against five passes at k = 0 (mid_atrous_joint) and against mid_bilateral_joint at
   radius 8, k = 2.  No ratio is fixed in advance.
3. Host to host over 64 RGBA8 frames with 4 RGBA8 layers, page-locked, overlap = 1: mid_sequence_atrous_joint_temporal at k = 2
   (five passes) against mid_sequence_bilateral_joint at k = 2, radius 8, and against mid_sequence_atrous_joint (k = 0)."""
import argparse
import ctypes
import statistics
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

import image_denoising_filter_amd as mid  # noqa: E402
from image_denoising_filter_amd._lib import lib  # noqa: E402
from image_denoising_filter_amd.api import fmt_with_guide  # noqa: E402

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
say(f"device {ctx.name}; 1080p RGBA32F frames; sigmas {SIGMAS} (repeated), no colour term; {args.rounds} rounds x {args.reps} calls per figure")
rng = np.random.default_rng(19)
yy, xx = np.mgrid[0:H, 0:W]


def guide(f, i):
    return np.clip(np.stack([(xx + 2 * f) * (i % 4 + 1) % 256, yy * 2 % 256, (xx + yy + f) // 2 % 256, np.full_like(xx, 255)], -1)
                   + rng.integers(-3, 4, (H, W, 4)), 0, 255).astype(np.uint8)


g8 = [[guide(f, i) for i in range(LRES)] for f in range(NF)]
f32 = [np.concatenate([rng.random((H, W, 3), dtype=np.float32), np.ones((H, W, 1), np.float32)], 2) for _ in range(NF)]
d_fr = [ctx.upload(f) for f in f32]
d_g = {"RGBA8": [[ctx.upload(g) for g in gs] for gs in g8],
       "RGBA32F": [[ctx.upload(g.astype(np.float32) / np.float32(255)) for g in gs] for gs in g8]}
d_out, d_scr = ctx.alloc(NPIX * 16), ctx.alloc(2 * NPIX * 16)
timer = ctypes.c_void_p()
ok(lib.mid_timer_create(ctx.handle, ctypes.byref(timer)), "mid_timer_create")


def word(gname):
    return mid.FMT_RGBA32F if gname == "RGBA8" else fmt_with_guide(mid.FMT_RGBA32F, mid.FMT_RGBA32F)


def sig(L):
    return (ctypes.c_float * L)(*[SIGMAS[l % 4] for l in range(L)])


def window(k):
    """The 2k + 1 middle frames of the five, the output in their middle."""
    return range(2 - k, 2 + k + 1)


def call_temporal(gname, L, k, passes):
    p = mid.AtrousParams(W, H, 0, passes, 0.0, word(gname))
    fr = (ctypes.c_void_p * (2 * k + 1))(*[d_fr[f].ptr for f in window(k)])
    tbl = (ctypes.c_void_p * ((2 * k + 1) * L))(*[d_g[gname][f][l % LRES].ptr for f in window(k) for l in range(L)])
    ou, sg = (ctypes.c_void_p * 1)(d_out.ptr), sig(L)
    return lambda: ok(lib.mid_atrous_joint_temporal(ctx.handle, ctypes.byref(p), sg, fr, tbl, L, 2 * k + 1, k, k, 1, ou, mid.FMT_RGBA32F, d_scr.ptr,
                                                    None), "mid_atrous_joint_temporal")


def call_single(gname, L, passes):
    p = mid.AtrousParams(W, H, 0, passes, 0.0, word(gname))
    tbl, sg = (ctypes.c_void_p * L)(*[d_g[gname][2][l % LRES].ptr for l in range(L)]), sig(L)
    return lambda: ok(lib.mid_atrous_joint(ctx.handle, ctypes.byref(p), sg, d_fr[2].ptr, tbl, L, d_out.ptr, mid.FMT_RGBA32F, d_scr.ptr, None),
                      "mid_atrous_joint")


def call_bilateral(gname, L, k, radius):
    p = mid.BilateralParams(W, H, 2.0, 0.2, radius, mid.LAYOUT_TEXTURE, word(gname))
    fr = (ctypes.c_void_p * (2 * k + 1))(*[d_fr[f].ptr for f in window(k)])
    tbl = (ctypes.c_void_p * ((2 * k + 1) * L))(*[d_g[gname][f][l % LRES].ptr for f in window(k) for l in range(L)])
    ou, sg = (ctypes.c_void_p * 1)(d_out.ptr), sig(L)
    return lambda: ok(lib.mid_bilateral_joint(ctx.handle, ctypes.byref(p), sg, fr, tbl, L, 2 * k + 1, k, k, 1, ou, mid.FMT_RGBA32F, None),
                      "mid_bilateral_joint")


def timed(fn, reps=args.reps):
    fn()
    ok(lib.mid_timer_tick(timer, None), "tick")
    for _ in range(reps):
        fn()
    ok(lib.mid_timer_tock(timer, None), "tock")
    ms = ctypes.c_float()
    ok(lib.mid_timer_ms(timer, ctypes.byref(ms)), "ms")
    return ms.value / reps


GUIDES, LS = ("RGBA8", "RGBA32F"), (1, 2, 3, 4, 16)
calls = {}
for gname in GUIDES:
    for L in LS:
        calls[("step 1", gname, L)] = call_single(gname, L, 1)
        for k in (1, 2):
            calls[(f"temporal k={k}", gname, L)] = call_temporal(gname, L, k, 1)
    calls[("5 passes k=0", gname, 3)] = call_single(gname, 3, 5)
    calls[("5 passes k=2", gname, 3)] = call_temporal(gname, 3, 2, 5)
    calls[("bil r8 k=2", gname, 3)] = call_bilateral(gname, 3, 2, 8)
res = {key: [] for key in calls}
for _ in range(args.rounds):
    for key, fn in calls.items():
        res[key].append(timed(fn))
med = {key: statistics.median(v) for key, v in res.items()}


def fig(key):
    return f"{med[key]:8.4f} ({min(res[key]):.4f}-{max(res[key]):.4f})"


say("\n1. the temporal pass over 2k + 1 frames against (2k + 1) x the step-1 pass of mid_atrous_joint; kernel ms per call (spread):")
say("  guides    L    step 1, one frame            k = 1: temporal pass           per neighbour   k = 2: temporal pass           per neighbour")
lo, hi, over = 1e9, 0.0, []
for gname in GUIDES:
    for L in LS:
        one = med[("step 1", gname, L)]
        r = [med[(f"temporal k={k}", gname, L)] / ((2 * k + 1) * one) for k in (1, 2)]
        lo, hi = min(lo, *r), max(hi, *r)
        over += [f"{gname} L={L} k={k} {x:.3f}" for k, x in zip((1, 2), r) if x > 1.1]
        say(f"  {gname:8} {L:2}   {fig(('step 1', gname, L))}   {fig(('temporal k=1', gname, L))}   {r[0]:7.3f}         "
            f"{fig(('temporal k=2', gname, L))}   {r[1]:7.3f}")
say(f"  per neighbour, temporal / ((2k + 1) x step 1): {lo:.3f} .. {hi:.3f} (expectation at most 1.1: "
    f"{'met in every row' if not over else 'missed in ' + ', '.join(over)})")

say("\n2. five passes with three layers: k = 2 against k = 0 (mid_atrous_joint) and against mid_bilateral_joint at radius 8, k = 2:")
for gname in GUIDES:
    a0, a2, b2 = ("5 passes k=0", gname, 3), ("5 passes k=2", gname, 3), ("bil r8 k=2", gname, 3)
    say(f"  {gname:8}  a-trous k = 0 {fig(a0)}   a-trous k = 2 {fig(a2)}   bilateral r = 8, k = 2 {fig(b2)}   "
        f"k = 2 / k = 0 {med[a2] / med[a0]:.3f}   a-trous / bilateral at k = 2 {med[a2] / med[b2]:.3f}")
for d in (*d_fr, d_out, d_scr, *[x for per in d_g.values() for ds in per for x in ds]):
    d.free()

# ---- 3. host to host ----
n, L, NSRC = args.frames, 4, 4
say(f"\n3. host to host, {n} x 1080p RGBA8 in and out, {L} RGBA8 layers per frame, pinned, overlap = 1")
src = [np.roll((f32[0] * 255).astype(np.uint8), 7 * i, 1) for i in range(NSRC)]
pin_in, pin_out, pin_l = mid.PinnedFrames(ctx, src), mid.PinnedFrames(ctx, n, NPIX * 4), mid.PinnedFrames(ctx, g8[0])
hin = [pin_in.ptrs[i % NSRC] for i in range(n)]
hl = [pin_l.ptrs[j] for i in range(n) for j in range(L)]
KINDS = ("bilateral joint r = 8, k = 2", "a-trous, 5 passes, k = 0", "a-trous, 5 passes, k = 2")
stats = {kind: ([], []) for kind in KINDS}
for _ in range(args.rounds):
    for kind, (walls, spans) in stats.items():
        if kind == KINDS[0]:
            t = ctx.sequence_bilateral_joint_pinned(hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, hl, L, SIGMAS, 2, 0, n, 8, 2.0, 0.2, True, np.uint8)
        elif kind == KINDS[1]:
            t = ctx.sequence_atrous_joint_pinned(hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, hl, L, SIGMAS, 5, 0, 0.0, 0, n, True, np.uint8)
        else:
            t = ctx.sequence_atrous_joint_temporal_pinned(hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, hl, L, SIGMAS, 2, 0, n, 5, 0.0, True, np.uint8)
        _, o = ctx.pipe_last_timeline()
        walls.append(t[0])
        spans.append(max(x[2] for x in o) - min(x[1] for x in o))
rate = {}
for kind, (walls, spans) in stats.items():
    wall = statistics.median(walls)
    rate[kind] = n * NPIX / wall / 1e3
    say(f"  {kind:30}: {wall:8.2f} ms wall ({min(walls):.2f}-{max(walls):.2f}), {rate[kind]:7.1f} Mpixel/s, {wall / n:.3f} ms per frame; "
        f"compute stage spans {statistics.median(spans) / wall:.3f} of the wall time")
say(f"  a-trous k = 2 / a-trous k = 0 {rate[KINDS[2]] / rate[KINDS[1]]:.3f}; a-trous k = 2 / bilateral joint k = 2 {rate[KINDS[2]] / rate[KINDS[0]]:.3f}")
say(f"  the rate of k = 0 (its upload bound) is {'reached at k = 2 within 5 %' if rate[KINDS[2]] >= 0.95 * rate[KINDS[1]] else 'missed at k = 2 by more than 5 %'}")
for bb in (pin_in, pin_out, pin_l):
    bb.free()
lib.mid_timer_destroy(timer)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
