"""Kernel and host-to-host rates of the joint bilateral against the layered bilateral on one MI355X (development aid; writes
profiles/r13_bilateral_joint.txt when given --out).  1080p, r = 8, one lease, variants interleaved round by round.

1. Resident, RGBA32F frames, output 2 of a five-frame sequence (k = 0: one neighbour, k = 2: five): the event time (mid_timer) of
   REPS back-to-back calls / REPS, median over the rounds, for L = 1 .. 4 layers and RGBA8 / RGBA32F guides:
     layered   mid_bilateral_temporal with the layer table: one complete filter per layer, L exps per tap (the yardstick: that
               kernel is not changed by the joint filter);
     joint     mid_bilateral_joint on the same frames and layers, one sigma per layer: one exp per tap.
   Expectation for L = 1: joint <= 1.1 x layered (the same tap loop plus a run-time layer count; the two give the same bits, which
   the tool checks).  For L >= 2 no threshold is fixed; the ratios are written down as they come out.
2. Host to host: mid_sequence_bilateral_joint against mid_sequence_bilateral_temporal (layered) over 64 RGBA8 frames in and out
   with 4 RGBA8 layers each, page-locked, overlap = 1, k = 0 and 2: wall time, Mpixel/s, and from mid_pipe_last_timeline the share
   of the wall time the compute stage spans."""
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


W, H, R, LMAX, NF, T = 1920, 1080, 8, 4, 5, 2
NPIX = W * H
SS, SC = 2.0, 0.2
SIGMAS = [0.2, 0.3, 0.15, 0.25]
ctx = mid.Context(0)
say(f"device {ctx.name}; 1080p, r = {R}, sigma_s = {SS}; layered: sigma_c = {SC}; joint: sigmas {SIGMAS}; "
    f"{args.rounds} rounds x {args.reps} calls per figure")
rng = np.random.default_rng(13)
yy, xx = np.mgrid[0:H, 0:W]


def guide(i):
    return np.clip(np.stack([xx * (i % 4 + 1) % 256, yy * 2 % 256, (xx + yy) // 2 % 256, np.full_like(xx, 255)], -1)
                   + rng.integers(-3, 4, (H, W, 4)), 0, 255).astype(np.uint8)


g8 = [guide(i) for i in range(NF * LMAX)]                                            # frame-major: [f * LMAX + l]
frames = [np.concatenate([rng.random((H, W, 3), dtype=np.float32), np.ones((H, W, 1), np.float32)], 2) for _ in range(NF)]

# ---- 1. resident ----
d_fr = [ctx.upload(f) for f in frames]
d_g = {"RGBA8": [ctx.upload(g) for g in g8], "RGBA32F": [ctx.upload(g.astype(np.float32) / np.float32(255)) for g in g8]}
d_out = {k: ctx.alloc(NPIX * 16) for k in ("layered", "joint")}
fr_tbl = (ctypes.c_void_p * NF)(*[d.ptr for d in d_fr])
timer = ctypes.c_void_p()
ok(lib.mid_timer_create(ctx.handle, ctypes.byref(timer)), "mid_timer_create")


def table(gname, L):
    return (ctypes.c_void_p * (NF * L))(*[d_g[gname][f * LMAX + l].ptr for f in range(NF) for l in range(L)])


def call_layered(p, tbl, L, k):
    ok(lib.mid_bilateral_temporal(ctx.handle, ctypes.byref(p), fr_tbl, tbl, L, NF, k, T, 1, (ctypes.c_void_p * 1)(d_out["layered"].ptr),
                                  mid.FMT_RGBA32F, None), "mid_bilateral_temporal")


def call_joint(p, sg, tbl, L, k):
    ok(lib.mid_bilateral_joint(ctx.handle, ctypes.byref(p), sg, fr_tbl, tbl, L, NF, k, T, 1, (ctypes.c_void_p * 1)(d_out["joint"].ptr),
                               mid.FMT_RGBA32F, None), "mid_bilateral_joint")


def timed(fn, reps=args.reps):
    fn()
    ok(lib.mid_timer_tick(timer, None), "tick")
    for _ in range(reps):
        fn()
    ok(lib.mid_timer_tock(timer, None), "tock")
    ms = ctypes.c_float()
    ok(lib.mid_timer_ms(timer, ctypes.byref(ms)), "ms")
    return ms.value / reps


calls = {}
for gname, gfmt in (("RGBA8", mid.FMT_RGBA8), ("RGBA32F", mid.FMT_RGBA32F)):
    word = mid.FMT_RGBA32F if gname == "RGBA8" else fmt_with_guide(mid.FMT_RGBA32F, gfmt)
    p = mid.BilateralParams(W, H, SS, SC, R, mid.LAYOUT_TEXTURE, word)
    for L in range(1, LMAX + 1):
        tbl = table(gname, L)
        sg = (ctypes.c_float * L)(*([SC] if L == 1 else SIGMAS[:L]))                   # L = 1: the layered filter's own sigma
        for k in (0, 2):
            calls[(gname, L, k, "layered")] = lambda p=p, tbl=tbl, L=L, k=k: call_layered(p, tbl, L, k)
            calls[(gname, L, k, "joint")] = lambda p=p, sg=sg, tbl=tbl, L=L, k=k: call_joint(p, sg, tbl, L, k)
res = {key: [] for key in calls}
for _ in range(args.rounds):
    for key, fn in calls.items():
        res[key].append(timed(fn))
med = {key: statistics.median(v) for key, v in res.items()}
same = []
for gname in ("RGBA8", "RGBA32F"):
    for k in (0, 2):
        calls[(gname, 1, k, "layered")]()
        calls[(gname, 1, k, "joint")]()
        a, b = (ctx.download(d_out[x], (H, W, 4), np.float32) for x in ("layered", "joint"))
        same.append(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
say("\nresident, output 2 of 5 RGBA32F frames, kernel time per call in ms (spread over the rounds):")
say("  guides    L  k   layered                      joint                        joint / layered")
worst_l1 = 0.0
for (gname, L, k, kind), m in med.items():
    if kind != "layered":
        continue
    j = (gname, L, k, "joint")
    ratio = med[j] / m
    if L == 1:
        worst_l1 = max(worst_l1, ratio)
    say(f"  {gname:8} {L:2} {k:2}  {m:8.4f} ({min(res[(gname, L, k, kind)]):.4f}-{max(res[(gname, L, k, kind)]):.4f})"
        f"   {med[j]:8.4f} ({min(res[j]):.4f}-{max(res[j]):.4f})   {ratio:7.3f}")
say(f"  L = 1: joint and layered outputs bit-identical: {all(same)}; worst joint / layered {worst_l1:.3f} "
    f"(expectation <= 1.1: {'met' if worst_l1 <= 1.1 else 'missed'})")
for L in range(2, LMAX + 1):
    rs = [med[(g, L, k, "joint")] / med[(g, L, k, "layered")] for g in ("RGBA8", "RGBA32F") for k in (0, 2)]
    say(f"  L = {L}: joint / layered {min(rs):.3f} .. {max(rs):.3f} (expectation 'cheaper than the layered form': "
        f"{'met' if max(rs) < 1.0 else 'missed'})")
for d in (*d_fr, *d_out.values(), *[x for ds in d_g.values() for x in ds]):
    d.free()

# ---- 2. host to host ----
n, L = args.frames, LMAX
say(f"\nhost to host, {n} x 1080p RGBA8 in and out, {L} RGBA8 layers per frame, pinned, overlap = 1")
src = [(f * 255).astype(np.uint8) for f in frames]
pin_in, pin_out, pin_l = mid.PinnedFrames(ctx, src), mid.PinnedFrames(ctx, n, NPIX * 4), mid.PinnedFrames(ctx, g8)
hin = [pin_in.ptrs[i % NF] for i in range(n)]
hl = [pin_l.ptrs[(i % NF) * LMAX + j] for i in range(n) for j in range(L)]
stats = {(kind, k): ([], []) for k in (0, 2) for kind in ("layered", "joint")}
for _ in range(args.rounds):
    for (kind, k), (walls, spans) in stats.items():
        if kind == "joint":
            t = ctx.sequence_bilateral_joint_pinned(hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, hl, L, SIGMAS, k, 0, n, R, SS, SC, True, np.uint8)
        else:
            t = ctx.sequence_bilateral_temporal_pinned(hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, k, 0, n, R, SS, SC, hl, L, True, np.uint8)
        _, o = ctx.pipe_last_timeline()
        walls.append(t[0])
        spans.append(max(x[2] for x in o) - min(x[1] for x in o))
for (kind, k), (walls, spans) in stats.items():
    wall = statistics.median(walls)
    say(f"  {kind:8} k = {k}: {wall:8.2f} ms wall ({min(walls):.2f}-{max(walls):.2f}), {n * NPIX / wall / 1e3:7.1f} Mpixel/s, {wall / n:.3f} ms per frame; "
        f"compute stage spans {statistics.median(spans) / wall:.3f} of the wall time")
for b in (pin_in, pin_out, pin_l):
    b.free()
lib.mid_timer_destroy(timer)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
