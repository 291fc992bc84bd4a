"""Kernel and host-to-host rates of the layer-guided bilateral by guide-layer format on one MI355X (development aid; writes
profiles/r12_bilateral_guide_formats.txt when given --out).  1080p, r = 8, L = 4 guide layers.

1. Resident, RGBA32F frame: the event time (mid_timer) of REPS back-to-back calls / REPS, median over the rounds, variants
   interleaved round by round so that every figure sees the same lease:
     yardstick   mid_bilateral_layers with RGBA8 guides: bilateral.hip's kernel;
     RGBA8       the same filter on bilateral_temporal.hip's kernel: mid_bilateral_temporal, one frame, k = 0;
     RGBA16F, RGBA32F   mid_bilateral_layers with MID_FMT_WITH_GUIDE: bilateral_temporal.hip's guide-format kernels.
   The float guides hold c / 255 of the RGBA8 guides and the half guides hold the float ones rounded, so all four filter the
   same picture (the first three to the same bits, which the tool checks).
2. Host to host: mid_sequence_bilateral over 64 RGBA8 frames in and out with 4 layers each of every format, page-locked,
   overlap = 1: wall time, Mpixel/s, and from mid_pipe_last_timeline the share of the wall time the compute stage spans."""
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
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--frames", type=int, default=64)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: {lib.mid_last_error().decode()}")


W, H, R, L, DISTINCT = 1920, 1080, 8, 4, 4
NPIX = W * H
SS, SC = 2.0, 0.2
FORMATS = {"RGBA8": mid.FMT_RGBA8, "RGBA16F": mid.FMT_RGBA16F, "RGBA32F": mid.FMT_RGBA32F}
ctx = mid.Context(0)
say(f"device {ctx.name}; 1080p, r = {R}, L = {L}, sigma_s = {SS}, sigma_c = {SC}; {args.rounds} rounds x {args.reps} calls per figure")
rng = np.random.default_rng(12)
yy, xx = np.mgrid[0:H, 0:W]


def guide(i):
    return np.clip(np.stack([xx * (i % 4 + 1) % 256, yy * 2 % 256, (xx + yy) // 2 % 256, np.full_like(xx, 255)], -1)
                   + rng.integers(-3, 4, (H, W, 4)), 0, 255).astype(np.uint8)


g8 = [guide(i) for i in range(DISTINCT * L)]
g32 = [g.astype(np.float32) / np.float32(255) for g in g8]
guides = {"RGBA8": g8, "RGBA16F": [g.astype(np.float16) for g in g32], "RGBA32F": g32}
frames = [np.concatenate([rng.random((H, W, 3), dtype=np.float32), np.ones((H, W, 1), np.float32)], 2) for _ in range(DISTINCT)]

# ---- 1. resident ----
d_in, d_out = ctx.upload(frames[0]), {name: ctx.alloc(NPIX * 16) for name in ("yardstick", *FORMATS)}
d_g = {name: [ctx.upload(g) for g in gs[:L]] for name, gs in guides.items()}
tbl = {name: (ctypes.c_void_p * L)(*[d.ptr for d in ds]) for name, ds in d_g.items()}
timer = ctypes.c_void_p()
ok(lib.mid_timer_create(ctx.handle, ctypes.byref(timer)), "mid_timer_create")


def params(fmt):
    return mid.BilateralParams(W, H, SS, SC, R, mid.LAYOUT_TEXTURE, fmt)


p_plain = params(mid.FMT_RGBA32F)
fr1 = (ctypes.c_void_p * 1)(d_in.ptr)
calls = {"yardstick": lambda: ok(lib.mid_bilateral_layers(ctx.handle, ctypes.byref(p_plain), d_in.ptr, tbl["RGBA8"], L, d_out["yardstick"].ptr, None), "layers"),
         "RGBA8": lambda: ok(lib.mid_bilateral_temporal(ctx.handle, ctypes.byref(p_plain), fr1, tbl["RGBA8"], L, 1, 0, 0, 1,
                                                        (ctypes.c_void_p * 1)(d_out["RGBA8"].ptr), mid.FMT_RGBA32F, None), "temporal")}
for name in ("RGBA16F", "RGBA32F"):
    calls[name] = lambda name=name, p=params(fmt_with_guide(mid.FMT_RGBA32F, FORMATS[name])): ok(
        lib.mid_bilateral_layers(ctx.handle, ctypes.byref(p), d_in.ptr, tbl[name], L, d_out[name].ptr, None), "layers")


def timed(fn, reps=args.reps):
    fn()
    ok(lib.mid_timer_tick(timer, None), "tick")
    for _ in range(reps):
        fn()
    ok(lib.mid_timer_tock(timer, None), "tock")
    ms = ctypes.c_float()
    ok(lib.mid_timer_ms(timer, ctypes.byref(ms)), "ms")
    return ms.value / reps


res = {k: [] for k in calls}
for _ in range(args.rounds):
    for k, fn in calls.items():
        res[k].append(timed(fn))
med = {k: statistics.median(v) for k, v in res.items()}
outs = {k: ctx.download(d, (H, W, 4), np.float32) for k, d in d_out.items()}
same = all(np.array_equal(outs["yardstick"].view(np.uint32), outs[k].view(np.uint32)) for k in ("RGBA8", "RGBA32F"))
say(f"\nresident, one RGBA32F frame, kernel time per call (guide traffic at L = {L}: {L * NPIX * 4 / 1e6:.0f} / {L * NPIX * 8 / 1e6:.0f} / {L * NPIX * 16 / 1e6:.0f} MB):")
say("  guides     kernel                              ms per call   (spread)          /yardstick")
for k, what in (("yardstick", "bilateral.hip, mid_bilateral_layers"), ("RGBA8", "bilateral_temporal.hip, k = 0"),
                ("RGBA16F", "bilateral_temporal.hip, guide kernel"), ("RGBA32F", "bilateral_temporal.hip, guide kernel")):
    say(f"  {'RGBA8' if k == 'yardstick' else k:9}  {what:36} {med[k]:9.4f}   ({min(res[k]):.4f}-{max(res[k]):.4f})  {med[k] / med['yardstick']:9.3f}")
say(f"  outputs of the yardstick, the RGBA8 and the RGBA32F (c / 255) guides bit-identical: {same}")
for d in (d_in, *d_out.values(), *[x for ds in d_g.values() for x in ds]):
    d.free()

# ---- 2. host to host ----
n = args.frames
say(f"\nhost to host, mid_sequence_bilateral, {n} x 1080p RGBA8 in and out, {L} layers per frame, pinned, overlap = 1")
src = [(f * 255).astype(np.uint8) for f in frames]
pin_in, pin_out = mid.PinnedFrames(ctx, src), mid.PinnedFrames(ctx, n, NPIX * 4)
pin_l = {name: mid.PinnedFrames(ctx, gs) for name, gs in guides.items()}
hin = [pin_in.ptrs[i % DISTINCT] for i in range(n)]
stats = {name: ([], []) for name in FORMATS}
for _ in range(args.rounds):
    for name, fmt in FORMATS.items():
        hl = [pin_l[name].ptrs[(i % DISTINCT) * L + j] for i in range(n) for j in range(L)]
        word = mid.FMT_RGBA8 if name == "RGBA8" else fmt_with_guide(mid.FMT_RGBA8, fmt)
        t = ctx.sequence_bilateral_pinned(hin, pin_out.ptrs, W, H, word, R, SS, SC, "texture", hl, L, True, np.uint8)
        _, o = ctx.pipe_last_timeline()
        stats[name][0].append(t[0])
        stats[name][1].append(max(x[2] for x in o) - min(x[1] for x in o))
for name, (walls, spans) in stats.items():
    wall = statistics.median(walls)
    up = (NPIX * 4 + L * NPIX * {"RGBA8": 4, "RGBA16F": 8, "RGBA32F": 16}[name]) / 1e6
    say(f"  {name:8} layers: {wall:8.2f} ms wall ({min(walls):.2f}-{max(walls):.2f}), {n * NPIX / wall / 1e3:7.1f} Mpixel/s, {wall / n:.3f} ms per frame, "
        f"{up:.0f} MB uploaded per frame = {up * n / wall:.1f} GB/s; compute stage spans {statistics.median(spans) / wall:.3f} of the wall time")
for b in (pin_in, pin_out, *pin_l.values()):
    b.free()
lib.mid_timer_destroy(timer)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
