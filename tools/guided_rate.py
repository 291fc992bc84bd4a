"""Rates of the guided filter on one MI355X (development aid; writes profiles/r26_guided.txt when given --out).  1080p, one lease,
variants interleaved round by round; a figure is the event time (mid_timer) of back-to-back calls / their number, median over the
rounds, with the spread over the rounds beside it (the method of DESIGN section 7).  Every call of a timed run has its own frame,
guide, workspace and output, and the sets of one variant add up to more than the 256 MiB cache.

1. mid_guided_filter (both launches) at radius 1, 2, 4, 8, 16 for RGBA8 / RGBA16F / RGBA32F frames and guides: is the time flat in
   the radius?  The geometry (csrc/guided_box.hpp) gives what "flat" can mean: a segment walks 32 + 2 r rows for 32 and a strip holds
   256 columns for 256 - 2 r, so radius 16 does (64 / 32) (256 / 224) = 2.29 and radius 2 (36 / 32) (256 / 252) = 1.14 of the
   radius-free work: a ratio of 2.00.
2. Against mid_bilateral_joint with one float guide layer at radius 8 and 16 on the same frames.
3. Against the call's algorithmic bytes (frame + guide in, 52 B per pixel through `work` each way, the output) at the
   device-to-device copy rate measured in the same run.
4. Host to host over --frames RGBA8 frames with an RGBA8 guide (mid_sequence_guided), against mid_sequence_atrous_joint with one
   layer: page-locked frames in, page-locked RGBA8 frames out.

No threshold is fixed for any of them."""
import argparse
import ctypes
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--frames", type=int, default=64)
args = ap.parse_args()

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import image_denoising_filter_amd as mid  # noqa: E402
from image_denoising_filter_amd._lib import lib  # noqa: E402
from image_denoising_filter_amd.api import PinnedFrames, fmt_with_guide  # noqa: E402

W, H = 1920, 1080
NPIX = W * H
RADII = (1, 2, 4, 8, 16)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: {lib.mid_last_error().decode()}")


F32, U8, F16 = mid.FMT_RGBA32F, mid.FMT_RGBA8, mid.FMT_RGBA16F
BYTES = {U8: 4, F16: 8, F32: 16}
NAME = {U8: "RGBA8", F16: "RGBA16F", F32: "RGBA32F"}
ctx = mid.Context(0)
say(f"device {ctx.name}; 1080p; {args.rounds} rounds x {args.reps} calls per figure")
rng = np.random.default_rng(26)
timer = ctypes.c_void_p()
ok(lib.mid_timer_create(ctx.handle, ctypes.byref(timer)), "mid_timer_create")


def timed(fns):
    for fn in fns:
        fn()
    ok(lib.mid_timer_tick(timer, None), "tick")
    for fn in fns:
        fn()
    ok(lib.mid_timer_tock(timer, None), "tock")
    ms = ctypes.c_float()
    ok(lib.mid_timer_ms(timer, ctypes.byref(ms)), "ms")
    return ms.value / len(fns)


def fig(r, key):
    return f"{statistics.median(r[key]):7.4f} ({min(r[key]):.4f}-{max(r[key]):.4f})"


# a blocky albedo as the guide, noisy albedo x light as the frame (the tests' recipe at 1080p, blocks of 32)
yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
alb = (0.15 + 0.8 * rng.random((H // 32 + 1, W // 32 + 1, 3), dtype=np.float32)).repeat(32, 0).repeat(32, 1)[:H, :W]
light = np.stack([0.6 + 0.3 * np.sin(xx * 0.005), 0.6 + 0.3 * np.cos(yy * 0.006), 0.5 + 0.2 * np.sin((xx + yy) * 0.004)], -1)
noisy = (alb * light * rng.gamma(4.0, 0.25, (H, W, 3))).astype(np.float32)
one = np.ones((H, W, 1), np.float32)
frame32, guide32 = np.concatenate([noisy, one], -1), np.concatenate([alb, one], -1)
as8 = lambda x: np.clip(np.rint(x * 255), 0, 255).astype(np.uint8)
host = {F32: (frame32, guide32), F16: (frame32.astype(np.float16), guide32.astype(np.float16)), U8: (as8(frame32), as8(guide32))}
SETS = args.reps
assert SETS * NPIX * (4 + 4 + 52 + 16) > 256 << 20, "the sets of the smallest variant must pass the cache"
pool = {fmt: [(ctx.upload(host[fmt][0]), ctx.upload(host[fmt][1])) for _ in range(SETS)] for fmt in (U8, F16, F32)}
works, outs = [ctx.alloc(52 * NPIX) for _ in range(SETS)], [ctx.alloc(16 * NPIX) for _ in range(SETS)]


def guided_calls(fmt, r):
    p = mid.GuidedParams(W, H, r, 1e-2, fmt_with_guide(fmt, fmt))
    return [lambda i=i: ok(lib.mid_guided_filter(ctx.handle, ctypes.byref(p), pool[fmt][i][0].ptr, pool[fmt][i][1].ptr, works[i].ptr, outs[i].ptr,
                                                 F32, None), "mid_guided_filter") for i in range(SETS)]


def joint_calls(r):
    p = mid.BilateralParams(W, H, 2.0, 0.2, r, mid.LAYOUT_TEXTURE, fmt_with_guide(F32, F32))
    calls = []
    for i in range(SETS):
        fr, ly, ou = (ctypes.c_void_p * 1)(pool[F32][i][0].ptr), (ctypes.c_void_p * 1)(pool[F32][i][1].ptr), (ctypes.c_void_p * 1)(outs[i].ptr)
        calls.append(lambda fr=fr, ly=ly, ou=ou: ok(lib.mid_bilateral_joint(ctx.handle, ctypes.byref(p), None, fr, ly, 1, 1, 0, 0, 1, ou, F32, None),
                                                    "mid_bilateral_joint"))
    return calls


variants = {(fmt, r): guided_calls(fmt, r) for fmt in (U8, F16, F32) for r in RADII}
variants.update({("joint", r): joint_calls(r) for r in (8, 16)})
a, b = torch.empty(64 << 20, dtype=torch.float32, device="cuda"), torch.empty(64 << 20, dtype=torch.float32, device="cuda")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed_copy():
    b.copy_(a)
    e0.record()
    for _ in range(args.reps):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps


res = {key: [] for key in variants}
res["copy"] = []
for _ in range(args.rounds):
    for key in res:
        res[key].append(timed_copy() if key == "copy" else timed(variants[key]))
med = {key: statistics.median(v) for key, v in res.items()}
copy_rate = 2 * a.numel() * 4 / (med["copy"] * 1e-3) / 1e9          # GB/s, bytes read + bytes written
say(f"device-to-device copy of 256 MiB: {med['copy']:.4f} ms = {copy_rate:.0f} GB/s (read + written)")
del a, b
PERIOD, LANES = 32, 256                                              # kGuidedPeriod, kGuidedLanes of csrc/guided_box.hpp
expected = ((PERIOD + 32) / PERIOD) * (LANES / (LANES - 32)) / (((PERIOD + 4) / PERIOD) * (LANES / (LANES - 4)))
say(f"\n1. mid_guided_filter (two launches), frame and guide of one format, RGBA32F out; call ms (spread) per radius; r = 16 : r = 2 against the "
    f"geometry's {expected:.2f} (warm-up rows and held columns):")
for fmt in (U8, F16, F32):
    ratio = med[(fmt, 16)] / med[(fmt, 2)]
    say(f"  {NAME[fmt]:7}: " + "  ".join(f"r={r} {fig(res, (fmt, r))}" for r in RADII))
    say(f"           r = 16 : r = 2 = {ratio:.2f}: 'flat within the restart's warm-up overhead' {'met' if ratio <= expected * 1.05 else 'missed'}; "
        f"{NPIX / med[(fmt, 8)] / 1e6:.2f} Gpixel/s at r = 8")
say("\n2. against mid_bilateral_joint with one RGBA32F guide layer on the same RGBA32F frames (sigma_s 2, sigma_c 0.2):")
for r in (8, 16):
    say(f"  r={r}: joint bilateral {fig(res, ('joint', r))}   guided {fig(res, (F32, r))}   guided is x {med[(F32, r)] / med[('joint', r)]:.2f} of it")
say("\n3. against the call's algorithmic bytes (frame + guide in twice -- each launch reads both --, 52 B/pixel written and read, 16 B/pixel out) at the copy rate:")
for fmt in (U8, F16, F32):
    bpp = 4 * BYTES[fmt] + 2 * 52 + 16
    at_copy = bpp * NPIX / (copy_rate * 1e9) * 1e3
    say(f"  {NAME[fmt]:7}: {bpp:3} B/pixel = {at_copy:.4f} ms at the copy rate; the call at r = 8 is x {med[(fmt, 8)] / at_copy:.1f} of it")
lib.mid_timer_destroy(timer)
for d in [x for v in pool.values() for pr in v for x in pr] + works + outs:
    d.free()

# ---- 4. host to host ----
n = args.frames
frames8 = [np.roll(host[U8][0], 7 * i, 1) for i in range(n)]
guides8 = [np.roll(host[U8][1], 7 * i, 1) for i in range(n)]
hin, hg, hout = PinnedFrames(ctx, frames8), PinnedFrames(ctx, guides8), PinnedFrames(ctx, n, NPIX * 4)
walls = {"guided r=8": [], "atrous 5 passes, 1 layer": []}
for _ in range(args.rounds + 1):
    walls["guided r=8"].append(ctx.sequence_guided_pinned(hin.ptrs, hout.ptrs, W, H, U8, hg.ptrs, 8, 1e-2, out_dtype=np.uint8))
    walls["atrous 5 passes, 1 layer"].append(ctx.sequence_atrous_joint_pinned(hin.ptrs, hout.ptrs, W, H, U8, hg.ptrs, 1, [0.2], out_dtype=np.uint8))
say(f"\n4. host to host, {n} RGBA8 1080p frames with one RGBA8 guide plane each, page-locked in and out, RGBA8 out; wall / kernel / copy ms of the call "
    f"(median of {args.rounds} after one warm-up call), Mpixel/s end to end:")
for kind, v in walls.items():
    v = v[1:]
    wall = statistics.median(t[0] for t in v)
    say(f"  {kind:26}: wall {wall:8.2f} ({min(t[0] for t in v):.2f}-{max(t[0] for t in v):.2f})  kernel {statistics.median(t[1] for t in v):8.2f}  "
        f"copy {statistics.median(t[2] for t in v):8.2f}   {n * NPIX / wall / 1e3:.0f} Mpixel/s")
for b_ in (hin, hg, hout):
    b_.free()
ctx.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
