"""Rates of the image metrics on one MI355X (development aid; writes profiles/r25_image_metrics.txt when given --out).  1080p, one
lease, variants interleaved round by round; a figure is the event time (mid_timer) of back-to-back calls / their number, median over
the rounds, with the spread over the rounds beside it (the method of DESIGN section 7).

1. mid_image_metrics with ssim == 0, u8 / f16 / f32 pairs: the call (both launches) against its algorithmic bytes -- both frames once
   -- at the device-to-device copy rate measured in the same run.  Every call of a timed run reads its own pair of frames and the
   pairs of one variant add up to more than the 256 MiB cache.
2. ssim == 1 without and with the map (4 B per pixel more to write), the same pairs, against (1) and against mid_color_bounds at
   radius 2 on the same frames: the nearest existing tiled statistics pass (25 taps in fp32 and fp64 against 22 separable ones in
   fp64).  And the same calls on ONE pair of planes, back to back: the warm-cache figure.
3. mi_denoise --compare --animation over --frames pairs of 1080p .png files (written by this tool into --dir): wall time of the run,
   split into decode + upload and the GPU part by a second run with --no-ssim and by (2)'s kernel time.

No threshold is fixed for any of them."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--dir", default=None, help="where part 3 writes its files (default: a temporary directory)")
args = ap.parse_args()

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import image_denoising_filter_amd as mid  # noqa: E402
from image_denoising_filter_amd._lib import lib  # noqa: E402

W, H = 1920, 1080
NPIX = W * H
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
rng = np.random.default_rng(25)
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


ref8 = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
test8 = np.clip(ref8.astype(np.int32) + rng.integers(-20, 21, (H, W, 4)), 0, 255).astype(np.uint8)
host = {U8: (test8, ref8), F32: ((test8 / np.float32(255)).astype(np.float32), (ref8 / np.float32(255)).astype(np.float32))}
host[F16] = (host[F32][0].astype(np.float16), host[F32][1].astype(np.float16))
SETS = 4 * args.reps
assert SETS * NPIX * 8 > 256 << 20, "the pairs of the smallest variant must pass the cache"
pool = {fmt: [(ctx.upload(host[fmt][0]), ctx.upload(host[fmt][1])) for _ in range(SETS)] for fmt in (U8, F16, F32)}
nw = lib.mid_image_metrics_workspace(W, H)
works, maps = [ctx.alloc(nw) for _ in range(SETS)], [ctx.alloc(NPIX * 4) for _ in range(SETS)]
los, his = [ctx.alloc(NPIX * 16) for _ in range(2)], [ctx.alloc(NPIX * 16) for _ in range(2)]


def metrics_calls(fmt, ssim, want_map, sets=SETS):
    p = mid.ImageMetricsParams(W, H, fmt, fmt, 1.0, 1e-2, ssim)
    return [lambda i=i: ok(lib.mid_image_metrics(ctx.handle, ctypes.byref(p), pool[fmt][i][0].ptr, pool[fmt][i][1].ptr, works[i].ptr,
                                                 maps[i].ptr if want_map else None, None), "mid_image_metrics") for i in range(sets)]


def bounds_calls(fmt, sets=SETS):
    p = mid.ColorBoundsParams(W, H, 2, 1.0, fmt)
    return [lambda i=i: ok(lib.mid_color_bounds(ctx.handle, ctypes.byref(p), pool[fmt][i][0].ptr, los[i % 2].ptr, his[i % 2].ptr, None), "mid_color_bounds")
            for i in range(sets)]


variants = {}
for fmt in (U8, F16, F32):
    variants[(fmt, "pointwise")] = metrics_calls(fmt, 0, False)
    variants[(fmt, "ssim")] = metrics_calls(fmt, 1, False)
    variants[(fmt, "ssim + map")] = metrics_calls(fmt, 1, True)
    variants[(fmt, "color_bounds r2")] = bounds_calls(fmt)
    variants[(fmt, "ssim + map, one pair (warm)")] = [metrics_calls(fmt, 1, True, 1)[0]] * args.reps
    variants[(fmt, "pointwise, one pair (warm)")] = [metrics_calls(fmt, 0, False, 1)[0]] * args.reps
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
say("\n1. mid_image_metrics, ssim == 0, every call on its own pair; call ms (spread), algorithmic bytes per pixel (both frames once), those bytes at the copy rate, ratio:")
for fmt in (U8, F16, F32):
    bpp = 2 * BYTES[fmt]
    at_copy = bpp * NPIX / (copy_rate * 1e9) * 1e3
    k = (fmt, "pointwise")
    say(f"  {NAME[fmt]:7}: {fig(res, k)}   {bpp:3} B/pixel = {at_copy:.4f} ms at the copy rate   x {med[k] / at_copy:.2f}   "
        f"{NPIX / med[k] / 1e6:.2f} Gpixel/s; one pair, warm: {fig(res, (fmt, 'pointwise, one pair (warm)'))}")
say("\n2. ssim == 1 without and with the map, against (1) and against mid_color_bounds at radius 2 on the same frames:")
for fmt in (U8, F16, F32):
    s, m, c, p0 = (fmt, "ssim"), (fmt, "ssim + map"), (fmt, "color_bounds r2"), (fmt, "pointwise")
    say(f"  {NAME[fmt]:7}: ssim {fig(res, s)} = x {med[s] / med[p0]:.2f} of (1); with the map {fig(res, m)} = x {med[m] / med[p0]:.2f}; "
        f"color_bounds r2 {fig(res, c)}: ssim + map is x {med[m] / med[c]:.2f} of it; one pair, warm: {fig(res, (fmt, 'ssim + map, one pair (warm)'))}; "
        f"{NPIX / med[m] / 1e6:.2f} Gpixel/s with the map")
lib.mid_timer_destroy(timer)
for d in [x for v in pool.values() for pr in v for x in pr] + works + maps + los + his:
    d.free()
gpu_ms_per_pair = med[(U8, "ssim")]
ctx.close()

# ---- 3. the CLI over files ----
n = args.frames
tmp = None
if args.dir is None:
    tmp = tempfile.TemporaryDirectory()
    args.dir = tmp.name
os.makedirs(os.path.join(args.dir, "test"), exist_ok=True)
os.makedirs(os.path.join(args.dir, "ref"), exist_ok=True)
for i in range(n):
    mid.save_image(os.path.join(args.dir, "test", f"out_{i:04d}.png"), np.roll(test8, 5 * i, 1))
    mid.save_image(os.path.join(args.dir, "ref", f"ref_{i:04d}.png"), np.roll(ref8, 5 * i, 1))
cli = os.path.join(os.path.dirname(mid.LIB_PATH), "mi_denoise")
base = [cli, "--compare", os.path.join(args.dir, "test", "out_0000.png"), os.path.join(args.dir, "ref", "ref_0000.png"), "--animation"]
walls = {"ssim": [], "--no-ssim": []}
for _ in range(args.rounds):
    for kind in walls:
        t0 = time.perf_counter()
        r = subprocess.run(base + ([] if kind == "ssim" else ["--no-ssim"]), capture_output=True, text=True, check=True)
        walls[kind].append((time.perf_counter() - t0) * 1e3)
        assert len(r.stdout.splitlines()) == n + 1
say(f"\n3. mi_denoise --compare --animation over {n} pairs of 1080p .png files (random bytes: the worst case for inflate), whole process, wall ms:")
for kind, v in walls.items():
    say(f"  {kind:9}: {statistics.median(v):8.1f} ({min(v):.1f}-{max(v):.1f}) = {statistics.median(v) / n:.2f} ms per pair")
t0 = time.perf_counter()
for i in range(n):
    mid.load_image(os.path.join(args.dir, "test", f"out_{i:04d}.png"))
    mid.load_image(os.path.join(args.dir, "ref", f"ref_{i:04d}.png"))
decode_ms = (time.perf_counter() - t0) * 1e3
say(f"  decode alone (mid_image_load of the {2 * n} files, one thread, this process): {decode_ms:.1f} ms = {decode_ms / n:.2f} ms per pair")
say(f"  the GPU part by (2): {gpu_ms_per_pair:.4f} ms per pair = {gpu_ms_per_pair * n:.1f} ms of {statistics.median(walls['ssim']):.1f}; the rest is process start, "
    f"context creation, the decode of a pair's two files side by side and two pageable uploads")
say("  the last run's (--no-ssim) mean line: " + r.stdout.splitlines()[-1][:200])
if tmp is not None:
    tmp.cleanup()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
