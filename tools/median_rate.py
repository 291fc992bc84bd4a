"""Rates of the median filters on one MI355X (development aid; writes profiles/r27_median.txt when given --out).  1080p, one lease,
variants interleaved round by round; a figure is the event time (mid_timer) of back-to-back calls / their number, median over the
rounds, with the spread over the rounds beside it (the method of DESIGN section 7).  Every call of a timed run has its own frame and
output, and the sets of one variant add up to more than the 256 MiB cache.

1. mid_median_filter at radius 1, 2, 3 with n_layers 0, 1, 3, 5 for RGBA32F and RGBA8 frames (RGBA8 layers), against the estimates from
   operation counts: 0.1 ms at radius 2 and 0.4 ms at radius 3.
2. mid_bilateral_joint at the same radius and layers in the same run: the same taps and guide tiles, the yardstick of the weighted
   classes ("weighted radius 2 within about 2 x the joint bilateral at radius 2").
3. mid_firefly_clamp at radius 1 and 2 and a device copy of the frame's bytes in and out: the yardsticks of the plain selection class at
   radius 1 ("plain radius 1 within a small factor of the copy").
4. The plain selection class against the general class on the same all-finite frame at radius 1, 2, 3: no layers against one all-zero
   layer, which gives the same values by rank counting -- the comparison that decides whether a radius keeps its network.
5. Host to host over --frames RGBA8 frames with one RGBA8 layer (mid_sequence_median at radius 2), against mid_sequence_atrous_joint with
   the same layer: page-locked frames in, page-locked RGBA8 frames out.

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
from image_denoising_filter_amd.api import PinnedFrames  # noqa: E402

W, H = 1920, 1080
NPIX = W * H
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: {lib.mid_last_error().decode()}")


F32, U8 = mid.FMT_RGBA32F, mid.FMT_RGBA8
ctx = mid.Context(0)
say(f"device {ctx.name}; 1080p; {args.rounds} rounds x {args.reps} calls per figure")
rng = np.random.default_rng(27)
timer = ctypes.c_void_p()
ok(lib.mid_timer_create(ctx.handle, ctypes.byref(timer)), "mid_timer_create")
dev = torch.device("cuda", 0)
NSETS = 8                                                   # 8 x (33 MB in + 33 MB out) > 256 MiB for RGBA32F

frames32 = [torch.from_numpy((rng.random((H, W, 4), dtype=np.float32) * 2).astype(np.float32)).to(dev) for _ in range(NSETS)]
frames8 = [torch.from_numpy(rng.integers(0, 256, (H, W, 4), dtype=np.uint8)).to(dev) for _ in range(NSETS)]
blocks = rng.integers(1, 5, (H // 6 + 1, W // 6 + 1, 4)).repeat(6, 0).repeat(6, 1)[:H, :W] * 51
yy, xx = np.mgrid[0:H, 0:W]
layers = [torch.from_numpy((blocks + ((3 * xx + 5 * yy + l) % 7)[..., None]).astype(np.uint8)).to(dev) for l in range(5)]
zero_layer = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
outs = [torch.empty((H, W, 4), dtype=torch.float32, device=dev) for _ in range(NSETS)]
SIG = [0.02, 0.1, 0.1, 0.1, 0.1]
torch.cuda.synchronize()


def timed(fn):
    """ms per call of args.reps back-to-back calls of fn(i)."""
    ok(lib.mid_timer_tick(timer, None), "tick")
    for i in range(args.reps):
        fn(i)
    ok(lib.mid_timer_tock(timer, None), "tock")
    ms = ctypes.c_float()
    ok(lib.mid_timer_ms(timer, ctypes.byref(ms)), "ms")
    return ms.value / args.reps


def median_call(fr, fmt, r, L, lay=None):
    p = mid.MedianParams(W, H, r, fmt)
    sg = (ctypes.c_float * max(L, 1))(*SIG[:L]) if L else None
    lt = (ctypes.c_void_p * max(L, 1))(*[(lay or layers)[l].data_ptr() for l in range(L)]) if L else None
    return lambda i: ok(lib.mid_median_filter(ctx.handle, ctypes.byref(p), sg, fr[i % NSETS].data_ptr(), lt, L, outs[i % NSETS].data_ptr(), F32, None), "median")


def joint_call(fr, fmt, r, L):
    p = mid.BilateralParams(W, H, 2.0, 0.2, r, 0, fmt)
    sg = (ctypes.c_float * L)(*SIG[:L])
    lt = (ctypes.c_void_p * L)(*[layers[l].data_ptr() for l in range(L)])

    def go(i):
        f = (ctypes.c_void_p * 1)(fr[i % NSETS].data_ptr())
        o = (ctypes.c_void_p * 1)(outs[i % NSETS].data_ptr())
        ok(lib.mid_bilateral_joint(ctx.handle, ctypes.byref(p), sg, f, lt, L, 1, 0, 0, 1, o, F32, None), "bilateral_joint")
    return go


def firefly_call(fr, fmt, r):
    p = mid.FireflyParams(W, H, r, 1, 1.0, 0.0, fmt)
    return lambda i: ok(lib.mid_firefly_clamp(ctx.handle, ctypes.byref(p), fr[i % NSETS].data_ptr(), outs[i % NSETS].data_ptr(), None), "firefly")


variants = {}
for fname, fr, fmt in (("RGBA32F", frames32, F32), ("RGBA8", frames8, U8)):
    for r in (1, 2, 3):
        for L in (0, 1, 3, 5):
            variants[f"median {fname} r={r} L={L}"] = median_call(fr, fmt, r, L)
            if L:
                variants[f"joint bilateral {fname} r={r} L={L}"] = joint_call(fr, fmt, r, L)
    for r in (1, 2):
        variants[f"firefly clamp {fname} r={r}"] = firefly_call(fr, fmt, r)
for r in (1, 2, 3):
    variants[f"median RGBA32F r={r} L=1 all-zero layer (general class)"] = median_call(frames32, F32, r, 1, [zero_layer])
results = {k: [] for k in variants}
copies = []
for k, fn in variants.items():                              # warm-up: code objects, LDS attributes
    fn(0)
ok(lib.mid_stream_sync(ctx.handle, None), "sync")
for _ in range(args.rounds):
    for k, fn in variants.items():
        results[k].append(timed(fn))
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(args.reps):
        outs[i % NSETS].copy_(frames32[i % NSETS])
    t1.record()
    torch.cuda.synchronize()
    copies.append(t0.elapsed_time(t1) / args.reps)


def fig(v):
    return f"{statistics.median(v):8.3f} ms  (spread {min(v):.3f} .. {max(v):.3f})"


say("")
say("1-4. per call, 1080p, RGBA32F output")
for k, v in results.items():
    say(f"  {k:58s} {fig(v)}")
say(f"  {'device copy of an RGBA32F frame (33 MB in, 33 MB out)':58s} {fig(copies)}")
med = lambda k: statistics.median(results[k])
say("")
say(f"  plain r=1 / copy: {med('median RGBA32F r=1 L=0') / statistics.median(copies):.2f};  plain r=1 / firefly r=1: "
    f"{med('median RGBA32F r=1 L=0') / med('firefly clamp RGBA32F r=1'):.2f}")
for r in (1, 2, 3):
    a, b = med(f'median RGBA32F r={r} L=0'), med(f'median RGBA32F r={r} L=1 all-zero layer (general class)')
    say(f"  plain selection class / general class at r={r}: {a:.3f} ms / {b:.3f} ms = {a / b:.2f}  (the frame's border tiles, 9.4 % of 2040, count ranks in both)")
for L in (1, 3, 5):
    say(f"  weighted r=2 L={L} / joint bilateral r=2 L={L}: {med(f'median RGBA32F r=2 L={L}') / med(f'joint bilateral RGBA32F r=2 L={L}'):.2f}")
say(f"  estimates from operation counts: r=2 0.1 ms, measured {med('median RGBA32F r=2 L=0'):.3f}; r=3 0.4 ms, measured {med('median RGBA32F r=3 L=0'):.3f}")

# 5. host to host
n = args.frames
hf = [rng.integers(0, 256, (H, W, 4), dtype=np.uint8) for _ in range(4)]
hl = (blocks + ((3 * xx + 5 * yy) % 7)[..., None]).astype(np.uint8)
pin_in, pin_l, pin_out = PinnedFrames(ctx, [hf[i % 4] for i in range(n)]), PinnedFrames(ctx, [hl] * n), PinnedFrames(ctx, n, NPIX * 4)
seq = {"mid_sequence_median r=2, 1 layer": lambda: ctx.sequence_median_pinned(pin_in.ptrs, pin_out.ptrs, W, H, U8, pin_l.ptrs, 1, [0.02], 2, out_dtype=np.uint8),
       "mid_sequence_atrous_joint 5 passes, 1 layer": lambda: ctx.sequence_atrous_joint_pinned(pin_in.ptrs, pin_out.ptrs, W, H, U8, pin_l.ptrs, 1, [0.02],
                                                                                               out_dtype=np.uint8)}
walls = {k: [] for k in seq}
for k, fn in seq.items():
    fn()
for _ in range(3):
    for k, fn in seq.items():
        walls[k].append(fn()[0])
say("")
say(f"5. host to host, {n} RGBA8 frames, page-locked in and out")
for k, v in walls.items():
    say(f"  {k:58s} {statistics.median(v):8.2f} ms  ({n * NPIX / 1e3 / statistics.median(v):.0f} Mpixel/s; spread {min(v):.2f} .. {max(v):.2f})")
for b in (pin_in, pin_l, pin_out):
    b.free()
ok(lib.mid_timer_destroy(timer), "mid_timer_destroy")
ctx.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
