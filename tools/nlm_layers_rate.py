"""Kernel and host-to-host rates of layer-guided NLM on one MI355X (development aid; writes profiles/r08_nlm_layers.txt when given
--out).

1. Kernel time per layer: mid_nlm_layers with L = 1, 2, 4, 8 guides on one 1080p RGBA32F frame, divided by L, against a one-frame
   mid_nlm_temporal launch (k = 0) of the same frame, at both tuned windows (--untuned: and at search (-2, 3), patch (-1, 3), which runs on the
   per-pixel kernels).  Device buffers only; each figure is the event time
   (mid_timer) of REPS back-to-back calls on the context's stream / REPS, median over the rounds; variants are interleaved round by
   round so that every figure sees the same lease.
2. Fused against the chain: mid_nlm_layers against L x mid_nlm_layers_accum + mid_normalize (the clear of W not counted).
3. Host to host: mid_sequence_nlm_layers over 16 and 64 x 1080p RGBA8 frames with 4 RGBA8 layers each, RGBA8 outputs, page-locked
   (outputs stored by the kernel), overlap = 1; wall time of the call, median over the rounds."""
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
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--untuned", action="store_true", help="a third window for the table of 1. and 2., one that runs on the per-pixel kernel")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: {lib.mid_last_error().decode()}")


W, H = 1920, 1080
NPIX = W * H
WINDOWS = {"7x7/14x14 (reference)": ((-7, 7), (-3, 3)), "7x7/21x21 (bench)": ((-10, 11), (-3, 4))}
TABLE_WINDOWS = dict(WINDOWS, **({"4x4/5x5 (untuned: per-pixel kernel)": ((-2, 3), (-1, 3))} if args.untuned else {}))
LS = (1, 2, 4, 8)
ctx = mid.Context(0)
say(f"device {ctx.name}; 1080p RGBA32F input, h = 0.5; {args.rounds} rounds x {args.reps} calls per figure")
rng = np.random.default_rng(8)
frame = np.concatenate([rng.random((H, W, 3), dtype=np.float32), np.ones((H, W, 1), np.float32)], 2)
yy, xx = np.mgrid[0:H, 0:W]
guides = [np.clip(np.stack([xx * (i + 1) % 256, yy * 2 % 256, (xx + yy) // 2 % 256, np.full_like(xx, 255)], -1)
                  + rng.integers(-3, 4, (H, W, 4)), 0, 255).astype(np.uint8) for i in range(8)]
d_in = ctx.upload(frame)
d_g = [ctx.upload(g) for g in guides]
d_out = ctx.alloc(NPIX * 16)
d_w = ctx.zeros(NPIX * 32)
tbl = (ctypes.c_void_p * 8)(*[d.ptr for d in d_g])
fr = (ctypes.c_void_p * 1)(d_in.ptr)
ou = (ctypes.c_void_p * 1)(d_out.ptr)
timer = ctypes.c_void_p()
ok(lib.mid_timer_create(ctx.handle, ctypes.byref(timer)), "mid_timer_create")
nparams = mid.NormalizeParams(W, H)


def timed(fn):
    fn()
    ok(lib.mid_timer_tick(timer, None), "tick")
    for _ in range(args.reps):
        fn()
    ok(lib.mid_timer_tock(timer, None), "tock")
    ms = ctypes.c_float()
    ok(lib.mid_timer_ms(timer, ctypes.byref(ms)), "ms")
    return ms.value / args.reps


def variants(p):
    v = {"nlm_temporal k=0": lambda: ok(lib.mid_nlm_temporal(ctx.handle, ctypes.byref(p), fr, 1, 0, 0, 1, ou, None), "temporal")}
    for L in LS:
        v[f"fused L={L}"] = lambda L=L: ok(lib.mid_nlm_layers(ctx.handle, ctypes.byref(p), d_in.ptr, tbl, L, d_out.ptr, None), "layers")

        def chain(L=L):
            for i in range(L):
                ok(lib.mid_nlm_layers_accum(ctx.handle, ctypes.byref(p), d_in.ptr, d_g[i].ptr, d_w.ptr, None), "accum")
            ok(lib.mid_normalize(ctx.handle, ctypes.byref(nparams), d_w.ptr, d_out.ptr, None), "normalize")
        v[f"chain L={L}"] = chain
    return v


for wname, (search, patch) in TABLE_WINDOWS.items():
    p = mid.NlmParams(W, H, 0.5, search[0], search[1], patch[0], patch[1], mid.FMT_RGBA32F)
    vs = variants(p)
    res = {k: [] for k in vs}
    for _ in range(args.rounds):
        for k, fn in vs.items():
            res[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in res.items()}
    base = med["nlm_temporal k=0"]
    say(f"\n{wname}: one-frame mid_nlm_temporal {base:.3f} ms (spread {min(res['nlm_temporal k=0']):.3f}-{max(res['nlm_temporal k=0']):.3f})")
    say("   L   fused ms  per layer  /NLM   chain ms  per layer  fused/chain")
    for L in LS:
        f, c = med[f"fused L={L}"], med[f"chain L={L}"]
        say(f"  {L:2d}  {f:8.3f}  {f / L:8.3f}  {f / L / base:5.2f}  {c:8.3f}  {c / L:8.3f}  {f / c:10.3f}")

# host to host
say("\nmid_sequence_nlm_layers, host to host, 1080p RGBA8 in and out, 4 RGBA8 layers per frame, pinned, overlap = 1 "
    "(reference window 7x7/14x14 and bench window 7x7/21x21)")
L = 4
src = [(f * 255).astype(np.uint8) for f in [np.concatenate([rng.random((H, W, 3), dtype=np.float32), np.ones((H, W, 1), np.float32)], 2)
                                            for _ in range(4)]]
pin_in = mid.PinnedFrames(ctx, src)
pin_l = mid.PinnedFrames(ctx, guides[:L])
for n in (16, 64):
    pin_out = mid.PinnedFrames(ctx, n, NPIX * 4)
    hin = [pin_in.ptrs[i % 4] for i in range(n)]
    hl = [pin_l.ptrs[j] for i in range(n) for j in range(L)]
    for wname, (search, patch) in WINDOWS.items():
        walls, kerns = [], []
        for _ in range(args.rounds):
            t = ctx.sequence_nlm_layers_pinned(hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, hl, L, True, 0.5, search, patch, np.uint8)
            walls.append(t[0])
            kerns.append(t[1])
        wall = statistics.median(walls)
        say(f"  {n:2d} frames, {wname}: {wall:8.2f} ms wall ({min(walls):.2f}-{max(walls):.2f}), {n * NPIX / wall / 1e3:7.1f} Mpixel/s, "
            f"kernel sum {statistics.median(kerns) / n:.3f} ms per frame")
    pin_out.free()
pin_in.free()
pin_l.free()
lib.mid_timer_destroy(timer)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
