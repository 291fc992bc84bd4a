"""Kernel rates of the firefly clamp on one MI355X (development aid; writes profiles/r23_firefly.txt when given --out).  1080p, one
lease, variants interleaved round by round; a figure is the event time (mid_timer) of REPS back-to-back calls / REPS, median over
the rounds, with the spread over the rounds beside it (the method of DESIGN section 7).

1. One mid_firefly_clamp call, RGBA8 / RGBA16F / RGBA32F frames, both radii, rank 2.  Every call of a timed run works on its own
   pair of planes and the pairs of one variant add up to more than the 256 MiB cache, so no call finds its planes where the
   previous one left them.  Beside each figure the call's algorithmic bytes -- input texel + 16 B out per pixel -- at the
   device-to-device copy rate measured in the same run.  Expectation, not a gate: at most 1.5 x for RGBA32F input.
2. The per-frame chain, three RGBA8 layers and an RGBA8 albedo, fractional motion, five passes, on illumination (tools/albedo_rate.py's
   row 2) -- and the same chain with mid_firefly_clamp between demodulate and the moments.  Expectation: the one call's warm time
   and no more.
3. Host to host over 64 RGBA8 frames with 4 RGBA8 layers, page-locked, overlap = 1, five passes: mid_sequence_atrous_recursive
   against mid_sequence_atrous_recursive_firefly (no albedo).  No expectation fixed."""
import argparse
import ctypes
import statistics
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import image_denoising_filter_amd as mid  # noqa: E402
from image_denoising_filter_amd._lib import lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--frames", type=int, default=64)
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
SIGMAS = [0.2, 0.3, 0.15, 0.25]
F32, U8, F16 = mid.FMT_RGBA32F, mid.FMT_RGBA8, mid.FMT_RGBA16F
BYTES = {U8: 4, F16: 8, F32: 16}
NAME = {U8: "RGBA8", F16: "RGBA16F", F32: "RGBA32F"}
ctx = mid.Context(0)
say(f"device {ctx.name}; 1080p; {args.rounds} rounds x {args.reps} calls per figure, every call of a run on its own planes")
rng = np.random.default_rng(23)
yy, xx = np.mgrid[0:H, 0:W]
timer = ctypes.c_void_p()
ok(lib.mid_timer_create(ctx.handle, ctypes.byref(timer)), "mid_timer_create")


def timed(fns):
    """Event time per call of the calls in `fns`, run once untimed first."""
    for fn in fns:
        fn()
    ok(lib.mid_timer_tick(timer, None), "tick")
    for fn in fns:
        fn()
    ok(lib.mid_timer_tock(timer, None), "tock")
    ms = ctypes.c_float()
    ok(lib.mid_timer_ms(timer, ctypes.byref(ms)), "ms")
    return ms.value / len(fns)


# ---- 1. the kernel ----
frame8 = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
spiky = (frame8 / np.float32(255)).astype(np.float32)
spiky[..., :3] *= np.where(rng.random((H, W, 1)) < 1 / 50, np.float32(4096), np.float32(1))      # one firefly in fifty
host = {U8: frame8, F16: spiky.astype(np.float16), F32: spiky}
SETS = 2 * args.reps
assert SETS * NPIX * (4 + 16) > 256 << 20, "the sets of the smallest variant must pass the cache"
pool = {fmt: [ctx.upload(host[fmt]) for _ in range(SETS)] for fmt in (U8, F16, F32)}
outs = [ctx.alloc(NPIX * 16) for _ in range(SETS)]


def clamp_calls(fmt, radius):
    p = mid.FireflyParams(W, H, radius, 2, 1.0, 0.0, fmt)
    return [lambda i=i: ok(lib.mid_firefly_clamp(ctx.handle, ctypes.byref(p), pool[fmt][i].ptr, outs[i].ptr, None), "mid_firefly_clamp") for i in range(SETS)]


kernels = {(fmt, radius): (clamp_calls(fmt, radius), BYTES[fmt] + 16) for fmt in (U8, F16, F32) for radius in (1, 2)}
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


res = {key: [] for key in kernels}
res["copy"] = []
for _ in range(args.rounds):
    for key in res:
        res[key].append(timed_copy() if key == "copy" else timed(kernels[key][0]))
med = {key: statistics.median(v) for key, v in res.items()}
copy_rate = 2 * a.numel() * 4 / (med["copy"] * 1e-3) / 1e9          # GB/s, bytes read + bytes written
say(f"device-to-device copy of 256 MiB: {med['copy']:.4f} ms = {copy_rate:.0f} GB/s (read + written)")
del a, b


def fig(r, key):
    return f"{statistics.median(r[key]):7.4f} ({min(r[key]):.4f}-{max(r[key]):.4f})"


say("\n1. one call, rank 2; kernel ms (spread), its algorithmic bytes per pixel, those bytes at the copy rate, ratio, expectation (at most 1.5 x):")
for key, (_, bpp) in kernels.items():
    at_copy = bpp * NPIX / (copy_rate * 1e9) * 1e3
    ratio = med[key] / at_copy
    say(f"  frame {NAME[key[0]]:7} radius {key[1]}: {fig(res, key)}   {bpp:3} B/pixel = {at_copy:.4f} ms at the copy rate   x {ratio:.2f}   {'met' if ratio <= 1.5 else 'missed'}")
for d in [x for v in pool.values() for x in v] + outs:
    d.free()

# ---- 2. the per-frame chain ----
L = 3
albedo8 = rng.integers(1, 256, (H, W, 4), dtype=np.uint8)
g8 = [[np.clip(np.stack([(xx + 2 * f) * (i % 4 + 1) % 256, yy * 2 % 256, (xx + yy + f) // 2 % 256, np.full_like(xx, 255)], -1)
               + rng.integers(-3, 4, (H, W, 4)), 0, 255).astype(np.uint8) for i in range(4)] for f in range(2)]
f32 = np.concatenate([rng.random((H, W, 3), dtype=np.float32), np.ones((H, W, 1), np.float32)], 2)
d_fr, d_alb = ctx.upload(f32), ctx.upload(albedo8)
d_g = [[ctx.upload(g) for g in gs] for gs in g8]
d_mv = ctx.upload(np.stack([6 * np.sin(xx * 0.005 + 0.4) * np.cos(yy * 0.007), 6 * np.cos(xx * 0.003 + yy * 0.005 + 1.0)], -1).astype(np.float32))
d_hc = ctx.upload(f32)
d_hs = ctx.upload(np.stack([f32[..., 0], f32[..., 0] ** 2 + 0.01, np.full((H, W), 5, np.float32), np.zeros((H, W), np.float32)], -1))
d_col, d_st, d_out, d_il, d_fin, d_cl = (ctx.alloc(NPIX * 16) for _ in range(6))
d_scr = ctx.alloc(2 * NPIX * 20)
d_vs, d_v0 = ctx.alloc(NPIX * 4), ctx.alloc(NPIX * 4)
sg = (ctypes.c_float * L)(*SIGMAS[:L])
cl = (ctypes.c_void_p * L)(*[d_g[1][l].ptr for l in range(L)])
pl = (ctypes.c_void_p * L)(*[d_g[0][l].ptr for l in range(L)])
word = mid.api.fmt_with_guide(F32, U8)
mp, tp, vp = mid.AtrousMomentsParams(W, H, word), mid.TemporalAccumParams(W, H, 0.2, 0.2, 32.0, 4.0, word), mid.AtrousVarianceParams(W, H, 0, 5, 4.0, 1e-3, word)
dp = mid.AlbedoParams(W, H, 1e-3, word)
fps = {r: mid.FireflyParams(W, H, r, 2, 1.0, 0.0, F32) for r in (1, 2)}


def clamp(radius):
    ok(lib.mid_firefly_clamp(ctx.handle, ctypes.byref(fps[radius]), d_il.ptr, d_cl.ptr, None), "mid_firefly_clamp")


def chain(radius):
    ok(lib.mid_demodulate(ctx.handle, ctypes.byref(dp), d_fr.ptr, d_alb.ptr, d_il.ptr, None), "mid_demodulate")
    frame = d_il
    if radius:
        clamp(radius)
        frame = d_cl
    fr = (ctypes.c_void_p * 1)(frame.ptr)
    ok(lib.mid_atrous_moments(ctx.handle, ctypes.byref(mp), sg, fr, cl, L, 1, 0, 0, d_vs.ptr, None), "mid_atrous_moments")
    ok(lib.mid_temporal_accumulate(ctx.handle, ctypes.byref(tp), sg, frame.ptr, cl, pl, L, d_mv.ptr, d_hc.ptr, d_hs.ptr, d_vs.ptr, d_col.ptr, d_st.ptr, d_v0.ptr, None),
       "mid_temporal_accumulate")
    ok(lib.mid_atrous_variance(ctx.handle, ctypes.byref(vp), sg, d_col.ptr, d_v0.ptr, cl, L, d_fin.ptr, F32, None, d_scr.ptr, None), "mid_atrous_variance")
    ok(lib.mid_modulate(ctx.handle, ctypes.byref(dp), d_fin.ptr, d_alb.ptr, d_out.ptr, F32, None), "mid_modulate")


chains = {"without": lambda: chain(0), "radius 1": lambda: chain(1), "radius 2": lambda: chain(2), "clamp 1 alone": lambda: clamp(1), "clamp 2 alone": lambda: clamp(2)}
cres = {key: [] for key in chains}
for _ in range(args.rounds):
    for key, fn in chains.items():
        cres[key].append(timed([fn] * 5))
cm = {key: statistics.median(v) for key, v in cres.items()}
say("\n2. the per-frame chain on illumination, RGBA32F frame, three RGBA8 layers and an RGBA8 albedo, fractional motion, five passes (planes reused: warm cache):")
say(f"  without the stage (demodulate, moments k = 0, accumulate, five passes, modulate): {fig(cres, 'without')}")
for r in (1, 2):
    extra, one = cm[f"radius {r}"] - cm["without"], cm[f"clamp {r} alone"]
    say(f"  with the clamp at radius {r}: {fig(cres, f'radius {r}')}; the call alone {fig(cres, f'clamp {r} alone')}; "
        f"with - without = {extra:.4f} ms: {'met (the one call and no more)' if extra <= 1.15 * one + 0.005 else 'missed'}; "
        f"with / without {cm[f'radius {r}'] / cm['without']:.3f}")
lib.mid_timer_destroy(timer)
for d in (d_fr, d_alb, d_mv, d_hc, d_hs, d_col, d_st, d_out, d_il, d_fin, d_cl, d_scr, d_vs, d_v0, *[x for row in d_g for x in row]):
    d.free()

# ---- 3. host to host ----
n, L, NSRC = args.frames, 4, 4
say(f"\n3. host to host, {n} x 1080p RGBA8 in and out, {L} RGBA8 layers per frame, pinned, overlap = 1, five passes, warm-up 0")
src = [np.roll(frame8, 7 * i, 1) for i in range(NSRC)]
pin_in, pin_out, pin_l = mid.PinnedFrames(ctx, src), mid.PinnedFrames(ctx, n, NPIX * 4), mid.PinnedFrames(ctx, g8[0])
hin = [pin_in.ptrs[i % NSRC] for i in range(n)]
hl = [pin_l.ptrs[j] for i in range(n) for j in range(L)]
KINDS = {"recursive": {}, "recursive + firefly radius 1": dict(firefly_rank=2), "recursive + firefly radius 2": dict(firefly_rank=2, firefly_radius=2)}
stats = {kind: ([], []) for kind in KINDS}
for _ in range(args.rounds):
    for kind, (walls, kerns) in stats.items():
        t = ctx.sequence_atrous_recursive_pinned(hin, pin_out.ptrs, W, H, U8, hl, L, SIGMAS, None, 1, 0, 0, n, overlap=True, out_dtype=np.uint8, **KINDS[kind])
        walls.append(t[0])
        kerns.append(t[1])
rate = {}
for kind, (walls, kerns) in stats.items():
    wall = statistics.median(walls)
    rate[kind] = n * NPIX / wall / 1e3
    say(f"  {kind:28}: {wall:8.2f} ms wall ({min(walls):.2f}-{max(walls):.2f}), {rate[kind]:7.1f} Mpixel/s, {wall / n:.3f} ms per frame, "
        f"{statistics.median(kerns) / n:.3f} ms of launches per frame")
for kind in list(KINDS)[1:]:
    say(f"  {kind} / recursive: {rate[kind] / rate['recursive']:.3f}")
for bb in (pin_in, pin_out, pin_l):
    bb.free()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
