"""Kernel rates of albedo demodulation on one MI355X (development aid; writes profiles/r22_albedo.txt when given --out).  1080p, one
lease, variants interleaved round by round; a figure is the event time (mid_timer) of REPS back-to-back calls / REPS, median over
the rounds, with the spread over the rounds beside it (the method of DESIGN section 7).

1. One mid_demodulate and one mid_modulate call, RGBA8 and RGBA32F frames / outputs and albedo planes.  Every call of a timed run
   works on its own set of planes and the sets of one variant add up to more than the 256 MiB cache, so no call finds its planes
   where the previous one left them.  Beside each figure the call's algorithmic bytes -- frame, albedo and output counted once --
   at the device-to-device copy rate measured in the same run.  Expectation from the code: the copy-rate time, the passes are pure
   streaming; "met" within 15 %.
2. The per-frame chain, three RGBA8 layers, fractional motion, five passes: mid_atrous_moments at k = 0, mid_temporal_accumulate,
   mid_atrous_variance -- and the same chain on illumination: mid_demodulate, the three on the RGBA32F plane with the passes' last
   level in RGBA32F, mid_modulate.  Expectation: the two passes' time and no more.
3. Host to host over 64 RGBA8 frames with 4 RGBA8 layers, page-locked, overlap = 1, five passes: mid_sequence_atrous_recursive
   against mid_sequence_atrous_recursive_albedo with an RGBA8 albedo plane per frame (4 B per pixel more upload)."""
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
F32, U8 = mid.FMT_RGBA32F, mid.FMT_RGBA8
BYTES = {U8: 4, F32: 16}
NAME = {U8: "RGBA8", F32: "RGBA32F"}
ctx = mid.Context(0)
say(f"device {ctx.name}; 1080p; {args.rounds} rounds x {args.reps} calls per figure, every call of a run on its own planes")
rng = np.random.default_rng(22)
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


# ---- 1. the two kernels ----
frame8 = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
albedo8 = rng.integers(1, 256, (H, W, 4), dtype=np.uint8)
host = {U8: (frame8, albedo8), F32: ((frame8 / np.float32(255)).astype(np.float32), (albedo8 / np.float32(255)).astype(np.float32))}
SETS = args.reps
pool = {(fmt, role): [ctx.upload(host[fmt][0 if role != "albedo" else 1]) for _ in range(SETS)] for fmt in (U8, F32) for role in ("frame", "albedo", "out")}
illum = [ctx.upload(host[F32][0]) for _ in range(SETS)]
assert SETS * NPIX * (4 + 4 + 16) > 256 << 20, "the sets of the smallest variant must pass the cache"


def demodulate_calls(fmt, gfmt):
    p = mid.AlbedoParams(W, H, 1e-3, mid.api.fmt_with_guide(fmt, gfmt))
    return [lambda i=i: ok(lib.mid_demodulate(ctx.handle, ctypes.byref(p), pool[(fmt, "frame")][i].ptr, pool[(gfmt, "albedo")][i].ptr, illum[i].ptr, None),
                           "mid_demodulate") for i in range(SETS)]


def modulate_calls(gfmt, ofmt):
    p = mid.AlbedoParams(W, H, 1e-3, mid.api.fmt_with_guide(F32, gfmt))
    return [lambda i=i: ok(lib.mid_modulate(ctx.handle, ctypes.byref(p), illum[i].ptr, pool[(gfmt, "albedo")][i].ptr, pool[(ofmt, "out")][i].ptr, ofmt, None),
                           "mid_modulate") for i in range(SETS)]


kernels = {}
for fmt in (U8, F32):
    for gfmt in (U8, F32):
        kernels[("demodulate", fmt, gfmt)] = (demodulate_calls(fmt, gfmt), BYTES[fmt] + BYTES[gfmt] + 16)
        kernels[("modulate", gfmt, fmt)] = (modulate_calls(gfmt, fmt), 16 + BYTES[gfmt] + BYTES[fmt])

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


say("\n1. one call; kernel ms (spread), its algorithmic bytes per pixel, those bytes at the copy rate, ratio, expectation (the copy-rate time within 15 %):")
for key, (_, bpp) in kernels.items():
    at_copy = bpp * NPIX / (copy_rate * 1e9) * 1e3
    what = (f"demodulate frame {NAME[key[1]]:7} albedo {NAME[key[2]]:7}" if key[0] == "demodulate" else f"modulate   albedo {NAME[key[1]]:7} out   {NAME[key[2]]:7}")
    ratio = med[key] / at_copy
    say(f"  {what}: {fig(res, key)}   {bpp:3} B/pixel = {at_copy:.4f} ms at the copy rate   x {ratio:.2f}   {'met' if ratio <= 1.15 else 'missed'}")
for d in [x for v in pool.values() for x in v] + illum:
    d.free()

# ---- 2. the per-frame chain ----
L = 3
g8 = [[np.clip(np.stack([(xx + 2 * f) * (i % 4 + 1) % 256, yy * 2 % 256, (xx + yy + f) // 2 % 256, np.full_like(xx, 255)], -1)
               + rng.integers(-3, 4, (H, W, 4)), 0, 255).astype(np.uint8) for i in range(4)] for f in range(2)]
f32 = np.concatenate([rng.random((H, W, 3), dtype=np.float32), np.ones((H, W, 1), np.float32)], 2)
d_fr, d_alb = ctx.upload(f32), ctx.upload(albedo8)
d_g = [[ctx.upload(g) for g in gs] for gs in g8]
d_mv = ctx.upload(np.stack([6 * np.sin(xx * 0.005 + 0.4) * np.cos(yy * 0.007), 6 * np.cos(xx * 0.003 + yy * 0.005 + 1.0)], -1).astype(np.float32))
d_hc = ctx.upload(f32)
d_hs = ctx.upload(np.stack([f32[..., 0], f32[..., 0] ** 2 + 0.01, np.full((H, W), 5, np.float32), np.zeros((H, W), np.float32)], -1))
d_col, d_st, d_out, d_il, d_fin = (ctx.alloc(NPIX * 16) for _ in range(5))
d_scr = ctx.alloc(2 * NPIX * 20)
d_vs, d_v0 = ctx.alloc(NPIX * 4), ctx.alloc(NPIX * 4)
sg = (ctypes.c_float * L)(*SIGMAS[:L])
cl = (ctypes.c_void_p * L)(*[d_g[1][l].ptr for l in range(L)])
pl = (ctypes.c_void_p * L)(*[d_g[0][l].ptr for l in range(L)])
word = mid.api.fmt_with_guide(F32, U8)
mp, tp, vp = mid.AtrousMomentsParams(W, H, word), mid.TemporalAccumParams(W, H, 0.2, 0.2, 32.0, 4.0, word), mid.AtrousVarianceParams(W, H, 0, 5, 4.0, 1e-3, word)
dp = mid.AlbedoParams(W, H, 1e-3, word)


def chain(frame, last):
    fr = (ctypes.c_void_p * 1)(frame.ptr)
    ok(lib.mid_atrous_moments(ctx.handle, ctypes.byref(mp), sg, fr, cl, L, 1, 0, 0, d_vs.ptr, None), "mid_atrous_moments")
    ok(lib.mid_temporal_accumulate(ctx.handle, ctypes.byref(tp), sg, frame.ptr, cl, pl, L, d_mv.ptr, d_hc.ptr, d_hs.ptr, d_vs.ptr, d_col.ptr, d_st.ptr, d_v0.ptr, None),
       "mid_temporal_accumulate")
    ok(lib.mid_atrous_variance(ctx.handle, ctypes.byref(vp), sg, d_col.ptr, d_v0.ptr, cl, L, last.ptr, F32, None, d_scr.ptr, None), "mid_atrous_variance")


def chain_albedo():
    ok(lib.mid_demodulate(ctx.handle, ctypes.byref(dp), d_fr.ptr, d_alb.ptr, d_il.ptr, None), "mid_demodulate")
    chain(d_il, d_fin)
    ok(lib.mid_modulate(ctx.handle, ctypes.byref(dp), d_fin.ptr, d_alb.ptr, d_out.ptr, F32, None), "mid_modulate")


chains = {"colour": lambda: chain(d_fr, d_out), "illumination": chain_albedo,
          "demodulate alone": lambda: ok(lib.mid_demodulate(ctx.handle, ctypes.byref(dp), d_fr.ptr, d_alb.ptr, d_il.ptr, None), "mid_demodulate"),
          "modulate alone": lambda: ok(lib.mid_modulate(ctx.handle, ctypes.byref(dp), d_fin.ptr, d_alb.ptr, d_out.ptr, F32, None), "mid_modulate")}
cres = {key: [] for key in chains}
for _ in range(args.rounds):
    for key, fn in chains.items():
        cres[key].append(timed([fn] * 5))
cm = {key: statistics.median(v) for key, v in cres.items()}
say("\n2. the per-frame chain, RGBA32F frame, three RGBA8 layers and an RGBA8 albedo, fractional motion, five passes (planes reused: warm cache):")
say(f"  on colour (moments k = 0, accumulate, five passes)              : {fig(cres, 'colour')}")
say(f"  on illumination (demodulate, the same, modulate)                : {fig(cres, 'illumination')}")
say(f"  the two passes alone: demodulate {fig(cres, 'demodulate alone')}, modulate {fig(cres, 'modulate alone')}")
extra, two = cm["illumination"] - cm["colour"], cm["demodulate alone"] + cm["modulate alone"]
say(f"  illumination - colour = {extra:.4f} ms against {two:.4f} ms for the two passes: "
    f"{'met (the two passes and no more)' if extra <= 1.15 * two + 0.005 else 'missed'}; illumination / colour {cm['illumination'] / cm['colour']:.3f}")
lib.mid_timer_destroy(timer)
for d in (d_fr, d_alb, d_mv, d_hc, d_hs, d_col, d_st, d_out, d_il, d_fin, d_scr, d_vs, d_v0, *[x for row in d_g for x in row]):
    d.free()

# ---- 3. host to host ----
n, L, NSRC = args.frames, 4, 4
say(f"\n3. host to host, {n} x 1080p RGBA8 in and out, {L} RGBA8 layers per frame, pinned, overlap = 1, five passes, warm-up 0")
src = [np.roll(frame8, 7 * i, 1) for i in range(NSRC)]
albs = [np.roll(albedo8, 5 * i, 0) for i in range(NSRC)]
pin_in, pin_out, pin_l, pin_a = mid.PinnedFrames(ctx, src), mid.PinnedFrames(ctx, n, NPIX * 4), mid.PinnedFrames(ctx, g8[0]), mid.PinnedFrames(ctx, albs)
hin = [pin_in.ptrs[i % NSRC] for i in range(n)]
hl = [pin_l.ptrs[j] for i in range(n) for j in range(L)]
ha = [pin_a.ptrs[i % NSRC] for i in range(n)]
KINDS = ("recursive on colour", "recursive on illumination")
stats = {kind: ([], []) for kind in KINDS}
for _ in range(args.rounds):
    for kind, (walls, kerns) in stats.items():
        t = ctx.sequence_atrous_recursive_pinned(hin, pin_out.ptrs, W, H, U8, hl, L, SIGMAS, None, 1, 0, 0, n, overlap=True, out_dtype=np.uint8,
                                                 halbedo=ha if kind == KINDS[1] else None)
        walls.append(t[0])
        kerns.append(t[1])
rate = {}
for kind, (walls, kerns) in stats.items():
    wall = statistics.median(walls)
    rate[kind] = n * NPIX / wall / 1e3
    say(f"  {kind:26}: {wall:8.2f} ms wall ({min(walls):.2f}-{max(walls):.2f}), {rate[kind]:7.1f} Mpixel/s, {wall / n:.3f} ms per frame, "
        f"{statistics.median(kerns) / n:.3f} ms of launches per frame")
say(f"  illumination / colour: {rate[KINDS[1]] / rate[KINDS[0]]:.3f}")
for bb in (pin_in, pin_out, pin_l, pin_a):
    bb.free()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
