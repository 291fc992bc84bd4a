"""Kernel and host-to-host rates of the bilateral over neighbouring frames on one MI355X (development aid; writes
profiles/r10_bilateral_temporal.txt when given --out).

1. Cost per (neighbour[, layer]) dispatch inside the fused kernel: mid_bilateral_temporal for ONE output with its whole window
   (frame k of 2k+1 frames), k = 1, 2, plain and L = 1, 4 guides per frame, 1080p RGBA32F, r = 4 and r = 8, divided by (2k+1)
   [x L] -- against mid_bilateral (plain) and mid_bilateral_layers' time per layer (L = 1, 4) of the same frame in the same run.
   Device buffers only; each figure is the event time (mid_timer) of REPS back-to-back calls on the context's stream / REPS,
   median over the rounds; variants are interleaved round by round so that every figure sees the same lease.
2. Fused against its chain: (2k+1) [x L] pair dispatches + mid_normalize (the clear of W not counted).
3. Host to host: mid_sequence_bilateral_temporal over 64 x 1080p RGBA8 frames with 4 RGBA8 layers each, k = 2, r = 8, RGBA8
   outputs, page-locked (outputs stored by the kernel), overlap = 1: wall time of the call, from mid_pipe_last_timeline the sum of
   the kernel intervals and the span of the compute stage (its busy share of the wall time) -- and beside it
   mid_sequence_nlm_layers_temporal (21x21 / 7x7) over the same frames and layers in the same run."""
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
KS, LS, NF, LMAX = (1, 2), (0, 1, 4), 5, 4          # L = 0: the plain form
SS, SC = 2.0, 0.2
ctx = mid.Context(0)
say(f"device {ctx.name}; 1080p RGBA32F frames, sigma_s = {SS}, sigma_c = {SC}; {args.rounds} rounds x {args.reps} calls per figure")
rng = np.random.default_rng(9)
yy, xx = np.mgrid[0:H, 0:W]


def guide(i):
    return np.clip(np.stack([xx * (i % 4 + 1) % 256, yy * 2 % 256, (xx + yy) // 2 % 256, np.full_like(xx, 255)], -1)
                   + rng.integers(-3, 4, (H, W, 4)), 0, 255).astype(np.uint8)


frames = [np.concatenate([rng.random((H, W, 3), dtype=np.float32), np.ones((H, W, 1), np.float32)], 2) for _ in range(NF)]
d_fr = [ctx.upload(f) for f in frames]
d_g = [[ctx.upload(guide(l)) for l in range(LMAX)] for _ in range(NF)]
d_out = ctx.alloc(NPIX * 16)
d_w = ctx.zeros(NPIX * 32)
ou = (ctypes.c_void_p * 1)(d_out.ptr)
timer = ctypes.c_void_p()
ok(lib.mid_timer_create(ctx.handle, ctypes.byref(timer)), "mid_timer_create")
nparams = mid.NormalizeParams(W, H)


def timed(fn, reps=args.reps):
    fn()
    ok(lib.mid_timer_tick(timer, None), "tick")
    for _ in range(reps):
        fn()
    ok(lib.mid_timer_tock(timer, None), "tock")
    ms = ctypes.c_float()
    ok(lib.mid_timer_ms(timer, ctypes.byref(ms)), "ms")
    return ms.value / reps


def variants(p):
    v = {"single L=0": lambda: ok(lib.mid_bilateral(ctx.handle, ctypes.byref(p), d_fr[0].ptr, d_out.ptr, None), "bilateral")}
    for L in LS[1:]:
        tbl = (ctypes.c_void_p * L)(*[d.ptr for d in d_g[0][:L]])
        v[f"single L={L}"] = lambda L=L, tbl=tbl: ok(lib.mid_bilateral_layers(ctx.handle, ctypes.byref(p), d_fr[0].ptr, tbl, L, d_out.ptr, None), "layers")
    for k in KS:
        n = 2 * k + 1
        fr = (ctypes.c_void_p * n)(*[d.ptr for d in d_fr[:n]])
        for L in LS:
            ly = (ctypes.c_void_p * (n * L))(*[d_g[f][l].ptr for f in range(n) for l in range(L)]) if L else None
            v[f"fused k={k} L={L}"] = lambda k=k, L=L, n=n, fr=fr, ly=ly: ok(
                lib.mid_bilateral_temporal(ctx.handle, ctypes.byref(p), fr, ly, L, n, k, k, 1, ou, mid.FMT_RGBA32F, None), "temporal")

            def chain(k=k, L=L, n=n):
                for f in range(n):
                    if not L:
                        ok(lib.mid_bilateral_pair_accum(ctx.handle, ctypes.byref(p), d_fr[k].ptr, d_fr[f].ptr, d_w.ptr, None), "pair")
                    for l in range(L):
                        ok(lib.mid_bilateral_layers_pair_accum(ctx.handle, ctypes.byref(p), d_g[k][l].ptr, d_g[f][l].ptr, d_fr[f].ptr, d_w.ptr, None), "pair")
                ok(lib.mid_normalize(ctx.handle, ctypes.byref(nparams), d_w.ptr, d_out.ptr, None), "normalize")
            v[f"chain k={k} L={L}"] = chain
    return v


for r in (4, 8):
    p = mid.BilateralParams(W, H, SS, SC, r, mid.LAYOUT_TEXTURE, mid.FMT_RGBA32F)
    vs = variants(p)
    res = {k: [] for k in vs}
    for _ in range(args.rounds):
        for k, fn in vs.items():
            res[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in res.items()}
    say(f"\nr = {r}: single frame per dispatch: " + ", ".join(
        f"{'mid_bilateral' if not L else f'mid_bilateral_layers L={L}'} {med[f'single L={L}'] / max(L, 1):.4f} ms "
        f"(spread {min(res[f'single L={L}']) / max(L, 1):.4f}-{max(res[f'single L={L}']) / max(L, 1):.4f})" for L in LS))
    say("   k      L  dispatches  fused ms  per dispatch  /single per dispatch   chain ms  fused/chain")
    for k in KS:
        for L in LS:
            nd = (2 * k + 1) * max(L, 1)
            f, c = med[f"fused k={k} L={L}"], med[f"chain k={k} L={L}"]
            say(f"  {k:2d}  {'plain' if not L else L:>5}  {nd:10d}  {f:8.4f}  {f / nd:12.4f}  {f / nd / (med[f'single L={L}'] / max(L, 1)):20.3f}  {c:9.4f}  {f / c:11.3f}")

# host to host
n, L, k, r = args.frames, 4, 2, 8
say(f"\nhost to host, {n} x 1080p RGBA8 in and out, {L} RGBA8 layers per frame, k = {k}, pinned, overlap = 1")
src = [(f * 255).astype(np.uint8) for f in frames[:4]]
lay = [guide(i) for i in range(4 * L)]
pin_in, pin_l, pin_out = mid.PinnedFrames(ctx, src), mid.PinnedFrames(ctx, lay), mid.PinnedFrames(ctx, n, NPIX * 4)
hin = [pin_in.ptrs[i % 4] for i in range(n)]
hl = [pin_l.ptrs[(i % 4) * L + j] for i in range(n) for j in range(L)]
calls = {
    f"mid_sequence_bilateral_temporal r = {r}, layered": lambda: ctx.sequence_bilateral_temporal_pinned(
        hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, k, 0, n, r, SS, SC, hl, L, True, np.uint8),
    f"mid_sequence_bilateral_temporal r = {r}, plain": lambda: ctx.sequence_bilateral_temporal_pinned(
        hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, k, 0, n, r, SS, SC, None, 0, True, np.uint8),
    "mid_sequence_nlm_layers_temporal 21x21/7x7": lambda: ctx.sequence_nlm_layers_temporal_pinned(
        hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, hl, L, k, 0, n, True, 0.5, (-10, 11), (-3, 4), np.uint8),
}
stats = {name: ([], [], []) for name in calls}
for _ in range(args.rounds):
    for name, call in calls.items():
        t = call()
        ups, outs = ctx.pipe_last_timeline()
        stats[name][0].append(t[0])
        stats[name][1].append(sum(o[2] - o[1] for o in outs))
        stats[name][2].append(max(o[2] for o in outs) - min(o[1] for o in outs))
for name, (walls, kerns, spans) in stats.items():
    wall = statistics.median(walls)
    say(f"  {name}: {wall:8.2f} ms wall ({min(walls):.2f}-{max(walls):.2f}), {n * NPIX / wall / 1e3:7.1f} Mpixel/s, {wall / n:.3f} ms per frame; "
        f"timeline: kernel intervals sum {statistics.median(kerns):.2f} ms (two streams overlap), compute stage spans "
        f"{statistics.median(spans):.2f} ms = {statistics.median(spans) / wall:.3f} of the wall time")
for b in (pin_in, pin_l, pin_out):
    b.free()
lib.mid_timer_destroy(timer)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
