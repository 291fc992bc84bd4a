"""Kernel and host-to-host rates of layer-guided NLM over neighbouring frames on one MI355X (development aid; writes
profiles/r09_nlm_layers_temporal.txt when given --out).

1. Cost per (neighbour, layer) dispatch inside the fused kernel: mid_nlm_layers_temporal for ONE output with its whole window
   (frame k of 2k+1 frames), k = 1, 2 and L = 1, 4 guides per frame, 1080p RGBA32F, both tuned windows, divided by (2k+1) L --
   against mid_nlm_layers' time per layer (L = 1, 4) of the same frame in the same run.  Device buffers only; each figure is the
   event time (mid_timer) of REPS back-to-back calls on the context's stream / REPS, median over the rounds; variants are
   interleaved round by round so that every figure sees the same lease.
2. Fused against its chain: (2k+1) L x mid_nlm_layers_pair_accum + mid_normalize (the clear of W not counted).
3. Host to host: mid_sequence_nlm_layers_temporal over 64 x 1080p RGBA8 frames with 4 RGBA8 layers each, k = 2, RGBA8 outputs,
   page-locked (outputs stored by the kernel), overlap = 1: wall time of the call, and against it the time of the resident
   mid_nlm_layers_temporal over the same 64 outputs; from mid_pipe_last_timeline the sum of the kernel intervals and the span of
   the compute stage."""
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


W, H = 1920, 1080
NPIX = W * H
WINDOWS = {"7x7/14x14 (reference)": ((-7, 7), (-3, 3)), "7x7/21x21 (bench)": ((-10, 11), (-3, 4))}
KS, LS, NF, LMAX = (1, 2), (1, 4), 5, 4
ctx = mid.Context(0)
say(f"device {ctx.name}; 1080p RGBA32F frames, h = 0.5; {args.rounds} rounds x {args.reps} calls per figure")
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
    v = {}
    for L in LS:
        tbl = (ctypes.c_void_p * L)(*[d.ptr for d in d_g[0][:L]])
        v[f"nlm_layers L={L}"] = lambda L=L, tbl=tbl: ok(lib.mid_nlm_layers(ctx.handle, ctypes.byref(p), d_fr[0].ptr, tbl, L, d_out.ptr, None), "layers")
    for k in KS:
        n = 2 * k + 1
        fr = (ctypes.c_void_p * n)(*[d.ptr for d in d_fr[:n]])
        for L in LS:
            ly = (ctypes.c_void_p * (n * L))(*[d_g[f][l].ptr for f in range(n) for l in range(L)])
            v[f"fused k={k} L={L}"] = lambda k=k, L=L, n=n, fr=fr, ly=ly: ok(
                lib.mid_nlm_layers_temporal(ctx.handle, ctypes.byref(p), fr, ly, L, n, k, k, 1, ou, mid.FMT_RGBA32F, None), "temporal")

            def chain(k=k, L=L, n=n):
                for f in range(n):
                    for l in range(L):
                        ok(lib.mid_nlm_layers_pair_accum(ctx.handle, ctypes.byref(p), d_g[k][l].ptr, d_g[f][l].ptr, d_fr[f].ptr, d_w.ptr, None), "pair")
                ok(lib.mid_normalize(ctx.handle, ctypes.byref(nparams), d_w.ptr, d_out.ptr, None), "normalize")
            v[f"chain k={k} L={L}"] = chain
    return v


for wname, (search, patch) in WINDOWS.items():
    p = mid.NlmParams(W, H, 0.5, search[0], search[1], patch[0], patch[1], mid.FMT_RGBA32F)
    vs = variants(p)
    res = {k: [] for k in vs}
    for _ in range(args.rounds):
        for k, fn in vs.items():
            res[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in res.items()}
    say(f"\n{wname}: mid_nlm_layers per layer " + ", ".join(
        f"L={L} {med[f'nlm_layers L={L}'] / L:.3f} ms (spread {min(res[f'nlm_layers L={L}']) / L:.3f}-{max(res[f'nlm_layers L={L}']) / L:.3f})" for L in LS))
    say("   k   L  dispatches  fused ms  per dispatch  /nlm_layers per layer   chain ms  fused/chain")
    for k in KS:
        for L in LS:
            nd = (2 * k + 1) * L
            f, c = med[f"fused k={k} L={L}"], med[f"chain k={k} L={L}"]
            say(f"  {k:2d}  {L:2d}  {nd:10d}  {f:8.3f}  {f / nd:12.3f}  {f / nd / (med[f'nlm_layers L={L}'] / L):21.3f}  {c:9.3f}  {f / c:11.3f}")

# host to host
n, L, k = args.frames, 4, 2
say(f"\nmid_sequence_nlm_layers_temporal, host to host, {n} x 1080p RGBA8 in and out, {L} RGBA8 layers per frame, k = {k}, pinned, overlap = 1")
src = [(f * 255).astype(np.uint8) for f in frames[:4]]
lay = [guide(i) for i in range(4 * L)]
pin_in, pin_l, pin_out = mid.PinnedFrames(ctx, src), mid.PinnedFrames(ctx, lay), mid.PinnedFrames(ctx, n, NPIX * 4)
hin = [pin_in.ptrs[i % 4] for i in range(n)]
hl = [pin_l.ptrs[(i % 4) * L + j] for i in range(n) for j in range(L)]
d_src = [ctx.upload(s) for s in src]
d_lay = [ctx.upload(g) for g in lay]
d_o = [ctx.alloc(NPIX * 4) for _ in range(n)]
r_fr = (ctypes.c_void_p * n)(*[d_src[i % 4].ptr for i in range(n)])
r_ly = (ctypes.c_void_p * (n * L))(*[d_lay[(i % 4) * L + j].ptr for i in range(n) for j in range(L)])
r_ou = (ctypes.c_void_p * n)(*[d.ptr for d in d_o])
for wname, (search, patch) in WINDOWS.items():
    p8 = mid.NlmParams(W, H, 0.5, search[0], search[1], patch[0], patch[1], mid.FMT_RGBA8)
    walls, kerns, spans, resident = [], [], [], []
    for _ in range(args.rounds):
        resident.append(timed(lambda: ok(lib.mid_nlm_layers_temporal(ctx.handle, ctypes.byref(p8), r_fr, r_ly, L, n, k, 0, n, r_ou,
                                                                     mid.FMT_RGBA8, None), "resident"), reps=1))
        t = ctx.sequence_nlm_layers_temporal_pinned(hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, hl, L, k, 0, n, True, 0.5, search, patch, np.uint8)
        walls.append(t[0])
        ups, outs = ctx.pipe_last_timeline()
        kerns.append(sum(o[2] - o[1] for o in outs))
        spans.append(max(o[2] for o in outs) - min(o[1] for o in outs))
    wall, res_ms = statistics.median(walls), statistics.median(resident)
    say(f"  {wname}: {wall:8.2f} ms wall ({min(walls):.2f}-{max(walls):.2f}), {n * NPIX / wall / 1e3:7.1f} Mpixel/s; resident kernels of the "
        f"same outputs {res_ms:.2f} ms = {res_ms / wall:.3f} of the wall time; timeline: kernel intervals sum {statistics.median(kerns):.2f} ms "
        f"(two streams overlap), compute stage spans {statistics.median(spans):.2f} ms")
for b in (pin_in, pin_l, pin_out):
    b.free()
lib.mid_timer_destroy(timer)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
