"""Kernel rates of the recursive temporal accumulation on one MI355X (development aid; writes profiles/r21_temporal_accumulate.txt
when given --out).  1080p, one lease, variants interleaved round by round; a figure is the event time (mid_timer) of REPS
back-to-back calls / REPS, median over the rounds, with the spread over the rounds beside it.

1. One mid_temporal_accumulate call: L = 1 .. 4 and 16, RGBA8 and RGBA32F guides, RGBA32F frame, with a history, var_spatial and
   var_out; motion NULL, an integer vector, and a smooth fractional field of up to +-6 texels.  Beside each figure the call's
   algorithmic bytes -- every plane counted once: frame 16, motion 8 (0 without), two histories 32, Vs 4, three outputs 36, and
   2 L layers of 4 or 16 B -- at the device-to-device copy rate measured in the same run.
   Expectation from the code: a small multiple of the copy time; fractional motion reads four texels of every gathered plane
   where integer motion reads one, all of them from cache lines the neighbouring lanes load anyway.
2. The per-frame chain, three layers: mid_atrous_moments at k = 0, mid_temporal_accumulate, five passes of mid_atrous_variance --
   against mid_atrous_moments at k = 2 and the same five passes (the window form of section a4i).
3. Host to host over 64 RGBA8 frames with 4 RGBA8 layers, page-locked, overlap = 1, five passes: mid_sequence_atrous_recursive with and
   without a motion plane per frame (8 B per pixel more upload) against mid_sequence_atrous_variance at k = 2; the compute stage's
   share of the call, and how much of that span the launches fill (the in-order schedule leaves the tail of one frame's last launch
   uncovered, where the other stages start the next frame on a second stream)."""
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


W, H, NF, LRES = 1920, 1080, 5, 4                  # five frames (k = 2), four distinct layers per frame (layer l of L = 16 is layer l mod 4)
NPIX = W * H
SIGMAS = [0.2, 0.3, 0.15, 0.25]
ctx = mid.Context(0)
say(f"device {ctx.name}; 1080p RGBA32F frames; sigmas {SIGMAS} (repeated); {args.rounds} rounds x {args.reps} calls per figure")
rng = np.random.default_rng(21)
yy, xx = np.mgrid[0:H, 0:W]


def guide(f, i):
    return np.clip(np.stack([(xx + 2 * f) * (i % 4 + 1) % 256, yy * 2 % 256, (xx + yy + f) // 2 % 256, np.full_like(xx, 255)], -1)
                   + rng.integers(-3, 4, (H, W, 4)), 0, 255).astype(np.uint8)


g8 = [[guide(f, i) for i in range(LRES)] for f in range(NF)]
f32 = [np.concatenate([rng.random((H, W, 3), dtype=np.float32), np.ones((H, W, 1), np.float32)], 2) for _ in range(NF)]
d_fr = [ctx.upload(f) for f in f32]
d_g = {np.uint8: [[ctx.upload(g) for g in gs] for gs in g8],
       np.float32: [[ctx.upload((g / np.float32(255)).astype(np.float32)) for g in gs] for gs in g8[1:3]]}      # frames 1 and 2 only
MOTION = {"none": None,
          "integer": ctx.upload(np.broadcast_to(np.float32([3, -2]), (H, W, 2)).copy()),
          "fractional": ctx.upload(np.stack([6 * np.sin(xx * 0.005 + 0.4) * np.cos(yy * 0.007), 6 * np.cos(xx * 0.003 + yy * 0.005 + 1.0)], -1).astype(np.float32))}
d_hc = ctx.upload(f32[1])
d_hs = ctx.upload(np.stack([f32[1][..., 0], f32[1][..., 0] ** 2 + 0.01, np.full((H, W), 5, np.float32), np.zeros((H, W), np.float32)], -1))
d_col, d_st, d_out, d_scr = ctx.alloc(NPIX * 16), ctx.alloc(NPIX * 16), ctx.alloc(NPIX * 16), ctx.alloc(2 * NPIX * 20)
d_vs, d_v0 = ctx.alloc(NPIX * 4), ctx.alloc(NPIX * 4)
ok(lib.mid_memset(ctx.handle, d_vs.ptr, 0, NPIX * 4, None), "mid_memset")
timer = ctypes.c_void_p()
ok(lib.mid_timer_create(ctx.handle, ctypes.byref(timer)), "mid_timer_create")
F32 = mid.FMT_RGBA32F


def sig(L):
    return (ctypes.c_float * L)(*[SIGMAS[l % 4] for l in range(L)])


def call_accumulate(L, gdt, motion):
    cur, prev = (2, 1) if gdt == np.uint8 else (1, 0)
    p = mid.TemporalAccumParams(W, H, 0.2, 0.2, 32.0, 4.0, mid.api.fmt_with_guide(F32, mid.FMT_RGBA8 if gdt == np.uint8 else F32))
    cl = (ctypes.c_void_p * L)(*[d_g[gdt][cur][l % LRES].ptr for l in range(L)])
    pl = (ctypes.c_void_p * L)(*[d_g[gdt][prev][l % LRES].ptr for l in range(L)])
    sg, mv = sig(L), MOTION[motion].ptr if MOTION[motion] else None
    return lambda: ok(lib.mid_temporal_accumulate(ctx.handle, ctypes.byref(p), sg, d_fr[2].ptr, cl, pl, L, mv, d_hc.ptr, d_hs.ptr, d_vs.ptr,
                                                  d_col.ptr, d_st.ptr, d_v0.ptr, None), "mid_temporal_accumulate")


def call_moments(L, k):
    p = mid.AtrousMomentsParams(W, H, F32)
    fr = (ctypes.c_void_p * (2 * k + 1))(*[d_fr[f].ptr for f in range(2 - k, 3 + k)])
    tbl = (ctypes.c_void_p * ((2 * k + 1) * L))(*[d_g[np.uint8][f][l % LRES].ptr for f in range(2 - k, 3 + k) for l in range(L)])
    sg, into = sig(L), d_vs if k == 0 else d_v0
    return lambda: ok(lib.mid_atrous_moments(ctx.handle, ctypes.byref(p), sg, fr, tbl, L, 2 * k + 1, k, k, into.ptr, None), "mid_atrous_moments")


def call_variance(L, src):
    p = mid.AtrousVarianceParams(W, H, 0, 5, 4.0, 1e-3, F32)
    tbl, sg = (ctypes.c_void_p * L)(*[d_g[np.uint8][2][l % LRES].ptr for l in range(L)]), sig(L)
    return lambda: ok(lib.mid_atrous_variance(ctx.handle, ctypes.byref(p), sg, src.ptr, d_v0.ptr, tbl, L, d_out.ptr, F32, None, d_scr.ptr, None),
                      "mid_atrous_variance")


def timed(fn, reps=args.reps):
    fn()
    ok(lib.mid_timer_tick(timer, None), "tick")
    for _ in range(reps):
        fn()
    ok(lib.mid_timer_tock(timer, None), "tock")
    ms = ctypes.c_float()
    ok(lib.mid_timer_ms(timer, ctypes.byref(ms)), "ms")
    return ms.value / reps


LS = (1, 2, 3, 4, 16)
calls = {(L, gdt, m): call_accumulate(L, gdt, m) for L in LS for gdt in (np.uint8, np.float32) for m in MOTION}
rec_m, rec_a, rec_v = call_moments(3, 0), call_accumulate(3, np.uint8, "fractional"), call_variance(3, d_col)
win_m, win_v = call_moments(3, 2), call_variance(3, d_fr[2])
calls["recursive chain"] = lambda: (rec_m(), rec_a(), rec_v())
calls["window chain"] = lambda: (win_m(), win_v())
calls["moments k = 0"], calls["moments k = 2"], calls["five passes"] = rec_m, win_m, win_v

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


calls["copy"] = None
res = {key: [] for key in calls}
for _ in range(args.rounds):
    for key, fn in calls.items():
        res[key].append(timed_copy() if key == "copy" else timed(fn))
med = {key: statistics.median(v) for key, v in res.items()}
copy_rate = 2 * a.numel() * 4 / (med["copy"] * 1e-3) / 1e9          # GB/s, bytes read + bytes written
say(f"device-to-device copy of 256 MiB: {med['copy']:.4f} ms = {copy_rate:.0f} GB/s (read + written)")


def fig(key):
    return f"{med[key]:7.4f} ({min(res[key]):.4f}-{max(res[key]):.4f})"


say("\n1. one mid_temporal_accumulate call; kernel ms per call (spread), its algorithmic bytes per pixel, those bytes at the copy rate, ratio:")
for gdt in (np.uint8, np.float32):
    for L in LS:
        for m in MOTION:
            bpp = 16 + (8 if MOTION[m] else 0) + 32 + 4 + 36 + 2 * L * (4 if gdt == np.uint8 else 16)
            floor = bpp * NPIX / (copy_rate * 1e9) * 1e3
            say(f"  guides {np.dtype(gdt).name:7} L = {L:2} motion {m:10}: {fig((L, gdt, m))}   {bpp:4} B/pixel = {floor:.4f} ms at the copy rate   x {med[(L, gdt, m)] / floor:.2f}")

say("\n2. the per-frame chain, three RGBA8 layers, five variance passes:")
say(f"  recursive: moments k = 0 {fig('moments k = 0')} + accumulate {fig((3, np.uint8, 'fractional'))} + five passes   = {fig('recursive chain')}")
say(f"  window:    moments k = 2 {fig('moments k = 2')} + five passes {fig('five passes')}   = {fig('window chain')}")
say(f"  recursive / window {med['recursive chain'] / med['window chain']:.3f}")
lib.mid_timer_destroy(timer)
for d in (*d_fr, d_hc, d_hs, d_col, d_st, d_out, d_scr, d_vs, d_v0, *[x for ds in d_g.values() for row in ds for x in row], *[m for m in MOTION.values() if m]):
    d.free()
del a, b

# ---- 3. host to host ----
n, L, NSRC = args.frames, 4, 4
say(f"\n3. host to host, {n} x 1080p RGBA8 in and out, {L} RGBA8 layers per frame, pinned, overlap = 1, five passes")
src = [np.roll((f32[0] * 255).astype(np.uint8), 7 * i, 1) for i in range(NSRC)]
mvs = [np.stack([6 * np.sin(xx * 0.005 + 0.4 + i) * np.cos(yy * 0.007), 6 * np.cos(xx * 0.003 + yy * 0.005 + i)], -1).astype(np.float32) for i in range(NSRC)]
pin_in, pin_out, pin_l, pin_m = mid.PinnedFrames(ctx, src), mid.PinnedFrames(ctx, n, NPIX * 4), mid.PinnedFrames(ctx, g8[0]), mid.PinnedFrames(ctx, mvs)
hin = [pin_in.ptrs[i % NSRC] for i in range(n)]
hl = [pin_l.ptrs[j] for i in range(n) for j in range(L)]
hm = [pin_m.ptrs[i % NSRC] for i in range(n)]
KINDS = ("variance-guided a-trous, k = 2", "recursive, no motion", "recursive, motion planes")
stats = {kind: ([], [], []) for kind in KINDS}
for _ in range(args.rounds):
    for kind, (walls, spans, kerns) in stats.items():
        if kind == KINDS[0]:
            t = ctx.sequence_atrous_variance_pinned(hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, hl, L, SIGMAS, 2, 0, n, 5, 4.0, 1e-3, True, np.uint8)
        else:
            t = ctx.sequence_atrous_recursive_pinned(hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, hl, L, SIGMAS, hm if kind == KINDS[2] else None, 1, 0, 0, n,
                                                     overlap=True, out_dtype=np.uint8)
        _, o = ctx.pipe_last_timeline()
        walls.append(t[0])
        spans.append(max(x[2] for x in o) - min(x[1] for x in o))
        kerns.append(t[1])
rate = {}
for kind, (walls, spans, kerns) in stats.items():
    wall = statistics.median(walls)
    rate[kind] = n * NPIX / wall / 1e3
    say(f"  {kind:32}: {wall:8.2f} ms wall ({min(walls):.2f}-{max(walls):.2f}), {rate[kind]:7.1f} Mpixel/s, {wall / n:.3f} ms per frame; "
        f"compute stage spans {statistics.median(spans) / wall:.3f} of the wall time, its launches fill {statistics.median(kerns) / statistics.median(spans):.3f} of that span "
        f"({statistics.median(kerns) / n:.3f} ms of launches per frame)")
say(f"  recursive / variance-guided at k = 2: {rate[KINDS[1]] / rate[KINDS[0]]:.3f} without motion, {rate[KINDS[2]] / rate[KINDS[0]]:.3f} with motion planes")
for bb in (pin_in, pin_out, pin_l, pin_m):
    bb.free()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
