"""Kernel rates of history clipping on one MI355X (development aid; writes profiles/r24_history_clip.txt when given --out).  1080p,
one lease, variants interleaved round by round; a figure is the event time (mid_timer) of back-to-back calls / their number, median
over the rounds, with the spread over the rounds beside it (the method of DESIGN section 7).

a. One mid_color_bounds call, RGBA8 / RGBA32F frames, both radii.  Every call of a timed run works on its own planes and the sets
   of one variant add up to more than the 256 MiB cache.  Beside each figure the call's algorithmic bytes -- input texel once + 32 B
   out per pixel -- at the device-to-device copy rate measured in the same run.
b. mid_temporal_accumulate_clip against mid_temporal_accumulate: the same RGBA32F frame, RGBA8 layers (L = 1, 3), history, fractional
   motion and spatial variance; the clip planes are mid_color_bounds of the frame at gamma 1.  Planes reused: warm cache.
c. The per-frame chain of DESIGN 3.13's row 2 (RGBA32F frame, three RGBA8 layers, fractional motion: moments at k = 0, accumulate,
   five passes) with and without the clip (mid_color_bounds + mid_temporal_accumulate_clip in place of mid_temporal_accumulate).
d. Host to host over 64 RGBA8 frames with 4 RGBA8 layers, page-locked, overlap = 1, five passes, warm-up 0:
   mid_sequence_atrous_recursive_clip with cp = NULL and with the clip at both radii -- and, with --parent-lib PATH, the parent
   commit's library through mid_sequence_atrous_recursive_firefly (fp = NULL), which is the same call there.  The parent's library
   lacks the new symbols, so it runs in a child process of this tool (--child), once per round, in the round's turn -- and so does
   this library once more, through the same entry point: a fresh process and context per round against a fresh process and context.

No threshold is fixed for any of them: (a) and the added part of (b) are streaming, about 64 B per pixel more traffic on a chain of
roughly 0.8 ms."""
import argparse
import ctypes
import json
import statistics
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--parent-lib", default=None, help="libmi_denoise.so of the parent commit, for part d")
ap.add_argument("--child", default=None, help="(internal) run part d's call once warm and once timed on this library, print JSON")
args = ap.parse_args()

W, H = 1920, 1080
NPIX = W * H
SIGMAS = [0.2, 0.3, 0.15, 0.25]


class TA(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("alpha", ctypes.c_float), ("alphaMoments", ctypes.c_float),
                ("historyMax", ctypes.c_float), ("historyFull", ctypes.c_float), ("format", ctypes.c_int32)]


class AV(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("first_pass", ctypes.c_int32), ("n_passes", ctypes.c_int32),
                ("sigmaLum", ctypes.c_float), ("epsilon", ctypes.c_float), ("format", ctypes.c_int32)]


def child(path):
    """Part d on any library that has mid_sequence_atrous_recursive_firefly, through ctypes alone (no package, no torch)."""
    import numpy as np
    so = ctypes.CDLL(path)
    P = ctypes.c_void_p
    so.mid_last_error.restype = ctypes.c_char_p
    ctx = P()

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {so.mid_last_error().decode()}")
    ok(so.mid_ctx_create(ctypes.c_int(0), ctypes.byref(ctx)), "mid_ctx_create")
    n, L, NSRC = args.frames, 4, 4
    rng = np.random.default_rng(23)
    yy, xx = np.mgrid[0:H, 0:W]

    def pinned(nbytes, src=None):
        p = P()
        ok(so.mid_alloc_host(ctx, ctypes.c_size_t(nbytes), ctypes.byref(p)), "mid_alloc_host")
        if src is not None:
            ctypes.memmove(p, src.ctypes.data, nbytes)
        return p
    frame8 = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    src = [pinned(NPIX * 4, np.ascontiguousarray(np.roll(frame8, 7 * i, 1))) for i in range(NSRC)]
    lay = [pinned(NPIX * 4, np.clip(np.stack([xx * (i % 4 + 1) % 256, yy * 2 % 256, (xx + yy) // 2 % 256, np.full_like(xx, 255)], -1)
                                    + rng.integers(-3, 4, (H, W, 4)), 0, 255).astype(np.uint8)) for i in range(L)]
    outs = [pinned(NPIX * 4) for _ in range(n)]
    tp, vp = TA(W, H, 0.2, 0.2, 32.0, 4.0, 1), AV(W, H, 0, 5, 4.0, 1e-3, 1)      # MID_FMT_RGBA8 frames; guide field 0: RGBA8 layers
    hin = (P * n)(*[src[i % NSRC] for i in range(n)])
    hl = (P * (n * L))(*[lay[j] for i in range(n) for j in range(L)])
    hout = (P * n)(*outs)
    t = (ctypes.c_float * 3)()
    walls = []
    for _ in range(2):
        ok(so.mid_sequence_atrous_recursive_firefly(ctx, ctypes.byref(tp), ctypes.byref(vp), (ctypes.c_float * L)(*SIGMAS), hin, n, hl, L, None, None,
                                                    ctypes.c_float(0), None, 1, 0, 0, n, hout, 1, 1, t), "mid_sequence_atrous_recursive_firefly")
        walls.append((t[0], t[1]))
    for p in src + lay + outs:
        so.mid_free_host(ctx, p)
    so.mid_ctx_destroy(ctx)
    print(json.dumps({"wall_ms": walls[1][0], "kernel_ms": walls[1][1]}))


if args.child:
    child(args.child)
    sys.exit(0)

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import image_denoising_filter_amd as mid  # noqa: E402
from image_denoising_filter_amd._lib import lib  # noqa: E402

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: {lib.mid_last_error().decode()}")


F32, U8 = mid.FMT_RGBA32F, mid.FMT_RGBA8
BYTES = {U8: 4, F32: 16}
NAME = {U8: "RGBA8", F32: "RGBA32F"}
ctx = mid.Context(0)
say(f"device {ctx.name}; 1080p; {args.rounds} rounds x {args.reps} calls per figure")
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


def fig(r, key):
    return f"{statistics.median(r[key]):7.4f} ({min(r[key]):.4f}-{max(r[key]):.4f})"


# ---- a. the kernel ----
frame8 = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
host = {U8: frame8, F32: (frame8 / np.float32(255)).astype(np.float32)}
SETS = 2 * args.reps
assert SETS * NPIX * (4 + 32) > 256 << 20, "the sets of the smallest variant must pass the cache"
pool = {fmt: [ctx.upload(host[fmt]) for _ in range(SETS)] for fmt in (U8, F32)}
los, his = [ctx.alloc(NPIX * 16) for _ in range(SETS)], [ctx.alloc(NPIX * 16) for _ in range(SETS)]


def bounds_calls(fmt, radius):
    p = mid.ColorBoundsParams(W, H, radius, 1.0, fmt)
    return [lambda i=i: ok(lib.mid_color_bounds(ctx.handle, ctypes.byref(p), pool[fmt][i].ptr, los[i].ptr, his[i].ptr, None), "mid_color_bounds") for i in range(SETS)]


kernels = {(fmt, radius): (bounds_calls(fmt, radius), BYTES[fmt] + 32) for fmt in (U8, F32) for radius in (1, 2)}
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
say("\na. one mid_color_bounds call, every call on its own planes; kernel ms (spread), its algorithmic bytes per pixel, those bytes at the copy rate, ratio:")
for key, (_, bpp) in kernels.items():
    at_copy = bpp * NPIX / (copy_rate * 1e9) * 1e3
    say(f"  frame {NAME[key[0]]:7} radius {key[1]}: {fig(res, key)}   {bpp:3} B/pixel = {at_copy:.4f} ms at the copy rate   x {med[key] / at_copy:.2f}")
for d in [x for v in pool.values() for x in v] + los + his:
    d.free()

# ---- b. the accumulation, c. the per-frame chain ----
g8 = [[np.clip(np.stack([(xx + 2 * f) * (i % 4 + 1) % 256, yy * 2 % 256, (xx + yy + f) // 2 % 256, np.full_like(xx, 255)], -1)
               + rng.integers(-3, 4, (H, W, 4)), 0, 255).astype(np.uint8) for i in range(4)] for f in range(2)]
f32 = np.concatenate([rng.random((H, W, 3), dtype=np.float32), np.ones((H, W, 1), np.float32)], 2)
d_fr = ctx.upload(f32)
d_g = [[ctx.upload(g) for g in gs] for gs in g8]
d_mv = ctx.upload(np.stack([6 * np.sin(xx * 0.005 + 0.4) * np.cos(yy * 0.007), 6 * np.cos(xx * 0.003 + yy * 0.005 + 1.0)], -1).astype(np.float32))
d_hc = ctx.upload(np.roll(f32, 3, 1))
d_hs = ctx.upload(np.stack([f32[..., 0], f32[..., 0] ** 2 + 0.01, np.full((H, W), 5, np.float32), np.zeros((H, W), np.float32)], -1))
d_col, d_st, d_out, d_lo, d_hi = (ctx.alloc(NPIX * 16) for _ in range(5))
d_scr = ctx.alloc(2 * NPIX * 20)
d_vs, d_v0 = ctx.alloc(NPIX * 4), ctx.alloc(NPIX * 4)
word = mid.api.fmt_with_guide(F32, U8)
tp = mid.TemporalAccumParams(W, H, 0.2, 0.2, 32.0, 4.0, word)
mp, vp = mid.AtrousMomentsParams(W, H, word), mid.AtrousVarianceParams(W, H, 0, 5, 4.0, 1e-3, word)
cps = {r: mid.ColorBoundsParams(W, H, r, 1.0, F32) for r in (1, 2)}


def tables(L):
    return (ctypes.c_float * L)(*SIGMAS[:L]), (ctypes.c_void_p * L)(*[d_g[1][l].ptr for l in range(L)]), (ctypes.c_void_p * L)(*[d_g[0][l].ptr for l in range(L)])


def bounds(radius):
    ok(lib.mid_color_bounds(ctx.handle, ctypes.byref(cps[radius]), d_fr.ptr, d_lo.ptr, d_hi.ptr, None), "mid_color_bounds")


def accumulate(L, clip):
    sg, cl, pl = tables(L)
    if clip:
        ok(lib.mid_temporal_accumulate_clip(ctx.handle, ctypes.byref(tp), sg, d_fr.ptr, cl, pl, L, d_mv.ptr, d_hc.ptr, d_hs.ptr, d_vs.ptr, d_lo.ptr, d_hi.ptr,
                                            d_col.ptr, d_st.ptr, d_v0.ptr, None), "mid_temporal_accumulate_clip")
    else:
        ok(lib.mid_temporal_accumulate(ctx.handle, ctypes.byref(tp), sg, d_fr.ptr, cl, pl, L, d_mv.ptr, d_hc.ptr, d_hs.ptr, d_vs.ptr, d_col.ptr, d_st.ptr,
                                       d_v0.ptr, None), "mid_temporal_accumulate")


def chain(radius):
    L = 3
    sg, cl, pl = tables(L)
    fr = (ctypes.c_void_p * 1)(d_fr.ptr)
    ok(lib.mid_atrous_moments(ctx.handle, ctypes.byref(mp), sg, fr, cl, L, 1, 0, 0, d_vs.ptr, None), "mid_atrous_moments")
    if radius:
        bounds(radius)
    accumulate(L, bool(radius))
    ok(lib.mid_atrous_variance(ctx.handle, ctypes.byref(vp), sg, d_col.ptr, d_v0.ptr, cl, L, d_out.ptr, F32, None, d_scr.ptr, None), "mid_atrous_variance")


bounds(1)
ok(lib.mid_memset(ctx.handle, d_vs.ptr, 0, NPIX * 4, None), "mid_memset")
runs = {"accumulate L=1": lambda: accumulate(1, False), "accumulate_clip L=1": lambda: accumulate(1, True),
        "accumulate L=3": lambda: accumulate(3, False), "accumulate_clip L=3": lambda: accumulate(3, True),
        "chain": lambda: chain(0), "chain + clip radius 1": lambda: chain(1), "chain + clip radius 2": lambda: chain(2),
        "bounds 1 alone (warm)": lambda: bounds(1), "bounds 2 alone (warm)": lambda: bounds(2)}
cres = {key: [] for key in runs}
for _ in range(args.rounds):
    for key, fn in runs.items():
        cres[key].append(timed([fn] * 5))
cm = {key: statistics.median(v) for key, v in cres.items()}
say("\nb. mid_temporal_accumulate_clip against mid_temporal_accumulate, RGBA32F frame, RGBA8 layers, fractional motion, the same planes (warm cache):")
for L in (1, 3):
    u, c = f"accumulate L={L}", f"accumulate_clip L={L}"
    say(f"  L = {L}: unclipped {fig(cres, u)}, clipped {fig(cres, c)}: + {cm[c] - cm[u]:.4f} ms, x {cm[c] / cm[u]:.3f}"
        f"   (32 B per pixel more to read = {32 * NPIX / (copy_rate * 1e9) * 1e3:.4f} ms at the copy rate)")
say("\nc. the per-frame chain (moments k = 0, accumulate, five passes; RGBA32F frame, three RGBA8 layers, fractional motion; planes reused):")
say(f"  without the clip: {fig(cres, 'chain')}")
for r in (1, 2):
    k = f"chain + clip radius {r}"
    say(f"  with the clip at radius {r}: {fig(cres, k)}: + {cm[k] - cm['chain']:.4f} ms, x {cm[k] / cm['chain']:.3f}; mid_color_bounds alone, warm, "
        f"{fig(cres, f'bounds {r} alone (warm)')}")
lib.mid_timer_destroy(timer)
for d in (d_fr, d_mv, d_hc, d_hs, d_col, d_st, d_out, d_lo, d_hi, d_scr, d_vs, d_v0, *[x for row in d_g for x in row]):
    d.free()

# ---- d. host to host ----
n, L, NSRC = args.frames, 4, 4
say(f"\nd. host to host, {n} x 1080p RGBA8 in and out, {L} RGBA8 layers per frame, pinned, overlap = 1, five passes, warm-up 0")
src = [np.roll(frame8, 7 * i, 1) for i in range(NSRC)]
pin_in, pin_out, pin_l = mid.PinnedFrames(ctx, src), mid.PinnedFrames(ctx, n, NPIX * 4), mid.PinnedFrames(ctx, g8[0])
hin = [pin_in.ptrs[i % NSRC] for i in range(n)]
hl = [pin_l.ptrs[j] for i in range(n) for j in range(L)]
KINDS = {"this library, cp = NULL": {}, "this library, clip radius 1": dict(clip_gamma=1.0), "this library, clip radius 2": dict(clip_gamma=1.0, clip_radius=2)}
CHILD = {}
if args.parent_lib:
    CHILD = {"the parent's library, child process": args.parent_lib, "this library, child process": mid.LIB_PATH}
    KINDS = {**{k: None for k in CHILD}, **KINDS}
stats = {kind: ([], []) for kind in KINDS}
for kind in KINDS:                                                      # one untimed call each: the context's cache grows here
    if KINDS[kind] is not None:
        ctx.sequence_atrous_recursive_pinned(hin, pin_out.ptrs, W, H, U8, hl, L, SIGMAS, None, 1, 0, 0, n, overlap=True, out_dtype=np.uint8, **KINDS[kind])
for _ in range(args.rounds):
    for kind, (walls, kerns) in stats.items():
        if KINDS[kind] is None:
            r = subprocess.run([sys.executable, __file__, "--child", CHILD[kind], "--frames", str(n)], capture_output=True, text=True, check=True)
            t = json.loads(r.stdout.strip().splitlines()[-1])
            t = (t["wall_ms"], t["kernel_ms"])
        else:
            t = ctx.sequence_atrous_recursive_pinned(hin, pin_out.ptrs, W, H, U8, hl, L, SIGMAS, None, 1, 0, 0, n, overlap=True, out_dtype=np.uint8, **KINDS[kind])
        walls.append(t[0])
        kerns.append(t[1])
rate = {}
for kind, (walls, kerns) in stats.items():
    wall = statistics.median(walls)
    rate[kind] = n * NPIX / wall / 1e3
    say(f"  {kind:36}: {wall:8.2f} ms wall ({min(walls):.2f}-{max(walls):.2f}), {rate[kind]:7.1f} Mpixel/s, {wall / n:.3f} ms per frame, "
        f"{statistics.median(kerns) / n:.3f} ms of launches per frame")
base = "this library, cp = NULL"
for kind in KINDS:
    if kind != base and kind not in CHILD:
        say(f"  {kind} / {base}: {rate[kind] / rate[base]:.3f}")
if CHILD:
    ours, theirs = list(CHILD)[1], list(CHILD)[0]
    say(f"  {ours} / {theirs}: {rate[ours] / rate[theirs]:.3f}")
for bb in (pin_in, pin_out, pin_l):
    bb.free()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
