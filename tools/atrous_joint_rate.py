"""Kernel and host-to-host rates of the edge-avoiding a-trous filter on one MI355X (development aid; writes
profiles/r18_atrous_joint.txt when given --out).  1080p, one lease, variants interleaved round by round; a figure is the event
time (mid_timer) of REPS back-to-back calls / REPS, median over the rounds, with the spread over the rounds beside it.

1. The step-1 pass (mid_atrous_joint, one pass, first_pass = 0) against mid_bilateral_joint at radius 2, k = 0, on the same frame
   and layers: the same 25 taps and guide terms.  RGBA32F and RGBA8 frames, L = 1 .. 4 RGBA8 and RGBA32F guides.
   Expectation: <= 1.1 x.
2. Every later step (one pass, first_pass = i) relative to step 1, and against the pass's algorithmic bytes -- 16 B + L (4 | 16) B
   read and 16 B written per pixel -- at the device-to-device copy rate measured in the same run.  No ratio is fixed in advance.
3. Five passes with three layers against mid_bilateral_joint at radius 8 with the same layers: a +-62 support next to a +-8 one.
4. Host to host over 64 RGBA8 frames with 4 RGBA8 layers, page-locked, overlap = 1: mid_sequence_atrous_joint (five passes) against
   mid_sequence_bilateral_joint at k = 0, radius 8.  Expectation: the same (upload) bound.

--alt NAME=PATH (repeatable): another build of the library (say, csrc/atrous.hip compiled with -DMID_ATROUS_COMB_MAX_STEP=0: every
step from 4 on with global taps), loaded side by side with plain ctypes; table 2 then carries its passes as well, interleaved with
the shipped library's in the same rounds: the numbers behind the choice of a class per step."""
import argparse
import ctypes
import statistics
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import image_denoising_filter_amd as mid  # noqa: E402
from image_denoising_filter_amd._lib import lib  # noqa: E402
from image_denoising_filter_amd.api import fmt_with_guide  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: {lib.mid_last_error().decode()}")


W, H, LMAX = 1920, 1080, 4
NPIX = W * H
SS = 2.0
SIGMAS = [0.2, 0.3, 0.15, 0.25]
FMTS = (("RGBA32F", mid.FMT_RGBA32F), ("RGBA8", mid.FMT_RGBA8))
ctx = mid.Context(0)
say(f"device {ctx.name}; 1080p; sigmas {SIGMAS}, no colour term; {args.rounds} rounds x {args.reps} calls per figure")
rng = np.random.default_rng(18)
yy, xx = np.mgrid[0:H, 0:W]


def guide(i):
    return np.clip(np.stack([xx * (i % 4 + 1) % 256, yy * 2 % 256, (xx + yy) // 2 % 256, np.full_like(xx, 255)], -1)
                   + rng.integers(-3, 4, (H, W, 4)), 0, 255).astype(np.uint8)


g8 = [guide(i) for i in range(LMAX)]
f32 = np.concatenate([rng.random((H, W, 3), dtype=np.float32), np.ones((H, W, 1), np.float32)], 2)
d_fr = {"RGBA32F": ctx.upload(f32), "RGBA8": ctx.upload((f32 * 255).astype(np.uint8))}
d_g = {"RGBA8": [ctx.upload(g) for g in g8], "RGBA32F": [ctx.upload(g.astype(np.float32) / np.float32(255)) for g in g8]}
d_out, d_scr = ctx.alloc(NPIX * 16), ctx.alloc(2 * NPIX * 16)
timer = ctypes.c_void_p()
ok(lib.mid_timer_create(ctx.handle, ctypes.byref(timer)), "mid_timer_create")
# builds loaded side by side: (library, its own context, its own timer); "" is the shipped one
BUILDS = {"": (lib, ctx.handle, timer)}
for spec in args.alt:
    name, path = spec.split("=", 1)
    alt = ctypes.CDLL(path)
    alt.mid_last_error.restype = ctypes.c_char_p
    alt.mid_atrous_joint.argtypes = lib.mid_atrous_joint.argtypes
    for fn in ("mid_timer_tick", "mid_timer_tock", "mid_timer_ms"):
        getattr(alt, fn).argtypes = getattr(lib, fn).argtypes
    h_alt, t_alt = ctypes.c_void_p(), ctypes.c_void_p()
    assert alt.mid_ctx_create(0, ctypes.byref(h_alt)) == 0 and alt.mid_timer_create(h_alt, ctypes.byref(t_alt)) == 0, path
    BUILDS[name] = (alt, h_alt, t_alt)


def word(fmt, gname):
    return fmt if gname == "RGBA8" else fmt_with_guide(fmt, mid.FMT_RGBA32F)


def call_atrous(fname, fmt, gname, L, first, passes, build=""):
    p = mid.AtrousParams(W, H, first, passes, 0.0, word(fmt, gname))
    sg = (ctypes.c_float * L)(*SIGMAS[:L])
    tbl = (ctypes.c_void_p * L)(*[d.ptr for d in d_g[gname][:L]])
    b_lib, b_ctx, _ = BUILDS[build]
    return lambda: ok(b_lib.mid_atrous_joint(b_ctx, ctypes.byref(p), sg, d_fr[fname].ptr, tbl, L, d_out.ptr, mid.FMT_RGBA32F, d_scr.ptr, None),
                      "mid_atrous_joint")


def call_bilateral(fname, fmt, gname, L, radius):
    p = mid.BilateralParams(W, H, SS, 0.2, radius, mid.LAYOUT_TEXTURE, word(fmt, gname))
    sg = (ctypes.c_float * L)(*SIGMAS[:L])
    tbl = (ctypes.c_void_p * L)(*[d.ptr for d in d_g[gname][:L]])
    fr, ou = (ctypes.c_void_p * 1)(d_fr[fname].ptr), (ctypes.c_void_p * 1)(d_out.ptr)
    return lambda: ok(lib.mid_bilateral_joint(ctx.handle, ctypes.byref(p), sg, fr, tbl, L, 1, 0, 0, 1, ou, mid.FMT_RGBA32F, None), "mid_bilateral_joint")


def timed(fn, reps=args.reps, build=""):
    b_lib, _, b_timer = BUILDS[build]
    fn()
    ok(b_lib.mid_timer_tick(b_timer, None), "tick")
    for _ in range(reps):
        fn()
    ok(b_lib.mid_timer_tock(b_timer, None), "tock")
    ms = ctypes.c_float()
    ok(b_lib.mid_timer_ms(b_timer, ctypes.byref(ms)), "ms")
    return ms.value / reps


calls = {}
for fname, fmt in FMTS:
    for gname in ("RGBA8", "RGBA32F"):
        for L in range(1, LMAX + 1):
            calls[("bil r2", fname, gname, L)] = call_bilateral(fname, fmt, gname, L, 2)
            for i in range(8 if fname == "RGBA32F" else 1):
                calls[(f"step {1 << i}", fname, gname, L)] = call_atrous(fname, fmt, gname, L, i, 1)
                for name in list(BUILDS)[1:]:
                    calls[(f"step {1 << i}", fname, gname, L, name)] = call_atrous(fname, fmt, gname, L, i, 1, name)
        calls[("bil r8", fname, gname, 3)] = call_bilateral(fname, fmt, gname, 3, 8)
        calls[("5 passes", fname, gname, 3)] = call_atrous(fname, fmt, gname, 3, 0, 5)
res = {key: [] for key in calls}
copy_ms = []
a, b = torch.empty(64 << 20, dtype=torch.float32, device="cuda"), torch.empty(64 << 20, dtype=torch.float32, device="cuda")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for _ in range(args.rounds):
    for key, fn in calls.items():
        res[key].append(timed(fn, build=key[4] if len(key) > 4 else ""))
    ctx.sync()
    b.copy_(a)
    e0.record()
    for _ in range(args.reps):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    copy_ms.append(e0.elapsed_time(e1) / args.reps)
med = {key: statistics.median(v) for key, v in res.items()}


def fig(key):
    return f"{med[key]:8.4f} ({min(res[key]):.4f}-{max(res[key]):.4f})"


copy_rate = 2 * a.numel() * 4 / (statistics.median(copy_ms) * 1e-3) / 1e9          # GB/s, bytes read + bytes written
say(f"device-to-device copy of 256 MiB: {statistics.median(copy_ms):.4f} ms = {copy_rate:.0f} GB/s (read + written)")

say("\n1. the step-1 pass against mid_bilateral_joint at radius 2, k = 0; kernel time per call in ms (spread over the rounds):")
say("  frames   guides    L   bilateral r = 2               a-trous step 1                a-trous / bilateral")
worst = 0.0
for fname, _ in FMTS:
    for gname in ("RGBA8", "RGBA32F"):
        for L in range(1, LMAX + 1):
            kb, ka = ("bil r2", fname, gname, L), ("step 1", fname, gname, L)
            ratio = med[ka] / med[kb]
            worst = max(worst, ratio)
            say(f"  {fname:8} {gname:8} {L:2}   {fig(kb)}   {fig(ka)}   {ratio:7.3f}")
say(f"  worst a-trous / bilateral {worst:.3f} (expectation <= 1.1: {'met' if worst <= 1.1 else 'missed'})")

say("\n2. every step, RGBA32F frames: ms per pass, relative to step 1, and the pass's algorithmic bytes at the copy rate above:")
say("  guides    L   bytes/pixel  at copy rate   " + "".join(f"step {1 << i:<10}" for i in range(8)))
for gname, gb in (("RGBA8", 4), ("RGBA32F", 16)):
    for L in range(1, LMAX + 1):
        bpp = 32 + L * gb
        floor = bpp * NPIX / (copy_rate * 1e9) * 1e3
        ms = [med[(f"step {1 << i}", "RGBA32F", gname, L)] for i in range(8)]
        say(f"  {gname:8} {L:2}   {bpp:5}        {floor:7.4f} ms    " + "".join(f"{m:7.4f}        " for m in ms))
        say(f"  {'':8} {'':2}   {'':5}        x step 1      " + "".join(f"{m / ms[0]:7.2f}        " for m in ms))
        say(f"  {'':8} {'':2}   {'':5}        x bytes       " + "".join(f"{m / floor:7.2f}        " for m in ms))
        for name in list(BUILDS)[1:]:
            alt_ms = [med[(f"step {1 << i}", "RGBA32F", gname, L, name)] for i in range(8)]
            say(f"  {'':8} {'':2}   build {name:16.16}         " + "".join(f"{m:7.4f}        " for m in alt_ms))
            say(f"  {'':8} {'':2}   shipped / {name:12.12}         " + "".join(f"{m / x:7.2f}        " for m, x in zip(ms, alt_ms)))

say("\n3. five passes (+-62) with three layers against mid_bilateral_joint at radius 8 (+-8) with the same layers:")
for fname, _ in FMTS:
    for gname in ("RGBA8", "RGBA32F"):
        kb, ka = ("bil r8", fname, gname, 3), ("5 passes", fname, gname, 3)
        say(f"  {fname:8} {gname:8}  bilateral r = 8 {fig(kb)}   a-trous, 5 passes {fig(ka)}   ratio {med[ka] / med[kb]:.3f}")
for d in (*d_fr.values(), d_out, d_scr, *[x for ds in d_g.values() for x in ds]):
    d.free()
del a, b

# ---- 4. host to host ----
n, L, NF = args.frames, LMAX, 4
say(f"\n4. host to host, {n} x 1080p RGBA8 in and out, {L} RGBA8 layers per frame, pinned, overlap = 1")
src = [np.roll((f32 * 255).astype(np.uint8), 7 * i, 1) for i in range(NF)]
pin_in, pin_out, pin_l = mid.PinnedFrames(ctx, src), mid.PinnedFrames(ctx, n, NPIX * 4), mid.PinnedFrames(ctx, g8)
hin = [pin_in.ptrs[i % NF] for i in range(n)]
hl = [pin_l.ptrs[j] for i in range(n) for j in range(L)]
stats = {kind: ([], []) for kind in ("bilateral joint r = 8, k = 0", "a-trous, 5 passes")}
for _ in range(args.rounds):
    for kind, (walls, spans) in stats.items():
        if kind.startswith("a-trous"):
            t = ctx.sequence_atrous_joint_pinned(hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, hl, L, SIGMAS, 5, 0, 0.0, 0, n, True, np.uint8)
        else:
            t = ctx.sequence_bilateral_joint_pinned(hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, hl, L, SIGMAS, 0, 0, n, 8, SS, 0.2, True, np.uint8)
        _, o = ctx.pipe_last_timeline()
        walls.append(t[0])
        spans.append(max(x[2] for x in o) - min(x[1] for x in o))
rate = {}
for kind, (walls, spans) in stats.items():
    wall = statistics.median(walls)
    rate[kind] = n * NPIX / wall / 1e3
    say(f"  {kind:30}: {wall:8.2f} ms wall ({min(walls):.2f}-{max(walls):.2f}), {rate[kind]:7.1f} Mpixel/s, {wall / n:.3f} ms per frame; "
        f"compute stage spans {statistics.median(spans) / wall:.3f} of the wall time")
ra, rb = rate["a-trous, 5 passes"], rate["bilateral joint r = 8, k = 0"]
say(f"  a-trous / bilateral joint {ra / rb:.3f} (expectation: the same upload bound, within 5 %: {'met' if ra >= 0.95 * rb else 'missed'})")
for bb in (pin_in, pin_out, pin_l):
    bb.free()
lib.mid_timer_destroy(timer)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
