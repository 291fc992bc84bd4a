"""Kernel and host-to-host rates of joint layer-guided NLM against layered NLM on one MI355X (development aid; writes
profiles/r16_nlm_joint.txt when given --out).  1080p, both tuned windows, one lease, variants interleaved round by round.

1. Resident, output 2 of a five-frame sequence (k = 0: one neighbour, k = 2: five): the event time (mid_timer) of REPS back-to-back
   calls / REPS, median over the rounds, for L = 1 .. 4 RGBA8 layers, RGBA32F and RGBA8 frames, 21x21 / 7x7 and 14x14 / 6x6:
     layered   mid_nlm_layers_temporal: one complete NLM pass per (neighbour, layer) (the yardstick: that kernel is not changed by
               the joint filter);
     joint     mid_nlm_joint on the same frames and layers, one h per layer: one pass per neighbour.
   Expectation for L = 1: joint <= 1.1 x layered (the same work; the two give the same bits, which the tool checks).  For L >= 2:
   cheaper than layered, towards (a + b L) / (L (a + b)) with a ~ b read from the source (0.6 at L = 4); reported as met or missed.
2. Host to host: mid_sequence_nlm_joint against mid_sequence_nlm_layers_temporal over 64 RGBA8 frames in and out with 4 RGBA8 layers
   each, page-locked, overlap = 1, k = 0 and 2, 21x21 / 7x7: wall time, Mpixel/s, and from mid_pipe_last_timeline the share of the
   wall time the compute stage spans."""
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--frames", type=int, default=64)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: {lib.mid_last_error().decode()}")


W, H, LMAX, NF, T = 1920, 1080, 4, 5, 2
NPIX = W * H
HP = 0.5
HS = [0.5, 0.8, 0.4, 0.6]
WINDOWS = {"21x21/7x7": ((-10, 11), (-3, 4)), "14x14/6x6": ((-7, 7), (-3, 3))}
ctx = mid.Context(0)
say(f"device {ctx.name}; 1080p; layered: h = {HP}; joint: h per layer {HS}; {args.rounds} rounds x {args.reps} calls per figure")
rng = np.random.default_rng(16)
yy, xx = np.mgrid[0:H, 0:W]


def guide(i):
    return np.clip(np.stack([xx * (i % 4 + 1) % 256, yy * 2 % 256, (xx + yy) // 2 % 256, np.full_like(xx, 255)], -1)
                   + rng.integers(-3, 4, (H, W, 4)), 0, 255).astype(np.uint8)


g8 = [guide(i) for i in range(NF * LMAX)]                                            # frame-major: [f * LMAX + l]
f32 = [np.concatenate([rng.random((H, W, 3), dtype=np.float32), np.ones((H, W, 1), np.float32)], 2) for _ in range(NF)]
u8 = [(f * 255).astype(np.uint8) for f in f32]

# ---- 1. resident ----
d_fr = {"RGBA32F": [ctx.upload(f) for f in f32], "RGBA8": [ctx.upload(f) for f in u8]}
d_g = [ctx.upload(g) for g in g8]
d_out = {k: ctx.alloc(NPIX * 16) for k in ("layered", "joint")}
fr_tbl = {name: (ctypes.c_void_p * NF)(*[d.ptr for d in ds]) for name, ds in d_fr.items()}
timer = ctypes.c_void_p()
ok(lib.mid_timer_create(ctx.handle, ctypes.byref(timer)), "mid_timer_create")


def table(L):
    return (ctypes.c_void_p * (NF * L))(*[d_g[f * LMAX + l].ptr for f in range(NF) for l in range(L)])


def call_layered(p, fr, tbl, L, k):
    ok(lib.mid_nlm_layers_temporal(ctx.handle, ctypes.byref(p), fr, tbl, L, NF, k, T, 1, (ctypes.c_void_p * 1)(d_out["layered"].ptr),
                                   mid.FMT_RGBA32F, None), "mid_nlm_layers_temporal")


def call_joint(p, hh, fr, tbl, L, k):
    ok(lib.mid_nlm_joint(ctx.handle, ctypes.byref(p), hh, fr, tbl, L, NF, k, T, 1, (ctypes.c_void_p * 1)(d_out["joint"].ptr),
                         mid.FMT_RGBA32F, None), "mid_nlm_joint")


def timed(fn, reps=args.reps):
    fn()
    ok(lib.mid_timer_tick(timer, None), "tick")
    for _ in range(reps):
        fn()
    ok(lib.mid_timer_tock(timer, None), "tock")
    ms = ctypes.c_float()
    ok(lib.mid_timer_ms(timer, ctypes.byref(ms)), "ms")
    return ms.value / reps


calls = {}
for win, (search, patch) in WINDOWS.items():
    for fname, ffmt in (("RGBA32F", mid.FMT_RGBA32F), ("RGBA8", mid.FMT_RGBA8)):
        p = mid.NlmParams(W, H, HP, search[0], search[1], patch[0], patch[1], ffmt)
        for L in range(1, LMAX + 1):
            tbl = table(L)
            hh = (ctypes.c_float * L)(*([HP] if L == 1 else HS[:L]))                   # L = 1: the layered filter's own h
            for k in (0, 2):
                calls[(win, fname, L, k, "layered")] = lambda p=p, fr=fr_tbl[fname], tbl=tbl, L=L, k=k: call_layered(p, fr, tbl, L, k)
                calls[(win, fname, L, k, "joint")] = lambda p=p, hh=hh, fr=fr_tbl[fname], tbl=tbl, L=L, k=k: call_joint(p, hh, fr, tbl, L, k)
res = {key: [] for key in calls}
for _ in range(args.rounds):
    for key, fn in calls.items():
        res[key].append(timed(fn))
med = {key: statistics.median(v) for key, v in res.items()}
same = []
for win in WINDOWS:
    for fname in ("RGBA32F", "RGBA8"):
        for k in (0, 2):
            calls[(win, fname, 1, k, "layered")]()
            calls[(win, fname, 1, k, "joint")]()
            a, b = (ctx.download(d_out[x], (H, W, 4), np.float32) for x in ("layered", "joint"))
            same.append(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
say("\nresident, output 2 of 5 frames, kernel time per call in ms (spread over the rounds):")
say("  window     frames    L  k   layered                      joint                        joint / layered   (a + bL) / (L (a + b)), a = b")
worst_l1 = 0.0
for (win, fname, L, k, kind), m in med.items():
    if kind != "layered":
        continue
    lay, j = (win, fname, L, k, kind), (win, fname, L, k, "joint")
    ratio = med[j] / m
    if L == 1:
        worst_l1 = max(worst_l1, ratio)
    say(f"  {win:10} {fname:8} {L:2} {k:2}  {m:8.4f} ({min(res[lay]):.4f}-{max(res[lay]):.4f})"
        f"   {med[j]:8.4f} ({min(res[j]):.4f}-{max(res[j]):.4f})   {ratio:7.3f}           {(1 + L) / (2 * L):.3f}")
say(f"  L = 1: joint and layered outputs bit-identical: {all(same)}; worst joint / layered {worst_l1:.3f} "
    f"(expectation <= 1.1: {'met' if worst_l1 <= 1.1 else 'missed'})")
for win in WINDOWS:
    for L in range(2, LMAX + 1):
        rs = [med[(win, f, L, k, "joint")] / med[(win, f, L, k, "layered")] for f in ("RGBA32F", "RGBA8") for k in (0, 2)]
        say(f"  {win} L = {L}: joint / layered {min(rs):.3f} .. {max(rs):.3f} (expectation 'cheaper than the layered form': "
            f"{'met' if max(rs) < 1.0 else 'missed'})")
for d in (*d_out.values(), *d_g, *[x for ds in d_fr.values() for x in ds]):
    d.free()

# ---- 2. host to host ----
n, L = args.frames, LMAX
search, patch = WINDOWS["21x21/7x7"]
say(f"\nhost to host, {n} x 1080p RGBA8 in and out, {L} RGBA8 layers per frame, 21x21/7x7, pinned, overlap = 1")
pin_in, pin_out, pin_l = mid.PinnedFrames(ctx, u8), mid.PinnedFrames(ctx, n, NPIX * 4), mid.PinnedFrames(ctx, g8)
hin = [pin_in.ptrs[i % NF] for i in range(n)]
hl = [pin_l.ptrs[(i % NF) * LMAX + j] for i in range(n) for j in range(L)]
stats = {(kind, k): ([], []) for k in (0, 2) for kind in ("layered", "joint")}
for _ in range(min(args.rounds, 3)):
    for (kind, k), (walls, spans) in stats.items():
        if kind == "joint":
            t = ctx.sequence_nlm_joint_pinned(hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, hl, L, HS, k, 0, n, True, HP, search, patch, np.uint8)
        else:
            t = ctx.sequence_nlm_layers_temporal_pinned(hin, pin_out.ptrs, W, H, mid.FMT_RGBA8, hl, L, k, 0, n, True, HP, search, patch, np.uint8)
        _, o = ctx.pipe_last_timeline()
        walls.append(t[0])
        spans.append(max(x[2] for x in o) - min(x[1] for x in o))
for (kind, k), (walls, spans) in stats.items():
    wall = statistics.median(walls)
    say(f"  {kind:8} k = {k}: {wall:8.2f} ms wall ({min(walls):.2f}-{max(walls):.2f}), {n * NPIX / wall / 1e3:7.1f} Mpixel/s, {wall / n:.3f} ms per frame; "
        f"compute stage spans {statistics.median(spans) / wall:.3f} of the wall time")
for k in (0, 2):
    say(f"  k = {k}: joint / layered wall time {statistics.median(stats[('joint', k)][0]) / statistics.median(stats[('layered', k)][0]):.3f}")
for b in (pin_in, pin_out, pin_l):
    b.free()
lib.mid_timer_destroy(timer)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
