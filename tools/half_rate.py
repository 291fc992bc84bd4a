"""RGBA16F vs RGBA32F on one MI355X (development aid; writes profiles/r07_half_rates.txt when given --out).

1. Kernel time by input format, interleaved runs: NLM 21x21/7x7 at 1080p with 8-frame and 1-frame launches, bilateral r = 8.
2. Host -> host frame pipeline over 16 and 64 frames at 1080p: RGBA32F -> RGBA32F (mid_sequence_nlm_range) against
   RGBA16F -> RGBA16F (mid_sequence_nlm_range_f16), pinned in and out, k = 0, with the each-way pinned-copy ceiling measured
   in the same run for both pixel sizes.
Prints the sha256 of the timed kernels' code (image_denoising_filter_amd/_codeobj.py) so that a figure can be tied to a build."""
import argparse
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import image_denoising_filter_amd as mid  # noqa: E402
from image_denoising_filter_amd import _codeobj  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
ctx = mid.Context(0)
W, H, NPIX = bench.W, bench.H, bench.NPIX
SEARCH, PATCH = (-10, 11), (-3, 4)
say(f"device {ctx.name}; library {os.path.relpath(mid.LIB_PATH)}")
for fmt in (0, 2):
    for name, mangled in (("nlm 21x21/7x7 fused single", f"_ZN3mid16nlm_strip_kernelILin10ELi11ELin3ELi4ELi8ELi4ELi{fmt}ELb1ELb0ELb0ELi0EEEvNS_7NlmArgsE"),
                          ("nlm 21x21/7x7 fused multi", f"_ZN3mid16nlm_strip_kernelILin10ELi11ELin3ELi4ELi8ELi4ELi{fmt}ELb1ELb1ELb0ELi0EEEvNS_7NlmArgsE"),
                          ("nlm 21x21/7x7 small (TAG 1)", f"_ZN3mid16nlm_strip_kernelILin10ELi11ELin3ELi4ELi8ELi4ELi{fmt}ELb1ELb0ELb0ELi1EEEvNS_7NlmArgsE"),
                          ("bilateral r8 texture", f"_ZN3mid16bilateral_kernelILi8ELi2ELi8ELi{fmt}ELb0ELi0ENS_6BilOneEEEvNS_7BilArgsET5_")):
        try:
            sha, nbytes = _codeobj.kernel_sha256(mid.LIB_PATH, mangled)
            sha = f"{sha} ({nbytes} B)"
        except Exception as e:  # noqa: BLE001
            sha = f"n/a ({e})"
        say(f"kernel sha256 fmt={fmt} {name}: {sha}")

# ---- 1. kernel time by input format ------------------------------------------------------------------------------
F = 8
f32 = bench.synth_frames(F, 100, dev)
f16 = [f.to(torch.float16).contiguous() for f in f32]
w32 = [f.to(torch.float32).contiguous() for f in f16]          # the widened frames: the same pixels in both formats
outs = [torch.empty((H, W, 4), device=dev) for _ in range(F)]
ts = torch.cuda.Stream()
torch.cuda.set_stream(ts)
s = ts.cuda_stream
op = [o.data_ptr() for o in outs]


def time_nlm(fp, fmt, nf, n):
    tm = bench.Timers(mid, ctx, 1)
    tm.tick(0, s)
    for _ in range(n):
        ctx.nlm_temporal_dev(fp[:nf], op[:nf], W, H, 0.5, SEARCH, PATCH, 0, 0, nf, fmt, s)
    tm.tock(0, s)
    torch.cuda.synchronize()
    ms = tm.ms()[0] / n
    tm.close()
    return ms


def time_bil(p, fmt, n):
    tm = bench.Timers(mid, ctx, 1)
    tm.tick(0, s)
    for _ in range(n):
        ctx.bilateral_dev(p, op[0], W, H, 8, 2.0, 0.2, mid.LAYOUT_TEXTURE, fmt, s)
    tm.tock(0, s)
    torch.cuda.synchronize()
    ms = tm.ms()[0] / n
    tm.close()
    return ms


cases = {"rgba32f": ([f.data_ptr() for f in w32], mid.FMT_RGBA32F), "rgba16f": ([f.data_ptr() for f in f16], mid.FMT_RGBA16F)}
res = {k: {"nlm8": [], "nlm1": [], "bil8": []} for k in cases}
for name, (fp, fmt) in cases.items():        # warm-up (LDS limits, code load)
    time_nlm(fp, fmt, 8, 1); time_nlm(fp, fmt, 1, 2); time_bil(fp[0], fmt, 3)
for rep in range(args.reps):                 # interleaved: 32F, 16F, 32F, 16F, ...
    for name, (fp, fmt) in cases.items():
        res[name]["nlm8"].append(time_nlm(fp, fmt, 8, 5))
        res[name]["nlm1"].append(time_nlm(fp, fmt, 1, 10))
        res[name]["bil8"].append(time_bil(fp[0], fmt, 20))
say(f"kernel time, ms per launch, median of {args.reps} interleaved repetitions (min..max):")
for key, what, frames in (("nlm8", "NLM 21x21/7x7 1080p 8-frame launch", 8), ("nlm1", "NLM 21x21/7x7 1080p 1-frame launch", 1),
                          ("bil8", "bilateral r=8 texture 1080p", 1)):
    m32, m16 = float(np.median(res["rgba32f"][key])), float(np.median(res["rgba16f"][key]))
    say(f"  {what}: RGBA32F {m32:.4f} ({min(res['rgba32f'][key]):.4f}..{max(res['rgba32f'][key]):.4f})  "
        f"RGBA16F {m16:.4f} ({min(res['rgba16f'][key]):.4f}..{max(res['rgba16f'][key]):.4f})  "
        f"16F/32F {m16 / m32:.4f}  [{frames * NPIX / m16 / 1e3:.0f} Mpixel/s at RGBA16F]")
# same bits, checked once here too (the tests check it exhaustively)
ctx.nlm_temporal_dev(cases["rgba16f"][0][:2], op[:2], W, H, 0.5, SEARCH, PATCH, 0, 0, 2, mid.FMT_RGBA16F, s)
torch.cuda.synchronize()
a = [o.clone() for o in outs[:2]]
ctx.nlm_temporal_dev(cases["rgba32f"][0][:2], op[:2], W, H, 0.5, SEARCH, PATCH, 0, 0, 2, mid.FMT_RGBA32F, s)
torch.cuda.synchronize()
say(f"  outputs RGBA16F == RGBA32F on the widened frames (bits): {all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, outs[:2]))}")
torch.cuda.set_stream(torch.cuda.default_stream())
del outs, f32, w32

# ---- 2. host -> host pipeline -------------------------------------------------------------------------------------


def ceiling(nbytes, n=16):
    up, down = mid.PinnedFrames(ctx, n, nbytes), mid.PinnedFrames(ctx, n, nbytes)
    d_up, d_down = ctx.alloc(nbytes), ctx.alloc(nbytes)
    s_up, s_down = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    try:
        def go():
            for i in range(n):
                assert mid.lib.mid_memcpy_h2d(ctx.handle, d_up.ptr, up.ptrs[i], nbytes, s_up.cuda_stream) == 0
                assert mid.lib.mid_memcpy_d2h(ctx.handle, down.ptrs[i], d_down.ptr, nbytes, s_down.cuda_stream) == 0
            ctx.sync(s_up.cuda_stream)
            ctx.sync(s_down.cuda_stream)
        go()
        ts_ = []
        for _ in range(3):
            t0 = time.perf_counter()
            go()
            ts_.append(time.perf_counter() - t0)
        t = sorted(ts_)[1]
        return n * nbytes / t / 1e9
    finally:
        up.free(); down.free(); d_up.free(); d_down.free()


hf16 = [f.cpu().numpy() for f in f16]
hf32 = [f.astype(np.float32) for f in hf16]
for nframes in (16, 64):
    seq16 = [hf16[i % F] for i in range(nframes)]
    seq32 = [hf32[i % F] for i in range(nframes)]
    pins = {}
    for name, seq, bpp in (("rgba32f", seq32, 16), ("rgba16f", seq16, 8)):
        uniq = mid.PinnedFrames(ctx, seq[:F])
        pins[name] = (uniq, [uniq.ptrs[i % F] for i in range(nframes)], mid.PinnedFrames(ctx, nframes, NPIX * bpp),
                      mid.FMT_RGBA32F if bpp == 16 else mid.FMT_RGBA16F, None if bpp == 16 else np.float16)
    walls = {"rgba32f": [], "rgba16f": []}
    for name, (_, hin, hout, fmt, odt) in pins.items():    # first calls: allocate the context's cache
        ctx.sequence_nlm_pinned(hin, hout.ptrs, W, H, fmt, k=0, search=SEARCH, patch=PATCH, out_dtype=odt)
    for rep in range(args.reps):
        for name, (_, hin, hout, fmt, odt) in pins.items():
            t0 = time.perf_counter()
            ctx.sequence_nlm_pinned(hin, hout.ptrs, W, H, fmt, k=0, search=SEARCH, patch=PATCH, out_dtype=odt)
            walls[name].append((time.perf_counter() - t0) * 1e3)
    c16, c8 = ceiling(NPIX * 16), ceiling(NPIX * 8)
    say(f"pipeline host->host, {nframes} x 1080p, k=0, pinned in/out, median of {args.reps} interleaved calls:")
    for name, bpp, c in (("rgba32f", 16, c16), ("rgba16f", 8, c8)):
        ms = float(np.median(walls[name]))
        mpx = nframes * NPIX / ms / 1e3
        say(f"  {name} -> {name}: {ms:.2f} ms  {mpx:.0f} Mpixel/s (min..max {nframes * NPIX / max(walls[name]) / 1e3:.0f}..{nframes * NPIX / min(walls[name]) / 1e3:.0f})  "
            f"link ceiling each way at {bpp} B/px {c:.1f} GB/s = {c * 1e9 / bpp / 1e6:.0f} Mpixel/s  frac {mpx * bpp * 1e6 / 1e9 / c:.3f}")
    # where the time of the last call of each format goes: mid_pipe_last_timeline (the call's own events, no profiler)
    for name, (_, hin, hout, fmt, odt) in pins.items():
        ctx.sequence_nlm_pinned(hin, hout.ptrs, W, H, fmt, k=0, search=SEARCH, patch=PATCH, out_dtype=odt)
        ups, outs_tl = ctx.pipe_last_timeline()
        kern = np.array([ke - ks for _, ks, ke, _, _ in outs_tl])
        dl = np.array([de - ds for _, _, _, ds, de in outs_tl])
        lag = np.array([de - ke for _, _, ke, _, de in outs_tl])
        up = np.array([e - b for _, b, e in ups])
        q = max(1, len(outs_tl) // 4)
        say(f"  timeline {name} ({nframes} frames, {'direct stores' if dl.max() == 0 else 'staged download'}): end {max(o[4] for o in outs_tl):.2f} ms; "
            f"kernel ms/frame first/last quarter {kern[:q].mean():.3f}/{kern[-q:].mean():.3f}; download ms/frame {dl[:q].mean():.3f}/{dl[-q:].mean():.3f}; "
            f"kernel end -> output on host {lag[:q].mean():.3f}/{lag[-q:].mean():.3f}; upload ms/frame {up[:q].mean():.3f}/{up[-q:].mean():.3f}")
    for name, (uniq, _, hout, _, _) in pins.items():
        uniq.free(); hout.free()
ctx.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
