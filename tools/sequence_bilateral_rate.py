"""Host -> host rate of mid_sequence_bilateral on one MI355X (development aid; writes profiles/r07_sequence_bilateral.txt when given
--out).

Variants, interleaved round by round so that every figure sees the same lease: 16 and 64 frames at 1080p, r = 8, texture layout;
  u8      RGBA8 in -> RGBA8 out, pinned (outputs stored by the kernel)
  f32     RGBA32F in -> RGBA32F out, pinned
  f16     RGBA16F in -> RGBA16F out, pinned (outputs stored by the kernel)
  L4      layers: 4 RGBA8 guides per frame, RGBA8 in and out, pinned
each with overlap = 1 and overlap = 0.  Beside every figure: the each-way link rate measured in the same run the way bench.py's
pcie_ceiling does it (pinned copies up and down concurrently on two streams, at the variant's own input / output sizes), the
resident kernel time per frame (mid_bilateral / mid_bilateral_layers on device buffers, event-timed), and the ceiling
max(upload bytes / link, kernel time, output bytes / link) per frame.  Frames per variant repeat over 8 distinct 1080p frames.
The last call's mid_pipe_last_timeline is summarised per variant (median upload, kernel and download span per frame)."""
import argparse
import ctypes
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import image_denoising_filter_amd as mid  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--frames", default="16,64")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


W, H, R, L = 1920, 1080, 8, 4
NPIX = W * H
ctx = mid.Context(0)
say(f"device {ctx.name}; 1080p, r = {R}, texture layout, sigmas 2.0 / 0.2")
rng = np.random.default_rng(7)
base_f32 = [np.concatenate([rng.random((H, W, 3), dtype=np.float32), np.ones((H, W, 1), np.float32)], 2) for _ in range(8)]
SRC = {"f32": base_f32, "u8": [(f * 255).astype(np.uint8) for f in base_f32], "f16": [f.astype(np.float16) for f in base_f32]}
LAYERS = [[rng.integers(0, 256, (H, W, 4), dtype=np.uint8) for _ in range(L)] for _ in range(8)]
VARIANTS = {"u8": ("u8", np.uint8, False), "f32": ("f32", np.float32, False), "f16": ("f16", np.float16, False),
            "L4": ("u8", np.uint8, True)}

pins = {k: mid.PinnedFrames(ctx, v) for k, v in SRC.items()}
pin_layers = mid.PinnedFrames(ctx, [l for ls in LAYERS for l in ls])


def link(nbytes_up, nbytes_down, n=16):
    """bench.py's pcie_ceiling: n pinned copies up and n down, concurrently on two streams, median of 3 -> GB/s each way."""
    up, down = mid.PinnedFrames(ctx, n, nbytes_up), mid.PinnedFrames(ctx, n, nbytes_down)
    d_up, d_down = ctx.alloc(nbytes_up), ctx.alloc(nbytes_down)
    s_up, s_down = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        def go():
            for i in range(n):
                assert mid.lib.mid_memcpy_h2d(ctx.handle, d_up.ptr, up.ptrs[i], nbytes_up, s_up.cuda_stream) == 0
                assert mid.lib.mid_memcpy_d2h(ctx.handle, down.ptrs[i], d_down.ptr, nbytes_down, s_down.cuda_stream) == 0
            ctx.sync(s_up.cuda_stream)
            ctx.sync(s_down.cuda_stream)
        go()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            go()
            ts.append(time.perf_counter() - t0)
        t = sorted(ts)[1]
        return n * nbytes_up / t / 1e9, n * nbytes_down / t / 1e9
    finally:
        up.free(); down.free(); d_up.free(); d_down.free()


def kernel_ms(src, layered, reps=20):
    """Resident kernel time per frame: mid_bilateral / mid_bilateral_layers on device buffers (RGBA32F output, as the public call)."""
    fr = SRC[src][0]
    d_in, d_out = ctx.upload(fr), ctx.alloc(NPIX * 16)
    d_l = [ctx.upload(l) for l in LAYERS[0]] if layered else []
    tbl = (ctypes.c_void_p * max(len(d_l), 1))(*[d.ptr for d in d_l])
    p = mid.BilateralParams(W, H, 2.0, 0.2, R, mid.LAYOUT_TEXTURE, {"u8": 1, "f32": 0, "f16": 2}[src])
    s = torch.cuda.Stream()

    def one():
        if layered:
            rc = mid.lib.mid_bilateral_layers(ctx.handle, ctypes.byref(p), d_in.ptr, tbl, len(d_l), d_out.ptr, s.cuda_stream)
        else:
            rc = mid.lib.mid_bilateral(ctx.handle, ctypes.byref(p), d_in.ptr, d_out.ptr, s.cuda_stream)
        assert rc == 0
    for _ in range(3):
        one()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        one()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def run(name, n, overlap):
    src, out_dt, layered = VARIANTS[name]
    hin = [pins[src].ptrs[i % 8] for i in range(n)]
    hl = [pin_layers.ptrs[(i % 8) * L + l] for i in range(n) for l in range(L)] if layered else None
    out_bytes = NPIX * 4 * np.dtype(out_dt).itemsize
    hout = mid.PinnedFrames(ctx, n, out_bytes)
    try:
        fmt = {"u8": 1, "f32": 0, "f16": 2}[src]
        kw = dict(hlayers=hl, n_layers=L if layered else 0, overlap=overlap, out_dtype=out_dt)
        ctx.sequence_bilateral_pinned(hin, hout.ptrs, W, H, fmt, R, **kw)          # warm: caches sized
        t0 = time.perf_counter()
        ctx.sequence_bilateral_pinned(hin, hout.ptrs, W, H, fmt, R, **kw)
        wall = time.perf_counter() - t0
        up, outs = ctx.pipe_last_timeline()
        tl = (statistics.median(e - s for _, s, e in up), statistics.median(ke - ks for _, ks, ke, _, _ in outs),
              statistics.median(de - ds for _, _, _, ds, de in outs), outs[-1][4] if outs else 0.0)
        return n * NPIX / wall / 1e6, wall * 1e3, tl
    finally:
        hout.free()


frames = [int(x) for x in args.frames.split(",")]
res = {}
for rnd in range(args.rounds):
    for n in frames:
        for name in VARIANTS:
            for overlap in (1, 0):
                res.setdefault((name, n, overlap), []).append(run(name, n, overlap))

say("")
say("variant  frames overlap | Mpixel/s median (min..max of rounds) | link up/down GB/s | kernel ms/frame | ceiling ms/frame "
    "(up, kernel, down) -> Mpixel/s | fraction | timeline medians per frame: upload / kernel / download ms, last output end ms")
kcache, lcache = {}, {}
for name, (src, out_dt, layered) in VARIANTS.items():
    in_bytes = NPIX * {"u8": 4, "f32": 16, "f16": 8}[src] + (NPIX * 4 * L if layered else 0)
    out_bytes = NPIX * 4 * np.dtype(out_dt).itemsize
    kcache[name] = kernel_ms(src, layered)
    lcache[name] = link(in_bytes, out_bytes)
    for n in frames:
        for overlap in (1, 0):
            r = res[(name, n, overlap)]
            mps = [x[0] for x in r]
            med = statistics.median(mps)
            lu, ld = lcache[name]
            c_up, c_k, c_dn = in_bytes / lu / 1e6, kcache[name], out_bytes / ld / 1e6
            ceil_ms = max(c_up, c_k, c_dn)
            ceil_mps = NPIX / ceil_ms / 1e3
            tl = r[-1][2]
            say(f"{name:5s} {n:4d} {overlap:2d} | {med:8.0f} ({min(mps):.0f}..{max(mps):.0f}) | {lu:5.1f} / {ld:5.1f} | {c_k:.4f} | "
                f"{c_up:.4f} {c_k:.4f} {c_dn:.4f} -> {ceil_mps:.0f} | {med / ceil_mps:.2f} | "
                f"{tl[0]:.4f} / {tl[1]:.4f} / {tl[2]:.4f}, {tl[3]:.2f}")
for p in list(pins.values()) + [pin_layers]:
    p.free()
ctx.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
