"""GPU suite: RGBA16F (half-float) frames end to end.

Contract (include/mi_denoise.h, MID_FMT_RGBA16F): a half texel widens to fp32 exactly, so every filter given an RGBA16F frame
returns the BITS of the same call on frame.astype(float32); RGBA16F outputs are numpy.float16 of the fp32 result.  Every
comparison below is on raw bits (view(uint32) / view(uint16))."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import image_denoising_filter_amd as mid
from conftest import ROOT
from test_half_codecs import _float_sweep

pytestmark = pytest.mark.gpu

W_SEARCH = {  # name: (search, patch)
    "21x21/7x7": ((-10, 11), (-3, 4)),
    "ref [-7,7)/[-3,3)": ((-7, 7), (-3, 3)),
    "15x15/5x5": ((-7, 8), (-2, 3)),
    "25x25/7x7": ((-12, 13), (-3, 4)),
    "11x11/12x12 (rt4)": ((-5, 6), (-6, 6)),
}


def half_frame(rng, h, w, translucent=True):
    """HDR-range colours (a few above 1, some tiny enough to be f16 subnormals), alpha 1 except for scattered translucent texels."""
    img = rng.gamma(2.0, 0.4, (h, w, 4))
    img[..., 3] = 1.0
    img.reshape(-1, 4)[::97, :3] *= 2.0 ** -20                   # f16 subnormal colours
    if translucent:
        m = rng.random((h, w)) < 0.01
        img[m, 3] = 0.5
    return img.astype(np.float16)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    view = np.uint16 if a.dtype == np.float16 else np.uint32
    return np.array_equal(a.view(view), b.view(view))


# ---- streaming passes -----------------------------------------------------------------------------------------------
def test_unpack_f16_every_code(ctx):
    codes = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    want = codes.view(np.float16).astype(np.float32)
    nan = np.isnan(want)
    for n in (len(codes), len(codes) - 3):                      # the whole pixels, and a tail of 1..3 values
        got = ctx.unpack_f16(codes[:n].view(np.float16))
        assert np.array_equal(got.view(np.uint32)[~nan[:n]], want[:n].view(np.uint32)[~nan[:n]])
        assert np.all(np.isnan(got[nan[:n]]))


def test_pack_f16_rounds_like_numpy(ctx):
    v = _float_sweep(np.random.default_rng(3), 4000)
    with np.errstate(over="ignore", invalid="ignore"):
        want = v.astype(np.float16)
    for n in (len(v) - len(v) % 4, len(v) - len(v) % 4 - 1):
        got = ctx.pack_f16(v[:n])
        nan = np.isnan(want[:n])
        assert np.array_equal(got.view(np.uint16)[~nan], want[:n].view(np.uint16)[~nan])
        assert np.all(np.isnan(got[nan]))


def test_refusals(ctx):
    h, w = 16, 16
    src = ctx.upload(np.zeros((h, w, 4), np.float16))
    sentinel = np.frombuffer(np.arange(h * w * 16 + 64, dtype=np.uint32).astype(np.uint8).tobytes(), np.uint8).copy()
    dst = ctx.upload(sentinel)                                  # the output buffer: nothing may be written into it
    with pytest.raises(mid.MidError) as e:                      # misaligned RGBA16F pointer
        ctx.bilateral_dev(src.ptr + 4, dst.ptr, w, h, 4, 2.0, 0.2, mid.LAYOUT_TEXTURE, mid.FMT_RGBA16F)
    assert e.value.code == 1
    with pytest.raises(mid.MidError) as e:
        ctx.nlm_temporal_dev([src.ptr + 2], [dst.ptr], w, h, 0.5, (-10, 11), (-3, 4), 0, 0, 1, mid.FMT_RGBA16F)
    assert e.value.code == 1
    for call in (lambda: ctx.bilateral_dev(src.ptr, dst.ptr, w, h, 4, 2.0, 0.2, mid.LAYOUT_TEXTURE, 3),
                 lambda: ctx.nlm_temporal_dev([src.ptr], [dst.ptr], w, h, 0.5, (-10, 11), (-3, 4), 0, 0, 1, 3)):
        with pytest.raises(mid.MidError) as e:                  # format 3 does not exist
            call()
        assert e.value.code == 1
    assert mid.lib.mid_pack_f16(ctx.handle, dst.ptr, 64, dst.ptr, None) == 1          # in place
    assert mid.lib.mid_unpack_f16(ctx.handle, dst.ptr, 64, dst.ptr, None) == 1
    assert mid.lib.mid_pack_f16(ctx.handle, dst.ptr, 64, dst.ptr + 4, None) == 1      # misaligned half buffer
    assert mid.lib.mid_pack_f16(ctx.handle, src.ptr, 0, dst.ptr, None) == 0           # zero length: a no-op
    ctx.sync()
    assert np.array_equal(ctx.download(dst, sentinel.shape, np.uint8), sentinel), "a refused call (or the no-op) wrote its output"


# ---- bilateral ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["texture", "linear"])
@pytest.mark.parametrize("radius", [1, 4, 8, 10, 13, 20, 24])
def test_bilateral_half_equals_widened(ctx, layout, radius):
    f = half_frame(np.random.default_rng(radius), 70, 130)
    assert same_bits(ctx.bilateral(f, radius, 2.0, 0.2, layout), ctx.bilateral(f.astype(np.float32), radius, 2.0, 0.2, layout))


@pytest.mark.parametrize("layout", ["texture", "linear"])
def test_bilateral_half_1080p(ctx, layout):
    f = half_frame(np.random.default_rng(8), 1080, 1920)
    assert same_bits(ctx.bilateral(f, 8, 2.0, 0.2, layout), ctx.bilateral(f.astype(np.float32), 8, 2.0, 0.2, layout))


@pytest.mark.parametrize("radius", [4, 13])
def test_bilateral_batch_and_layers_half(ctx, radius):
    rng = np.random.default_rng(40 + radius)
    fr = [half_frame(rng, 70, 130) for _ in range(3)]
    for lay in ("texture", "linear"):
        got, want = ctx.bilateral_batch(fr, radius, layout=lay), ctx.bilateral_batch([f.astype(np.float32) for f in fr], radius, layout=lay)
        assert all(same_bits(a, b) for a, b in zip(got, want))
    layers = [rng.integers(0, 256, (70, 130, 4), dtype=np.uint8) for _ in range(4)]
    W = rng.random((70, 130, 8), dtype=np.float32)
    assert same_bits(ctx.bilateral_layers_accum(fr[0], layers[0], W, radius), ctx.bilateral_layers_accum(fr[0].astype(np.float32), layers[0], W, radius))
    assert same_bits(ctx.bilateral_layers(fr[1], layers, radius), ctx.bilateral_layers(fr[1].astype(np.float32), layers, radius))


# ---- NLM ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", list(W_SEARCH))
@pytest.mark.parametrize("n,k", [(1, 0), (2, 1), (3, 1), (8, 2)])
def test_nlm_half_equals_widened(ctx, window, n, k):
    search, patch = W_SEARCH[window]
    rng = np.random.default_rng(n * 10 + k)
    fr = [half_frame(rng, 70, 130) for _ in range(n)]
    got = ctx.nlm_temporal(fr, k=k, search=search, patch=patch)
    want = ctx.nlm_temporal([f.astype(np.float32) for f in fr], k=k, search=search, patch=patch)
    assert all(same_bits(a, b) for a, b in zip(got, want))


def test_nlm_half_lopsided_patch_and_accum(ctx):
    rng = np.random.default_rng(77)
    fr = [half_frame(rng, 40, 50) for _ in range(3)]
    f32 = [f.astype(np.float32) for f in fr]
    cfg = dict(search=(-3, 4), patch=(-1, 3))                  # lopsided: the per-pixel kernel
    assert all(same_bits(a, b) for a, b in zip(ctx.nlm_temporal(fr, k=1, **cfg), ctx.nlm_temporal(f32, k=1, **cfg)))
    W = np.zeros((40, 50, 8), np.float32)
    for search, patch in list(W_SEARCH.values())[:2] + [((-3, 4), (-1, 3))]:
        assert same_bits(ctx.nlm_accum(fr[0], fr[1], W, search=search, patch=patch), ctx.nlm_accum(f32[0], f32[1], W, search=search, patch=patch))


@pytest.mark.parametrize("window", ["21x21/7x7", "ref [-7,7)/[-3,3)"])
@pytest.mark.parametrize("n,k", [(1, 0), (8, 2)])
def test_nlm_half_1080p_tuned_windows(ctx, window, n, k):
    search, patch = W_SEARCH[window]
    rng = np.random.default_rng(1080 + n)
    fr = [half_frame(rng, 1080, 1920) for _ in range(n)]
    got = ctx.nlm_temporal(fr, k=k, search=search, patch=patch)
    want = ctx.nlm_temporal([f.astype(np.float32) for f in fr], k=k, search=search, patch=patch)
    assert all(same_bits(a, b) for a, b in zip(got, want))


# ---- frame pipeline -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 2])
@pytest.mark.parametrize("pinned_out", [True, False])
def test_sequence_f16_outputs(ctx, k, pinned_out):
    rng = np.random.default_rng(16 + k)
    fr = [half_frame(rng, 90, 160) for _ in range(16)]
    f32 = [f.astype(np.float32) for f in fr]
    for first, count in ((0, 16), (3, 9)):
        ref, _ = ctx.sequence_nlm(f32, k=k, first=first, count=count, **mid.NLM_BENCH)
        got, _ = ctx.sequence_nlm(fr, k=k, first=first, count=count, out_dtype=np.float16, pinned_out=pinned_out, **mid.NLM_BENCH)
        assert all(same_bits(g, r.astype(np.float16)) for g, r in zip(got, ref))
        # RGBA16F in, RGBA32F out: the widened frames' outputs
        got32, _ = ctx.sequence_nlm(fr, k=k, first=first, count=count, pinned=False, **mid.NLM_BENCH)
        assert all(same_bits(g, r) for g, r in zip(got32, ref))


def test_sequence_f16_outputs_from_f32_and_u8(ctx):
    rng = np.random.default_rng(5)
    f32 = [half_frame(rng, 60, 100).astype(np.float32) for _ in range(5)]
    u8 = [rng.integers(0, 256, (60, 100, 4), dtype=np.uint8) for _ in range(5)]
    for fr in (f32, u8):
        ref, _ = ctx.sequence_nlm(fr, k=1, **mid.NLM_BENCH)
        got, _ = ctx.sequence_nlm(fr, k=1, out_dtype=np.float16, **mid.NLM_BENCH)
        assert all(same_bits(g, r.astype(np.float16)) for g, r in zip(got, ref))


def _direct(ctx):
    """Did the last pipeline call store its outputs directly (no download stage: mid_pipe_last_timeline reports an empty
    download interval at the kernel's end)?"""
    _, outs = ctx.pipe_last_timeline()
    return all(ds == ke and de == ke for _, _, ke, ds, de in outs)


def test_sequence_f16_direct_stores_only_inside_one_allocation(ctx):
    rng = np.random.default_rng(21)
    h, w = 64, 128
    F = h * w * 8                                               # one RGBA16F frame: 64 KiB, page multiple
    fr = [half_frame(rng, h, w) for _ in range(3)]
    ref, _ = ctx.sequence_nlm([f.astype(np.float32) for f in fr], k=1, first=1, count=1, **mid.NLM_BENCH)
    want = ref[0].astype(np.float16)
    hin = [f.ctypes.data for f in fr]
    # outputs from mid_alloc_host: each one lies inside one allocation -> stored by the kernel
    hout = mid.PinnedFrames(ctx, 1, F)
    try:
        ctx.sequence_nlm_pinned(hin, hout.ptrs, w, h, mid.FMT_RGBA16F, k=1, first=1, count=1, out_dtype=np.float16, **mid.NLM_BENCH)
        assert _direct(ctx)
        assert np.array_equal(hout.array(0, (h, w, 4), np.float16).view(np.uint16), want.view(np.uint16))
    finally:
        hout.free()
    # an output whose first and last bytes are page-locked but which spans TWO adjacent registrations: never stored by the kernel.
    # (The staged download of such a range is refused by the runtime -- hipMemcpyAsync: invalid argument, as for every output format
    # -- so the call reports MID_ERR_HIP; the point here is that nothing was written through the mapping and the next call works.)
    raw = np.zeros(3 * F + 4096, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data) % 4096
    assert mid.lib.mid_host_register(ctx.handle, base, F) == 0
    try:
        assert mid.lib.mid_host_register(ctx.handle, base + F, F) == 0
        try:
            out_ptr = base + F // 2
            with pytest.raises(mid.MidError) as e:
                ctx.sequence_nlm_pinned(hin, [out_ptr], w, h, mid.FMT_RGBA16F, k=1, first=1, count=1, out_dtype=np.float16, **mid.NLM_BENCH)
            assert e.value.code == 2 and "DeviceToHost" in str(e.value), str(e.value)
            assert not raw.any(), "the kernel stored into a range that spans two registrations"
        finally:
            assert mid.lib.mid_host_unregister(ctx.handle, base + F) == 0
    finally:
        assert mid.lib.mid_host_unregister(ctx.handle, base) == 0
    got, _ = ctx.sequence_nlm(fr, k=1, first=1, count=1, out_dtype=np.float16, **mid.NLM_BENCH)   # the context works on
    assert np.array_equal(got[0].view(np.uint16), want.view(np.uint16))


def test_multiframe_half(ctx):
    rng = np.random.default_rng(9)
    fr = [half_frame(rng, 60, 100) for _ in range(4)]
    got, _ = ctx.nlm_multiframe(fr[0], fr[1:], **mid.NLM_BENCH)
    want, _ = ctx.nlm_multiframe(fr[0].astype(np.float32), [f.astype(np.float32) for f in fr[1:]], **mid.NLM_BENCH)
    assert same_bits(got, want)


# ---- sharded temporal NLM (stand-in transport, ranks share cuda:0; set-up as tests/test_gpu_sharded_multirank.py) -------
_WORKER = r'''
import json, sys, threading
sys.path.insert(0, sys.argv[1])
import numpy as np
import image_denoising_filter_amd as mid
CFG = dict(search=(-10, 11), patch=(-3, 4))
ref_ctx = mid.Context(0)
rep = []
for world, n, k in ((2, 9, 2), (3, 12, 2), (3, 7, 1)):
    h, w = 70, 130
    rng = np.random.default_rng(world * 100 + n)
    seq = [(rng.gamma(2.0, 0.4, (h, w, 4))).astype(np.float16) for _ in range(n)]
    whole = ref_ctx.nlm_temporal([f.astype(np.float32) for f in seq], k=k, **CFG)
    ctxs = [mid.Context(0) for _ in range(world)]
    comms = mid.comm_create_all(ctxs)
    outs, errs, stats = {}, [], {}
    def rank_main(r, fmt, frames, res):
        try:
            c, comm = ctxs[r], comms[r]
            start, count = mid.shard_block(n, world, r)
            d_in = [c.upload(frames[start + i]) for i in range(count)]
            d_out = [c.alloc(h * w * 16) for _ in range(count)]
            comm.nlm_temporal_sharded_dev([d.ptr for d in d_in], [d.ptr for d in d_out], w, h, n, k, 0.5, CFG["search"], CFG["patch"], fmt)
            c.sync()
            res[r] = ([c.download(d, (h, w, 4), np.float32) for d in d_out], comm.last_exchange()[:2])
        except Exception as e:  # noqa: BLE001
            errs.append(f"rank {r}: {e}")
    per_fmt = {}
    for fmt, frames in ((mid.FMT_RGBA16F, seq), (mid.FMT_RGBA32F, [f.astype(np.float32) for f in seq])):
        res = {}
        th = [threading.Thread(target=rank_main, args=(r, fmt, frames, res), daemon=True) for r in range(world)]
        for t in th: t.start()
        for t in th: t.join(timeout=120)
        assert not any(t.is_alive() for t in th), "a rank hangs"
        assert not errs, errs
        per_fmt[fmt] = res
    for r in range(world):
        start, count = mid.shard_block(n, world, r)
        got, (rv, sd) = per_fmt[mid.FMT_RGBA16F][r]
        _, (rv32, sd32) = per_fmt[mid.FMT_RGBA32F][r]
        for i in range(count):
            assert np.array_equal(got[i].view(np.uint32), whole[start + i].view(np.uint32)), (world, n, k, r, i)
        assert 2 * rv == rv32 and 2 * sd == sd32, (rv, sd, rv32, sd32)
        recv, send = mid.shard_halo_plan(n, world, k, r)
        assert (rv, sd) == (len(recv) * h * w * 8, len(send) * h * w * 8)
    rep.append([world, n, k])
    for cm in comms: cm.close()
    for c in ctxs: c.close()
print("HALFSHARD " + json.dumps(rep), flush=True)
'''


def test_sharded_half_blocks(tmp_path):
    standin = os.path.join(ROOT, "tests", "standin_rccl", "libstandin_rccl.so")
    if not os.path.exists(standin):
        subprocess.run(["make", "-C", os.path.dirname(standin)], check=True, capture_output=True, timeout=600)
    env = dict(os.environ, MID_RCCL_LIBRARY=standin)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rep = json.loads([l for l in r.stdout.splitlines() if l.startswith("HALFSHARD ")][0][10:])
    assert len(rep) == 3
