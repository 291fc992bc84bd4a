"""The opaque-tile vote of every tuned kernel, held against the float64 checkers with ONE odd texel in an otherwise opaque interior tile.

Every tuned kernel chooses its loop form per workgroup from the alpha of the colour tile it has just staged (csrc/bilateral.hip,
bilateral_temporal.hip, nlm_strip.hpp, nlm_layers.hip, nlm_layers_temporal.hip).  A vote that wrongly says "opaque" changes alpha
alone -- the bilateral kernels then write exactly 1.0 for every output of that tile -- so the frames here are opaque but for one texel,
placed by the tile geometry of tests/opaque_vote_cases.py at the slots a faulty fill or vote would miss (slot 0, the last slot of the
last partial fill trip, the first slot of that trip, the other two halo corners, the middle, a junction of four tiles, the linear
layout's row wrap), and flat enough that the far halo tap still moves the reference's alpha by more than 5 x the tolerance: check_alpha
asserts that on the reference before it compares (tests/test_opaque_vote_cases.py works the same figures out on the CPU).  Over
neighbouring frames the odd texel sits in exactly one frame of the window -- the first neighbour, the last, the target or a middle one --
which is what shows a flag carried over from the previous neighbour.

The references are f64_checker.bilateral_sums / nlm_sums, np_bilateral_temporal, np_nlm_layers and np_nlm_layers_temporal.  Their
weights do not depend on alpha and rgb is the same in every case of a frame, so a frame's rgb sums are worked out once and up to four
cases' alpha sums come from one further call (an image whose channels are the four cases' alpha planes).  Tolerances are the
project's: 1e-5 bilateral, 2e-5 NLM, on all four channels (conftest.rel_err), and check_alpha on top.

Out of scope: the kernels without a vote -- the run-time-radius and generic bilateral, the run-time NLM windows, the per-pixel kernels.
"""
import functools

import numpy as np
import pytest
import torch

import f64_checker
import image_denoising_filter_amd as mid
import np_bilateral_temporal as nbt
import np_nlm_layers
import np_nlm_layers_temporal as nlt
import opaque_vote_cases as ov
from conftest import rel_err
from opaque_vote_cases import BIL_TOL, NLM_TOL

pytestmark = pytest.mark.gpu

U8, F16, F32 = np.dtype(np.uint8), np.dtype(np.float16), np.dtype(np.float32)
Z = lambda h, w: np.zeros((h, w, 8), np.float32)  # noqa: E731


def odd_value(dtype):
    """The odd texel's alpha as the kernels decode it."""
    return float(ov.decode(np.array([ov.ODD_ALPHA[np.dtype(dtype)]], dtype))[0])


def packed(h, w, group, value):
    """An image whose channel c is the alpha plane of case c of `group` (opaque where there is no case)."""
    A = np.ones((h, w, 4), np.float32)
    for c, p in enumerate(group):
        A[p.xy[1], p.xy[0], c] = value
    return A


def groups(ps):
    return [ps[i:i + 4] for i in range(0, len(ps), 4)]


def with_alpha(rgb_num, alpha_num):
    return np.concatenate([rgb_num[..., :3], alpha_num[..., None]], -1)


def w0(rng, h, w):
    """A random, non-zero WeightInfo buffer whose alpha sum equals its norm weight: an opaque tile's two sums then stay the same bits."""
    W = rng.random((h, w, 8), dtype=np.float32) + np.float32(0.25)
    W[..., 4] = W[..., 3]
    return W


def normalized(W):
    """[h, w, 4] float64: weightColor / normWeight."""
    W = np.asarray(W, np.float64)
    return W[..., :4] / W[..., 4:5]


def compare(label, got, ref, texels, tile, tol, worst, linear=False, exact_outside=True):
    """All four channels, then check_alpha; the case's worst errors go into `worst`."""
    e = rel_err(got, ref)
    assert e < tol, f"{label}: rel_err {e:.3g}"
    ea, dev = ov.check_alpha(got, ref, texels, tile.reach, tol, linear, exact_outside)
    worst.append((e, ea, dev))


def report(name, worst):
    print(f"{name}: {len(worst)} cases, worst rel_err {max(x[0] for x in worst):.3g}, worst alpha error in a window {max(x[1] for x in worst):.3g}, "
          f"smallest window deviation of the reference {min(x[2] for x in worst):.3g}")


# ---- single-frame bilateral -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def bil_single_ref(R, linear, guide, dtype):
    """(frame, guides, {position name: (Position, num [h,w,4], den [h,w])}) float64 NumPy.  guide: 'self' (plain), 1 or 2 layers."""
    t = ov.bil_tile(R)
    h, w = ov.frame_size(t)
    frames, layers = ov.base_frames(t, dtype)
    frame = frames[0]
    guides = [frame] if guide == "self" else layers[0][:guide]
    args = (R, ov.sigma_s(R), ov.SIGMA_C, linear)

    def sums(img):
        num = den = 0
        for g in guides:
            n_, d_ = f64_checker.bilateral_sums(img, ov.decode(g), *args)
            num, den = num + n_.cpu().numpy(), den + d_.cpu().numpy()
        return num, den
    rgb, den = sums(ov.decode(frame))
    out = {}
    for group in groups(ov.bil_positions(R, linear)):
        al, _ = sums(packed(h, w, group, odd_value(dtype)))
        for c, p in enumerate(group):
            out[p.name] = (p, with_alpha(rgb, al[..., c]), den)
    return frame, guides, out


@pytest.mark.parametrize("variant", ["texture", "linear", "accum", "fused", "batch"])
@pytest.mark.parametrize("R", list(ov.BIL_SHAPES))
def test_single_frame_bilateral(ctx, R, variant):
    """bilateral_kernel MODE 0 (texture, linear, batch: __syncthreads_and), MODE 1 (accumulate) and MODE 2 (fused, L = 2: the vote goes through
    the guide tile's first word, which commit() overwrites afterwards), at every odd-texel position, for an RGBA8 and an RGBA16F input.
    batch: four frames, only frame 2 carries the texel (RGBA8: texture layout, RGBA16F: linear); the others keep alpha == 1.0 inside."""
    t = ov.bil_tile(R)
    h, w = ov.frame_size(t)
    ss, sc = ov.sigma_s(R), ov.SIGMA_C
    rng = np.random.default_rng(R)
    worst = []
    for dtype in (U8, F16):
        linear = variant == "linear" or (variant == "batch" and dtype == F16)
        layout = "linear" if linear else "texture"
        frame, guides, cases = bil_single_ref(R, linear, {"accum": 1, "fused": 2}.get(variant, "self"), dtype)
        for name, (p, num, den) in cases.items():
            odd = ov.with_odd(frame, p.xy)
            label = f"r={R} {variant} {dtype} {name}"
            ref = num / den[..., None]
            if variant == "accum":
                W0 = w0(rng, h, w)
                W = ctx.bilateral_layers_accum(odd, guides[0], W0, R, ss, sc)
                W64 = W0.astype(np.float64)
                assert rel_err(W[..., :3], W64[..., :3] + num[..., :3]) < BIL_TOL, label
                assert rel_err(W[..., 3], W64[..., 3] + num[..., 3]) < BIL_TOL, label + ": alpha sum"
                assert rel_err(W[..., 4], W64[..., 4] + den) < BIL_TOL, label + ": norm weight"
                assert np.array_equal(W[..., 5:], W0[..., 5:])
                got, ref = normalized(W), (W64[..., :4] + num) / (W64[..., 4] + den)[..., None]
            elif variant == "fused":
                got = ctx.bilateral_layers(odd, guides, R, ss, sc)
            elif variant == "batch":
                batch = ctx.bilateral_batch([frame, frame, odd, frame], R, ss, sc, layout)
                got = batch[2]
                inside = ov.interior_mask(h, w, t.reach, linear)
                for i in (0, 1, 3):
                    assert np.all(batch[i][..., 3][inside] == 1.0), f"{label}: frame {i} has no odd texel"
                    assert np.array_equal(batch[i], batch[0])
            else:
                got = ctx.bilateral(odd, R, ss, sc, layout)
            compare(label, got, ref, [p.xy], t, BIL_TOL, worst, linear)
    report(f"bilateral r={R} {variant}", worst)


# ---- bilateral over neighbouring frames -------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def bil_temporal_ref(R, layered, dtype, seqs):
    """(frames, layers, {sequence index: (positions, [per output t: {position name: ref [h,w,4]}])})."""
    t = ov.bil_tile(R)
    h, w = ov.frame_size(t)
    frames, layers = ov.base_frames(t, dtype)
    guides = layers if layered else [[f] for f in frames]
    dec = [ov.decode(f) for f in frames]
    out = {}
    for i in seqs:
        n, k, f_odd = ov.SEQUENCES[i]
        group = ov.seq_positions(t, i)
        base = nbt.bilateral_temporal(dec[:n], k, R, ov.sigma_s(R), ov.SIGMA_C, layers=guides[:n])
        alpha = nbt.bilateral_temporal([packed(h, w, group if f == f_odd else [], odd_value(dtype)) for f in range(n)], k, R, ov.sigma_s(R),
                                       ov.SIGMA_C, layers=guides[:n])
        out[i] = (group, [{p.name: with_alpha(base[t_], alpha[t_][..., c]) for c, p in enumerate(group)} for t_ in range(n)])
    return frames, layers, out


def run_sequence(label, seq, group, refs, tile, tol, worst, run, exact_outside=True):
    """One sequence (n, k, f_odd): for each position, run(frames' odd position) -> n outputs, each against its reference."""
    n, k, f_odd = seq
    for p in group:
        outs = run(p)
        for t_out in range(n):
            place, ref = ov.placement(n, k, f_odd, t_out), refs[t_out][p.name]
            lab = f"{label} {seq} {p.name} output {t_out} ({place})"
            if place == "unseen":
                assert rel_err(outs[t_out], ref) < tol, lab
                if exact_outside:
                    assert np.all(outs[t_out][..., 3][ov.interior_mask(*ref.shape[:2], tile.reach)] == 1.0), lab
            else:
                compare(lab, outs[t_out], ref, [p.xy], tile, tol, worst, exact_outside=exact_outside)


@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("R", list(ov.BIL_SHAPES))
def test_bilateral_over_neighbouring_frames_fused(ctx, R, layered):
    """bilateral_pair_kernel, fused (mid_bilateral_temporal), plain and with two layers: the vote is taken again for every neighbour frame.
    RGBA32F sequences (3,1,1), (5,1,2), (5,2,2), (3,2,0), (3,2,2) of opaque_vote_cases.SEQUENCES -- three and five frames, k = 1 and 2, the
    odd frame the first, the last, a middle neighbour or the target, windows clipped at both ends -- and (3,1,1) as RGBA8 as well."""
    t = ov.bil_tile(R)
    worst = []
    for dtype, seqs in ((F32, tuple(range(len(ov.SEQUENCES)))), (U8, (0,))):
        frames, layers, refs = bil_temporal_ref(R, layered, dtype, seqs)
        for i in seqs:
            n, k, f_odd = ov.SEQUENCES[i]
            group, ref = refs[i]

            def run(p):
                seq = [ov.with_odd(f, p.xy) if j == f_odd else f for j, f in enumerate(frames[:n])]
                return ctx.bilateral_temporal(seq, k, radius=R, sigma_s=ov.sigma_s(R), sigma_c=ov.SIGMA_C, layers=layers[:n] if layered else None)
            run_sequence(f"r={R} {'layers' if layered else 'plain'} {dtype}", ov.SEQUENCES[i], group, ref, t, BIL_TOL, worst, run)
    report(f"bilateral over neighbouring frames r={R} {'2 layers' if layered else 'plain'} fused", worst)


@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("R", list(ov.BIL_SHAPES))
def test_bilateral_over_neighbouring_frames_accumulate(ctx, R, layered):
    """The accumulate forms, mid_bilateral_pair_accum / mid_bilateral_layers_pair_accum, chained per output as the fused call chains them:
    sequences (3,1,1) and (3,2,2), RGBA32F, slot 0 and slot n-1 and one more position."""
    t = ov.bil_tile(R)
    h, w = ov.frame_size(t)
    ss, sc = ov.sigma_s(R), ov.SIGMA_C
    worst = []
    seqs = (0, 4)
    frames, layers, refs = bil_temporal_ref(R, layered, F32, tuple(range(len(ov.SEQUENCES))))
    for i in seqs:
        n, k, f_odd = ov.SEQUENCES[i]
        group, ref = refs[i]

        def run(p):
            seq = [ov.with_odd(f, p.xy) if j == f_odd else f for j, f in enumerate(frames[:n])]
            outs = []
            for t_out in range(n):
                W = Z(h, w)
                for f in nbt.window(n, t_out, k):
                    if layered:
                        for l in range(2):
                            W = ctx.bilateral_layers_pair_accum(layers[t_out][l], layers[f][l], seq[f], W, R, ss, sc)
                    else:
                        W = ctx.bilateral_pair_accum(seq[t_out], seq[f], W, R, ss, sc)
                outs.append(normalized(W))
            return outs
        run_sequence(f"r={R} {'layers' if layered else 'plain'} accumulate", ov.SEQUENCES[i], group, ref, t, BIL_TOL, worst, run)
    report(f"bilateral over neighbouring frames r={R} {'2 layers' if layered else 'plain'} accumulate", worst)


# ---- layer-guided NLM -------------------------------------------------------------------------------------------------------------------
LAYER_DTYPE = {"ref": U8, "bench": F32}      # the input format of each window's cases


@functools.lru_cache(None)
def nlm_layers_single_ref(window, n_layers):
    t = ov.nlm_layers_tile(window)
    h, w = ov.frame_size(t)
    search, patch = ov.NLM_WINDOWS[window]
    dtype = LAYER_DTYPE[window]
    frames, layers = ov.base_frames(t, dtype)
    frame, guides = frames[0], layers[0][:n_layers]
    rgb, den = np_nlm_layers.nlm_layers_sums(ov.decode(frame), guides, ov.HPARAM, search, patch)
    out = {}
    for group in groups(ov.positions(t)):
        al, _ = np_nlm_layers.nlm_layers_sums(packed(h, w, group, odd_value(dtype)), guides, ov.HPARAM, search, patch)
        for c, p in enumerate(group):
            out[p.name] = (p, with_alpha(rgb, al[..., c]), den)
    return frame, guides, out


@pytest.mark.parametrize("form", ["fused", "accum"])
@pytest.mark.parametrize("window", list(ov.NLM_WINDOWS))
def test_layer_guided_nlm(ctx, window, form):
    """nlm_layers_strip_kernel, fused (two layers) and accumulate (one layer into a random W), every position; the 'ref' window on an RGBA8
    input, 'bench' on RGBA32F.  (NLM's norm carries nonlocal.comp's 0.001, so an opaque pixel's alpha is sum / (0.001 + sum), not 1.0: the
    pixels outside the odd texel's window are held by the four-channel comparison, not by an exact 1.0.)"""
    t = ov.nlm_layers_tile(window)
    h, w = ov.frame_size(t)
    search, patch = ov.NLM_WINDOWS[window]
    frame, guides, cases = nlm_layers_single_ref(window, 2 if form == "fused" else 1)
    rng = np.random.default_rng(7)
    worst = []
    for name, (p, num, den) in cases.items():
        odd = ov.with_odd(frame, p.xy)
        label = f"nlm layers {window} {form} {name}"
        if form == "fused":
            got, ref = ctx.nlm_layers(odd, guides, ov.HPARAM, search, patch), num / den[..., None]
        else:
            W0 = w0(rng, h, w)
            W = ctx.nlm_layers_accum(odd, guides[0], W0, ov.HPARAM, search, patch)
            W64 = W0.astype(np.float64)
            assert rel_err(W[..., :4], W64[..., :4] + num) < NLM_TOL and rel_err(W[..., 4], W64[..., 4] + den) < NLM_TOL, label
            assert np.array_equal(W[..., 5:], W0[..., 5:])
            got, ref = normalized(W), (W64[..., :4] + num) / (W64[..., 4] + den)[..., None]
        compare(label, got, ref, [p.xy], t, NLM_TOL, worst, exact_outside=False)
    report(f"layer-guided nlm {window} {form}", worst)


@functools.lru_cache(None)
def nlm_layers_temporal_ref(window):
    """The (t, f, l) dispatch sums of the base frames once (np_nlm_layers_temporal's own cache), the odd frame's dispatches again with the
    alpha planes of the sequence's positions."""
    t = ov.nlm_layers_tile(window)
    h, w = ov.frame_size(t)
    search, patch = ov.NLM_WINDOWS[window]
    dtype = LAYER_DTYPE[window]
    frames, layers = ov.base_frames(t, dtype)
    cache, out = {}, {}
    for i, (n, k, f_odd) in enumerate(ov.NLM_SEQUENCES[window]):
        group = ov.seq_positions(t, i)
        base = nlt.nlm_layers_temporal(frames[:n], layers[:n], k, ov.HPARAM, search, patch, cache=cache)
        # the dispatches the odd frame has no part in: every channel of the alpha image is the base frame's (opaque) alpha
        sub = {key: (val[0][..., 3:4], val[1]) for key, val in cache.items() if key[1] != f_odd}
        alpha = nlt.nlm_layers_temporal([packed(h, w, group if f == f_odd else [], odd_value(dtype)) for f in range(n)], layers[:n], k,
                                        ov.HPARAM, search, patch, cache=sub)
        out[i] = (group, [{p.name: with_alpha(base[t_], alpha[t_][..., c]) for c, p in enumerate(group)} for t_ in range(n)])
    return frames, layers, out


@pytest.mark.parametrize("form", ["fused", "accum"])
@pytest.mark.parametrize("window", list(ov.NLM_WINDOWS))
def test_layer_guided_nlm_over_neighbouring_frames(ctx, window, form):
    """nlm_layers_pair_strip_kernel, two layers, fused (mid_nlm_layers_temporal) and as the chain of mid_nlm_layers_pair_accum dispatches:
    the sequences of opaque_vote_cases.NLM_SEQUENCES -- 'ref' (RGBA8): (3,1,1) and (5,2,2); 'bench' (RGBA32F): (3,1,1) and (3,2,1)."""
    t = ov.nlm_layers_tile(window)
    h, w = ov.frame_size(t)
    search, patch = ov.NLM_WINDOWS[window]
    frames, layers, refs = nlm_layers_temporal_ref(window)
    worst = []
    for i, (n, k, f_odd) in enumerate(ov.NLM_SEQUENCES[window]):
        group, ref = refs[i]

        def run(p):
            seq = [ov.with_odd(f, p.xy) if j == f_odd else f for j, f in enumerate(frames[:n])]
            if form == "fused":
                return ctx.nlm_layers_temporal(seq, layers[:n], k, hparam=ov.HPARAM, search=search, patch=patch)
            outs = []
            for t_out in range(n):
                W = Z(h, w)
                for f in nbt.window(n, t_out, k):
                    for l in range(2):
                        W = ctx.nlm_layers_pair_accum(layers[t_out][l], layers[f][l], seq[f], W, ov.HPARAM, search, patch)
                outs.append(normalized(W))
            return outs
        run_sequence(f"nlm layers {window} {form}", (n, k, f_odd), group if form == "fused" else group[:2], ref, t, NLM_TOL, worst, run, exact_outside=False)
    report(f"layer-guided nlm over neighbouring frames {window} {form}", worst)


# ---- plain NLM strip kernels ------------------------------------------------------------------------------------------------------------
def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(None)
def nlm_single_ref(window, size=None):
    """(frame, {xy: (Position, num [h,w,4], den [h,w])}): f64_checker.nlm_sums of the frame against itself, per position."""
    t = ov.nlm_strip_tile(window)
    search, patch = ov.NLM_WINDOWS[window]
    frame = ov.base_frames(t, F32, size=size)[0][0]
    out = {}
    for p in ov.strip_positions(window):
        odd = ov.with_odd(frame, p.xy)
        num, den = f64_checker.nlm_sums(odd, [odd], ov.HPARAM, search, patch)
        out[p.xy] = (p, num.cpu().numpy(), den.cpu().numpy())
    return frame, out


def run_many(ctx, base, odd, n, i_odd, window):
    """n frames in one k = 0 launch, frame i_odd the odd one; the opaque siblings share one device buffer (inputs may alias)."""
    h, w = base.shape[:2]
    search, patch = ov.NLM_WINDOWS[window]
    d_base, d_odd = ctx.upload(base), ctx.upload(odd)
    d_out = [ctx.alloc(h * w * 16) for _ in range(n)]
    ctx.nlm_temporal_dev([d_odd.ptr if i == i_odd else d_base.ptr for i in range(n)], [d.ptr for d in d_out], w, h, ov.HPARAM, search, patch,
                         0, 0, n, mid.FMT_RGBA32F)
    ctx.sync()
    return [ctx.download(d, (h, w, 4), np.float32) for d in d_out]


@pytest.mark.parametrize("window", list(ov.NLM_WINDOWS))
def test_plain_nlm_one_small_frame_is_all_half_shape(ctx, window):
    """Shape (a): one small frame at k = 0 is tiles_x * tiles_y = 9 workgroups <= CU count, so tail_split sends all of them to the HALF shape
    (eight waves on the 32-row tile, 512 threads filling it): every position of the HALF tile and of the whole-strip tile.
    Shape (e): mid_nlm_accum of the same frame against itself into a random W -- the accumulate-only HALF kernel."""
    t = ov.nlm_strip_tile(window, "half")
    h, w = ov.frame_size(t)
    search, patch = ov.NLM_WINDOWS[window]
    assert ov.nlm_launch_shape(w, h, patch[1] - patch[0], 1, cu_count()) == dict(copy="small", whole=0, half=9)
    frame, cases = nlm_single_ref(window)
    rng = np.random.default_rng(8)
    worst, worst_e = [], []
    for xy, (p, num, den) in cases.items():
        odd = ov.with_odd(frame, xy)
        compare(f"nlm {window} k=0 {p.name}", ctx.nlm_temporal([odd], k=0, hparam=ov.HPARAM, search=search, patch=patch)[0], num / den[..., None],
                [xy], t, NLM_TOL, worst, exact_outside=False)
        W0 = w0(rng, h, w)
        W = ctx.nlm_accum(odd, odd, W0, ov.HPARAM, search, patch)
        W64 = W0.astype(np.float64)
        assert rel_err(W[..., :4], W64[..., :4] + num) < NLM_TOL and rel_err(W[..., 4], W64[..., 4] + den) < NLM_TOL, (window, p.name)
        compare(f"nlm_accum {window} {p.name}", normalized(W), (W64[..., :4] + num) / (W64[..., 4] + den)[..., None], [xy], t, NLM_TOL, worst_e,
                exact_outside=False)
    report(f"plain nlm {window}, one frame (all HALF)", worst)
    report(f"plain nlm {window}, nlm_accum (HALF)", worst_e)


@pytest.mark.parametrize("window", list(ov.NLM_WINDOWS))
def test_plain_nlm_whole_strips_of_the_small_copy(ctx, window):
    """Shape (b): enough copies of the small frame in one k = 0 launch that nwg >= slots = 2 x CUs (57 frames of 9 workgroups at 256 CUs):
    the first `slots` workgroups run as whole strips of nlm_small.hip's copy, the remainder as a HALF tail.  The odd frame is frame 3, in
    the whole strips; it is compared with the checker, its opaque siblings -- whole strips and HALF tail alike -- are the same bits."""
    t = ov.nlm_strip_tile(window)
    h, w = ov.frame_size(t)
    patch_w = ov.NLM_WINDOWS[window][1][1] - ov.NLM_WINDOWS[window][1][0]
    cu = cu_count()
    n = next(n for n in range(1, 97) if (s := ov.nlm_launch_shape(w, h, patch_w, n, cu))["whole"] >= 2 * cu and s["half"] > 0)
    shape = ov.nlm_launch_shape(w, h, patch_w, n, cu)
    assert shape["copy"] == "small" and ov.nlm_tile_workgroups(w, h, patch_w, 4) <= shape["whole"], shape
    frame, cases = nlm_single_ref(window)
    worst = []
    for xy, (p, num, den) in cases.items():
        outs = run_many(ctx, frame, ov.with_odd(frame, xy), n, 3, window)
        compare(f"nlm {window} {n} frames {p.name}", outs[3], num / den[..., None], [xy], t, NLM_TOL, worst, exact_outside=False)
        assert all(np.array_equal(o, outs[0]) for i, o in enumerate(outs) if i != 3), "the opaque siblings differ"
    report(f"plain nlm {window}, {n} frames (whole strips of the small copy + HALF tail)", worst)


@pytest.mark.parametrize("window", list(ov.NLM_WINDOWS))
def test_plain_nlm_long_copy(ctx, window):
    """Shape (c): one k = 0 launch of at most 96 frames with nwg > 7 x slots runs nlm.hip's copy of the kernel: 13 tile columns x 3 tile rows
    = 39 workgroups per frame, 92 frames at 256 CUs.  Slot 0, slot n-1 and the first slot of the last fill trip; the odd frame against the
    checker, its opaque siblings the same bits."""
    t = ov.nlm_strip_tile(window)
    h = ov.frame_size(t)[0]
    w = 13 * t.out_w
    patch_w = ov.NLM_WINDOWS[window][1][1] - ov.NLM_WINDOWS[window][1][0]
    cu = cu_count()
    n = ov.NLM_SMALL_ROUNDS * 2 * cu // ov.nlm_tile_workgroups(w, h, patch_w, 1) + 1
    assert n <= 96 and ov.nlm_launch_shape(w, h, patch_w, n, cu)["copy"] == "long"
    frame, cases = nlm_single_ref(window, (h, w))
    worst = []
    for p in ov.positions(t)[:3]:
        _, num, den = cases[p.xy]
        outs = run_many(ctx, frame, ov.with_odd(frame, p.xy), n, n // 2, window)
        compare(f"nlm {window} long copy {p.name}", outs[n // 2], num / den[..., None], [p.xy], t, NLM_TOL, worst, exact_outside=False)
        assert all(np.array_equal(o, outs[0]) for i, o in enumerate(outs) if i != n // 2), "the opaque siblings differ"
    report(f"plain nlm {window}, {n} frames of {h}x{w} (long copy)", worst)


@functools.lru_cache(None)
def nlm_temporal_ref(window):
    """Per (target, neighbour) pair of the base frames one f64_checker.nlm_sums; per position the pairs with the odd neighbour again."""
    t = ov.nlm_strip_tile(window)
    search, patch = ov.NLM_WINDOWS[window]
    frames, _ = ov.base_frames(t, F32)

    def pair(t_, nb):
        num, den = f64_checker.nlm_sums(frames[t_], [nb], ov.HPARAM, search, patch)
        return num.cpu().numpy(), den.cpu().numpy()
    base = functools.lru_cache(None)(lambda t_, f: pair(t_, frames[f]))
    out = {}
    for i, (n, k, f_odd) in enumerate(ov.NLM_SEQUENCES[window]):
        group = ov.seq_positions(t, i)
        refs = [{} for _ in range(n)]
        for p in group:
            odd = ov.with_odd(frames[f_odd], p.xy)
            for t_out in range(n):
                parts = [pair(t_out, odd) if f == f_odd else base(t_out, f) for f in nbt.window(n, t_out, k)]
                refs[t_out][p.name] = sum(x[0] for x in parts) / sum(x[1] for x in parts)[..., None]
        out[i] = (group, refs)
    return frames, out


@pytest.mark.parametrize("window", list(ov.NLM_WINDOWS))
def test_plain_nlm_over_neighbouring_frames(ctx, window):
    """Shape (d): k > 0 runs the MULTI kernels of nlm.hip, which vote again for every neighbour frame: the sequences of
    opaque_vote_cases.NLM_SEQUENCES -- 'ref': (3,1,1) and (5,2,2); 'bench': (3,1,1) and (3,2,1)."""
    t = ov.nlm_strip_tile(window)
    search, patch = ov.NLM_WINDOWS[window]
    frames, refs = nlm_temporal_ref(window)
    worst = []
    for i, (n, k, f_odd) in enumerate(ov.NLM_SEQUENCES[window]):
        group, ref = refs[i]

        def run(p):
            seq = [ov.with_odd(f, p.xy) if j == f_odd else f for j, f in enumerate(frames[:n])]
            return ctx.nlm_temporal(seq, k=k, hparam=ov.HPARAM, search=search, patch=patch)
        run_sequence(f"nlm {window}", (n, k, f_odd), group, ref, t, NLM_TOL, worst, run, exact_outside=False)
    report(f"plain nlm over neighbouring frames {window}", worst)
