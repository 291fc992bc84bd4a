"""GPU suite: what the recursive temporal accumulation (include/mi_denoise.h, section a4j) touches beside its buffers, what wild
motion does to it, a strip, and its refusals.

    * Guard bands.  Through the raw C call the three outputs sit in the middle of larger device allocations with a 4096-byte band
      of sentinel bytes on either side; after the call every band and every input has its bytes and the outputs have the bits of
      the plain ctx call.
    * Poisoned surroundings.  Every input plane sits in an allocation whose other bytes are 0xff (NaN as float32 and as float16)
      while the motion points off every edge of the frame: a tap outside the image is SKIPPED, not weighed 0, so nothing of that
      reaches the sums, and the outputs are finite wherever the history met no weight (S == 0).
    * Non-finite and huge motion gives exactly the no-history result for that pixel.  (tests/test_reproject_taps_sanitize.py has
      fed the tap geometry this motion on the CPU, under sanitizers, before any kernel sees it.)
    * A strip of 262 149 x 2 texels with motion +-3, against the float64 checker.
    * Every refusal of the header, with the outputs untouched.
"""
import ctypes

import numpy as np
import pytest

import image_denoising_filter_amd as mid
import temporal_accumulate_inputs as tai
from np_temporal_accumulate import temporal_accumulate as check
from test_gpu_atrous_bounds import FMT, Banded, same
from test_gpu_temporal_accumulate import TOL, case, errors

pytestmark = pytest.mark.gpu


def raw(ctx, fr, ly, pl, sg, hist=None, motion=None, var_spatial=None, alpha=0.2, alpha_moments=0.2, history_max=32, history_full=4,
        fill=None, keep_variance=True):
    h, w = fr.shape[:2]
    L = len(ly)

    def banded(a, seed):
        return None if a is None else Banded(ctx, a.nbytes, a, fill, seed=seed)
    d_in = banded(fr, 1)
    d_l, d_p = [banded(l, 10 + i) for i, l in enumerate(ly)], [banded(l, 30 + i) for i, l in enumerate(pl)]
    d_hc, d_hs = (banded(hist[0], 50), banded(hist[1], 51)) if hist is not None else (None, None)
    d_mv, d_vs = banded(motion, 52), banded(var_spatial, 53)
    d_col, d_st = Banded(ctx, h * w * 16, seed=60), Banded(ctx, h * w * 16, seed=61)
    d_var = Banded(ctx, h * w * 4, seed=62) if keep_variance else None
    p = mid.TemporalAccumParams(w, h, alpha, alpha_moments, history_max, history_full,
                                mid.api.fmt_with_guide(FMT[fr.dtype], FMT[ly[0].dtype] if L else mid.FMT_RGBA8))
    ptr = lambda d: d.ptr if d is not None else None
    rc = mid.lib.mid_temporal_accumulate(ctx.handle, ctypes.byref(p), (ctypes.c_float * 16)(*sg), d_in.ptr,
                                         (ctypes.c_void_p * 17)(*[d.ptr for d in d_l]), (ctypes.c_void_p * 17)(*[d.ptr for d in d_p]), L,
                                         ptr(d_mv), ptr(d_hc), ptr(d_hs), ptr(d_vs), d_col.ptr, d_st.ptr, ptr(d_var), None)
    assert rc == 0, mid.lib.mid_last_error()
    ctx.sync()
    assert d_col.bands_intact() and d_st.bands_intact() and (d_var is None or d_var.bands_intact()), "a store beside an output"
    assert all(d.unchanged() for d in [d_in, d_hc, d_hs, d_mv, d_vs] + d_l + d_p if d is not None), "an input changed"
    return d_col.middle((h, w, 4), np.float32), d_st.middle((h, w, 4), np.float32), d_var.middle((h, w), np.float32) if d_var else None


@pytest.mark.parametrize("L", (0, 1, 5, 16))
@pytest.mark.parametrize("shape", [(5, 63), (9, 65), (21, 130)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_guard_bands(ctx, shape, L):
    for mi, motion in enumerate(tai.MOTIONS):
        fdt, gdt = (np.float32, np.float16, np.uint8)[(mi + L) % 3], (np.uint8, np.float32, np.float16)[(mi + L) % 3]
        args, kw = case(shape, L, fdt, gdt, motion, mi % 2 == 0, mi % 2)
        got = raw(ctx, *args, **kw)
        want = ctx.temporal_accumulate(*args, **kw)
        assert all(same(g, w_) for g, w_ in zip(got, want)), (shape, L, motion)
        col, st, none = raw(ctx, *args, keep_variance=False, **kw)
        assert none is None and same(col, want[0]) and same(st, want[1]), (shape, L, motion, "var_out NULL")


def off_every_edge(shape):
    """Motion that points outwards everywhere: by up to 3 texels, in quarters, so taps straddle and cross all four edges."""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    m = np.stack([np.where(xx < w / 2, -1, 1) * (0.25 + (xx + yy) % 12 / 4), np.where(yy < h / 2, -1, 1) * (0.5 + (2 * xx + yy) % 11 / 4)], -1)
    return m.astype(np.float32)


@pytest.mark.parametrize("L", (0, 3, 5))
def test_nan_around_every_input_with_motion_off_every_edge(ctx, L):
    assert np.isnan(np.full(4, 0xff, np.uint8).view(np.float32)).all() and np.isnan(np.full(2, 0xff, np.uint8).view(np.float16)).all()
    shape = (21, 70)
    for dt in (np.float32, np.float16):
        args, kw = case(shape, L, dt, dt, "none", True, 0)
        kw["motion"] = off_every_edge(shape)
        got = raw(ctx, *args, fill=0xff, **kw)
        ref = check(*args, **kw)
        assert all(np.isfinite(g).all() for g in got), (L, np.dtype(dt).name)
        assert (ref["S"] == 0).mean() > 0.05 and ((ref["S"] > 0) & (ref["S"] < 1)).mean() > 0.05     # (L = 0: 0.16 and 0.09)
        e = errors(got, ref)
        assert max(e.values()) <= TOL, e
        assert all(same(g, w_) for g, w_ in zip(got, ctx.temporal_accumulate(*args, **kw)))
        # where the history met no weight the pixel is the no-history pixel, bit for bit
        kw0 = dict(kw, hist=None, motion=None)
        none = ctx.temporal_accumulate(*args, **kw0)
        # (S == 0 in float64 and in fp32 alike: the label layer's exponent is below -1000, the skipped taps are skipped in both)
        z = ref["S"] == 0
        assert all(same(g[z], n[z]) for g, n in zip(got, none))


def test_non_finite_and_huge_motion_is_no_history(ctx):
    shape, L = (9, 65), 3
    h, w = shape
    args, kw = case(shape, L, np.float32, np.uint8, "fractional", True, 0)
    bad = [np.nan, np.inf, -np.inf, 1e30, -1e30, 1e9, -1e9, 3.4e38, float(w), -1.0, float(-w)]
    mv = kw["motion"].copy()
    yy, xx = np.mgrid[0:h, 0:w]
    hit_x, hit_y = (xx + yy) % 3 == 0, (xx + yy) % 3 == 1
    mv[..., 0][hit_x] = np.float32(bad)[(xx[hit_x] + 2 * yy[hit_x]) % len(bad)]
    mv[..., 1][hit_y] = np.float32(bad)[(xx[hit_y] + 2 * yy[hit_y]) % len(bad)]
    # -1 and -w in x are inside for some columns: only what leaves (-1, w) x (-1, h), NaN included, counts as hit
    with np.errstate(invalid="ignore"):
        ppx, ppy = xx.astype(np.float32) + mv[..., 0], yy.astype(np.float32) + mv[..., 1]
        gone = ~((ppx > -1) & (ppx < w) & (ppy > -1) & (ppy < h))
    assert gone.mean() > 0.4 and (~gone).mean() > 0.2
    got = ctx.temporal_accumulate(*args, **dict(kw, motion=mv))
    none = ctx.temporal_accumulate(*args, **dict(kw, hist=None, motion=None))
    kept = ctx.temporal_accumulate(*args, **kw)
    assert all(np.isfinite(g).all() for g in got)
    assert all(same(g[gone], n[gone]) for g, n in zip(got, none))
    untouched = ~gone & ~hit_x & ~hit_y
    assert all(same(g[untouched], k[untouched]) for g, k in zip(got, kept))


def test_a_long_strip(ctx):
    shape, L = (2, 262149), 3                               # 262 149 x 2 texels: 4097 workgroups along x
    args, kw = case(shape, L, np.float32, np.uint8, "none", True, 0)
    xx = np.arange(shape[1])
    mv = np.zeros(shape + (2,), np.float32)
    mv[..., 0] = np.where(xx % 2 == 0, 3.0, -3.0) * np.where(xx % 5 == 0, 0.5, 1.0)
    mv[..., 1] = np.where(xx % 3 == 0, 0.25, 0.0)
    kw["motion"] = mv
    got = ctx.temporal_accumulate(*args, **kw)
    e = errors(got, check(*args, **kw))
    print(f"{shape} L={L}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert all(np.isfinite(g).all() for g in got) and max(e.values()) <= TOL, e


# ---- refusals -------------------------------------------------------------------------------------------------------------------

class Call:
    """One valid raw call on 16 x 8 texels, whose arguments a test bends one at a time."""

    def __init__(self, ctx, L=2, fdt=np.float32, gdt=np.uint8):
        self.ctx, self.shape, self.L = ctx, (8, 16), L
        (fr, ly, pl, sg), kw = case(self.shape, L, fdt, gdt, "fractional", True, 0)
        up = ctx.upload
        self.keep = [up(fr)] + [up(l) for l in ly] + [up(l) for l in pl] + [up(kw["motion"]), up(kw["hist"][0]), up(kw["hist"][1]), up(kw["var_spatial"])]
        self.cur = self.keep[0].ptr
        self.cl, self.pl = [d.ptr for d in self.keep[1:1 + L]], [d.ptr for d in self.keep[1 + L:1 + 2 * L]]
        self.motion, self.hc, self.hs, self.vs = (d.ptr for d in self.keep[1 + 2 * L:])
        self.sentinel = np.random.default_rng(5).integers(0, 256, 8 * 16 * 16 + 64, dtype=np.uint8)
        self.outs = [up(self.sentinel) for _ in range(3)]
        self.col, self.st, self.var = (d.ptr for d in self.outs)
        self.sg = list(sg)
        self.p = dict(width=16, height=8, alpha=0.2, alphaMoments=0.2, historyMax=32.0, historyFull=4.0,
                      format=mid.api.fmt_with_guide(FMT[np.dtype(fdt)], FMT[np.dtype(gdt)]))

    def run(self, **over):
        a = {k: over.pop(k, getattr(self, k)) for k in ("cur", "cl", "pl", "L", "motion", "hc", "hs", "vs", "col", "st", "var", "sg")}
        pd = dict(self.p, **over)
        p = mid.TemporalAccumParams(pd["width"], pd["height"], pd["alpha"], pd["alphaMoments"], pd["historyMax"], pd["historyFull"], pd["format"])
        tbl = lambda t: None if t is None else (ctypes.c_void_p * 17)(*t)
        sg = None if a["sg"] is None else (ctypes.c_float * 16)(*a["sg"])
        rc = mid.lib.mid_temporal_accumulate(self.ctx.handle, ctypes.byref(p), sg, a["cur"], tbl(a["cl"]), tbl(a["pl"]), a["L"], a["motion"],
                                             a["hc"], a["hs"], a["vs"], a["col"], a["st"], a["var"], None)
        self.ctx.sync()
        return rc, mid.lib.mid_last_error().decode()

    def refused(self, word, **over):
        rc, msg = self.run(**over)
        assert rc == 1 and word in msg, (over, rc, msg)
        for d in self.outs:
            assert np.array_equal(self.ctx.download(d, self.sentinel.shape, np.uint8), self.sentinel), ("an output was touched", over)


def test_refusals_leave_the_outputs_untouched(ctx):
    c = Call(ctx)
    assert c.run()[0] == 0                                  # the call itself is valid ...
    c.outs = [ctx.upload(c.sentinel) for _ in range(3)]     # ... (fresh sentinels for what follows)
    c.col, c.st, c.var = (d.ptr for d in c.outs)
    nan, inf = float("nan"), float("inf")
    # NULL pointers
    c.refused("NULL", cur=None)
    c.refused("NULL", col=None)
    c.refused("NULL", st=None)
    c.refused("both or neither", hc=None)
    c.refused("both or neither", hs=None)
    # layers
    c.refused("outside 0..16", L=-1)
    c.refused("outside 0..16", L=17)
    c.refused("table is NULL", cl=None)
    c.refused("table is NULL", pl=None)
    c.refused("layer 1 is NULL", cl=[c.cl[0], None])
    c.refused("layer 0 is NULL", pl=[None, c.pl[1]])
    c.refused("layer_sigma is NULL", sg=None)
    for bad in (0.0, -1.0, nan, inf):
        c.refused("sigmas must be finite", sg=[0.1, bad])
    # parameters
    for bad in (0.0, -0.1, 1.0001, nan, inf):
        c.refused("alpha ", alpha=bad)
        c.refused("alphaMoments", alphaMoments=bad)
    for bad in (0.999, 0.0, -1.0, nan, inf):
        c.refused("historyMax", historyMax=bad)
    for bad in (1.0, 0.5, -2.0, nan, inf):
        c.refused("historyFull", historyFull=bad)
    # formats and sizes
    c.refused("unknown format", format=3)
    c.refused("unknown format", format=0x10000)
    c.refused("unknown guide-layer format", format=mid.FMT_RGBA32F | (4 << 8))
    c.refused("bad size", width=0)
    c.refused("bad size", height=-1)
    c.refused("too large", width=1 << 15, height=1 << 15)
    # alignment
    c.refused("motion is not 8-byte aligned", motion=c.motion + 4)
    c.refused("history plane is not 16-byte aligned", hc=c.hc + 8)
    c.refused("history plane is not 16-byte aligned", hs=c.hs + 4)
    c.refused("not 16-byte aligned", col=c.col + 8)
    c.refused("not 16-byte aligned", st=c.st + 4)
    c.refused("variance plane is not 16-byte aligned", var=c.var + 4)
    c.refused("variance plane is not 16-byte aligned", vs=c.vs + 8)
    # overlaps: every output against every input and the other outputs
    for out in ("col", "st", "var"):
        for name in ("cur", "motion", "hc", "hs", "vs"):
            c.refused("overlaps", **{out: getattr(c, name)})
        c.refused("overlaps layer 1", **{out: c.cl[1]})
        c.refused("overlaps layer 0", **{out: c.pl[0]})
    c.refused("color_out overlaps hist_color_in", col=c.hc + 16)      # in place, shifted by one texel: the gather reads neighbours
    c.refused("overlaps", col=c.st)
    c.refused("overlaps", st=c.var)
    c.refused("overlaps", var=c.col + 16)
    # and valid variants still run: no layers with NULL tables, no history, no motion, no variance planes
    assert c.run(L=0, cl=None, pl=None, sg=None)[0] == 0
    assert c.run(hc=None, hs=None, motion=None, vs=None, var=None)[0] == 0


def test_alignment_rules_of_half_and_float_frames_and_guides(ctx):
    c = Call(ctx, fdt=np.float16, gdt=np.float16)
    assert c.run()[0] == 0
    c.outs = [ctx.upload(c.sentinel) for _ in range(3)]
    c.col, c.st, c.var = (d.ptr for d in c.outs)
    c.refused("not 8-byte aligned (RGBA16F)", cur=c.cur + 4)
    c.refused("not 8-byte aligned (RGBA16F guide)", cl=[c.cl[0] + 4, c.cl[1]])
    c.refused("not 8-byte aligned (RGBA16F guide)", pl=[c.pl[0], c.pl[1] + 2])
    c = Call(ctx, gdt=np.float32)
    c.refused("not 16-byte aligned (RGBA32F guide)", pl=[c.pl[0] + 8, c.pl[1]])
