"""GPU suite: mid_median_filter (section a4p) against its float64 checker (tests/np_median.py) on the recipe tests/test_median_args.py
holds to its conditions.  Acceptance: the plain form is bit for bit the checker's value; the weighted form is bit for bit wherever the
checker's margin exceeds delta = 2^-16 (or every weight of the window is exactly 0 or 1), and elsewhere a valid tap value that meets
the two float64 inequalities of the header's precision clause.

Frames from 1 x 1, through frames smaller than the window, to one past the wave and tile seams (widths 63, 64, 65, 129; heights one
past the tile height of each class); every height 1 .. 34 at width 37; radius 1, 2, 3; n_layers 0, 1, 3, 4, 5, 16; every frame format
with u8 / f16 / f32 guides; every output format (the packed ones are the library's own packing of the float output); radiance x 1/64
.. 1024.

The worst margin-rule case these tests met on an MI355X: see DESIGN 3.19."""
import functools

import numpy as np
import pytest

import median_inputs as mi
import np_median

pytestmark = pytest.mark.gpu
DTYPES = (np.uint8, np.float16, np.float32)


@functools.lru_cache(maxsize=None)
def reference(h, w, radius, n_layers, frame_dt=np.float32, guide_dt=np.uint8, gain=1.0):
    """(frame, layers or None, sigmas or None, checker result) of the recipe at one shape; computed once and shared."""
    noisy, g0, _ = mi.scene(h, w, seed=h * 1000 + w, gain=gain)
    frame = mi.as_dtype(noisy, frame_dt)
    layers, sigmas = mi.layer_set(g0, n_layers, guide_dt)
    ref = np_median.median(frame, layers, sigmas, radius)
    for a in [frame, *layers, *ref]:
        a.setflags(write=False)
    return frame, (layers or None), (sigmas or None), ref


def check(ctx, h, w, radius, n_layers, **kw):
    frame, layers, sigmas, ref = reference(h, w, radius, n_layers, **kw)
    got = ctx.median_filter(frame, layers, sigmas, radius)
    res = np_median.accept(got, frame, layers, sigmas, radius, ref=ref)
    print(f"{w}x{h} r={radius} L={n_layers} {frame.dtype.name}: {int(res['bad'].sum())} pixel-channels break the rule, "
          f"{res['near']:.4f} held to the inequalities, worst margin held to the bits {res['worst']:.3e}")
    assert res["alpha_ok"]
    assert not res["bad"].any()
    if n_layers == 0:
        assert res["near"] == 0.0 and np_median.same_values(got, ref[0]).all()
    return got


@pytest.mark.parametrize("n_layers", mi.LAYER_COUNTS)
@pytest.mark.parametrize("radius", mi.RADII)
def test_seam_shapes(ctx, radius, n_layers):
    for h, w in mi.seam_shapes(n_layers):
        check(ctx, h, w, radius, n_layers)


@pytest.mark.parametrize("n_layers", (0, 3, 5))
@pytest.mark.parametrize("radius", mi.RADII)
def test_every_height_across_two_tiles(ctx, radius, n_layers):
    for h in range(1, 35):
        check(ctx, h, 37, radius, n_layers)


@pytest.mark.parametrize("frame_dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("guide_dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_format_pairs(ctx, frame_dt, guide_dt):
    for radius, n_layers in ((1, 0), (2, 1), (3, 4), (2, 5)):
        check(ctx, 35, 131, radius, n_layers, frame_dt=frame_dt, guide_dt=guide_dt)


@pytest.mark.parametrize("out_dt", (np.uint8, np.float16), ids=lambda d: np.dtype(d).name)
def test_packed_outputs_are_the_packing_of_the_float_output(ctx, out_dt):
    for radius, n_layers in ((1, 0), (2, 3), (3, 5)):
        frame, layers, sigmas, _ = reference(34, 67, radius, n_layers)
        f32 = ctx.median_filter(frame, layers, sigmas, radius)
        packed = ctx.median_filter(frame, layers, sigmas, radius, out_dtype=out_dt)
        want = ctx.pack_u8(f32) if out_dt == np.uint8 else ctx.pack_f16(f32)
        assert packed.dtype == np.dtype(out_dt) and packed.tobytes() == want.tobytes()


@pytest.mark.parametrize("gain", (1 / 64, 1 / 4, 16.0, 1024.0))
def test_radiance_scales(ctx, gain):
    for radius, n_layers in ((1, 0), (2, 1), (3, 3), (2, 16)):
        check(ctx, 33, 70, radius, n_layers, gain=gain)
