"""RGBA16F image I/O (host only, no GPU): mid_image_load_f16 / load_image(path, np.float16) and save_image of float16 arrays.

HALF files must come back bit for bit; FLOAT files as np.float16(values) and UINT files as np.float16(np.float32(values)) --
round to nearest even with the special values numpy gives them.  The EXR files are built by hand with test_codecs._exr."""
import ctypes
import struct

import numpy as np
import pytest

import image_denoising_filter_amd as mid
from image_denoising_filter_amd._lib import Image, lib
from image_denoising_filter_amd.api import _fmt_of
from test_codecs import _exr

_IDX = {"R": 0, "G": 1, "B": 2, "A": 3}


def _lines(px, chans):
    return [{n: np.ascontiguousarray(px[y, :, _IDX[n]]).tobytes() for n, _ in chans} for y in range(px.shape[0])]


def _special_halves():
    """Every class of binary16 code: zeros, subnormals, normals, the largest finite, infinities and NaNs."""
    return np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x83ff, 0x0400, 0x3c00, 0xbc00, 0x3555, 0x7bff, 0xfbff,
                     0x7c00, 0xfc00, 0x7e00, 0xfe00, 0x7c01, 0x7d23], np.uint16)


@pytest.mark.parametrize("compression", [0, 1, 2, 3, 4])
def test_half_exr_loads_bit_for_bit(tmp_path, compression):
    rng = np.random.default_rng(11 + compression)
    h, w = 35, 19
    bits = rng.integers(0, 1 << 16, (h, w, 4), dtype=np.uint16)
    bits.reshape(-1)[:len(_special_halves())] = _special_halves()
    px = bits.view(np.float16)
    chans = [("A", 1), ("B", 1), ("G", 1), ("R", 1)]
    p = tmp_path / "h.exr"
    p.write_bytes(_exr(w, h, chans, compression, _lines(px, chans), None))
    got = mid.load_image(p, np.float16)
    assert got.dtype == np.float16 and got.shape == (h, w, 4)
    assert np.array_equal(got.view(np.uint16), bits), "HALF channels must be copied bit for bit (NaN payloads included)"
    # the float32 loader of the same file is the exact widening
    f32 = mid.load_image(p)
    finite = ~np.isnan(px)
    assert np.array_equal(f32[finite], px[finite].astype(np.float32)) and np.all(np.isnan(f32[~finite]))


def _float_sweep(rng, n):
    """fp32 values that exercise every rounding path of fp32 -> binary16."""
    f16max, tiny = 65504.0, 2.0 ** -24
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, f16max, -f16max, 65519.996, 65520.0, 65520.004, 1e6, -1e30,
         tiny, tiny / 2, tiny / 2 * 1.0000001, tiny * 1.5, tiny * 2.5, 2.0 ** -14, 2.0 ** -14 * (1 - 2 ** -12), 1e-42, -1e-42,
         1.0 + 2 ** -11, 1.0 + 3 * 2 ** -11, 1.0 + 2 ** -11 + 2 ** -20, 2048.0 + 1.0, 2048.0 + 3.0, 0.1, -0.3333333]
    halfway = (np.arange(1, 0x7bff, 97, dtype=np.uint32) << 13 | 0x1000) + np.uint32(0x38000000)   # exact ties between halves
    v = np.concatenate([np.float32(v), halfway.view(np.float32), np.float32(rng.standard_normal(n) * 100),
                        np.float32(rng.random(n) * 2 ** -14), (rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)).view(np.float32)])
    return v.astype(np.float32)


def test_float_exr_loads_as_rounded_half(tmp_path):
    rng = np.random.default_rng(5)
    v = _float_sweep(rng, 400)
    w = 16
    v = np.concatenate([v, np.zeros((-len(v)) % (4 * w), np.float32)])
    px = v.reshape(-1, w, 4)
    chans = [("A", 2), ("B", 2), ("G", 2), ("R", 2)]
    p = tmp_path / "f.exr"
    p.write_bytes(_exr(w, px.shape[0], chans, 3, _lines(px, chans), None))
    with np.errstate(over="ignore", invalid="ignore"):
        want = px.astype(np.float16)
    got = mid.load_image(p, np.float16)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), "FLOAT channels must round like np.float16"


def test_uint_exr_and_missing_alpha(tmp_path):
    rng = np.random.default_rng(6)
    h, w = 7, 11
    u = rng.integers(0, 2 ** 32, (h, w, 3), dtype=np.uint64).astype(np.uint32)
    u[0, :6, 0] = [0, 1, 2049, 65504, 65519, 65520]
    chans = [("B", 0), ("G", 0), ("R", 0)]
    p = tmp_path / "u.exr"
    p.write_bytes(_exr(w, h, chans, 2, [{"R": u[y, :, 0].tobytes(), "G": u[y, :, 1].tobytes(), "B": u[y, :, 2].tobytes()}
                                       for y in range(h)], None))
    got = mid.load_image(p, np.float16)
    with np.errstate(over="ignore"):
        want = u.astype(np.float32).astype(np.float16)
    assert np.array_equal(got[..., :3].view(np.uint16), want.view(np.uint16))
    assert np.all(got[..., 3].view(np.uint16) == 0x3C00), "a missing alpha is 1.0"
    # a HALF file without alpha, too
    hp = rng.random((h, w, 3)).astype(np.float16)
    p2 = tmp_path / "h3.exr"
    p2.write_bytes(_exr(w, h, [("B", 1), ("G", 1), ("R", 1)], 0,
                        [{"R": hp[y, :, 0].tobytes(), "G": hp[y, :, 1].tobytes(), "B": hp[y, :, 2].tobytes()} for y in range(h)], None))
    g2 = mid.load_image(p2, np.float16)
    assert np.array_equal(g2[..., :3].view(np.uint16), hp.view(np.uint16)) and np.all(g2[..., 3] == 1.0)


@pytest.mark.parametrize("shape", [(3, 5), (16, 16), (40, 33)])
def test_save_half_declares_half_and_round_trips(tmp_path, shape):
    rng = np.random.default_rng(shape[0])
    bits = rng.integers(0, 1 << 16, (*shape, 4), dtype=np.uint16)
    bits.reshape(-1)[:len(_special_halves())] = _special_halves()
    a = bits.view(np.float16)
    p = tmp_path / "s.exr"
    mid.save_image(p, a)
    blob = p.read_bytes()
    pos = blob.index(b"chlist\0") + 7 + 4
    for n in (b"A\0", b"B\0", b"G\0", b"R\0"):                    # A,B,G,R as HALF (pixel type 1)
        assert blob[pos:pos + 2] == n and struct.unpack("<i", blob[pos + 2:pos + 6])[0] == 1
        pos += 2 + 16
    comp = blob[blob.index(b"compression\0compression\0") + 24 + 4]
    assert comp == (0 if shape[0] < 16 and shape[1] < 16 else 3), "the FLOAT writer's compression"
    assert np.array_equal(mid.load_image(p, np.float16).view(np.uint16), bits)
    f32 = mid.load_image(p)
    assert f32.dtype == np.float32
    finite = ~np.isnan(a)
    assert np.array_equal(f32[finite], a[finite].astype(np.float32)) and np.all(np.isnan(f32[~finite]))


def test_refusals(tmp_path):
    png = tmp_path / "x.png"
    mid.save_image(png, np.zeros((4, 4, 4), np.uint8))
    img = Image()
    assert lib.mid_image_load_f16(None, str(png).encode(), ctypes.byref(img)) == 1     # MID_ERR_INVALID
    assert img.data is None
    with pytest.raises(mid.MidError):
        mid.load_image(png, np.float16)
    assert mid.load_image(png).dtype == np.uint8                                        # the default loader is unchanged
    assert _fmt_of(np.zeros((2, 2, 4), np.float16)) == 2 == mid.FMT_RGBA16F
    with pytest.raises(TypeError):
        _fmt_of(np.zeros((2, 2, 4), np.float64))
