"""Device-side helpers of the tall-frame and later-tile GPU tests (tests/test_gpu_tall_frames.py, tests/test_gpu_later_tiles.py): planes
between guard bands that repeat a 37-row pattern (tests/tall_inputs.py), tiled on the device; the comparison of every row of a tall
output with a small frame's output through row_map, on the device; the device's grid limits."""
import ctypes
import functools

import numpy as np
import torch

import image_denoising_filter_amd as mid
import tall_inputs as ti

BAND = 4096
DEV = torch.device("cuda", 0)
HIP_DEVICE_ATTRIBUTE_MAX_GRID_DIM_Y = 30            # hip_runtime_api.h: hipDeviceAttributeMaxGridDimX, ..Y, ..Z are 29, 30, 31
F32U8 = mid.api.fmt_with_guide(mid.FMT_RGBA32F, mid.FMT_RGBA8)
F32F32 = mid.api.fmt_with_guide(mid.FMT_RGBA32F, mid.FMT_RGBA32F)


@functools.lru_cache(maxsize=None)
def max_grid_dim_y():
    """hipDeviceAttributeMaxGridDimY of device 0, asked of the HIP runtime this process has already loaded (torch's)."""
    torch.cuda.init()
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "no HIP runtime is loaded"
    hip = ctypes.CDLL(paths[0])
    x, y, z = (ctypes.c_int(-1) for _ in range(3))
    for v, attr in ((x, 29), (y, HIP_DEVICE_ATTRIBUTE_MAX_GRID_DIM_Y), (z, 31)):
        assert hip.hipDeviceGetAttribute(ctypes.byref(v), attr, 0) == 0
    assert x.value >= 2 ** 31 - 1 and 0 < z.value <= y.value <= x.value, "not the three grid limits: another header's numbering?"
    return y.value


def announce(what, h, rows):
    print(f"{what}: h = {h}, gridDim.y = {ti.cdiv(h, rows)}, hipDeviceAttributeMaxGridDimY = {max_grid_dim_y()}")
    assert ti.cdiv(h, rows) == ti.GRID_Y


class Plane:
    """A plane of `shape` x dtype between two guard bands of BAND bytes in one device allocation.  rows: the 37-row pattern (numpy) it
    repeats, or a whole array; None: an output, every byte 0xff (NaN as float32)."""

    def __init__(self, shape, dtype, rows=None):
        self.shape, self.dtype = tuple(shape), dtype
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.empty(self.nbytes + 2 * BAND, dtype=torch.uint8, device=DEV)
        self.band = (torch.arange(BAND, device=DEV) * 7 % 251).to(torch.uint8)
        self.buf[:BAND] = self.band
        self.buf[BAND + self.nbytes:] = self.band
        self.mid = self.buf[BAND:BAND + self.nbytes].view(dtype).view(self.shape)
        if rows is None:
            self.buf[BAND:BAND + self.nbytes] = 0xff
            self.before = None
        else:
            src = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
            assert src.dtype == dtype
            if src.shape[0] != shape[0]:
                assert src.shape[0] == ti.PERIOD
                src = src.repeat((ti.cdiv(shape[0], ti.PERIOD),) + (1,) * (src.dim() - 1))[:shape[0]]
            self.mid.copy_(src.view(self.shape))
            self.before = int(self.buf.sum(dtype=torch.int64))
        self.ptr = self.buf.data_ptr() + BAND

    def intact(self):
        ok = torch.equal(self.buf[:BAND], self.band) and torch.equal(self.buf[BAND + self.nbytes:], self.band)
        return ok and (self.before is None or int(self.buf.sum(dtype=torch.int64)) == self.before)


def planes_of(patterns, h, names):
    out = {}
    for n in names:
        v = patterns[n]
        mk = lambda a: Plane((h,) + a.shape[1:], torch.from_numpy(a[:1]).dtype, a)
        out[n] = [mk(a) for a in v] if isinstance(v, list) else mk(v)
    return out


def table(planes, n=17):
    return (ctypes.c_void_p * n)(*[p.ptr for p in planes])


def finish(ctx, rc, ins, outs):
    assert rc == 0, mid.lib.mid_last_error()
    ctx.sync()
    flat = [p for v in ins.values() for p in (v if isinstance(v, list) else [v])]
    assert all(p.intact() for p in flat), "an input or its guard band changed"
    assert all(p.intact() for p in outs), "a store beside an output"


def wrong_rows(got, small, rows, values=False):
    """The rows of `got` [H, ...] that differ from small[rows]: bits, or values (+0 == -0, NaN == NaN)."""
    want = small.index_select(0, rows)
    if values:
        ok = (got == want) | (torch.isnan(got) & torch.isnan(want))
    else:
        ok = got.view(torch.int32) == want.view(torch.int32)
    return torch.nonzero(~ok.reshape(got.shape[0], -1).all(1)).flatten().tolist()[:8]


def rows_on_device(H, r, hs):
    return torch.from_numpy(ti.row_map(H, r, hs)).to(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
