"""Host-side mirror of the reference's kernel interface, over the C-ABI.

The reference drives its kernels through ComputeApplication::RunOnGPU (src/main.cpp:1307-1730):
bind {output / WeightInfo buffer, image(s)}, push {w, h, sigmas | h}, dispatch.  `Context`
offers the same operators with the same argument meaning; every call goes through
libmi_denoise.so (ctypes) -- there is no NumPy/PyTorch compute path here, and a missing
library or GPU is an error, not a fallback.

NumPy arrays are (h, w, 4): float32 = RGBA32F (.exr path), uint8 = RGBA8 (.png path), float16 = RGBA16F (half-float
frames: EXR HALF channels, a renderer's RGBA16F buffers).  Filters read RGBA16F exactly as the float32 frame it widens to.
WeightInfo buffers are float32 (h, w, 8): [wc.r, wc.g, wc.b, wc.a, normWeight, pad, pad, pad].
"""
import ctypes
import weakref

import numpy as np

from ._lib import AlbedoParams, AtrousMomentsParams, AtrousParams, AtrousVarianceParams, BilateralParams, ColorBoundsParams, FireflyParams, GuidedParams, Image, ImageMetricsParams, ImageMetricsResult, METRICS_N, MedianParams, NlmParams, NormalizeParams, TemporalAccumParams, c_void_pp, lib

FMT_RGBA32F, FMT_RGBA8, FMT_RGBA16F = 0, 1, 2


def fmt_with_guide(fmt, guide_fmt):
    """MID_FMT_WITH_GUIDE: the format word of a bilateral call whose guide layers are not RGBA8."""
    return fmt | ((guide_fmt + 1) << 8)
LAYOUT_TEXTURE, LAYOUT_LINEAR = 0, 1

# nonlocal.comp:5-6 as shipped, and the 21x21 / 7x7 benchmark configuration (half-open ranges)
NLM_REFERENCE = dict(search=(-7, 7), patch=(-3, 3))
NLM_BENCH = dict(search=(-10, 11), patch=(-3, 4))


class MidError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = lib.mid_last_error().decode("utf-8", "replace")
        super().__init__(f"{where}: error {code}: {msg}")


def _check(code, where):
    if code != 0:
        raise MidError(code, where)


def load_image(path, dtype=None):
    """LoadImages (src/main.cpp:145-229): '.exr' -> float32 (h,w,4), anything else as PNG -> uint8 (h,w,4).
    dtype=np.float16: an .exr as RGBA16F (mid_image_load_f16: HALF channels bit for bit, FLOAT / UINT rounded to nearest
    even); PNG files are refused.  Host-only (no GPU)."""
    img = Image()
    half = dtype is not None and np.dtype(dtype) == np.float16
    if dtype is not None and not half:
        raise TypeError(f"load_image: dtype must be None or float16, got {dtype}")
    if half:
        _check(lib.mid_image_load_f16(None, str(path).encode(), ctypes.byref(img)), "mid_image_load_f16")
    else:
        _check(lib.mid_image_load(str(path).encode(), ctypes.byref(img)), "mid_image_load")
    try:
        dt = {FMT_RGBA32F: np.float32, FMT_RGBA8: np.uint8, FMT_RGBA16F: np.float16}[img.format]
        n = img.width * img.height * 4
        raw = (ctypes.c_uint8 * (n * np.dtype(dt).itemsize)).from_address(img.data)
        arr = np.frombuffer(raw, dtype=dt).reshape(img.height, img.width, 4).copy()
    finally:
        lib.mid_image_free(ctypes.byref(img))
    return arr


def save_image(path, arr):
    """SaveEXR(rgba,w,h,4,0) for float32, lodepng::encode for uint8 (src/main.cpp:1699,1717); float16 -> EXR with HALF channels."""
    arr = _img(arr)
    _check(lib.mid_image_save(str(path).encode(), arr.ctypes.data, arr.shape[1], arr.shape[0], _fmt_of(arr)),
           "mid_image_save")


class DeviceBuffer:
    """A hipMalloc'd buffer owned by Python (the application owns every buffer, like the reference)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = ctypes.c_void_p()
        _check(lib.mid_alloc(ctx.handle, self.nbytes, ctypes.byref(p)), "mid_alloc")
        self.ptr = p.value
        ctx._live.add(self)

    def free(self):
        # a buffer that outlives its context was already released by Context.close() (ptr is None then)
        if self.ptr and self.ctx.handle:
            lib.mid_free(self.ctx.handle, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _fmt_of(a):
    if a.dtype == np.float32:
        return FMT_RGBA32F
    if a.dtype == np.uint8:
        return FMT_RGBA8
    if a.dtype == np.float16:
        return FMT_RGBA16F
    raise TypeError(f"image dtype must be float32, uint8 or float16, got {a.dtype}")


_GUIDE_DTYPES = (np.uint8, np.float16, np.float32)
_OUT_FMT = {np.dtype(np.uint8): FMT_RGBA8, np.dtype(np.float16): FMT_RGBA16F, np.dtype(np.float32): FMT_RGBA32F}


def _guide_fmt(fmt, layers, who):
    """The format word of a bilateral call with guide layers: the frames' FMT_* with the guide field set from the layers' dtype
    (uint8 leaves it 0: RGBA8, as always).  All layers of a call share one dtype."""
    dts = {np.dtype(l.dtype) for l in layers}
    if len(dts) > 1:
        raise ValueError(f"{who}: all guide layers of a call share one dtype, got {sorted(str(d) for d in dts)}")
    if not dts or dts == {np.dtype(np.uint8)}:
        return fmt
    (dt,) = dts
    if dt not in (np.dtype(np.float16), np.dtype(np.float32)):
        raise TypeError(f"{who}: guide layers must be uint8, float16 or float32, got {dt}")
    return fmt_with_guide(fmt, _fmt_of(layers[0]))


def _img(a):
    a = np.ascontiguousarray(a)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"image must be (h, w, 4), got {a.shape}")
    return a


def _same_frames(frames, what):
    """Every frame of a sequence is read with frames[0]'s size and format: refuse anything else up front."""
    frames = [_img(f) for f in frames]
    if not frames:
        raise ValueError(f"{what}: no frames")
    _fmt_of(frames[0])
    for i, f in enumerate(frames):
        if f.shape != frames[0].shape or f.dtype != frames[0].dtype:
            raise ValueError(f"{what}: frame {i} is {f.shape} {f.dtype}, frame 0 is {frames[0].shape} {frames[0].dtype}")
    return frames


class Context:
    """One device + its streams (mid_ctx).  Replaces the reference's Vulkan instance/device/queue."""

    def __init__(self, device=0):
        h = ctypes.c_void_p()
        _check(lib.mid_ctx_create(int(device), ctypes.byref(h)), "mid_ctx_create")
        self.handle = h
        self.device = device
        self._live = weakref.WeakSet()      # DeviceBuffers allocated through this context and not yet freed

    def close(self):
        if self.handle:
            for buf in list(self._live):    # mid_free needs a live context: release what is still held, then the context
                buf.free()
            lib.mid_ctx_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def release_cached(self):
        """Free the device ring / output slots / events the frame pipeline keeps in the context between calls."""
        _check(lib.mid_ctx_release_cached(self.handle), "mid_ctx_release_cached")

    @property
    def name(self):
        buf = ctypes.create_string_buffer(160)
        _check(lib.mid_device_name(self.handle, buf, 160), "mid_device_name")
        return buf.value.decode()

    # ---- memory ---------------------------------------------------------------------------
    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    # NumPy arrays are pageable memory.  The C-ABI itself keeps such memory away from the HIP runtime's pin-on-the-fly path
    # (mid_memcpy_h2d / mid_memcpy_d2h move it through the context's page-locked bounce buffers, csrc/hostcopy.cpp), so
    # these two are plain calls: what the tests exercise here is what any caller of the library gets.
    def upload(self, arr, stream=None):
        arr = np.ascontiguousarray(arr)
        buf = DeviceBuffer(self, max(arr.nbytes, 16))
        if arr.nbytes:
            _check(lib.mid_memcpy_h2d(self.handle, buf.ptr, arr.ctypes.data, arr.nbytes, stream), "mid_memcpy_h2d")
            self.sync(stream)
        return buf

    def download(self, buf, shape, dtype, stream=None):
        out = np.empty(shape, dtype=dtype)
        ptr = buf.ptr if isinstance(buf, DeviceBuffer) else int(buf)
        if out.nbytes:
            _check(lib.mid_memcpy_d2h(self.handle, out.ctypes.data, ptr, out.nbytes, stream), "mid_memcpy_d2h")
            self.sync(stream)
        return out

    def zeros(self, nbytes, stream=None):
        buf = DeviceBuffer(self, nbytes)
        _check(lib.mid_memset(self.handle, buf.ptr, 0, nbytes, stream), "mid_memset")
        return buf

    def sync(self, stream=None):
        _check(lib.mid_stream_sync(self.handle, stream), "mid_stream_sync")

    # ---- raw (device pointer) operators: what bench.py and the pipeline use ------------------
    def record(self, stream=None):
        """`with ctx.record(stream) as rec:` -- the kernel-level calls issued on `stream` inside the block are RECORDED instead of executed
        (vkBeginCommandBuffer ... vkEndCommandBuffer, src/main.cpp:791/846); afterwards `rec.submit(stream)` runs the sequence
        (vkQueueSubmit, :1091) as often as needed."""
        return Recording(self, stream)

    def bilateral_dev(self, in_ptr, out_ptr, w, h, radius, sigma_s, sigma_c, layout, fmt, stream=None):
        p = BilateralParams(w, h, sigma_s, sigma_c, radius, layout, fmt)
        _check(lib.mid_bilateral(self.handle, ctypes.byref(p), in_ptr, out_ptr, stream), "mid_bilateral")

    def bilateral_batch_dev(self, in_ptrs, out_ptrs, w, h, radius, sigma_s, sigma_c, layout, fmt, stream=None):
        if len(out_ptrs) != len(in_ptrs) or not in_ptrs:
            raise ValueError(f"{len(in_ptrs)} input and {len(out_ptrs)} output pointers")
        p = BilateralParams(w, h, sigma_s, sigma_c, radius, layout, fmt)
        fi = (ctypes.c_void_p * len(in_ptrs))(*in_ptrs)
        fo = (ctypes.c_void_p * len(out_ptrs))(*out_ptrs)
        _check(lib.mid_bilateral_batch(self.handle, ctypes.byref(p), fi, fo, len(in_ptrs), stream), "mid_bilateral_batch")

    def nlm_temporal_dev(self, frame_ptrs, out_ptrs, w, h, hparam, search, patch, k, first, count, fmt, stream=None):
        # (the frame range itself is checked by the C side -> MID_ERR_INVALID; what C cannot see is the length of
        # the ctypes output table it is about to read `count` entries of)
        if len(out_ptrs) < count:
            raise ValueError(f"{count} output frames asked for, only {len(out_ptrs)} output pointers given")
        p = NlmParams(w, h, hparam, search[0], search[1], patch[0], patch[1], fmt)
        fr = (ctypes.c_void_p * len(frame_ptrs))(*frame_ptrs)
        ou = (ctypes.c_void_p * len(out_ptrs))(*out_ptrs)
        _check(lib.mid_nlm_temporal(self.handle, ctypes.byref(p), fr, len(frame_ptrs), k, first, count, ou, stream),
               "mid_nlm_temporal")

    # ---- NumPy-level operators (tests, smoke) ----------------------------------------------
    def bilateral(self, img, radius, sigma_s=2.0, sigma_c=0.2, layout="texture"):
        """bialteral.comp (layout='texture') / bialteral_linear.comp (layout='linear')."""
        img = _img(img)
        h, w = img.shape[:2]
        lay = {"texture": LAYOUT_TEXTURE, "linear": LAYOUT_LINEAR}[layout]
        d_in, d_out = self.upload(img), self.alloc(w * h * 16)
        self.bilateral_dev(d_in.ptr, d_out.ptr, w, h, radius, sigma_s, sigma_c, lay, _fmt_of(img))
        return self.download(d_out, (h, w, 4), np.float32)

    def bilateral_batch(self, frames, radius, sigma_s=2.0, sigma_c=0.2, layout="texture"):
        """n independent frames, one launch (mid_bilateral_batch)."""
        frames = _same_frames(frames, "bilateral_batch")
        h, w = frames[0].shape[:2]
        lay = {"texture": LAYOUT_TEXTURE, "linear": LAYOUT_LINEAR}[layout]
        d_in = [self.upload(f) for f in frames]
        d_out = [self.alloc(w * h * 16) for _ in frames]
        self.bilateral_batch_dev([d.ptr for d in d_in], [d.ptr for d in d_out], w, h, radius, sigma_s, sigma_c, lay, _fmt_of(frames[0]))
        return [self.download(d, (h, w, 4), np.float32) for d in d_out]

    def bilateral_layers_accum(self, img, layer, W, radius, sigma_s=2.0, sigma_c=0.2):
        """One dispatch of bialteral_layers.comp: returns W + this layer's sums.  layer: uint8, float16 or float32 (h, w, 4)."""
        img, layer = _img(img), _img(layer)
        fmt = _guide_fmt(_fmt_of(img), [layer], "bilateral_layers_accum")
        h, w = img.shape[:2]
        W = np.ascontiguousarray(W, dtype=np.float32)
        d_in, d_l, d_w = self.upload(img), self.upload(layer), self.upload(W)
        p = BilateralParams(w, h, sigma_s, sigma_c, radius, LAYOUT_TEXTURE, fmt)
        _check(lib.mid_bilateral_layers_accum(self.handle, ctypes.byref(p), d_in.ptr, d_l.ptr, d_w.ptr, None),
               "mid_bilateral_layers_accum")
        return self.download(d_w, (h, w, 8), np.float32)

    def bilateral_layers(self, img, layers, radius, sigma_s=2.0, sigma_c=0.2):
        """The per-layer loop + normalize, fused (src/main.cpp:1610-1623,1649-1652).  layers: uint8, float16 or float32
        (h, w, 4) guides, all of one dtype."""
        img = _img(img)
        h, w = img.shape[:2]
        layers = [_img(l) for l in layers]
        fmt = _guide_fmt(_fmt_of(img), layers, "bilateral_layers")
        d_in, d_out = self.upload(img), self.alloc(w * h * 16)
        d_layers = [self.upload(l) for l in layers]
        tbl = (ctypes.c_void_p * max(len(d_layers), 1))(*[d.ptr for d in d_layers])
        p = BilateralParams(w, h, sigma_s, sigma_c, radius, LAYOUT_TEXTURE, fmt)
        _check(lib.mid_bilateral_layers(self.handle, ctypes.byref(p), d_in.ptr, tbl, len(d_layers), d_out.ptr, None),
               "mid_bilateral_layers")
        return self.download(d_out, (h, w, 4), np.float32)

    def nlm_accum(self, target, neighbour, W, hparam=0.5, search=(-7, 7), patch=(-3, 3)):
        """One dispatch of nonlocal.comp: returns W + this neighbour frame's sums."""
        target, neighbour = _img(target), _img(neighbour)
        h, w = target.shape[:2]
        W = np.ascontiguousarray(W, dtype=np.float32)
        d_t, d_n, d_w = self.upload(target), self.upload(neighbour), self.upload(W)
        p = NlmParams(w, h, hparam, search[0], search[1], patch[0], patch[1], _fmt_of(target))
        _check(lib.mid_nlm_accum(self.handle, ctypes.byref(p), d_t.ptr, d_n.ptr, d_w.ptr, None), "mid_nlm_accum")
        return self.download(d_w, (h, w, 8), np.float32)

    def nlm_temporal(self, frames, k=0, first=0, count=None, hparam=0.5, search=(-7, 7), patch=(-3, 3)):
        """Fused accumulate-over-neighbour-frames + normalize for `count` output frames."""
        frames = _same_frames(frames, "nlm_temporal")
        count = len(frames) - first if count is None else count
        h, w = frames[0].shape[:2]
        d_fr = [self.upload(f) for f in frames]
        d_out = [self.alloc(w * h * 16) for _ in range(count)]
        self.nlm_temporal_dev([d.ptr for d in d_fr], [d.ptr for d in d_out], w, h, hparam, search, patch,
                              k, first, count, _fmt_of(frames[0]))
        return [self.download(d, (h, w, 4), np.float32) for d in d_out]

    def nlm_layers_accum(self, img, layer, W, hparam=0.5, search=(-7, 7), patch=(-3, 3)):
        """One dispatch of nonlocal.comp with the patch distance on the uint8 guide `layer` and the colour from `img`:
        returns W + this layer's sums (mid_nlm_layers_accum)."""
        img, layer = _img(img), _img(layer)
        if layer.dtype != np.uint8:
            raise TypeError("layers are always RGBA8 (src/main.cpp:1396)")
        h, w = img.shape[:2]
        W = np.ascontiguousarray(W, dtype=np.float32)
        d_in, d_l, d_w = self.upload(img), self.upload(layer), self.upload(W)
        p = NlmParams(w, h, hparam, search[0], search[1], patch[0], patch[1], _fmt_of(img))
        _check(lib.mid_nlm_layers_accum(self.handle, ctypes.byref(p), d_in.ptr, d_l.ptr, d_w.ptr, None), "mid_nlm_layers_accum")
        return self.download(d_w, (h, w, 8), np.float32)

    def nlm_layers(self, img, layers, hparam=0.5, search=(-7, 7), patch=(-3, 3)):
        """Layer-guided NLM: one accumulate dispatch per uint8 guide layer + normalize, fused (mid_nlm_layers)."""
        img = _img(img)
        h, w = img.shape[:2]
        layers = [_img(l) for l in layers]
        for l in layers:
            if l.dtype != np.uint8:
                raise TypeError("layers are always RGBA8 (src/main.cpp:1396)")
        d_in, d_out = self.upload(img), self.alloc(w * h * 16)
        d_layers = [self.upload(l) for l in layers]
        tbl = (ctypes.c_void_p * max(len(d_layers), 1))(*[d.ptr for d in d_layers])
        p = NlmParams(w, h, hparam, search[0], search[1], patch[0], patch[1], _fmt_of(img))
        _check(lib.mid_nlm_layers(self.handle, ctypes.byref(p), d_in.ptr, tbl, len(d_layers), d_out.ptr, None), "mid_nlm_layers")
        return self.download(d_out, (h, w, 4), np.float32)

    def nlm_layers_pair_accum(self, target_layer, neighbour_layer, neighbour, W, hparam=0.5, search=(-7, 7), patch=(-3, 3)):
        """One dispatch with the patch distance between two uint8 guides -- the target frame's layer and the neighbour frame's
        layer -- and the colour from the `neighbour` frame: returns W + its sums (mid_nlm_layers_pair_accum)."""
        neighbour, target_layer, neighbour_layer = _img(neighbour), _img(target_layer), _img(neighbour_layer)
        if target_layer.dtype != np.uint8 or neighbour_layer.dtype != np.uint8:
            raise TypeError("layers are always RGBA8 (src/main.cpp:1396)")
        h, w = neighbour.shape[:2]
        W = np.ascontiguousarray(W, dtype=np.float32)
        d_in, d_n, d_w = self.upload(neighbour), self.upload(neighbour_layer), self.upload(W)
        d_t = d_n if target_layer is neighbour_layer else self.upload(target_layer)
        p = NlmParams(w, h, hparam, search[0], search[1], patch[0], patch[1], _fmt_of(neighbour))
        _check(lib.mid_nlm_layers_pair_accum(self.handle, ctypes.byref(p), d_t.ptr, d_n.ptr, d_in.ptr, d_w.ptr, None),
               "mid_nlm_layers_pair_accum")
        return self.download(d_w, (h, w, 8), np.float32)

    def nlm_layers_temporal(self, frames, layers, k=0, first=0, count=None, hparam=0.5, search=(-7, 7), patch=(-3, 3), out_dtype=None):
        """Layer-guided NLM over the frames t-k..t+k for `count` output frames, fused (mid_nlm_layers_temporal).
        layers: one list per frame of equally many uint8 (h, w, 4) guide layers; out_dtype: None = float32, uint8 or float16."""
        frames = _same_frames(frames, "nlm_layers_temporal")
        n = len(frames)
        count = n - first if count is None else count
        h, w = frames[0].shape[:2]
        n_layers, flat = _flat_layers(layers, n, h, w, "nlm_layers_temporal")
        out_dtype = _out_dtype(False, out_dtype)
        out_fmt = {np.dtype(np.uint8): FMT_RGBA8, np.dtype(np.float16): FMT_RGBA16F, np.dtype(np.float32): FMT_RGBA32F}[out_dtype]
        d_fr = [self.upload(f) for f in frames]
        d_l = [self.upload(l) for l in flat]
        d_out = [self.alloc(w * h * 4 * out_dtype.itemsize) for _ in range(max(count, 0))]
        p = NlmParams(w, h, hparam, search[0], search[1], patch[0], patch[1], _fmt_of(frames[0]))
        _check(lib.mid_nlm_layers_temporal(self.handle, ctypes.byref(p), (ctypes.c_void_p * n)(*[d.ptr for d in d_fr]),
                                           (ctypes.c_void_p * max(len(d_l), 1))(*[d.ptr for d in d_l]), n_layers, n, k, first, count,
                                           (ctypes.c_void_p * max(len(d_out), 1))(*[d.ptr for d in d_out]), out_fmt, None),
               "mid_nlm_layers_temporal")
        return [self.download(d, (h, w, 4), out_dtype) for d in d_out]

    def nlm_joint(self, frames, layers, hs=None, k=0, first=0, count=None, hparam=0.5, search=(-7, 7), patch=(-3, 3), out_dtype=None):
        """Joint layer-guided NLM over the frames t-k..t+k for `count` output frames (mid_nlm_joint): one weight per search
        offset from the patch distances of all guide layers.  layers: one list per frame of equally many (1..16) uint8 (h, w, 4)
        guide layers; hs: one h per layer, or None for hparam in every layer; out_dtype: None = float32, uint8 or float16."""
        frames = _same_frames(frames, "nlm_joint")
        n = len(frames)
        count = n - first if count is None else count
        h, w = frames[0].shape[:2]
        n_layers, flat = _flat_layers(layers, n, h, w, "nlm_joint")
        out_dtype = _out_dtype(False, out_dtype)
        out_fmt = {np.dtype(np.uint8): FMT_RGBA8, np.dtype(np.float16): FMT_RGBA16F, np.dtype(np.float32): FMT_RGBA32F}[out_dtype]
        d_fr = [self.upload(f) for f in frames]
        d_l = [self.upload(l) for l in flat]
        d_out = [self.alloc(w * h * 4 * out_dtype.itemsize) for _ in range(max(count, 0))]
        p = NlmParams(w, h, hparam, search[0], search[1], patch[0], patch[1], _fmt_of(frames[0]))
        _check(lib.mid_nlm_joint(self.handle, ctypes.byref(p), _layer_sigmas(hs, n_layers, "nlm_joint", "values of h"),
                                 (ctypes.c_void_p * n)(*[d.ptr for d in d_fr]),
                                 (ctypes.c_void_p * max(len(d_l), 1))(*[d.ptr for d in d_l]), n_layers, n, k, first, count,
                                 (ctypes.c_void_p * max(len(d_out), 1))(*[d.ptr for d in d_out]), out_fmt, None),
               "mid_nlm_joint")
        return [self.download(d, (h, w, 4), out_dtype) for d in d_out]

    def bilateral_pair_accum(self, target, neighbour, W, radius, sigma_s=2.0, sigma_c=0.2):
        """One plain pair dispatch: the range weight between the `target` frame's centre and the `neighbour` frame's taps, the
        colour from `neighbour`: returns W + its sums (mid_bilateral_pair_accum)."""
        target, neighbour = _img(target), _img(neighbour)
        if target.shape != neighbour.shape or target.dtype != neighbour.dtype:
            raise ValueError(f"bilateral_pair_accum: target is {target.shape} {target.dtype}, neighbour {neighbour.shape} {neighbour.dtype}")
        h, w = neighbour.shape[:2]
        W = np.ascontiguousarray(W, dtype=np.float32)
        d_n, d_w = self.upload(neighbour), self.upload(W)
        d_t = d_n if target is neighbour else self.upload(target)
        p = BilateralParams(w, h, sigma_s, sigma_c, radius, LAYOUT_TEXTURE, _fmt_of(neighbour))
        _check(lib.mid_bilateral_pair_accum(self.handle, ctypes.byref(p), d_t.ptr, d_n.ptr, d_w.ptr, None), "mid_bilateral_pair_accum")
        return self.download(d_w, (h, w, 8), np.float32)

    def bilateral_layers_pair_accum(self, target_layer, neighbour_layer, neighbour, W, radius, sigma_s=2.0, sigma_c=0.2):
        """One layered pair dispatch: the range weight between two guides of one dtype (uint8, float16 or float32) -- the target frame's layer at the centre, the
        neighbour frame's layer under the taps -- and the colour from the `neighbour` frame: returns W + its sums
        (mid_bilateral_layers_pair_accum)."""
        neighbour, target_layer, neighbour_layer = _img(neighbour), _img(target_layer), _img(neighbour_layer)
        fmt = _guide_fmt(_fmt_of(neighbour), [target_layer, neighbour_layer], "bilateral_layers_pair_accum")
        h, w = neighbour.shape[:2]
        W = np.ascontiguousarray(W, dtype=np.float32)
        d_in, d_n, d_w = self.upload(neighbour), self.upload(neighbour_layer), self.upload(W)
        d_t = d_n if target_layer is neighbour_layer else self.upload(target_layer)
        p = BilateralParams(w, h, sigma_s, sigma_c, radius, LAYOUT_TEXTURE, fmt)
        _check(lib.mid_bilateral_layers_pair_accum(self.handle, ctypes.byref(p), d_t.ptr, d_n.ptr, d_in.ptr, d_w.ptr, None),
               "mid_bilateral_layers_pair_accum")
        return self.download(d_w, (h, w, 8), np.float32)

    def bilateral_temporal(self, frames, k=0, first=0, count=None, radius=8, sigma_s=2.0, sigma_c=0.2, layers=None, out_dtype=None):
        """The bilateral over the frames t-k..t+k for `count` output frames, fused (mid_bilateral_temporal).
        layers: None (plain form: the frames guide themselves), or one list per frame of equally many (h, w, 4) guide
        layers, uint8, float16 or float32 and all of one dtype; out_dtype: None = float32, uint8 or float16."""
        frames = _same_frames(frames, "bilateral_temporal")
        n = len(frames)
        count = n - first if count is None else count
        h, w = frames[0].shape[:2]
        n_layers, flat = (0, None) if layers is None else _flat_layers(layers, n, h, w, "bilateral_temporal", _GUIDE_DTYPES)
        out_dtype = _out_dtype(False, out_dtype)
        out_fmt = {np.dtype(np.uint8): FMT_RGBA8, np.dtype(np.float16): FMT_RGBA16F, np.dtype(np.float32): FMT_RGBA32F}[out_dtype]
        d_fr = [self.upload(f) for f in frames]
        d_l = None if flat is None else [self.upload(l) for l in flat]
        d_out = [self.alloc(w * h * 4 * out_dtype.itemsize) for _ in range(max(count, 0))]
        tl = None if d_l is None else (ctypes.c_void_p * max(len(d_l), 1))(*[d.ptr for d in d_l])
        p = BilateralParams(w, h, sigma_s, sigma_c, radius, LAYOUT_TEXTURE, _guide_fmt(_fmt_of(frames[0]), flat or [], "bilateral_temporal"))
        _check(lib.mid_bilateral_temporal(self.handle, ctypes.byref(p), (ctypes.c_void_p * n)(*[d.ptr for d in d_fr]), tl, n_layers, n,
                                          k, first, count, (ctypes.c_void_p * max(len(d_out), 1))(*[d.ptr for d in d_out]), out_fmt, None),
               "mid_bilateral_temporal")
        return [self.download(d, (h, w, 4), out_dtype) for d in d_out]

    def bilateral_joint(self, frames, layers, sigmas=None, k=0, first=0, count=None, radius=8, sigma_s=2.0, sigma_c=0.2, out_dtype=None):
        """The joint (cross) bilateral over the frames t-k..t+k for `count` output frames (mid_bilateral_joint): one weight per
        tap, the product of the spatial term and one range term per guide layer.  layers: one list per frame of equally many
        (1..16) (h, w, 4) guide layers, uint8, float16 or float32 and all of one dtype; sigmas: one sigma per layer, or None for
        sigma_c in every layer; out_dtype: None = float32, uint8 or float16."""
        frames = _same_frames(frames, "bilateral_joint")
        n = len(frames)
        count = n - first if count is None else count
        h, w = frames[0].shape[:2]
        n_layers, flat = _flat_layers(layers, n, h, w, "bilateral_joint", _GUIDE_DTYPES)
        out_dtype = _out_dtype(False, out_dtype)
        out_fmt = {np.dtype(np.uint8): FMT_RGBA8, np.dtype(np.float16): FMT_RGBA16F, np.dtype(np.float32): FMT_RGBA32F}[out_dtype]
        d_fr = [self.upload(f) for f in frames]
        d_l = [self.upload(l) for l in flat]
        d_out = [self.alloc(w * h * 4 * out_dtype.itemsize) for _ in range(max(count, 0))]
        p = BilateralParams(w, h, sigma_s, sigma_c, radius, LAYOUT_TEXTURE, _guide_fmt(_fmt_of(frames[0]), flat, "bilateral_joint"))
        _check(lib.mid_bilateral_joint(self.handle, ctypes.byref(p), _layer_sigmas(sigmas, n_layers, "bilateral_joint"),
                                       (ctypes.c_void_p * n)(*[d.ptr for d in d_fr]),
                                       (ctypes.c_void_p * max(len(d_l), 1))(*[d.ptr for d in d_l]), n_layers, n, k, first, count,
                                       (ctypes.c_void_p * max(len(d_out), 1))(*[d.ptr for d in d_out]), out_fmt, None),
               "mid_bilateral_joint")
        return [self.download(d, (h, w, 4), out_dtype) for d in d_out]

    def atrous_joint(self, frame, layers, sigmas, passes=5, first_pass=0, color_sigma=0.0, out_dtype=None):
        """The edge-avoiding a-trous filter of one frame (mid_atrous_joint): `passes` passes of the 5x5 B3-spline kernel, pass i
        at step 2^i starting with i = first_pass, every tap weighed by all guide layers at once.  layers: 1..16 (h, w, 4) guide
        layers, uint8, float16 or float32 and all of one dtype; sigmas: one sigma per layer; color_sigma: 0 = no colour term;
        out_dtype: None = float32, uint8 or float16."""
        (frame,) = _same_frames([frame], "atrous_joint")
        h, w = frame.shape[:2]
        n_layers, flat = _flat_layers([layers], 1, h, w, "atrous_joint", _GUIDE_DTYPES)
        out_dtype = _out_dtype(False, out_dtype)
        p = AtrousParams(w, h, first_pass, passes, color_sigma, _guide_fmt(_fmt_of(frame), flat, "atrous_joint"))
        d_in = self.upload(frame)
        d_l = [self.upload(l) for l in flat]
        d_out = self.alloc(w * h * 4 * out_dtype.itemsize)
        nbytes = lib.mid_atrous_scratch_bytes(ctypes.byref(p))
        d_scratch = self.alloc(nbytes) if nbytes else None
        _check(lib.mid_atrous_joint(self.handle, ctypes.byref(p), _layer_sigmas(sigmas, n_layers, "atrous_joint"), d_in.ptr,
                                    (ctypes.c_void_p * max(len(d_l), 1))(*[d.ptr for d in d_l]), n_layers, d_out.ptr, _OUT_FMT[out_dtype],
                                    d_scratch.ptr if d_scratch else None, None), "mid_atrous_joint")
        return self.download(d_out, (h, w, 4), out_dtype)

    def atrous_joint_temporal(self, frames, layers, sigmas, k=2, first=0, count=None, passes=5, color_sigma=0.0, out_dtype=None):
        """The a-trous filter over the frames t-k..t+k for `count` output frames (mid_atrous_joint_temporal): pass 0 takes its
        taps from every frame of the window, the centre from frame t; passes 1.. are atrous_joint's on that estimate with frame
        t's layers.  layers: one list per frame of equally many (1..16) (h, w, 4) guide layers, uint8, float16 or float32 and all
        of one dtype; sigmas: one sigma per layer; color_sigma: 0 = no colour term; out_dtype: None = float32, uint8 or float16."""
        frames = _same_frames(frames, "atrous_joint_temporal")
        n = len(frames)
        count = n - first if count is None else count
        h, w = frames[0].shape[:2]
        n_layers, flat = _flat_layers(layers, n, h, w, "atrous_joint_temporal", _GUIDE_DTYPES)
        out_dtype = _out_dtype(False, out_dtype)
        p = AtrousParams(w, h, 0, passes, color_sigma, _guide_fmt(_fmt_of(frames[0]), flat, "atrous_joint_temporal"))
        d_fr = [self.upload(f) for f in frames]
        d_l = [self.upload(l) for l in flat]
        d_out = [self.alloc(w * h * 4 * out_dtype.itemsize) for _ in range(max(count, 0))]
        nbytes = lib.mid_atrous_scratch_bytes(ctypes.byref(p))
        d_scratch = self.alloc(nbytes) if nbytes else None
        _check(lib.mid_atrous_joint_temporal(self.handle, ctypes.byref(p), _layer_sigmas(sigmas, n_layers, "atrous_joint_temporal"),
                                             (ctypes.c_void_p * n)(*[d.ptr for d in d_fr]),
                                             (ctypes.c_void_p * max(len(d_l), 1))(*[d.ptr for d in d_l]), n_layers, n, k, first, count,
                                             (ctypes.c_void_p * max(len(d_out), 1))(*[d.ptr for d in d_out]), _OUT_FMT[out_dtype],
                                             d_scratch.ptr if d_scratch else None, None), "mid_atrous_joint_temporal")
        return [self.download(d, (h, w, 4), out_dtype) for d in d_out]

    def atrous_moments(self, frames, layers, sigmas, k=0, t=0):
        """The luminance variance estimate of output frame t over the frames t-k..t+k (mid_atrous_moments): a 7x7 neighbourhood in
        every frame of the window, every tap weighed by all guide layers at once.  layers: one list per frame of equally many
        (1..16) (h, w, 4) guide layers, uint8, float16 or float32 and all of one dtype; sigmas: one sigma per layer.  Returns the
        float32 plane (h, w)."""
        frames = _same_frames(frames, "atrous_moments")
        n = len(frames)
        h, w = frames[0].shape[:2]
        n_layers, flat = _flat_layers(layers, n, h, w, "atrous_moments", _GUIDE_DTYPES)
        p = AtrousMomentsParams(w, h, _guide_fmt(_fmt_of(frames[0]), flat, "atrous_moments"))
        d_fr = [self.upload(f) for f in frames]
        d_l = [self.upload(l) for l in flat]
        d_var = self.alloc(w * h * 4)
        _check(lib.mid_atrous_moments(self.handle, ctypes.byref(p), _layer_sigmas(sigmas, n_layers, "atrous_moments"),
                                      (ctypes.c_void_p * n)(*[d.ptr for d in d_fr]),
                                      (ctypes.c_void_p * max(len(d_l), 1))(*[d.ptr for d in d_l]), n_layers, n, k, t, d_var.ptr, None),
               "mid_atrous_moments")
        return self.download(d_var, (h, w), np.float32)

    def atrous_variance(self, frame, variance, layers, sigmas, passes=5, first_pass=0, sigma_lum=4.0, epsilon=1e-3, out_dtype=None,
                        return_variance=False):
        """The variance-guided a-trous filter of one frame (mid_atrous_variance): atrous_joint's passes with a luminance term whose
        width follows the per-pixel `variance` (a float32 (h, w) plane, atrous_moments' output or a renderer's own), which is
        filtered along with the colour.  sigma_lum: 0 = no luminance term.  return_variance: also return the variance plane of
        the last pass, as (frame, variance)."""
        (frame,) = _same_frames([frame], "atrous_variance")
        h, w = frame.shape[:2]
        variance = np.ascontiguousarray(variance, dtype=np.float32)
        if variance.shape != (h, w):
            raise ValueError(f"atrous_variance: the variance plane must be {(h, w)}, got {variance.shape}")
        n_layers, flat = _flat_layers([layers], 1, h, w, "atrous_variance", _GUIDE_DTYPES)
        out_dtype = _out_dtype(False, out_dtype)
        p = AtrousVarianceParams(w, h, first_pass, passes, sigma_lum, epsilon, _guide_fmt(_fmt_of(frame), flat, "atrous_variance"))
        d_in, d_vin = self.upload(frame), self.upload(variance)
        d_l = [self.upload(l) for l in flat]
        d_out = self.alloc(w * h * 4 * out_dtype.itemsize)
        d_vout = self.alloc(w * h * 4) if return_variance else None
        nbytes = lib.mid_atrous_variance_scratch_bytes(ctypes.byref(p))
        d_scratch = self.alloc(nbytes) if nbytes else None
        _check(lib.mid_atrous_variance(self.handle, ctypes.byref(p), _layer_sigmas(sigmas, n_layers, "atrous_variance"), d_in.ptr, d_vin.ptr,
                                       (ctypes.c_void_p * max(len(d_l), 1))(*[d.ptr for d in d_l]), n_layers, d_out.ptr, _OUT_FMT[out_dtype],
                                       d_vout.ptr if d_vout else None, d_scratch.ptr if d_scratch else None, None), "mid_atrous_variance")
        out = self.download(d_out, (h, w, 4), out_dtype)
        return (out, self.download(d_vout, (h, w), np.float32)) if return_variance else out

    def temporal_accumulate(self, frame, layers, prev_layers, sigmas, hist=None, motion=None, var_spatial=None, alpha=0.2,
                            alpha_moments=0.2, history_max=32, history_full=4, clip_lo=None, clip_hi=None):
        """One step of the recursive temporal accumulation (mid_temporal_accumulate): the history `hist` = (colour, state), two
        float32 (h, w, 4) planes of the previous step (state = (m1, m2, N, 0)), or None for no history, is reprojected by `motion`
        (float32 (h, w, 2), pixels: p was at p + motion(p); None = zero motion), weighed by the guide layers (`layers` of this frame
        against `prev_layers` of the previous one: 0..16 (h, w, 4) layers each, uint8, float16 or float32 and all of one dtype;
        prev_layers None = `layers`) and blended with `frame`.  var_spatial: a float32 (h, w) plane (atrous_moments at k = 0) or
        None.  clip_lo, clip_hi: two float32 (h, w, 4) planes (color_bounds of the frame, usually) to which the reprojected history
        is clipped before the blend (mid_temporal_accumulate_clip), or both None.
        Returns (colour, state, variance): float32 (h, w, 4), (h, w, 4) and (h, w)."""
        who = "temporal_accumulate"
        if (clip_lo is None) != (clip_hi is None):
            raise ValueError(f"{who}: clip_lo and clip_hi are one box: both or neither")
        (frame,) = _same_frames([frame], who)
        h, w = frame.shape[:2]
        layers = list(layers)
        prev_layers = layers if prev_layers is None else list(prev_layers)
        n_layers, flat = _flat_layers([layers, prev_layers], 2, h, w, who, _GUIDE_DTYPES)
        hc, hs = (None, None) if hist is None else hist
        planes = []
        for name, a, shape in (("hist[0]", hc, (h, w, 4)), ("hist[1]", hs, (h, w, 4)), ("motion", motion, (h, w, 2)), ("var_spatial", var_spatial, (h, w)),
                               ("clip_lo", clip_lo, (h, w, 4)), ("clip_hi", clip_hi, (h, w, 4))):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float32)
                if a.shape != shape:
                    raise ValueError(f"{who}: {name} must be {shape}, got {a.shape}")
                a = self.upload(a)
            planes.append(a)                                   # (the buffers live until the call has been downloaded)
        p_hc, p_hs, p_mv, p_vs, p_lo, p_hi = (d.ptr if d is not None else None for d in planes)
        p = TemporalAccumParams(w, h, alpha, alpha_moments, history_max, history_full, _guide_fmt(_fmt_of(frame), flat, who))
        d_in = self.upload(frame)
        d_l = [self.upload(l) for l in flat]
        d_col, d_st, d_var = self.alloc(w * h * 16), self.alloc(w * h * 16), self.alloc(w * h * 4)
        head = (self.handle, ctypes.byref(p), _layer_sigmas(sigmas, n_layers, who), d_in.ptr,
                (ctypes.c_void_p * max(n_layers, 1))(*[d.ptr for d in d_l[:n_layers]]),
                (ctypes.c_void_p * max(n_layers, 1))(*[d.ptr for d in d_l[n_layers:]]), n_layers, p_mv, p_hc, p_hs, p_vs)
        if clip_lo is None:
            _check(lib.mid_temporal_accumulate(*head, d_col.ptr, d_st.ptr, d_var.ptr, None), "mid_temporal_accumulate")
        else:
            _check(lib.mid_temporal_accumulate_clip(*head, p_lo, p_hi, d_col.ptr, d_st.ptr, d_var.ptr, None), "mid_temporal_accumulate_clip")
        return self.download(d_col, (h, w, 4), np.float32), self.download(d_st, (h, w, 4), np.float32), self.download(d_var, (h, w), np.float32)

    def _albedo_plane(self, albedo, shape, who):
        albedo = _img(albedo)
        if albedo.dtype not in [np.dtype(d) for d in _GUIDE_DTYPES] or albedo.shape != shape:
            raise ValueError(f"{who}: the albedo must be uint8 / float16 / float32 {shape}, got {albedo.dtype} {albedo.shape}")
        return albedo

    def demodulate(self, frame, albedo, floor=1e-3):
        """Illumination of a frame (mid_demodulate): RGB divided by max(albedo, floor), alpha unchanged.  frame: (h, w, 4) uint8,
        float16 or float32; albedo: (h, w, 4) uint8, float16 or float32, read as a guide layer is.  Returns float32 (h, w, 4)."""
        (frame,) = _same_frames([frame], "demodulate")
        h, w = frame.shape[:2]
        albedo = self._albedo_plane(albedo, (h, w, 4), "demodulate")
        p = AlbedoParams(w, h, floor, fmt_with_guide(_fmt_of(frame), _fmt_of(albedo)))
        d_in, d_a, d_out = self.upload(frame), self.upload(albedo), self.alloc(w * h * 16)
        _check(lib.mid_demodulate(self.handle, ctypes.byref(p), d_in.ptr, d_a.ptr, d_out.ptr, None), "mid_demodulate")
        return self.download(d_out, (h, w, 4), np.float32)

    def modulate(self, illum, albedo, floor=1e-3, out_dtype=None):
        """The colour of an illumination plane (mid_modulate): RGB times max(albedo, floor), alpha unchanged, in out_dtype (None =
        float32; uint8 and float16 with the rounding of pack_u8 / pack_f16).  illum: float32 (h, w, 4); albedo as for demodulate."""
        illum = _img(illum)
        if illum.dtype != np.float32:
            raise TypeError(f"modulate: the illumination must be float32, got {illum.dtype}")
        h, w = illum.shape[:2]
        albedo = self._albedo_plane(albedo, (h, w, 4), "modulate")
        out_dtype = _out_dtype(False, out_dtype)
        p = AlbedoParams(w, h, floor, fmt_with_guide(FMT_RGBA32F, _fmt_of(albedo)))
        d_in, d_a, d_out = self.upload(illum), self.upload(albedo), self.alloc(w * h * 4 * out_dtype.itemsize)
        _check(lib.mid_modulate(self.handle, ctypes.byref(p), d_in.ptr, d_a.ptr, d_out.ptr, _OUT_FMT[out_dtype], None), "mid_modulate")
        return self.download(d_out, (h, w, 4), out_dtype)

    def firefly_clamp(self, frame, radius=1, rank=1, gain=1.0, floor=0.0):
        """Firefly clamp and NaN repair of a frame (mid_firefly_clamp): a pixel whose luminance exceeds gain times the rank-th largest
        finite luminance of its (2 radius + 1)^2 neighbourhood (and floor) is scaled down to that limit, a pixel with a non-finite
        colour becomes a grey of the limit; alpha unchanged.  frame: (h, w, 4) uint8, float16 or float32.  Returns float32 (h, w, 4)."""
        (frame,) = _same_frames([frame], "firefly_clamp")
        _firefly_args(rank, radius, gain, floor, "firefly_clamp", off_allowed=False)
        h, w = frame.shape[:2]
        p = FireflyParams(w, h, radius, rank, gain, floor, _fmt_of(frame))
        d_in, d_out = self.upload(frame), self.alloc(w * h * 16)
        _check(lib.mid_firefly_clamp(self.handle, ctypes.byref(p), d_in.ptr, d_out.ptr, None), "mid_firefly_clamp")
        return self.download(d_out, (h, w, 4), np.float32)

    def color_bounds(self, frame, radius=1, gamma=1.0):
        """The neighbourhood colour box of a frame (mid_color_bounds): per pixel and colour channel mean -+ gamma standard deviations
        over the finite texels of the (2 radius + 1)^2 window, centre included; .w of both planes is the number of those texels
        (-Inf / +Inf and 0 where there is none).  frame: (h, w, 4) uint8, float16 or float32.  Returns (lo, hi), float32 (h, w, 4)."""
        (frame,) = _same_frames([frame], "color_bounds")
        radius, gamma = _clip_args(gamma, radius, "color_bounds", off_allowed=False)
        h, w = frame.shape[:2]
        p = ColorBoundsParams(w, h, radius, gamma, _fmt_of(frame))
        d_in, d_lo, d_hi = self.upload(frame), self.alloc(w * h * 16), self.alloc(w * h * 16)
        _check(lib.mid_color_bounds(self.handle, ctypes.byref(p), d_in.ptr, d_lo.ptr, d_hi.ptr, None), "mid_color_bounds")
        return self.download(d_lo, (h, w, 4), np.float32), self.download(d_hi, (h, w, 4), np.float32)

    def image_metrics(self, a, b, peak=1.0, eps=1e-2, ssim=True, want_map=False):
        """Full-reference quality metrics of a test image `a` against a reference `b` (mid_image_metrics, section a4n), over the
        pixels whose R, G and B are finite in both; alpha is ignored.  a, b: (h, w, 4) uint8, float16 or float32 of one shape, each
        with its own dtype.  peak: the data range (1 for unit-range frames); eps: relMSE's regulariser.  Returns a dict: n_valid,
        n_invalid, mse, mse_r, mse_g, mse_b, mae, max_abs, psnr, relmse, ssim (mid_image_metrics_derive's values; ssim is NaN with
        ssim=False), `sums` (the 16 raw float64 sums) and, with want_map, `map`: float32 (h, w), ssim per pixel, NaN where the pixel
        is not valid."""
        who = "image_metrics"
        a, b = _img(a), _img(b)
        for name, x in (("a", a), ("b", b)):
            if x.dtype not in [np.dtype(d) for d in _GUIDE_DTYPES]:
                raise ValueError(f"{who}: {name} must be uint8 / float16 / float32, got {x.dtype}")
        if a.shape != b.shape:
            raise ValueError(f"{who}: a is {a.shape} but b is {b.shape}: the two images must have one size")
        peak, eps, ssim, want_map = _metrics_args(peak, eps, ssim, want_map, who)
        h, w = a.shape[:2]
        p = ImageMetricsParams(w, h, _fmt_of(a), _fmt_of(b), peak, eps, int(ssim))
        d_a, d_b = self.upload(a), self.upload(b)
        d_work = self.alloc(lib.mid_image_metrics_workspace(w, h))
        d_map = self.alloc(w * h * 4) if want_map else None
        _check(lib.mid_image_metrics(self.handle, ctypes.byref(p), d_a.ptr, d_b.ptr, d_work.ptr, d_map.ptr if want_map else None, None),
               "mid_image_metrics")
        sums = self.download(d_work, (METRICS_N,), np.float64)
        out = metrics_derive(sums, peak, ssim)
        out["sums"] = sums
        if want_map:
            out["map"] = self.download(d_map, (h, w), np.float32)
        return out

    def guided_filter(self, frame, guide=None, radius=8, eps=1e-2, out_dtype=None):
        """The guided filter (mid_guided_filter, section a4o): inside every (2 radius + 1)^2 window the frame is fitted as an affine
        function of the guide's colour, and the averaged fit is evaluated at the pixel's own guide texel; alpha unchanged, a pixel
        with a non-finite colour (in the frame or in the guide) passes through.  frame, guide: (h, w, 4) uint8, float16 or float32 of
        one shape, each with its own dtype; guide=None: the frame guides itself.  eps: the regulariser, in squared guide units.
        Returns (h, w, 4) in out_dtype (None = float32; uint8 and float16 with the rounding of pack_u8 / pack_f16)."""
        who = "guided_filter"
        frame = _img(frame)
        if frame.dtype not in [np.dtype(d) for d in _GUIDE_DTYPES]:
            raise ValueError(f"{who}: the frame must be uint8 / float16 / float32, got {frame.dtype}")
        if guide is not None:
            guide = _img(guide)
            if guide.dtype not in [np.dtype(d) for d in _GUIDE_DTYPES]:
                raise ValueError(f"{who}: the guide must be uint8 / float16 / float32, got {guide.dtype}")
            if guide.shape != frame.shape:
                raise ValueError(f"{who}: the frame is {frame.shape} but the guide is {guide.shape}: the two must have one size")
        radius, eps = _guided_args(radius, eps, who)
        out_dtype = _guided_out_dtype(out_dtype, who)
        h, w = frame.shape[:2]
        p = GuidedParams(w, h, radius, eps, fmt_with_guide(_fmt_of(frame), _fmt_of(frame if guide is None else guide)))
        nbytes = ctypes.c_size_t()
        _check(lib.mid_guided_workspace(ctypes.byref(p), ctypes.byref(nbytes)), "mid_guided_workspace")
        d_in, d_g = self.upload(frame), None if guide is None else self.upload(guide)
        d_work, d_out = self.alloc(nbytes.value), self.alloc(w * h * 4 * out_dtype.itemsize)
        _check(lib.mid_guided_filter(self.handle, ctypes.byref(p), d_in.ptr, None if d_g is None else d_g.ptr, d_work.ptr, d_out.ptr,
                                     _OUT_FMT[out_dtype], None), "mid_guided_filter")
        return self.download(d_out, (h, w, 4), out_dtype)

    def median_filter(self, frame, layers=None, sigmas=None, radius=1, out_dtype=None):
        """The median of the (2 radius + 1)^2 window, per channel of r, g, b (mid_median_filter, section a4p); alpha unchanged.
        layers=None: the plain median.  Otherwise the lower weighted median under one weight per tap from all guide layers, the
        product of exp(-0.5 |G_l(p) - G_l(q)|^2 / sigma_l^2): 1..16 (h, w, 4) layers, uint8, float16 or float32 and all of one dtype,
        with one sigma per layer.  Texels that are not finite take no part, so a NaN pixel with valid neighbours is repaired.
        Returns (h, w, 4) in out_dtype (None = float32; uint8 and float16 with the rounding of pack_u8 / pack_f16)."""
        who = "median_filter"
        (frame,) = _same_frames([frame], who)
        h, w = frame.shape[:2]
        radius = _median_args(radius, layers, sigmas, who)
        n_layers, flat = (0, []) if layers is None else _flat_layers([layers], 1, h, w, who, _GUIDE_DTYPES)
        out_dtype = _guided_out_dtype(out_dtype, who)
        p = MedianParams(w, h, radius, _guide_fmt(_fmt_of(frame), flat, who))
        sg = None if layers is None else _layer_sigmas(sigmas, n_layers, who)
        d_in = self.upload(frame)
        d_l = [self.upload(l) for l in flat]
        d_out = self.alloc(w * h * 4 * out_dtype.itemsize)
        _check(lib.mid_median_filter(self.handle, ctypes.byref(p), sg, d_in.ptr,
                                     None if layers is None else (ctypes.c_void_p * max(len(d_l), 1))(*[d.ptr for d in d_l]), n_layers, d_out.ptr,
                                     _OUT_FMT[out_dtype], None), "mid_median_filter")
        return self.download(d_out, (h, w, 4), out_dtype)

    def sequence_median_pinned(self, hin, hout, w, h, fmt, hlayers=None, n_layers=0, sigmas=None, radius=1, first=0, count=None, overlap=True,
                               out_dtype=None):
        """mid_sequence_median on host pointers the caller already holds: nothing but the C call.  hin: all n frames of the sequence;
        hlayers: None (the plain median) or n * n_layers host pointers, frame-major (RGBA8, or what fmt_with_guide names in `fmt`);
        hout: `count` output buffers; sigmas: n_layers sigmas.  Returns (wall_ms of the whole call, kernel_ms, copy_ms)."""
        count = len(hin) - first if count is None else count
        return self._sequence_call("mid_sequence_median", "mid_sequence_median", MedianParams(w, h, radius, fmt), hin, hout, count,
                                   f"{count} outputs", overlap, layers=(hlayers, n_layers), plain=True, window=(first, count),
                                   out_dtype=(out_dtype,), sigmas=(None if hlayers is None else sigmas,))

    def sequence_median(self, frames, layers=None, sigmas=None, radius=1, first=0, count=None, overlap=True, pinned=True, pinned_out=True,
                        out_dtype=None):
        """Outputs [first, first+count) of an animation through the overlapped pipeline with the median as its compute stage
        (mid_sequence_median): output t is ctx.median_filter(frames[t], layers[t], sigmas, radius) in out_dtype.  layers: None, or one
        list of guide layers per frame.  pinned, pinned_out, out_dtype as for sequence_bilateral.
        Returns (outputs, (wall_ms, kernel_ms, copy_ms))."""
        who = "sequence_median"
        radius = _median_args(radius, layers, sigmas, who)
        out_dtype = _guided_out_dtype(out_dtype, who)
        frames = _same_frames(frames, who)
        if layers is not None:
            n_layers, _ = _flat_layers(layers, len(frames), frames[0].shape[0], frames[0].shape[1], who, _GUIDE_DTYPES)
            _layer_sigmas(sigmas, n_layers, who)
        return self._sequence_host(who, lambda hin, hout, w, h, fmt, hlayers, n_layers, count: self.sequence_median_pinned(
            hin, hout, w, h, fmt, hlayers, n_layers, sigmas, radius, first, count, overlap, out_dtype),
            frames, layers, _GUIDE_DTYPES, first, count, pinned, pinned_out, out_dtype, plain=True)

    def normalize(self, W):
        """normalize.comp."""
        W = np.ascontiguousarray(W, dtype=np.float32)
        h, w = W.shape[:2]
        d_w, d_out = self.upload(W), self.alloc(w * h * 16)
        p = NormalizeParams(w, h)
        _check(lib.mid_normalize(self.handle, ctypes.byref(p), d_w.ptr, d_out.ptr, None), "mid_normalize")
        return self.download(d_out, (h, w, 4), np.float32)

    def unpack_u8(self, u8, flavour=0):
        u8 = np.ascontiguousarray(u8, dtype=np.uint8)
        n = u8.size
        d_in, d_out = self.upload(u8), self.alloc(max(n * 4, 16))
        _check(lib.mid_unpack_u8(self.handle, d_in.ptr, n, flavour, d_out.ptr, None), "mid_unpack_u8")
        return self.download(d_out, u8.shape, np.float32)

    def pack_u8(self, f32):
        f32 = np.ascontiguousarray(f32, dtype=np.float32)
        n = f32.size
        d_in, d_out = self.upload(f32), self.alloc(max(n, 16))
        _check(lib.mid_pack_u8(self.handle, d_in.ptr, n, d_out.ptr, None), "mid_pack_u8")
        return self.download(d_out, f32.shape, np.uint8)

    def unpack_f16(self, f16):
        """binary16 -> float32, exact (mid_unpack_f16)."""
        f16 = np.ascontiguousarray(f16, dtype=np.float16)
        n = f16.size
        d_in, d_out = self.upload(f16), self.alloc(max(n * 4, 16))
        _check(lib.mid_unpack_f16(self.handle, d_in.ptr, n, d_out.ptr, None), "mid_unpack_f16")
        return self.download(d_out, f16.shape, np.float32)

    def pack_f16(self, f32):
        """float32 -> binary16, round to nearest even: the bits of np.float16(f32) (mid_pack_f16)."""
        f32 = np.ascontiguousarray(f32, dtype=np.float32)
        n = f32.size
        d_in, d_out = self.upload(f32), self.alloc(max(n * 2, 16))
        _check(lib.mid_pack_f16(self.handle, d_in.ptr, n, d_out.ptr, None), "mid_pack_f16")
        return self.download(d_out, f32.shape, np.float16)

    def nlm_multiframe(self, target, frames, overlap=True, hparam=0.5, search=(-7, 7), patch=(-3, 3)):
        """The reference's multi-frame mode: one target, neighbour frames streamed (mid_nlm_multiframe)."""
        target = _img(target)
        frames = _same_frames([target] + list(frames), "nlm_multiframe")[1:]
        h, w = target.shape[:2]
        out = np.empty((h, w, 4), np.float32)
        prm = NlmParams(w, h, hparam, search[0], search[1], patch[0], patch[1], _fmt_of(target))
        t = (ctypes.c_float * 3)()
        tbl = (ctypes.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        _check(lib.mid_nlm_multiframe(self.handle, ctypes.byref(prm), target.ctypes.data, tbl, len(frames),
                                      out.ctypes.data, 1 if overlap else 0, t), "mid_nlm_multiframe")
        return out, tuple(t)

    def _sequence_call(self, entry, where, prm, hin, hout, count, asked, overlap, layers=(), plain=False, window=(), out_dtype=(), sigmas=()):
        """What every sequence_*_pinned method does: check the buffer counts, build the pointer tables and make the C call
        entry(ctx, prm, [layer_sigma], frames, n, [layers, n_layers], [k, first, count], outputs, [out_format], overlap, timings).
        layers: () or (hlayers, n_layers), hlayers None being the form without layers where the method has one (plain);
        window: () or (k, first, count); out_dtype: () or (the outputs' dtype or None,); sigmas: () or (n_layers sigmas or None,);
        asked: how the method's ValueError names the outputs it was asked for."""
        n = len(hin)
        if len(hout) < count:
            raise ValueError(f"{asked}, {len(hout)} output buffers given")
        if layers and not (plain and layers[0] is None):
            hlayers, n_layers = layers
            if len(hlayers) != n * n_layers:
                raise ValueError(f"{n} frames x {n_layers} layers, {len(hlayers)} layer pointers given")
            layers = ((ctypes.c_void_p * max(len(hlayers), 1))(*hlayers), n_layers)
        out_fmt = [_OUT_FMT[_out_dtype(False, dt)] for dt in out_dtype]
        pre = [_layer_sigmas(sg, layers[1], where[len("mid_"):], "values of h" if "nlm" in entry else "sigmas") for sg in sigmas]
        t = (ctypes.c_float * 3)()
        # (the output table holds at least one entry, so that count = 0 still reaches the library's refusal)
        _check(getattr(lib, entry)(self.handle, ctypes.byref(prm), *pre, (ctypes.c_void_p * n)(*hin), n, *layers, *window,
                                   (ctypes.c_void_p * max(count, 1))(*hout[:max(count, 0)]), *out_fmt, 1 if overlap else 0, t), where)
        return tuple(t)

    def _sequence_host(self, who, call, frames, layers, dtypes, first, count, pinned, pinned_out, out_dtype, plain=False, inside=False):
        """What every host wrapper of the frame pipeline does: check the frames and the layers (dtypes: what the filter takes;
        plain: layers may be None, the form without layers), pin them and the outputs or borrow the NumPy arrays, make
        call(hin, hout, w, h, fmt, hlayers, n_layers, count) -- the method's own *_pinned -- and return (outputs, timings).
        inside: refuse an output range that leaves the sequence here (sequence_nlm) instead of in the library."""
        frames = _same_frames(frames, who)
        n = len(frames)
        count = n - first if count is None else count
        if inside and not (0 <= first and count >= 1 and first + count <= n):
            raise ValueError(f"outputs [{first}, {first + count}) are not inside the {n} frames given")
        h, w = frames[0].shape[:2]
        n_layers, flat = (0, None) if plain and layers is None else _flat_layers(layers, n, h, w, who, dtypes)
        out_shape = (h, w, 4)
        hin = hlay = hout = None
        try:
            hin = PinnedFrames(self, frames) if pinned else None
            hlay = PinnedFrames(self, flat) if pinned and flat else None
            hout = PinnedFrames(self, max(count, 1), w * h * 4 * out_dtype.itemsize) if pinned_out else None
            outs = None if pinned_out else [np.empty(out_shape, out_dtype) for _ in range(max(count, 0))]
            lptr = None if flat is None else (hlay.ptrs if hlay is not None else [lyr.ctypes.data for lyr in flat])
            t = call(hin.ptrs if pinned else [f.ctypes.data for f in frames], hout.ptrs if pinned_out else [o.ctypes.data for o in outs],
                     w, h, _guide_fmt(_fmt_of(frames[0]), flat or [], who), lptr, n_layers, count)
            return (outs if outs is not None else [hout.array(i, out_shape, out_dtype) for i in range(count)]), t
        finally:
            for b in (hin, hlay, hout):
                if b is not None:
                    b.free()

    def sequence_nlm_pinned(self, hin, hout, w, h, fmt, k=2, first=0, count=None, overlap=True, hparam=0.5,
                            search=(-7, 7), patch=(-3, 3), out_u8=False, out_dtype=None):
        """mid_sequence_nlm_range[_u8|_f16] on host pointers the caller already holds (PinnedFrames.ptrs): nothing but the C call,
        so a clock around it measures what a C caller sees.  out_dtype=np.float16 selects the RGBA16F outputs.
        Returns (wall_ms of the whole call, kernel_ms, copy_ms)."""
        count = len(hin) - first if count is None else count
        entry = "mid_sequence_nlm_range" + {FMT_RGBA8: "_u8", FMT_RGBA16F: "_f16", FMT_RGBA32F: ""}[_OUT_FMT[_out_dtype(out_u8, out_dtype)]]
        return self._sequence_call(entry, "mid_sequence_nlm_range", NlmParams(w, h, hparam, search[0], search[1], patch[0], patch[1], fmt),
                                   hin, hout, count, f"{count} outputs asked for", overlap, window=(k, first, count))

    def pipe_last_timeline(self, cap=4096):
        """mid_pipe_last_timeline: the device timeline of this context's last mid_sequence_nlm* / mid_sequence_bilateral call,
        from its own events.
        Returns (uploads, outputs): uploads = [(frame, start_ms, end_ms)], outputs = [(frame, kernel_start, kernel_end,
        download_start, download_end)], ms from the start of the call's first upload."""
        up, out = (ctypes.c_float * (2 * cap))(), (ctypes.c_float * (4 * cap))()
        nu, fu, no, fo = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(lib.mid_pipe_last_timeline(self.handle, cap, up, ctypes.byref(nu), ctypes.byref(fu), out, ctypes.byref(no),
                                          ctypes.byref(fo)), "mid_pipe_last_timeline")
        return ([(fu.value + i, up[2 * i], up[2 * i + 1]) for i in range(nu.value)],
                [(fo.value + j, out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]) for j in range(no.value)])

    def sequence_nlm(self, frames, k=2, overlap=True, hparam=0.5, search=(-7, 7), patch=(-3, 3), pinned=True,
                     first=0, count=None, out_u8=False, pinned_out=True, out_dtype=None):
        """Host frames in, host frames out through the overlapped pipeline (mid_sequence_nlm_range[_u8|_f16]).
        out_u8: outputs converted to RGBA8 on the device like the reference's read-back (src/main.cpp:97-103).
        out_dtype=np.float16: RGBA16F outputs, rounded to nearest even in the kernel's epilogue (the bits of np.float16 of the
        float32 outputs).  Input frames may be float32, uint8 or float16.
        pinned / pinned_out = False: the NumPy arrays themselves (pageable memory) are the sources / destinations, which
        the library moves through its bounce buffers (csrc/hostcopy.cpp).
        Returns (outputs for frames first..first+count-1, (wall_ms, kernel_ms, copy_ms))."""
        out_dtype = _out_dtype(out_u8, out_dtype)
        return self._sequence_host("sequence_nlm", lambda hin, hout, w, h, fmt, hlayers, n_layers, count: self.sequence_nlm_pinned(
            hin, hout, w, h, fmt, k, first, count, overlap, hparam, search, patch, out_dtype=out_dtype),
            frames, None, None, first, count, pinned, pinned_out, out_dtype, plain=True, inside=True)

    def sequence_bilateral_pinned(self, hin, hout, w, h, fmt, radius, sigma_s=2.0, sigma_c=0.2, layout="texture", hlayers=None,
                                  n_layers=0, overlap=True, out_dtype=None):
        """mid_sequence_bilateral on host pointers the caller already holds: nothing but the C call, so a clock around it
        measures what a C caller sees.  hlayers: None (plain bilateral) or len(hin) * n_layers host pointers, frame-major: RGBA8
        layers, or what fmt_with_guide(frames' format, layers' format) names in `fmt`.
        Returns (wall_ms of the whole call, kernel_ms, copy_ms)."""
        lay = {"texture": LAYOUT_TEXTURE, "linear": LAYOUT_LINEAR}[layout]
        return self._sequence_call("mid_sequence_bilateral", "mid_sequence_bilateral", BilateralParams(w, h, sigma_s, sigma_c, radius, lay, fmt),
                                   hin, hout, len(hin), f"{len(hin)} frames", overlap, layers=(hlayers, n_layers), plain=True, out_dtype=(out_dtype,))

    def sequence_bilateral(self, frames, radius, sigma_s=2.0, sigma_c=0.2, layout="texture", layers=None, overlap=True,
                           pinned=True, pinned_out=True, out_dtype=None):
        """A whole animation through the overlapped pipeline with the bilateral as its compute stage (mid_sequence_bilateral):
        output i is ctx.bilateral(frames[i]) -- or, with `layers`, ctx.bilateral_layers(frames[i], layers[i]) -- packed to
        out_dtype (None = float32; uint8 = the reference's read-back conversion, float16 = round to nearest even) by the kernel.
        layers: None, or one list per frame of equally many (h, w, 4) guide layers, uint8, float16 or float32 and all of one
        dtype (texture layout only).
        pinned / pinned_out = False: the NumPy arrays themselves (pageable memory) are the sources / destinations.
        Returns (outputs, (wall_ms, kernel_ms, copy_ms))."""
        out_dtype = _out_dtype(False, out_dtype)
        return self._sequence_host("sequence_bilateral", lambda hin, hout, w, h, fmt, hlayers, n_layers, count: self.sequence_bilateral_pinned(
            hin, hout, w, h, fmt, radius, sigma_s, sigma_c, layout, hlayers, n_layers, overlap, out_dtype),
            frames, layers, _GUIDE_DTYPES, 0, None, pinned, pinned_out, out_dtype, plain=True)

    def sequence_nlm_layers_pinned(self, hin, hout, w, h, fmt, hlayers, n_layers, overlap=True, hparam=0.5, search=(-7, 7),
                                   patch=(-3, 3), out_dtype=None):
        """mid_sequence_nlm_layers on host pointers the caller already holds: nothing but the C call, so a clock around it
        measures what a C caller sees.  hlayers: len(hin) * n_layers RGBA8 host pointers, frame-major.
        Returns (wall_ms of the whole call, kernel_ms, copy_ms)."""
        return self._sequence_call("mid_sequence_nlm_layers", "mid_sequence_nlm_layers",
                                   NlmParams(w, h, hparam, search[0], search[1], patch[0], patch[1], fmt), hin, hout, len(hin),
                                   f"{len(hin)} frames", overlap, layers=(hlayers, n_layers), out_dtype=(out_dtype,))

    def sequence_nlm_layers(self, frames, layers, overlap=True, hparam=0.5, search=(-7, 7), patch=(-3, 3), pinned=True,
                            pinned_out=True, out_dtype=None):
        """A whole animation through the overlapped pipeline with layer-guided NLM as its compute stage (mid_sequence_nlm_layers):
        output i is ctx.nlm_layers(frames[i], layers[i]) packed to out_dtype (None = float32; uint8 = the reference's read-back
        conversion, float16 = round to nearest even) by the kernel.
        layers: one list per frame of equally many uint8 (h, w, 4) guide layers.
        pinned / pinned_out = False: the NumPy arrays themselves (pageable memory) are the sources / destinations.
        Returns (outputs, (wall_ms, kernel_ms, copy_ms))."""
        out_dtype = _out_dtype(False, out_dtype)
        return self._sequence_host("sequence_nlm_layers", lambda hin, hout, w, h, fmt, hlayers, n_layers, count: self.sequence_nlm_layers_pinned(
            hin, hout, w, h, fmt, hlayers, n_layers, overlap, hparam, search, patch, out_dtype),
            frames, layers, (np.uint8,), 0, None, pinned, pinned_out, out_dtype)

    def sequence_nlm_layers_temporal_pinned(self, hin, hout, w, h, fmt, hlayers, n_layers, k, first=0, count=None, overlap=True,
                                            hparam=0.5, search=(-7, 7), patch=(-3, 3), out_dtype=None):
        """mid_sequence_nlm_layers_temporal on host pointers the caller already holds: nothing but the C call.  hin: all n frames of
        the sequence (only those of [first-k, first+count+k) are read); hlayers: n * n_layers RGBA8 host pointers, frame-major;
        hout: `count` output buffers.  Returns (wall_ms of the whole call, kernel_ms, copy_ms)."""
        count = len(hin) - first if count is None else count
        return self._sequence_call("mid_sequence_nlm_layers_temporal", "mid_sequence_nlm_layers_temporal",
                                   NlmParams(w, h, hparam, search[0], search[1], patch[0], patch[1], fmt), hin, hout, count,
                                   f"{count} outputs", overlap, layers=(hlayers, n_layers), window=(k, first, count), out_dtype=(out_dtype,))

    def sequence_nlm_layers_temporal(self, frames, layers, k=2, first=0, count=None, overlap=True, hparam=0.5, search=(-7, 7),
                                     patch=(-3, 3), pinned=True, pinned_out=True, out_dtype=None):
        """Outputs [first, first+count) of an animation through the overlapped pipeline with layer-guided NLM over the frames
        t-k..t+k as its compute stage (mid_sequence_nlm_layers_temporal): output t is ctx.nlm_layers_temporal(frames, layers, k)
        of frame t in out_dtype.  layers, pinned, pinned_out, out_dtype as for sequence_nlm_layers.
        Returns (outputs, (wall_ms, kernel_ms, copy_ms))."""
        out_dtype = _out_dtype(False, out_dtype)
        return self._sequence_host("sequence_nlm_layers_temporal", lambda hin, hout, w, h, fmt, hlayers, n_layers, count: self.sequence_nlm_layers_temporal_pinned(
            hin, hout, w, h, fmt, hlayers, n_layers, k, first, count, overlap, hparam, search, patch, out_dtype),
            frames, layers, (np.uint8,), first, count, pinned, pinned_out, out_dtype)

    def sequence_bilateral_temporal_pinned(self, hin, hout, w, h, fmt, k, first=0, count=None, radius=8, sigma_s=2.0, sigma_c=0.2,
                                           hlayers=None, n_layers=0, overlap=True, out_dtype=None):
        """mid_sequence_bilateral_temporal on host pointers the caller already holds: nothing but the C call.  hin: all n frames
        of the sequence (only those of [first-k, first+count+k) are read); hlayers: None (plain form) or n * n_layers host
        pointers, frame-major (RGBA8, or what fmt_with_guide names in `fmt`); hout: `count` output buffers.  Returns (wall_ms of the whole call, kernel_ms, copy_ms)."""
        count = len(hin) - first if count is None else count
        return self._sequence_call("mid_sequence_bilateral_temporal", "mid_sequence_bilateral_temporal",
                                   BilateralParams(w, h, sigma_s, sigma_c, radius, LAYOUT_TEXTURE, fmt), hin, hout, count,
                                   f"{count} outputs", overlap, layers=(hlayers, n_layers), plain=True, window=(k, first, count), out_dtype=(out_dtype,))

    def sequence_bilateral_temporal(self, frames, k=2, first=0, count=None, overlap=True, radius=8, sigma_s=2.0, sigma_c=0.2,
                                    layers=None, pinned=True, pinned_out=True, out_dtype=None):
        """Outputs [first, first+count) of an animation through the overlapped pipeline with the bilateral over the frames
        t-k..t+k as its compute stage (mid_sequence_bilateral_temporal): output t is ctx.bilateral_temporal(frames, k,
        layers=layers) of frame t in out_dtype.  layers, pinned, pinned_out, out_dtype as for sequence_bilateral.
        Returns (outputs, (wall_ms, kernel_ms, copy_ms))."""
        out_dtype = _out_dtype(False, out_dtype)
        return self._sequence_host("sequence_bilateral_temporal", lambda hin, hout, w, h, fmt, hlayers, n_layers, count: self.sequence_bilateral_temporal_pinned(
            hin, hout, w, h, fmt, k, first, count, radius, sigma_s, sigma_c, hlayers, n_layers, overlap, out_dtype),
            frames, layers, _GUIDE_DTYPES, first, count, pinned, pinned_out, out_dtype, plain=True)

    def sequence_bilateral_joint_pinned(self, hin, hout, w, h, fmt, hlayers, n_layers, sigmas=None, k=0, first=0, count=None, radius=8,
                                        sigma_s=2.0, sigma_c=0.2, overlap=True, out_dtype=None):
        """mid_sequence_bilateral_joint on host pointers the caller already holds: nothing but the C call.  hin, hlayers, hout as
        for sequence_bilateral_temporal_pinned (hlayers is required); sigmas: n_layers sigmas or None.
        Returns (wall_ms of the whole call, kernel_ms, copy_ms)."""
        count = len(hin) - first if count is None else count
        return self._sequence_call("mid_sequence_bilateral_joint", "mid_sequence_bilateral_joint",
                                   BilateralParams(w, h, sigma_s, sigma_c, radius, LAYOUT_TEXTURE, fmt), hin, hout, count,
                                   f"{count} outputs", overlap, layers=(hlayers, n_layers), window=(k, first, count), out_dtype=(out_dtype,),
                                   sigmas=(sigmas,))

    def sequence_bilateral_joint(self, frames, layers, sigmas=None, k=0, first=0, count=None, overlap=True, radius=8, sigma_s=2.0,
                                 sigma_c=0.2, pinned=True, pinned_out=True, out_dtype=None):
        """Outputs [first, first+count) of an animation through the overlapped pipeline with the joint bilateral over the frames
        t-k..t+k as its compute stage (mid_sequence_bilateral_joint): output t is ctx.bilateral_joint(frames, layers, sigmas, k)
        of frame t in out_dtype.  pinned, pinned_out, out_dtype as for sequence_bilateral.
        Returns (outputs, (wall_ms, kernel_ms, copy_ms))."""
        out_dtype = _out_dtype(False, out_dtype)
        return self._sequence_host("sequence_bilateral_joint", lambda hin, hout, w, h, fmt, hlayers, n_layers, count: self.sequence_bilateral_joint_pinned(
            hin, hout, w, h, fmt, hlayers, n_layers, sigmas, k, first, count, radius, sigma_s, sigma_c, overlap, out_dtype),
            frames, layers, _GUIDE_DTYPES, first, count, pinned, pinned_out, out_dtype)


    def sequence_nlm_joint_pinned(self, hin, hout, w, h, fmt, hlayers, n_layers, hs=None, k=0, first=0, count=None, overlap=True,
                                  hparam=0.5, search=(-7, 7), patch=(-3, 3), out_dtype=None):
        """mid_sequence_nlm_joint on host pointers the caller already holds: nothing but the C call.  hin, hlayers, hout as for
        sequence_nlm_layers_temporal_pinned; hs: n_layers values of h or None.
        Returns (wall_ms of the whole call, kernel_ms, copy_ms)."""
        count = len(hin) - first if count is None else count
        return self._sequence_call("mid_sequence_nlm_joint", "mid_sequence_nlm_joint",
                                   NlmParams(w, h, hparam, search[0], search[1], patch[0], patch[1], fmt), hin, hout, count,
                                   f"{count} outputs", overlap, layers=(hlayers, n_layers), window=(k, first, count), out_dtype=(out_dtype,),
                                   sigmas=(hs,))

    def sequence_nlm_joint(self, frames, layers, hs=None, k=0, first=0, count=None, overlap=True, hparam=0.5, search=(-7, 7),
                           patch=(-3, 3), pinned=True, pinned_out=True, out_dtype=None):
        """Outputs [first, first+count) of an animation through the overlapped pipeline with joint layer-guided NLM over the
        frames t-k..t+k as its compute stage (mid_sequence_nlm_joint): output t is ctx.nlm_joint(frames, layers, hs, k) of frame
        t in out_dtype.  layers, pinned, pinned_out, out_dtype as for sequence_nlm_layers.
        Returns (outputs, (wall_ms, kernel_ms, copy_ms))."""
        out_dtype = _out_dtype(False, out_dtype)
        return self._sequence_host("sequence_nlm_joint", lambda hin, hout, w, h, fmt, hlayers, n_layers, count: self.sequence_nlm_joint_pinned(
            hin, hout, w, h, fmt, hlayers, n_layers, hs, k, first, count, overlap, hparam, search, patch, out_dtype),
            frames, layers, (np.uint8,), first, count, pinned, pinned_out, out_dtype)


    def sequence_atrous_joint_pinned(self, hin, hout, w, h, fmt, hlayers, n_layers, sigmas, passes=5, first_pass=0, color_sigma=0.0,
                                     first=0, count=None, overlap=True, out_dtype=None):
        """mid_sequence_atrous_joint on host pointers the caller already holds: nothing but the C call.  hin: all n frames of the
        sequence; hlayers: n * n_layers host pointers, frame-major (RGBA8, or what fmt_with_guide names in `fmt`); hout: `count`
        output buffers; sigmas: n_layers sigmas.  Returns (wall_ms of the whole call, kernel_ms, copy_ms)."""
        count = len(hin) - first if count is None else count
        return self._sequence_call("mid_sequence_atrous_joint", "mid_sequence_atrous_joint",
                                   AtrousParams(w, h, first_pass, passes, color_sigma, fmt), hin, hout, count,
                                   f"{count} outputs", overlap, layers=(hlayers, n_layers), window=(first, count), out_dtype=(out_dtype,),
                                   sigmas=(sigmas,))

    def sequence_atrous_joint(self, frames, layers, sigmas, passes=5, first_pass=0, color_sigma=0.0, first=0, count=None, overlap=True,
                              pinned=True, pinned_out=True, out_dtype=None):
        """Outputs [first, first+count) of an animation through the overlapped pipeline with the a-trous filter as its compute
        stage (mid_sequence_atrous_joint): output t is ctx.atrous_joint(frames[t], layers[t], sigmas, passes, first_pass,
        color_sigma) in out_dtype.  pinned, pinned_out, out_dtype as for sequence_bilateral.
        Returns (outputs, (wall_ms, kernel_ms, copy_ms))."""
        out_dtype = _out_dtype(False, out_dtype)
        return self._sequence_host("sequence_atrous_joint", lambda hin, hout, w, h, fmt, hlayers, n_layers, count: self.sequence_atrous_joint_pinned(
            hin, hout, w, h, fmt, hlayers, n_layers, sigmas, passes, first_pass, color_sigma, first, count, overlap, out_dtype),
            frames, layers, _GUIDE_DTYPES, first, count, pinned, pinned_out, out_dtype)

    def sequence_guided_pinned(self, hin, hout, w, h, fmt, hguides=None, radius=8, eps=1e-2, first=0, count=None, overlap=True, out_dtype=None):
        """mid_sequence_guided on host pointers the caller already holds: nothing but the C call.  hin: all n frames of the sequence;
        hguides: None (the frames guide themselves) or n host pointers, one guide plane per frame (RGBA8, or what fmt_with_guide
        names in `fmt`); hout: `count` output buffers.  Returns (wall_ms of the whole call, kernel_ms, copy_ms)."""
        n = len(hin)
        count = n - first if count is None else count
        radius, eps = _guided_args(radius, eps, "sequence_guided")
        if len(hout) < count:
            raise ValueError(f"{count} outputs, {len(hout)} output buffers given")
        if hguides is not None and len(hguides) != n:
            raise ValueError(f"{n} frames, {len(hguides)} guide pointers given")
        prm = GuidedParams(w, h, radius, eps, fmt)
        t = (ctypes.c_float * 3)()
        _check(lib.mid_sequence_guided(self.handle, ctypes.byref(prm), (ctypes.c_void_p * n)(*hin), n,
                                       None if hguides is None else (ctypes.c_void_p * n)(*hguides), first, count,
                                       (ctypes.c_void_p * max(count, 1))(*hout[:max(count, 0)]), _OUT_FMT[_guided_out_dtype(out_dtype, "sequence_guided")],
                                       1 if overlap else 0, t), "mid_sequence_guided")
        return tuple(t)

    def sequence_guided(self, frames, guides=None, radius=8, eps=1e-2, first=0, count=None, overlap=True, pinned=True, out_dtype=None):
        """Outputs [first, first+count) of an animation through the overlapped pipeline with the guided filter as its compute stage
        (mid_sequence_guided): output t is ctx.guided_filter(frames[t], guides[t], radius, eps) in out_dtype.  guides: None, or one
        (h, w, 4) uint8 / float16 / float32 plane per frame, all of one dtype.  pinned=False: the NumPy arrays themselves (pageable
        memory) are the sources and destinations.  Returns (outputs, (wall_ms, kernel_ms, copy_ms))."""
        who = "sequence_guided"
        _guided_args(radius, eps, who)
        out_dtype = _guided_out_dtype(out_dtype, who)
        frames = [_img(f) for f in frames]
        for i, f in enumerate(frames):
            if f.dtype not in [np.dtype(d) for d in _GUIDE_DTYPES]:
                raise ValueError(f"{who}: frame {i} must be uint8 / float16 / float32, got {f.dtype}")
        if guides is not None and len(guides) != len(frames):
            raise ValueError(f"{who}: {len(guides)} guides for {len(frames)} frames")
        layers = None if guides is None else [[g] for g in guides]
        frames = _same_frames(frames, who)
        if layers is not None:
            _flat_layers(layers, len(frames), frames[0].shape[0], frames[0].shape[1], who, _GUIDE_DTYPES)
        return self._sequence_host(who, lambda hin, hout, w, h, fmt, hlayers, n_layers, count: self.sequence_guided_pinned(
            hin, hout, w, h, fmt, hlayers, radius, eps, first, count, overlap, out_dtype),
            frames, layers, _GUIDE_DTYPES, first, count, pinned, pinned, out_dtype, plain=True)

    def sequence_atrous_joint_temporal_pinned(self, hin, hout, w, h, fmt, hlayers, n_layers, sigmas, k=2, first=0, count=None, passes=5,
                                              color_sigma=0.0, overlap=True, out_dtype=None):
        """mid_sequence_atrous_joint_temporal on host pointers the caller already holds: nothing but the C call.  hin, hlayers,
        hout as for sequence_bilateral_joint_pinned; sigmas: n_layers sigmas.
        Returns (wall_ms of the whole call, kernel_ms, copy_ms)."""
        count = len(hin) - first if count is None else count
        return self._sequence_call("mid_sequence_atrous_joint_temporal", "mid_sequence_atrous_joint_temporal",
                                   AtrousParams(w, h, 0, passes, color_sigma, fmt), hin, hout, count,
                                   f"{count} outputs", overlap, layers=(hlayers, n_layers), window=(k, first, count), out_dtype=(out_dtype,),
                                   sigmas=(sigmas,))

    def sequence_atrous_joint_temporal(self, frames, layers, sigmas, k=2, first=0, count=None, passes=5, color_sigma=0.0, overlap=True,
                                       pinned=True, pinned_out=True, out_dtype=None):
        """Outputs [first, first+count) of an animation through the overlapped pipeline with the a-trous filter over the frames
        t-k..t+k as its compute stage (mid_sequence_atrous_joint_temporal): output t is ctx.atrous_joint_temporal(frames, layers,
        sigmas, k, passes=passes, color_sigma=color_sigma) of frame t in out_dtype.  pinned, pinned_out, out_dtype as for
        sequence_bilateral.  Returns (outputs, (wall_ms, kernel_ms, copy_ms))."""
        out_dtype = _out_dtype(False, out_dtype)
        return self._sequence_host("sequence_atrous_joint_temporal", lambda hin, hout, w, h, fmt, hlayers, n_layers, count: self.sequence_atrous_joint_temporal_pinned(
            hin, hout, w, h, fmt, hlayers, n_layers, sigmas, k, first, count, passes, color_sigma, overlap, out_dtype),
            frames, layers, _GUIDE_DTYPES, first, count, pinned, pinned_out, out_dtype)

    def sequence_atrous_variance_pinned(self, hin, hout, w, h, fmt, hlayers, n_layers, sigmas, k=2, first=0, count=None, passes=5,
                                        sigma_lum=4.0, epsilon=1e-3, overlap=True, out_dtype=None):
        """mid_sequence_atrous_variance on host pointers the caller already holds: nothing but the C call.  hin, hlayers, hout as
        for sequence_bilateral_joint_pinned; sigmas: n_layers sigmas; k: the window of the moments.
        Returns (wall_ms of the whole call, kernel_ms, copy_ms)."""
        count = len(hin) - first if count is None else count
        return self._sequence_call("mid_sequence_atrous_variance", "mid_sequence_atrous_variance",
                                   AtrousVarianceParams(w, h, 0, passes, sigma_lum, epsilon, fmt), hin, hout, count,
                                   f"{count} outputs", overlap, layers=(hlayers, n_layers), window=(k, first, count), out_dtype=(out_dtype,),
                                   sigmas=(sigmas,))

    def sequence_atrous_variance(self, frames, layers, sigmas, k=2, first=0, count=None, passes=5, sigma_lum=4.0, epsilon=1e-3,
                                 overlap=True, pinned=True, pinned_out=True, out_dtype=None):
        """Outputs [first, first+count) of an animation through the overlapped pipeline with the variance-guided a-trous filter
        as its compute stage (mid_sequence_atrous_variance): output t is ctx.atrous_variance(frames[t], ctx.atrous_moments(frames,
        layers, sigmas, k, t), layers[t], sigmas, passes, 0, sigma_lum, epsilon) in out_dtype.  pinned, pinned_out, out_dtype as
        for sequence_bilateral.  Returns (outputs, (wall_ms, kernel_ms, copy_ms))."""
        out_dtype = _out_dtype(False, out_dtype)
        return self._sequence_host("sequence_atrous_variance", lambda hin, hout, w, h, fmt, hlayers, n_layers, count: self.sequence_atrous_variance_pinned(
            hin, hout, w, h, fmt, hlayers, n_layers, sigmas, k, first, count, passes, sigma_lum, epsilon, overlap, out_dtype),
            frames, layers, _GUIDE_DTYPES, first, count, pinned, pinned_out, out_dtype)

    def sequence_atrous_recursive_pinned(self, hin, hout, w, h, fmt, hlayers, n_layers, sigmas, hmotion=None, feedback=1, warmup=16, first=0,
                                         count=None, passes=5, sigma_lum=4.0, epsilon=1e-3, alpha=0.2, alpha_moments=0.2, history_max=32,
                                         history_full=4, overlap=True, out_dtype=None, halbedo=None, albedo_floor=1e-3,
                                         firefly_rank=0, firefly_radius=1, firefly_gain=1.0, firefly_floor=0.0, clip_gamma=None, clip_radius=1):
        """mid_sequence_atrous_recursive[_albedo | _firefly | _clip] on host pointers the caller already holds: nothing but the C call.  hin,
        hlayers, hout as for sequence_atrous_variance_pinned; hmotion: one pointer per frame to a float32 (h, w, 2) plane, or None: zero
        motion; halbedo: one pointer per frame to an (h, w, 4) albedo plane in the layers' format, or None: no demodulation;
        firefly_rank 1..4: mid_firefly_clamp in front of the chain (0: the existing call); clip_gamma: the history is clipped to
        mid_color_bounds(clip_radius, clip_gamma) of the plane the accumulation reads (None: the existing call).
        Returns (wall_ms of the whole call, kernel_ms, copy_ms)."""
        n = len(hin)
        count = n - first if count is None else count
        firefly = _firefly_args(firefly_rank, firefly_radius, firefly_gain, firefly_floor, "sequence_atrous_recursive")
        clip = _clip_args(clip_gamma, clip_radius, "sequence_atrous_recursive")
        if len(hout) < count:
            raise ValueError(f"{count} outputs, {len(hout)} output buffers given")
        if len(hlayers) != n * n_layers:
            raise ValueError(f"{n} frames x {n_layers} layers, {len(hlayers)} layer pointers given")
        if hmotion is not None and len(hmotion) != n:
            raise ValueError(f"{n} frames, {len(hmotion)} motion planes given")
        if halbedo is not None and len(halbedo) != n:
            raise ValueError(f"{n} frames, {len(halbedo)} albedo planes given")
        ap = TemporalAccumParams(w, h, alpha, alpha_moments, history_max, history_full, fmt)
        vp = AtrousVarianceParams(w, h, 0, passes, sigma_lum, epsilon, fmt)
        t = (ctypes.c_float * 3)()
        head = (self.handle, ctypes.byref(ap), ctypes.byref(vp), _layer_sigmas(sigmas, n_layers, "sequence_atrous_recursive"), (ctypes.c_void_p * n)(*hin), n,
                (ctypes.c_void_p * max(len(hlayers), 1))(*hlayers), n_layers, None if hmotion is None else (ctypes.c_void_p * n)(*hmotion))
        tail = (feedback, warmup, first, count, (ctypes.c_void_p * max(count, 1))(*hout[:max(count, 0)]), _OUT_FMT[_out_dtype(False, out_dtype)],
                1 if overlap else 0, t)
        fp = None
        if firefly is not None:
            radius, rank, gain, floor = firefly
            fp = FireflyParams(w, h, radius, rank, gain, floor, fmt & 0xff)
        if clip is not None:
            cp = ColorBoundsParams(w, h, clip[0], clip[1], fmt & 0xff)
            _check(lib.mid_sequence_atrous_recursive_clip(*head, None if halbedo is None else (ctypes.c_void_p * n)(*halbedo), albedo_floor,
                                                          None if fp is None else ctypes.byref(fp), ctypes.byref(cp), *tail),
                   "mid_sequence_atrous_recursive_clip")
        elif fp is not None:
            _check(lib.mid_sequence_atrous_recursive_firefly(*head, None if halbedo is None else (ctypes.c_void_p * n)(*halbedo), albedo_floor,
                                                             ctypes.byref(fp), *tail), "mid_sequence_atrous_recursive_firefly")
        elif halbedo is None:
            _check(lib.mid_sequence_atrous_recursive(*head, *tail), "mid_sequence_atrous_recursive")
        else:
            _check(lib.mid_sequence_atrous_recursive_albedo(*head, (ctypes.c_void_p * n)(*halbedo), albedo_floor, *tail), "mid_sequence_atrous_recursive_albedo")
        return tuple(t)

    def sequence_atrous_recursive(self, frames, layers, sigmas, motion=None, feedback=1, warmup=16, first=0, count=None, passes=5, sigma_lum=4.0,
                                  epsilon=1e-3, alpha=0.2, alpha_moments=0.2, history_max=32, history_full=4, overlap=True, pinned=True,
                                  pinned_out=True, out_dtype=None, albedo=None, albedo_floor=1e-3, firefly_rank=0, firefly_radius=1,
                                  firefly_gain=1.0, firefly_floor=0.0, clip_gamma=None, clip_radius=1):
        """Outputs [first, first+count) of an animation through the pipeline with the recursive temporal accumulation as its compute
        stage (mid_sequence_atrous_recursive).  From frame s = max(0, first - warmup) on, per frame t: Vs = atrous_moments([frame], k=0),
        (colour, state, var) = temporal_accumulate(frame t, layers t, layers t-1, history, motion[t], Vs), output = atrous_variance(colour,
        var, layers t, passes); the next history is (colour, state) with feedback=0 and (the level after pass 0, state) with
        feedback=1.  motion: one float32 (h, w, 2) plane per frame, or None.  A run with first > 0 equals the whole run bit for bit
        only when warmup reaches frame 0.  pinned, pinned_out, out_dtype as for sequence_bilateral.
        albedo: one (h, w, 4) plane per frame in the layers' dtype, or None.  With it the chain runs on illumination
        (mid_sequence_atrous_recursive_albedo): frame t is demodulate(frame, albedo[t], albedo_floor) first, the passes return
        float32, and output t is modulate(that, albedo[t], albedo_floor, out_dtype); the histories hold illumination.
        firefly_rank 1..4 (0: off) puts firefly_clamp(frame, firefly_radius, firefly_rank, firefly_gain, firefly_floor) in front of
        the chain (mid_sequence_atrous_recursive_firefly), AFTER the demodulation: firefly_floor is in illumination units then.
        clip_gamma (None: off; finite and >= 0) clips the reprojected history of every frame to color_bounds(the plane the
        accumulation reads, clip_radius, clip_gamma) -- temporal_accumulate(..., clip_lo, clip_hi); mid_sequence_atrous_recursive_clip.
        Returns (outputs, (wall_ms, kernel_ms, copy_ms))."""
        out_dtype = _out_dtype(False, out_dtype)
        _firefly_args(firefly_rank, firefly_radius, firefly_gain, firefly_floor, "sequence_atrous_recursive")
        _clip_args(clip_gamma, clip_radius, "sequence_atrous_recursive")
        halb = None
        if albedo is not None:
            shape = np.asarray(frames[0]).shape[:2] + (4,)
            halb = [self._albedo_plane(a, shape, "sequence_atrous_recursive") for a in albedo]
            ldt = _img(layers[0][0]).dtype if len(layers) and len(layers[0]) else None
            if len(halb) != len(frames) or any(a.dtype != ldt for a in halb):
                raise ValueError(f"sequence_atrous_recursive: albedo must be one {shape} plane per frame in the layers' dtype ({ldt})")
        hmv = None
        if motion is not None:
            hmv = [np.ascontiguousarray(m, dtype=np.float32) for m in motion]
            shape = np.asarray(frames[0]).shape[:2] + (2,)
            if len(hmv) != len(frames) or any(m.shape != shape for m in hmv):
                raise ValueError(f"sequence_atrous_recursive: motion must be one {shape} plane per frame")
        pmv = palb = None
        try:
            pmv = PinnedFrames(self, hmv) if hmv is not None and pinned else None
            palb = PinnedFrames(self, halb) if halb is not None and pinned else None
            ptrs = None if hmv is None else (pmv.ptrs if pmv is not None else [m.ctypes.data for m in hmv])
            aptrs = None if halb is None else (palb.ptrs if palb is not None else [a.ctypes.data for a in halb])
            return self._sequence_host("sequence_atrous_recursive", lambda hin, hout, w, h, fmt, hlayers, n_layers, count: self.sequence_atrous_recursive_pinned(
                hin, hout, w, h, fmt, hlayers, n_layers, sigmas, ptrs, feedback, warmup, first, count, passes, sigma_lum, epsilon, alpha, alpha_moments,
                history_max, history_full, overlap, out_dtype, aptrs, albedo_floor, firefly_rank, firefly_radius, firefly_gain, firefly_floor,
                clip_gamma, clip_radius), frames, layers, _GUIDE_DTYPES, first, count, pinned, pinned_out, out_dtype)
        finally:
            for b in (pmv, palb):
                if b is not None:
                    b.free()


def _firefly_args(rank, radius, gain, floor, who, off_allowed=True):
    """The firefly keywords of a call, checked before any GPU work: None for rank 0 (the stage is off; the other three must then be
    their defaults), otherwise (radius, rank, gain, floor) in the ranges of mid_firefly_params."""
    if off_allowed and rank == 0:
        if (radius, gain, floor) != (1, 1.0, 0.0):
            raise ValueError(f"{who}: firefly_radius, firefly_gain and firefly_floor need firefly_rank 1..4 (it is 0: the stage is off)")
        return None
    if not isinstance(rank, (int, np.integer)) or isinstance(rank, bool) or not 1 <= rank <= 4:
        raise ValueError(f"{who}: the firefly rank must be an integer in 1..4, got {rank!r}")
    if not isinstance(radius, (int, np.integer)) or isinstance(radius, bool) or radius not in (1, 2):
        raise ValueError(f"{who}: the firefly radius must be 1 or 2, got {radius!r}")
    gain, floor = float(gain), float(floor)
    f32_max = float(np.finfo(np.float32).max)          # (the C side reads floats: a double beyond them would arrive as Inf)
    if not (0 < gain <= f32_max and float(np.float32(gain)) > 0):
        raise ValueError(f"{who}: the firefly gain must be finite and > 0, got {gain}")
    if not 0 <= floor <= f32_max:
        raise ValueError(f"{who}: the firefly floor must be finite and >= 0, got {floor}")
    return int(radius), int(rank), gain, floor


def _clip_args(gamma, radius, who, off_allowed=True):
    """The history-clip keywords of a call, checked before any GPU work: None for gamma None (the clip is off; the radius must then
    be its default), otherwise (radius, gamma) in the ranges of mid_color_bounds_params."""
    if off_allowed and gamma is None:
        if radius != 1:
            raise ValueError(f"{who}: clip_radius needs clip_gamma (it is None: the history clip is off)")
        return None
    if not isinstance(radius, (int, np.integer)) or isinstance(radius, bool) or radius not in (1, 2):
        raise ValueError(f"{who}: the clip radius must be 1 or 2, got {radius!r}")
    if gamma is None or isinstance(gamma, bool):
        raise ValueError(f"{who}: the clip gamma must be a number, finite and >= 0, got {gamma!r}")
    gamma = float(gamma)
    if not 0 <= gamma <= float(np.finfo(np.float32).max):      # (the C side reads floats: a double beyond them would arrive as Inf)
        raise ValueError(f"{who}: the clip gamma must be finite and >= 0, got {gamma}")
    return int(radius), gamma


def _metrics_args(peak, eps, ssim, want_map, who):
    """The keywords of image_metrics, checked before any GPU work: (peak, eps, ssim, want_map) in the ranges of
    mid_image_metrics_params."""
    f32_max = float(np.finfo(np.float32).max)          # (the C side reads floats: a double beyond them would arrive as Inf)
    for name, v in (("peak", peak), ("eps", eps)):
        if v is None or isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{who}: {name} must be a number, finite and > 0, got {v!r}")
        if not (0 < float(v) <= f32_max and float(np.float32(v)) > 0):
            raise ValueError(f"{who}: {name} must be finite and > 0, got {float(v)}")
    if not isinstance(ssim, (bool, np.bool_)) or not isinstance(want_map, (bool, np.bool_)):
        raise ValueError(f"{who}: ssim and want_map must be True or False, got {ssim!r} and {want_map!r}")
    if want_map and not ssim:
        raise ValueError(f"{who}: want_map needs ssim (it is False: no SSIM is computed)")
    return float(np.float32(peak)), float(np.float32(eps)), bool(ssim), bool(want_map)


def _guided_args(radius, eps, who):
    """The keywords of guided_filter, checked before any GPU work: (radius, eps) in the ranges of mid_guided_params."""
    if not isinstance(radius, (int, np.integer)) or isinstance(radius, bool) or not 1 <= radius <= 16:
        raise ValueError(f"{who}: the radius must be an integer in 1..16, got {radius!r}")
    if eps is None or isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)):
        raise ValueError(f"{who}: eps must be a number, finite and > 0, got {eps!r}")
    if not (0 < float(eps) <= float(np.finfo(np.float32).max) and float(np.float32(eps)) > 0):   # (the C side reads a float)
        raise ValueError(f"{who}: eps must be finite and > 0, got {float(eps)}")
    return int(radius), float(np.float32(eps))


def _median_args(radius, layers, sigmas, who):
    """The keywords of median_filter, checked before any GPU work: the radius of mid_median_params; sigmas come with layers, and
    layers with sigmas."""
    if not isinstance(radius, (int, np.integer)) or isinstance(radius, bool) or not 1 <= radius <= 3:
        raise ValueError(f"{who}: the radius must be an integer in 1..3, got {radius!r}")
    if layers is None and sigmas is not None:
        raise ValueError(f"{who}: sigmas without layers (the plain median takes neither)")
    if layers is not None and sigmas is None:
        raise ValueError(f"{who}: layers without sigmas (one sigma per layer)")
    return int(radius)


def _guided_out_dtype(out_dtype, who):
    dt = np.dtype(np.float32 if out_dtype is None else out_dtype)
    if dt not in _OUT_FMT:
        raise ValueError(f"{who}: out_dtype must be uint8, float16 or float32, got {dt}")
    return dt


def metrics_derive(sums, peak=1.0, ssim=True):
    """mid_image_metrics_derive: the derived values of 16 raw sums as a dict.  Host-only (no GPU)."""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    if sums.shape != (METRICS_N,):
        raise ValueError(f"metrics_derive: sums must be {METRICS_N} float64 values, got {sums.shape}")
    p = ImageMetricsParams(0, 0, 0, 0, peak, 1.0, int(bool(ssim)))
    r = ImageMetricsResult()
    _check(lib.mid_image_metrics_derive(sums.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(p), ctypes.byref(r)),
           "mid_image_metrics_derive")
    return {name: getattr(r, name) for name, _ in ImageMetricsResult._fields_}


def _layer_sigmas(sigmas, n_layers, who, noun="sigmas"):
    """The layer_sigma argument of the joint bilateral (layer_h of joint NLM, noun="values of h"): None, or a C array of n_layers floats."""
    if sigmas is None:
        return None
    sigmas = [float(s) for s in sigmas]
    if len(sigmas) != n_layers:
        raise ValueError(f"{who}: {len(sigmas)} {noun} for {n_layers} layers")
    return (ctypes.c_float * max(n_layers, 1))(*sigmas)


def _flat_layers(layers, n, h, w, who, dtypes=(np.uint8,)):
    """(layers per frame, the frames' (h, w, 4) guide layers as one frame-major list) of one list of layers per frame.  dtypes: what
    the filter takes -- uint8 alone (layer-guided NLM), or uint8 / float16 / float32 (the bilateral family); all layers of a call
    share one of them."""
    if len(layers) != n:
        raise ValueError(f"{who}: {len(layers)} layer lists for {n} frames")
    n_layers = len(layers[0])
    flat = []
    for i, ls in enumerate(layers):
        if len(ls) != n_layers:
            raise ValueError(f"{who}: frame {i} has {len(ls)} layers, frame 0 has {n_layers}")
        for lyr in ls:
            lyr = _img(lyr)
            if lyr.dtype not in [np.dtype(d) for d in dtypes] or lyr.shape != (h, w, 4):
                raise ValueError(f"{who}: the layers of frame {i} must be {' / '.join(np.dtype(d).name for d in dtypes)} {(h, w, 4)}, "
                                 f"got {lyr.dtype} {lyr.shape}")
            if flat and lyr.dtype != flat[0].dtype:
                raise ValueError(f"{who}: all guide layers of a call share one dtype: layer 0 of frame 0 is {flat[0].dtype}, "
                                 f"a layer of frame {i} is {lyr.dtype}")
            flat.append(lyr)
    return n_layers, flat


def _out_dtype(out_u8, out_dtype):
    """Output dtype of the frame pipeline: out_u8=True is uint8; otherwise out_dtype (None = float32; float16 allowed)."""
    if out_u8:
        if out_dtype is not None and np.dtype(out_dtype) != np.uint8:
            raise ValueError(f"out_u8=True and out_dtype={out_dtype} contradict each other")
        return np.dtype(np.uint8)
    dt = np.dtype(np.float32 if out_dtype is None else out_dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float16), np.dtype(np.uint8)):
        raise TypeError(f"sequence_nlm: out_dtype must be float32, float16 or uint8, got {dt}")
    return dt


class Recording:
    """A recorded sequence of kernel-level calls (mid_record_begin / mid_record_end / mid_recording_submit, csrc/recording.cpp)."""

    def __init__(self, ctx, stream=None):
        self.ctx, self.stream, self.handle = ctx, stream, None

    def __enter__(self):
        _check(lib.mid_record_begin(self.ctx.handle, self.stream), "mid_record_begin")
        return self

    def __exit__(self, exc_type, exc, tb):
        h = ctypes.c_void_p()
        rc = lib.mid_record_end(self.ctx.handle, self.stream, ctypes.byref(h))      # (always: the stream must leave capture mode)
        if exc_type is None:
            _check(rc, "mid_record_end")
            self.handle = h
        elif rc == 0:
            lib.mid_recording_destroy(h)
        return False

    def submit(self, stream=None):
        if self.handle is None:
            raise ValueError("the recording was not completed")
        _check(lib.mid_recording_submit(self.handle, stream), "mid_recording_submit")

    def info(self):
        n, k = ctypes.c_int(), ctypes.c_int()
        _check(lib.mid_recording_info(self.handle, ctypes.byref(n), ctypes.byref(k)), "mid_recording_info")
        return n.value, k.value

    def close(self):
        if self.handle is not None:
            lib.mid_recording_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


class PinnedFrames:
    """Page-locked host buffers (mid_alloc_host): the DMA source / destination of the frame pipeline, as the reference's
    mapped staging buffer is (src/main.cpp:247-275).  PinnedFrames(ctx, frames) copies the frames in; PinnedFrames(ctx, n,
    nbytes) allocates n empty buffers."""

    def __init__(self, ctx, frames_or_n, nbytes=None):
        self.ctx, self.ptrs = ctx, []
        frames = None if nbytes is not None else [np.ascontiguousarray(f) for f in frames_or_n]
        sizes = [nbytes] * int(frames_or_n) if frames is None else [f.nbytes for f in frames]
        self.nbytes = sizes[0] if sizes else 0
        try:
            for i, sz in enumerate(sizes):
                p = ctypes.c_void_p()
                _check(lib.mid_alloc_host(ctx.handle, sz, ctypes.byref(p)), "mid_alloc_host")
                self.ptrs.append(p.value)
                if frames is not None:
                    ctypes.memmove(p.value, frames[i].ctypes.data, sz)
        except Exception:
            self.free()
            raise

    def array(self, i, shape, dtype):
        out = np.empty(shape, dtype)
        ctypes.memmove(out.ctypes.data, self.ptrs[i], out.nbytes)
        return out

    def free(self):
        for p in self.ptrs:
            if self.ctx.handle:
                lib.mid_free_host(self.ctx.handle, p)
        self.ptrs = []


# ---- an animation sharded over GPUs: the C++ RCCL path (csrc/sharded.cpp) ----------------------------------------
COMM_ID_BYTES = 128


def shard_block(n_frames, world, rank):
    """(start, count) of rank's contiguous frame block (mid_shard_block) -- host only."""
    a, b = ctypes.c_int(), ctypes.c_int()
    _check(lib.mid_shard_block(n_frames, world, rank, ctypes.byref(a), ctypes.byref(b)), "mid_shard_block")
    return a.value, b.value


def shard_halo_plan(n_frames, world, k, rank):
    """(recv, send): lists of (peer rank, global frame id) in the order csrc/sharded.cpp issues them -- host only."""
    cap = 2 * max(k, 1) * max(world, 1) + 4 * max(k, 1) + 8
    arr = [(ctypes.c_int * cap)() for _ in range(4)]
    nr, ns = ctypes.c_int(), ctypes.c_int()
    _check(lib.mid_shard_halo_plan(n_frames, world, k, rank, cap, arr[0], arr[1], ctypes.byref(nr), arr[2], arr[3], ctypes.byref(ns)),
           "mid_shard_halo_plan")
    return ([(arr[0][i], arr[1][i]) for i in range(nr.value)], [(arr[2][i], arr[3][i]) for i in range(ns.value)])


def shard_launch_plan(n_frames, world, k, rank):
    """[(phase, w_lo, w_hi, first, count, out_offset)] like sharding.block_launch_plan, from the C++ side -- host only."""
    rows = (ctypes.c_int * (6 * 8))()
    n = ctypes.c_int()
    _check(lib.mid_shard_launch_plan(n_frames, world, k, rank, 8, rows, ctypes.byref(n)), "mid_shard_launch_plan")
    return [("interior" if rows[6 * i] else "boundary",) + tuple(rows[6 * i + 1:6 * i + 6]) for i in range(n.value)]


def comm_unique_id():
    """ncclGetUniqueId through the C-ABI: 128 bytes rank 0 hands to the other ranks (file, MPI, torch.distributed)."""
    buf = (ctypes.c_uint8 * COMM_ID_BYTES)()
    _check(lib.mid_comm_unique_id(buf), "mid_comm_unique_id")
    return bytes(buf)


def comm_create_all(ctxs):
    """One process, one rank per context (mid_comm_create_all = ncclCommInitAll): the list of Comm objects, rank i on ctxs[i]."""
    world = len(ctxs)
    tbl = (ctypes.c_void_p * world)(*[c.handle for c in ctxs])
    out = (ctypes.c_void_p * world)()
    _check(lib.mid_comm_create_all(tbl, world, out), "mid_comm_create_all")
    return [Comm(ctxs[i], None, i, world, _handle=ctypes.c_void_p(out[i])) for i in range(world)]


class Comm:
    """One rank of an RCCL communicator bound to a Context (mid_comm_create): one process per GPU."""

    def __init__(self, ctx, unique_id, rank, world, _handle=None):
        self.ctx, self.rank, self.world = ctx, rank, world
        if _handle is not None:                      # made by comm_create_all
            self.handle = _handle
            return
        h = ctypes.c_void_p()
        idb = (ctypes.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        _check(lib.mid_comm_create(ctx.handle, idb, rank, world, ctypes.byref(h)), "mid_comm_create")
        self.handle = h

    def close(self):
        if self.handle:
            lib.mid_comm_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def abort(self):
        """ncclCommAbort: the way out of a collective a rank could not enter; the handle then only accepts close()."""
        _check(lib.mid_comm_abort(self.handle), "mid_comm_abort")

    def reserve(self, max_frame_bytes, k):
        """Allocate the 2k halo receive buffers up front (mid_comm_reserve)."""
        _check(lib.mid_comm_reserve(self.handle, int(max_frame_bytes), int(k)), "mid_comm_reserve")

    def loopback(self, src_ptr, dst_ptr, nbytes, stream=None):
        _check(lib.mid_comm_loopback(self.handle, src_ptr, dst_ptr, nbytes, stream), "mid_comm_loopback")

    def last_loopback(self):
        """(start ms, end ms) of the last loopback's send+receive group on the exchange stream, from the moment the caller's
        stream reached the call (mid_comm_last_loopback; waits for it)."""
        t = (ctypes.c_float * 2)()
        _check(lib.mid_comm_last_loopback(self.handle, t), "mid_comm_last_loopback")
        return float(t[0]), float(t[1])

    def nlm_temporal_sharded_dev(self, block_ptrs, out_ptrs, w, h, n_frames, k, hparam, search, patch, fmt, stream=None):
        """This rank's block (device pointers, in order) -> its outputs; halo over RCCL, interior launches meanwhile."""
        _, count = shard_block(n_frames, self.world, self.rank)
        if len(block_ptrs) != count or len(out_ptrs) != count:
            raise ValueError(f"rank {self.rank} owns {count} frames, got {len(block_ptrs)} inputs / {len(out_ptrs)} outputs")
        p = NlmParams(w, h, hparam, search[0], search[1], patch[0], patch[1], fmt)
        fr = (ctypes.c_void_p * max(count, 1))(*block_ptrs)
        ou = (ctypes.c_void_p * max(count, 1))(*out_ptrs)
        _check(lib.mid_nlm_temporal_sharded(self.handle, ctypes.byref(p), fr, n_frames, k, ou, stream), "mid_nlm_temporal_sharded")

    def last_exchange(self):
        """(bytes received, bytes sent, exchange ms) of the last sharded call; waits for that exchange."""
        a, b, ms = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_float()
        _check(lib.mid_comm_last_exchange(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(ms)), "mid_comm_last_exchange")
        return a.value, b.value, ms.value

    def last_timeline(self):
        """Device timeline of the last sharded call (mid_comm_last_timeline; waits for the call), ms from its first event:
        dict(exchange_start, exchange_end, interior_end, end, halo_hidden_frac).  halo_hidden_frac is the share of the
        exchange that ran while interior launches were still executing (None when nothing was exchanged)."""
        t = (ctypes.c_float * 4)()
        _check(lib.mid_comm_last_timeline(self.handle, t), "mid_comm_last_timeline")
        x0, x1, i1, end = (float(v) for v in t)
        hidden = None
        if x1 > x0:
            hidden = max(0.0, min(1.0, (min(x1, i1) - x0) / (x1 - x0)))
        return {"exchange_start_ms": x0, "exchange_end_ms": x1, "interior_end_ms": i1, "end_ms": end, "halo_hidden_frac": hidden}

    def last_issue_order(self):
        """'X' exchange group, 'I' interior launch, 'W' wait for the exchange, 'B' boundary launch -- in host issue order."""
        buf = ctypes.create_string_buffer(64)
        _check(lib.mid_comm_last_issue_order(self.handle, buf, 64), "mid_comm_last_issue_order")
        return buf.value.decode()

    def stream_priority(self):
        """(priority of the exchange stream, least, greatest) -- numerically lower is higher."""
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(lib.mid_comm_stream_priority(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "mid_comm_stream_priority")
        return a.value, b.value, c.value

    def boundary_priority(self):
        """Priorities of the two boundary streams (the device's lowest: a pool of hardware queues of their own)."""
        pr = (ctypes.c_int * 2)()
        _check(lib.mid_comm_boundary_priority(self.handle, pr), "mid_comm_boundary_priority")
        return pr[0], pr[1]

    def rccl_info(self):
        """(ncclCommCount, ncclCommUserRank, ncclGetVersion) as RCCL reports them; -1 where the loaded library lacks the call."""
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(lib.mid_comm_rccl_info(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "mid_comm_rccl_info")
        return a.value, b.value, c.value
