// albedo.hip -- albedo demodulation and modulation (include/mi_denoise.h, section a4k): SVGF filters ILLUMINATION, the radiance
// divided by the surface albedo, and multiplies the albedo back at the end.
//
// Per pixel, per channel c in {R, G, B}, A = the albedo texel read as a guide texel (IEEE values, u8 as the correctly rounded c / 255):
//   d_c = fmaxf(A_c, floor)            a NaN or negative albedo gives floor
//   demodulate   I_c = C_c / d_c       one IEEE division; C widened as a4i widens a frame; RGBA32F out
//   modulate     O_c = I_c * d_c       one multiplication; out in out_format through store_out
//   alpha passes through in both.
//
// Kernel class: pointwise.hip's -- HBM-bound, one pixel per lane (a 16 / 8 / 4-byte load of the frame and one of the albedo),
// grid-stride with the index arithmetic in size_t, the formats run-time wave-uniform values, no LDS, no scratch.  The passes are
// pointwise, so neither pointer is __restrict__: demodulate and modulate may run exactly in place on an RGBA32F plane.
#include "common.hpp"
#include <cmath>

namespace mid {

namespace {

// One texel at flat index idx, the format a run-time (wave-uniform) value: restated from atrous_variance.hip, which keeps its text.
__device__ __forceinline__ float4 load_texel(const void *img, int fmt, size_t idx)
{
    if (fmt == MID_FMT_RGBA8) return decode_rgba8(((const uint32_t *)img)[idx]);
    if (fmt == MID_FMT_RGBA16F) return decode_rgba16f(((const uint2 *)img)[idx]);
    return ((const float4 *)img)[idx];
}

__global__ __launch_bounds__(256) void demodulate_kernel(const void *in, const void *albedo, float4 *out, size_t npix, int fmt, int gfmt, float floor_)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        const float4 c = load_texel(in, fmt, i);
        const float4 a = load_texel(albedo, gfmt, i);
        out[i] = make_float4(c.x / fmaxf(a.x, floor_), c.y / fmaxf(a.y, floor_), c.z / fmaxf(a.z, floor_), c.w);
    }
}

__global__ __launch_bounds__(256) void modulate_kernel(const float4 *in, const void *albedo, void *out, size_t npix, int gfmt, int out_fmt, float floor_)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        const float4 c = in[i];
        const float4 a = load_texel(albedo, gfmt, i);
        store_out(out, i, out_fmt, make_float4(c.x * fmaxf(a.x, floor_), c.y * fmaxf(a.y, floor_), c.z * fmaxf(a.z, floor_), c.w));
    }
}

// pointwise.hip's launch shape: at most 8 workgroups per CU, the stride loop takes the rest
unsigned stream_grid(mid_ctx *ctx, size_t n)
{
    const size_t want = (n + 255) / 256, cap = (size_t)ctx->cu_count * 8;
    return (unsigned)(want < cap ? (want ? want : 1) : cap);
}

bool ranges_overlap(const void *p, size_t np, const void *q, size_t nq)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return np && nq && a < b + nq && b < a + np;
}

bool texel_aligned(int fmt, const void *p) { return ((uintptr_t)p & (fmt_bytes(fmt) - 1)) == 0; }

}  // namespace

// What both entry points and the sequence check before their pointers: the size, the floor and the format word.
int albedo_check(const mid_albedo_params *p, const char *who)
{
    MID_REQUIRE(p != nullptr, "%s: params is NULL", who);
    MID_REQUIRE(p->width > 0 && p->height > 0, "%s: bad size %dx%d", who, p->width, p->height);
    MID_REQUIRE((long)p->width * p->height < (1l << 30), "%s: image too large", who);
    MID_REQUIRE(std::isfinite(p->floor) && p->floor > 0.f, "%s: floor %g must be finite and > 0", who, (double)p->floor);
    MID_REQUIRE((p->format & ~0xffff) == 0 && fmt_known(fmt_frames(p->format)), "%s: unknown format %d", who, p->format);
    MID_REQUIRE(fmt_guide(p->format) >= 0, "%s: unknown guide-layer format code %d in format 0x%x", who, p->format >> 8, p->format);
    return MID_OK;
}

int demodulate_out(mid_ctx *ctx, const mid_albedo_params *p, const void *in, const void *albedo, mid_pixel *out, hipStream_t s)
{
    const size_t npix = (size_t)p->width * p->height;
    hipLaunchKernelGGL(demodulate_kernel, dim3(stream_grid(ctx, npix)), dim3(256), 0, s, in, albedo, (float4 *)out, npix, fmt_frames(p->format),
                       fmt_guide(p->format), p->floor);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

int modulate_out(mid_ctx *ctx, const mid_albedo_params *p, const mid_pixel *in, const void *albedo, void *out, int out_fmt, hipStream_t s)
{
    const size_t npix = (size_t)p->width * p->height;
    hipLaunchKernelGGL(modulate_kernel, dim3(stream_grid(ctx, npix)), dim3(256), 0, s, (const float4 *)in, albedo, out, npix, fmt_guide(p->format), out_fmt,
                       p->floor);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

// The pointer checks the two entry points share: in_fmt / out_fmt are the texel formats of `in` and `out`.
static int albedo_check_planes(const mid_albedo_params *p, const char *who, const void *in, int in_fmt, const void *albedo, const void *out, int out_fmt)
{
    MID_REQUIRE(in && albedo && out, "%s: NULL pointer", who);
    const int gfmt = fmt_guide(p->format);
    const size_t npix = (size_t)p->width * p->height;
    MID_REQUIRE(texel_aligned(in_fmt, in), "%s: in is not %d-byte aligned", who, (int)fmt_bytes(in_fmt));
    MID_REQUIRE(texel_aligned(gfmt, albedo), "%s: albedo is not %d-byte aligned", who, (int)fmt_bytes(gfmt));
    MID_REQUIRE(texel_aligned(out_fmt, out), "%s: out is not %d-byte aligned", who, (int)fmt_bytes(out_fmt));
    const size_t in_bytes = npix * fmt_bytes(in_fmt), out_bytes = npix * fmt_bytes(out_fmt);
    MID_REQUIRE(!ranges_overlap(out, out_bytes, albedo, npix * fmt_bytes(gfmt)), "%s: out overlaps albedo", who);
    MID_REQUIRE(!ranges_overlap(out, out_bytes, in, in_bytes) || (out == in && in_bytes == out_bytes),
                "%s: out overlaps in (only exactly in place, RGBA32F to RGBA32F, is allowed)", who);
    return MID_OK;
}

}  // namespace mid

using namespace mid;

extern "C" int mid_demodulate(mid_ctx *ctx, const mid_albedo_params *p, const void *in, const void *albedo, mid_pixel *out, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    const char *who = "demodulate";
    if (int rc = albedo_check(p, who)) return rc;
    if (int rc = albedo_check_planes(p, who, in, fmt_frames(p->format), albedo, out, MID_FMT_RGBA32F)) return rc;
    return demodulate_out(ctx, p, in, albedo, out, b.s);
}

extern "C" int mid_modulate(mid_ctx *ctx, const mid_albedo_params *p, const mid_pixel *in, const void *albedo, void *out, int out_format, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    const char *who = "modulate";
    if (int rc = albedo_check(p, who)) return rc;
    MID_REQUIRE(fmt_frames(p->format) == MID_FMT_RGBA32F, "%s: the input is the RGBA32F illumination; frame format %d in the format word is refused", who,
                fmt_frames(p->format));
    MID_REQUIRE(fmt_known(out_format), "%s: unknown output format %d", who, out_format);
    if (int rc = albedo_check_planes(p, who, in, MID_FMT_RGBA32F, albedo, out, out_format)) return rc;
    return modulate_out(ctx, p, in, albedo, out, out_format, b.s);
}
