// color_bounds.hip -- the neighbourhood colour box that clips the reprojected history (include/mi_denoise.h, section a4m).
//
// Per pixel p, C the widened texel:
//   the valid q are those of the (2 R + 1)^2 window, centre INCLUDED, inside the image, whose R, G and B are all finite; n of them
//   n == 0:   lo_rgb = -Inf, hi_rgb = +Inf
//   else, per channel:  mu = (sum v) / n rounded to fp32;  var = (sum (v - mu)^2) / n -- the two-pass form;  sigma = sqrtf(var)
//             lo = fmaf(-gamma, sigma, mu);  hi = fmaf(gamma, sigma, mu)
//   lo.w = hi.w = (float)n
//
// Kernel class: one tiled kernel, R a template value, the frame format a run-time wave-uniform value.  The geometry is the firefly
// clamp's (csrc/firefly_tile.hpp, unchanged): a workgroup of four waves covers 64 x 16 pixels, lanes along x, a lane owning four
// pixels of one column.  The LDS tile holds three floats per texel, planar: (64 + 2 R) x (16 + 2 R) x 3 floats (16320 bytes at
// R = 2).  The R plane holds NaN where the texel is outside the image or not valid (G and B hold 0 there): "outside" and "not valid"
// are one case and the tap loops have no edge branch.  A lane reads its 4 + 2 R tile rows once per loop, 2 R + 1 floats of each
// plane (64 consecutive floats per wave and read: conflict-free), and feeds every value to those of its four pixels whose window
// holds it.
//   mean loop       the sums of a window are taken in binary64 -- the sum of at most 25 binary32 values is then exact to 2^-48 of
//                   it and mu is the correctly rounded mean for all but those: a constant window gives mu == the constant, bit for
//                   bit, whatever the constant.  A tile row is summed along x once and that sum serves the (up to) four pixels.
//   deviation loop  binary32: d = v - mu (0 for a tap that is not valid), acc = fmaf(d, d, acc), taps in row-major order.
// Tiles are dealt to at most 8 workgroups per CU; a workgroup strides.
//
// The device helper shared with firefly.hip (load_texel) is restated here: that file keeps its text and its code object.
#include "common.hpp"
#include "firefly_tile.hpp"
#include <cmath>

namespace mid {

namespace {

__device__ __forceinline__ float4 load_texel(const void *img, int fmt, size_t idx)
{
    if (fmt == MID_FMT_RGBA8) return decode_rgba8(((const uint32_t *)img)[idx]);
    if (fmt == MID_FMT_RGBA16F) return decode_rgba16f(((const uint2 *)img)[idx]);
    return ((const float4 *)img)[idx];
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }

template <int R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void color_bounds_kernel(const void *in, float4 *lo, float4 *hi, int width, int height, int fmt, float gamma)
{
    constexpr int TW = kFireflyTileW + 2 * R, TH = kFireflyTileH + 2 * R, ROWS = 4 + 2 * R, PLANE = TW * TH;
    __shared__ float tile[3 * PLANE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned tiles_x = (unsigned)firefly_tiles_x(width), tiles = tiles_x * (unsigned)firefly_tiles_y(height);

    for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int tile_y = (int)(t / tiles_x), tile_x = (int)(t - (unsigned)tile_y * tiles_x);
        for (int f = tid; f < PLANE; f += 256) {                // the tile's own pixels (f < 1024) and the halo: nothing stays in registers
            const FireflySlot s = firefly_fill_slot(R, tile_x, tile_y, f, width, height);
            float r = NAN, g = 0.f, b = 0.f;
            if (s.inside) {
                const float4 c = load_texel(in, fmt, firefly_flat(s.x, s.y, width));
                if (finite_f(c.x) && finite_f(c.y) && finite_f(c.z)) { r = c.x; g = c.y; b = c.z; }
            }
            tile[s.lds] = r; tile[PLANE + s.lds] = g; tile[2 * PLANE + s.lds] = b;
        }
        __syncthreads();

        // slot (lane, 4 wave): the top-left of the lane's 4 + 2 R rows; pixel j's centre is slot row j + R, column R
        const float *col = tile + (4 * wave) * TW + lane;
        double sum[4][3];
        int n[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { sum[j][0] = sum[j][1] = sum[j][2] = 0.0; n[j] = 0; }
        // (the rows are a loop, not unrolled, as in firefly.hip: the row tests are scalar)
#pragma unroll 1
        for (int r = 0; r < ROWS; ++r) {
            double rs[3] = {0.0, 0.0, 0.0};
            int rn = 0;
#pragma unroll
            for (int i = 0; i <= 2 * R; ++i) {
                const float vr = col[r * TW + i];
                const bool ok = finite_f(vr);
                rn += ok ? 1 : 0;
                rs[0] += (double)(ok ? vr : 0.f);
                rs[1] += (double)col[PLANE + r * TW + i];
                rs[2] += (double)col[2 * PLANE + r * TW + i];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (r < j || r > j + 2 * R) continue;
                sum[j][0] += rs[0]; sum[j][1] += rs[1]; sum[j][2] += rs[2];
                n[j] += rn;
            }
        }
        float mu[4][3], acc[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double dn = (double)(n[j] > 0 ? n[j] : 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) { mu[j][c] = (float)(sum[j][c] / dn); acc[j][c] = 0.f; }
        }
#pragma unroll 1
        for (int r = 0; r < ROWS; ++r) {
            float v[3][2 * R + 1];
            bool ok[2 * R + 1];
#pragma unroll
            for (int i = 0; i <= 2 * R; ++i) {
                v[0][i] = col[r * TW + i];
                v[1][i] = col[PLANE + r * TW + i];
                v[2][i] = col[2 * PLANE + r * TW + i];
                ok[i] = finite_f(v[0][i]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (r < j || r > j + 2 * R) continue;
#pragma unroll
                for (int i = 0; i <= 2 * R; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float d = ok[i] ? v[c][i] - mu[j][c] : 0.f;
                        acc[j][c] = fmaf(d, d, acc[j][c]);
                    }
            }
        }
        const int px = tile_x * kFireflyTileW + lane, py = tile_y * kFireflyTileH + 4 * wave;
        if (px < width) {
            const size_t at0 = firefly_flat(px, py, width);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (py + j >= height) continue;
                const float fn = (float)n[j];
                float4 l = make_float4(-INFINITY, -INFINITY, -INFINITY, fn), h = make_float4(INFINITY, INFINITY, INFINITY, fn);
                if (n[j] > 0) {
                    const float sx = sqrtf(acc[j][0] / fn), sy = sqrtf(acc[j][1] / fn), sz = sqrtf(acc[j][2] / fn);
                    l = make_float4(fmaf(-gamma, sx, mu[j][0]), fmaf(-gamma, sy, mu[j][1]), fmaf(-gamma, sz, mu[j][2]), fn);
                    h = make_float4(fmaf(gamma, sx, mu[j][0]), fmaf(gamma, sy, mu[j][1]), fmaf(gamma, sz, mu[j][2]), fn);
                }
                lo[at0 + (size_t)j * (size_t)width] = l;
                hi[at0 + (size_t)j * (size_t)width] = h;
            }
        }
        __syncthreads();                                        // the tile is filled again
    }
}

bool ranges_overlap(const void *p, size_t np, const void *q, size_t nq)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return np && nq && a < b + nq && b < a + np;
}

}  // namespace

// What the entry point and the sequence check before their pointers.
int color_bounds_check(const mid_color_bounds_params *p, const char *who)
{
    MID_REQUIRE(p != nullptr, "%s: params is NULL", who);
    MID_REQUIRE(p->width > 0 && p->height > 0, "%s: bad size %dx%d", who, p->width, p->height);
    MID_REQUIRE((long)p->width * p->height < (1l << 30), "%s: image too large", who);
    MID_REQUIRE(p->radius == 1 || p->radius == 2, "%s: radius %d is neither 1 nor 2", who, p->radius);
    MID_REQUIRE(std::isfinite(p->gamma) && p->gamma >= 0.f, "%s: gamma %g must be finite and >= 0", who, (double)p->gamma);
    MID_REQUIRE((p->format & ~0xffff) == 0 && fmt_known(fmt_frames(p->format)), "%s: unknown format %d", who, p->format);
    MID_REQUIRE((p->format >> 8) == 0, "%s: guide bits set in format 0x%x (the box reads no guide layer)", who, p->format);
    return MID_OK;
}

int color_bounds_out(mid_ctx *ctx, const mid_color_bounds_params *p, const void *in, mid_pixel *lo, mid_pixel *hi, hipStream_t s)
{
    const size_t tiles = (size_t)firefly_tiles_x(p->width) * firefly_tiles_y(p->height), cap = (size_t)ctx->cu_count * 8;
    const dim3 grid((unsigned)(tiles < cap ? tiles : cap));
    if (p->radius == 1)
        hipLaunchKernelGGL(color_bounds_kernel<1>, grid, dim3(256), 0, s, in, (float4 *)lo, (float4 *)hi, p->width, p->height, fmt_frames(p->format), p->gamma);
    else
        hipLaunchKernelGGL(color_bounds_kernel<2>, grid, dim3(256), 0, s, in, (float4 *)lo, (float4 *)hi, p->width, p->height, fmt_frames(p->format), p->gamma);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

}  // namespace mid

using namespace mid;

extern "C" int mid_color_bounds(mid_ctx *ctx, const mid_color_bounds_params *p, const void *in, mid_pixel *lo, mid_pixel *hi, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    const char *who = "color_bounds";
    if (int rc = color_bounds_check(p, who)) return rc;
    MID_REQUIRE(in && lo && hi, "%s: NULL pointer", who);
    const int fmt = fmt_frames(p->format);
    const size_t npix = (size_t)p->width * p->height;
    MID_REQUIRE(((uintptr_t)in & (fmt_bytes(fmt) - 1)) == 0, "%s: in is not %d-byte aligned", who, (int)fmt_bytes(fmt));
    MID_REQUIRE(((uintptr_t)lo & 15) == 0 && ((uintptr_t)hi & 15) == 0, "%s: lo or hi is not 16-byte aligned", who);
    MID_REQUIRE(!ranges_overlap(lo, npix * 16, in, npix * fmt_bytes(fmt)) && !ranges_overlap(hi, npix * 16, in, npix * fmt_bytes(fmt)),
                "%s: lo or hi overlaps in (the pass is a stencil)", who);
    MID_REQUIRE(!ranges_overlap(lo, npix * 16, hi, npix * 16), "%s: lo overlaps hi", who);
    return color_bounds_out(ctx, p, in, lo, hi, b.s);
}
