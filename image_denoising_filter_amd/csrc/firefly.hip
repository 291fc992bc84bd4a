// firefly.hip -- the firefly clamp and NaN repair in front of the recursive a-trous chain (include/mi_denoise.h, section a4l).
//
// Per pixel p, C the widened texel, l() a4i's luminance fma(0.0722, b, fma(0.7152, g, 0.2126 r)):
//   the valid neighbours are the q != p of the (2 R + 1)^2 window inside the image whose l(C(q)) is finite; n of them
//   n == 0:              out = C
//   m = the min(rank, n)-th largest valid neighbour luminance;  T = fmaxf(gain * m, floor)
//   lc = l(C(p)) finite:  lc <= T: out = C;  lc > T: out_rgb = C_rgb * (T / lc)
//   lc not finite:        out_rgb = (T, T, T)
//   alpha passes through.
//
// Kernel class: one tiled kernel, R a template value, the frame format a run-time wave-uniform value.  A workgroup of four waves
// covers 64 x 16 pixels, lanes along x, a lane owning four pixels of one column whose colours stay in registers from the fill.  The
// LDS tile holds one LUMINANCE per texel, (64 + 2 R) x (16 + 2 R) floats (5440 bytes at R = 2), NaN where the texel is outside the
// image: "outside" and "not valid" are one case and the tap loop has no edge branch.  A lane reads its 4 + 2 R tile rows once,
// 2 R + 1 floats each (64 consecutive floats per wave and read: conflict-free), and feeds every value to those of its four pixels
// whose window holds it.  The top-4 list of a pixel is four registers kept sorted by max / min under constant indices.
// The geometry of the fill is csrc/firefly_tile.hpp's.  Tiles are dealt to at most 8 workgroups per CU; a workgroup strides.
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

// a4i's luminance, literally
__device__ __forceinline__ float lum(float4 c) { return fmaf(0.0722f, c.z, fmaf(0.7152f, c.y, 0.2126f * c.x)); }

// a[0] >= a[1] >= a[2] >= a[3] stays so; v is not NaN
__device__ __forceinline__ void top4_insert(float (&a)[4], float v)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float hi = fmaxf(a[i], v);
        v = fminf(a[i], v);
        a[i] = hi;
    }
}

template <int R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void firefly_kernel(const void *in, float4 *out, int width, int height, int fmt, int rank, float gain, float floor_)
{
    constexpr int TW = kFireflyTileW + 2 * R, TH = kFireflyTileH + 2 * R, ROWS = 4 + 2 * R;
    __shared__ float tile[TW * TH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned tiles_x = (unsigned)firefly_tiles_x(width), tiles = tiles_x * (unsigned)firefly_tiles_y(height);
    const float ninf = -INFINITY;

    for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int tile_y = (int)(t / tiles_x), tile_x = (int)(t - (unsigned)tile_y * tiles_x);
        for (int f = kFireflyOwn + tid; f < TW * TH; f += 256) {        // the halo: only the luminance is kept
            const FireflySlot s = firefly_fill_slot(R, tile_x, tile_y, f, width, height);
            tile[s.lds] = s.inside ? lum(load_texel(in, fmt, firefly_flat(s.x, s.y, width))) : NAN;
        }
        // the lane's own pixels, rows 4 wave .. 4 wave + 3 of column lane: colour kept, luminance to the tile
        const FireflySlot s0 = firefly_fill_slot(R, tile_x, tile_y, kFireflyTileW * 4 * wave + lane, width, height);
        const size_t at0 = firefly_flat(s0.x, s0.y, width);
        float4 c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const FireflySlot s = firefly_fill_slot(R, tile_x, tile_y, kFireflyTileW * (4 * wave + j) + lane, width, height);
            c[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (s.inside) c[j] = load_texel(in, fmt, at0 + (size_t)j * (size_t)width);
            tile[s.lds] = s.inside ? lum(c[j]) : NAN;
        }
        __syncthreads();

        float top[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) top[j][i] = ninf;
        const float *col = tile + (4 * wave) * TW + lane;       // slot (lane, 4 wave): the top-left of the lane's 4 + 2 R rows
        // (the rows are a loop, not unrolled: 2 R + 1 reads in flight beside the 32 registers of colours and lists keep the kernel
        // inside the 64 VGPRs of occupancy 8; the row tests are scalar)
#pragma unroll 1
        for (int r = 0; r < ROWS; ++r) {
            float v[2 * R + 1];
#pragma unroll
            for (int i = 0; i <= 2 * R; ++i) {
                v[i] = col[r * TW + i];
                v[i] = fabsf(v[i]) < INFINITY ? v[i] : ninf;    // not valid (NaN, +-Inf, outside the image): below every finite value
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {                       // pixel j's centre is slot row j + R, column R
                if (r < j || r > j + 2 * R) continue;
#pragma unroll
                for (int i = 0; i <= 2 * R; ++i)
                    if (i != R) top4_insert(top[j], v[i]);
                if (r != j + R) top4_insert(top[j], v[R]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!(s0.x < width && s0.y + j < height)) continue;
            const float lc = col[(j + R) * TW + R];              // the centre's luminance, as the fill stored it
            float m = top[j][0];
            if (rank >= 2 && top[j][1] > ninf) m = top[j][1];
            if (rank >= 3 && top[j][2] > ninf) m = top[j][2];
            if (rank >= 4 && top[j][3] > ninf) m = top[j][3];
            float4 o = c[j];
            if (top[j][0] > ninf) {                             // n >= 1
                const float T = fmaxf(gain * m, floor_);
                if (!(fabsf(lc) < INFINITY)) o = make_float4(T, T, T, c[j].w);
                else if (lc > T) {
                    const float s = T / lc;
                    o = make_float4(c[j].x * s, c[j].y * s, c[j].z * s, c[j].w);
                }
            }
            out[at0 + (size_t)j * (size_t)width] = o;
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
int firefly_check(const mid_firefly_params *p, const char *who)
{
    MID_REQUIRE(p != nullptr, "%s: params is NULL", who);
    MID_REQUIRE(p->width > 0 && p->height > 0, "%s: bad size %dx%d", who, p->width, p->height);
    MID_REQUIRE((long)p->width * p->height < (1l << 30), "%s: image too large", who);
    MID_REQUIRE(p->radius == 1 || p->radius == 2, "%s: radius %d is neither 1 nor 2", who, p->radius);
    MID_REQUIRE(p->rank >= 1 && p->rank <= 4, "%s: rank %d outside 1..4", who, p->rank);
    MID_REQUIRE(std::isfinite(p->gain) && p->gain > 0.f, "%s: gain %g must be finite and > 0", who, (double)p->gain);
    MID_REQUIRE(std::isfinite(p->floor) && p->floor >= 0.f, "%s: floor %g must be finite and >= 0", who, (double)p->floor);
    MID_REQUIRE((p->format & ~0xffff) == 0 && fmt_known(fmt_frames(p->format)), "%s: unknown format %d", who, p->format);
    MID_REQUIRE((p->format >> 8) == 0, "%s: guide bits set in format 0x%x (the clamp reads no guide layer)", who, p->format);
    return MID_OK;
}

int firefly_clamp_out(mid_ctx *ctx, const mid_firefly_params *p, const void *in, mid_pixel *out, hipStream_t s)
{
    const size_t tiles = (size_t)firefly_tiles_x(p->width) * firefly_tiles_y(p->height), cap = (size_t)ctx->cu_count * 8;
    const dim3 grid((unsigned)(tiles < cap ? tiles : cap));
    if (p->radius == 1)
        hipLaunchKernelGGL(firefly_kernel<1>, grid, dim3(256), 0, s, in, (float4 *)out, p->width, p->height, fmt_frames(p->format), p->rank, p->gain, p->floor);
    else
        hipLaunchKernelGGL(firefly_kernel<2>, grid, dim3(256), 0, s, in, (float4 *)out, p->width, p->height, fmt_frames(p->format), p->rank, p->gain, p->floor);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

}  // namespace mid

using namespace mid;

extern "C" int mid_firefly_clamp(mid_ctx *ctx, const mid_firefly_params *p, const void *in, mid_pixel *out, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    const char *who = "firefly_clamp";
    if (int rc = firefly_check(p, who)) return rc;
    MID_REQUIRE(in && out, "%s: NULL pointer", who);
    const int fmt = fmt_frames(p->format);
    const size_t npix = (size_t)p->width * p->height;
    MID_REQUIRE(((uintptr_t)in & (fmt_bytes(fmt) - 1)) == 0, "%s: in is not %d-byte aligned", who, (int)fmt_bytes(fmt));
    MID_REQUIRE(((uintptr_t)out & 15) == 0, "%s: out is not 16-byte aligned", who);
    MID_REQUIRE(!ranges_overlap(out, npix * 16, in, npix * fmt_bytes(fmt)), "%s: out overlaps in (the pass is a stencil: not even exactly in place)", who);
    return firefly_clamp_out(ctx, p, in, out, b.s);
}
