// image_metrics.hip -- full-reference image quality metrics (include/mi_denoise.h, section a4n): the sums behind MSE, PSNR, MAE,
// the largest difference, relMSE and SSIM of a test image `a` against a reference `b`, reduced on the GPU to bits that depend on
// the inputs and the parameters alone, and the host function that states the derived values.
//
// Kernel class: one tiled kernel, SSIM and MAP template values, the two frame formats run-time wave-uniform values.  The geometry is
// the firefly clamp's (csrc/firefly_tile.hpp, unchanged, R = 5): a workgroup of four waves covers 64 x 16 pixels, lanes along x, a
// lane owning four pixels of one column.  The pointwise terms of a lane's pixels come from the loads that fill the tile.
//   SSIM   two LDS tiles of 74 x 26 fp32 luminances, of a and of b; the first holds NaN where the pixel is outside the image or not
//          VALID: "outside" and "not valid" are one case, and a tap's weight is chosen by a select, never by multiplying a NaN by 0.
//          A lane reads the eleven taps of each of its 4 + 10 tile rows once (64 consecutive floats per wave and read:
//          conflict-free), forms the row's six horizontal sums (w, w la, w lb, w la^2, w lb^2, w la lb) in binary64 registers and
//          feeds them, times the vertical weight, to those of its four pixels whose window holds the row.  The taps of a row are
//          unrolled, the rows are a loop whose vertical weight is a scalar select: no register array is indexed by a run-time value.
//   !SSIM  the same kernel without the halo, the tiles and the windows: a streaming pass with the same reduction, so its pointwise
//          sums have the bits of the other's.
// Reduction: G = min(tiles, kMetricsGroups) workgroups, a function of the size alone; workgroup g takes the tiles g, g + G, ...; a
// lane adds its pixels in order; the 64 lanes of a wave are added by an xor butterfly (every lane holds the same bits afterwards:
// the addition commutes), the four waves in index order through LDS; one row of MID_METRICS_N doubles per workgroup goes to
// work[MID_METRICS_N * (1 + g)].  metrics_final_kernel, one workgroup, adds the rows: thread (k, c) the rows k, k + 64, ... of
// column c, then the sixty-four chains by a fixed tree.  Slot MID_METRICS_MAX_ABS is joined by fmax instead of +.  No atomics.
#include "common.hpp"
#include "firefly_tile.hpp"
#include <cmath>

namespace mid {

namespace {

constexpr int kMetricsR = 5;
constexpr unsigned kMetricsGroups = 4096;

__device__ __forceinline__ float4 load_texel(const void *img, int fmt, size_t idx)
{
    if (fmt == MID_FMT_RGBA8) return decode_rgba8(((const uint32_t *)img)[idx]);
    if (fmt == MID_FMT_RGBA16F) return decode_rgba16f(((const uint2 *)img)[idx]);
    return ((const float4 *)img)[idx];
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }
__device__ __forceinline__ bool valid_pair(float4 a, float4 b)
{
    return finite_f(a.x) && finite_f(a.y) && finite_f(a.z) && finite_f(b.x) && finite_f(b.y) && finite_f(b.z);
}

// a4i's luminance, literally
__device__ __forceinline__ float lum(float4 c) { return fmaf(0.0722f, c.z, fmaf(0.7152f, c.y, 0.2126f * c.x)); }

__device__ __forceinline__ constexpr double gauss(int k)
{
    return k == 0 ? MID_METRICS_G0 : k == 1 ? MID_METRICS_G1 : k == 2 ? MID_METRICS_G2 : k == 3 ? MID_METRICS_G3 : k == 4 ? MID_METRICS_G4 : MID_METRICS_G5;
}

// one channel's pointwise terms of a VALID pixel
__device__ __forceinline__ void pointwise(float af, float bf, double eps, double &sq, double &ab, double &mx, double &rel)
{
    const double a = (double)af, b = (double)bf, d = a - b, d2 = d * d, ad = fabs(d);
    sq += d2;
    ab += ad;
    mx = fmax(mx, ad);
    rel += d2 / (b * b + eps);
}

__device__ __forceinline__ double wave_sum(double v, bool is_max)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double o = __shfl_xor(v, m, 64);
        v = is_max ? fmax(v, o) : v + o;
    }
    return v;
}

template <bool SSIM, bool MAP>
__global__ __launch_bounds__(256) void metrics_kernel(const void *a, const void *b, double *work, float *map, int width, int height, int fmt_a,
                                                      int fmt_b, double eps, double c1, double c2)
{
    constexpr int R = kMetricsR, TW = kFireflyTileW + 2 * R, TH = kFireflyTileH + 2 * R, ROWS = 4 + 2 * R;
    __shared__ float tile_a[SSIM ? TW * TH : 1], tile_b[SSIM ? TW * TH : 1];
    __shared__ double wave_part[4][MID_METRICS_N];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned tiles_x = (unsigned)firefly_tiles_x(width), tiles = tiles_x * (unsigned)firefly_tiles_y(height);

    double acc[MID_METRICS_N];
#pragma unroll
    for (int i = 0; i < MID_METRICS_N; ++i) acc[i] = 0.0;

    for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int tile_y = (int)(t / tiles_x), tile_x = (int)(t - (unsigned)tile_y * tiles_x);
        if (SSIM) {
            for (int f = kFireflyOwn + tid; f < TW * TH; f += 256) {        // the halo: only the luminances are kept
                const FireflySlot s = firefly_fill_slot(R, tile_x, tile_y, f, width, height);
                float la = NAN, lb = 0.f;
                if (s.inside) {
                    const size_t at = firefly_flat(s.x, s.y, width);
                    const float4 ca = load_texel(a, fmt_a, at), cb = load_texel(b, fmt_b, at);
                    if (valid_pair(ca, cb)) { la = lum(ca); lb = lum(cb); }
                }
                tile_a[s.lds] = la; tile_b[s.lds] = lb;
            }
        }
        // the lane's own pixels, rows 4 wave .. 4 wave + 3 of column lane: the pointwise terms, and the luminances to the tiles
        const FireflySlot s0 = firefly_fill_slot(R, tile_x, tile_y, kFireflyTileW * 4 * wave + lane, width, height);
        const size_t at0 = firefly_flat(s0.x, s0.y, width);
        bool own_valid[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const FireflySlot s = firefly_fill_slot(R, tile_x, tile_y, kFireflyTileW * (4 * wave + j) + lane, width, height);
            float la = NAN, lb = 0.f;
            own_valid[j] = false;
            if (s.inside) {
                const size_t at = at0 + (size_t)j * (size_t)width;
                const float4 ca = load_texel(a, fmt_a, at), cb = load_texel(b, fmt_b, at);
                if (valid_pair(ca, cb)) {
                    own_valid[j] = true;
                    la = lum(ca); lb = lum(cb);
                    acc[MID_METRICS_N_VALID] += 1.0;
                    pointwise(ca.x, cb.x, eps, acc[MID_METRICS_SQ_R], acc[MID_METRICS_ABS_R], acc[MID_METRICS_MAX_ABS], acc[MID_METRICS_REL_R]);
                    pointwise(ca.y, cb.y, eps, acc[MID_METRICS_SQ_G], acc[MID_METRICS_ABS_G], acc[MID_METRICS_MAX_ABS], acc[MID_METRICS_REL_G]);
                    pointwise(ca.z, cb.z, eps, acc[MID_METRICS_SQ_B], acc[MID_METRICS_ABS_B], acc[MID_METRICS_MAX_ABS], acc[MID_METRICS_REL_B]);
                } else {
                    acc[MID_METRICS_N_INVALID] += 1.0;
                }
            }
            if (SSIM) { tile_a[s.lds] = la; tile_b[s.lds] = lb; }
        }
        if (SSIM) {
            __syncthreads();
            const int base = (4 * wave) * TW + lane;                // slot (lane, 4 wave): the top-left of the lane's 4 + 2 R rows
            double v[4][6];                                         // per pixel: W, sum w la, sum w lb, sum w la^2, sum w lb^2, sum w la lb
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < 6; ++q) v[j][q] = 0.0;
            // (the rows are a loop, not unrolled, as in firefly.hip: the row tests and the vertical weight are scalar)
#pragma unroll 1
            for (int r = 0; r < ROWS; ++r) {
                double h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int i = 0; i <= 2 * R; ++i) {
                    const float fa = tile_a[base + r * TW + i], fb = tile_b[base + r * TW + i];
                    const bool ok = fa == fa;                       // the marker is NaN
                    const double w = ok ? gauss(i < R ? R - i : i - R) : 0.0;
                    const double la = ok ? (double)fa : 0.0, lb = ok ? (double)fb : 0.0;
                    const double wa = w * la, wb = w * lb;
                    h[0] += w;
                    h[1] += wa;
                    h[2] += wb;
                    h[3] = fma(wa, la, h[3]);
                    h[4] = fma(wb, lb, h[4]);
                    h[5] = fma(wa, lb, h[5]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {                       // pixel j's centre is slot row j + R
                    if (r < j || r > j + 2 * R) continue;
                    const double g = gauss(r - j < R ? R - (r - j) : r - j - R);
#pragma unroll
                    for (int q = 0; q < 6; ++q) v[j][q] = fma(g, h[q], v[j][q]);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!(s0.x < width && s0.y + j < height)) continue;
                float m = NAN;
                if (own_valid[j]) {                                 // W >= g_0^2 = 1: the centre is a tap
                    const double W = v[j][0], mu_a = v[j][1] / W, mu_b = v[j][2] / W;
                    const double ab = mu_a * mu_b, aa = mu_a * mu_a, bb = mu_b * mu_b;
                    const double s_aa = v[j][3] / W - aa, s_bb = v[j][4] / W - bb, s_ab = v[j][5] / W - ab;
                    const double num = (2.0 * ab + c1) * (2.0 * s_ab + c2);
                    const double den = (aa + bb + c1) * (s_aa + s_bb + c2);
                    const double ssim = num / den;
                    acc[MID_METRICS_SSIM] += ssim;
                    m = (float)ssim;
                }
                if (MAP) map[at0 + (size_t)j * (size_t)width] = m;
            }
            __syncthreads();                                        // the tiles are filled again
        }
    }

#pragma unroll
    for (int i = 0; i < MID_METRICS_N; ++i) {
        const double s = wave_sum(acc[i], i == MID_METRICS_MAX_ABS);
        if (lane == 0) wave_part[wave][i] = s;
    }
    __syncthreads();
    if (tid < MID_METRICS_N) {
        const bool is_max = tid == MID_METRICS_MAX_ABS;
        double s = wave_part[0][tid];
        for (int k = 1; k < 4; ++k) s = is_max ? fmax(s, wave_part[k][tid]) : s + wave_part[k][tid];
        work[(size_t)MID_METRICS_N * (1 + blockIdx.x) + tid] = s;
    }
}

// One workgroup of 1024: thread (k, c) = (tid / 16, tid % 16) adds the rows k, k + 64, ... of column c in that order (the loads of
// eight rows are in flight together; the additions keep their order); the sixty-four chains of a column are then joined by the tree
// ((0 1)(2 3))((4 5)(6 7)) ...
constexpr int kFinalChains = 64;
__global__ __launch_bounds__(kFinalChains * MID_METRICS_N) void metrics_final_kernel(double *work, unsigned rows)
{
    __shared__ double part[kFinalChains][MID_METRICS_N];
    const int tid = threadIdx.x, k = tid >> 4, c = tid & 15;
    const bool is_max = c == MID_METRICS_MAX_ABS;
    double s = 0.0;
#pragma unroll 8
    for (unsigned r = (unsigned)k; r < rows; r += kFinalChains) {
        const double x = work[(size_t)MID_METRICS_N * (1 + r) + c];
        s = is_max ? fmax(s, x) : s + x;
    }
    part[k][c] = s;
    __syncthreads();
    for (int step = 1; step < kFinalChains; step <<= 1) {
        if ((k & (2 * step - 1)) == 0) part[k][c] = is_max ? fmax(part[k][c], part[k + step][c]) : part[k][c] + part[k + step][c];
        __syncthreads();
    }
    if (k == 0) work[c] = part[0][c];
}

bool ranges_overlap(const void *p, size_t np, const void *q, size_t nq)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return np && nq && a < b + nq && b < a + np;
}

unsigned metrics_groups(int width, int height)
{
    const size_t tiles = (size_t)firefly_tiles_x(width) * firefly_tiles_y(height);
    return (unsigned)(tiles < kMetricsGroups ? tiles : kMetricsGroups);
}

bool size_ok(int width, int height) { return width > 0 && height > 0 && (long)width * height < (1l << 30); }

}  // namespace

int image_metrics_check(const mid_image_metrics_params *p, const char *who)
{
    MID_REQUIRE(p != nullptr, "%s: params is NULL", who);
    MID_REQUIRE(p->width > 0 && p->height > 0, "%s: bad size %dx%d", who, p->width, p->height);
    MID_REQUIRE((long)p->width * p->height < (1l << 30), "%s: image too large", who);
    MID_REQUIRE((p->format_a & ~0xffff) == 0 && fmt_known(fmt_frames(p->format_a)), "%s: unknown format_a %d", who, p->format_a);
    MID_REQUIRE((p->format_b & ~0xffff) == 0 && fmt_known(fmt_frames(p->format_b)), "%s: unknown format_b %d", who, p->format_b);
    MID_REQUIRE((p->format_a >> 8) == 0 && (p->format_b >> 8) == 0, "%s: guide bits set in format 0x%x / 0x%x (the metrics read no guide layer)", who,
                p->format_a, p->format_b);
    MID_REQUIRE(std::isfinite(p->peak) && p->peak > 0.f, "%s: peak %g must be finite and > 0", who, (double)p->peak);
    MID_REQUIRE(std::isfinite(p->eps) && p->eps > 0.f, "%s: eps %g must be finite and > 0", who, (double)p->eps);
    MID_REQUIRE(p->ssim == 0 || p->ssim == 1, "%s: ssim %d is neither 0 nor 1", who, p->ssim);
    return MID_OK;
}

int image_metrics_out(mid_ctx *ctx, const mid_image_metrics_params *p, const void *a, const void *b, void *work, float *map, hipStream_t s)
{
    (void)ctx;
    const unsigned groups = metrics_groups(p->width, p->height);
    const double eps = (double)p->eps, k1 = 0.01 * (double)p->peak, k2 = 0.03 * (double)p->peak, c1 = k1 * k1, c2 = k2 * k2;
    const int fa = fmt_frames(p->format_a), fb = fmt_frames(p->format_b);
    if (!p->ssim)
        hipLaunchKernelGGL((metrics_kernel<false, false>), dim3(groups), dim3(256), 0, s, a, b, (double *)work, map, p->width, p->height, fa, fb, eps, c1, c2);
    else if (!map)
        hipLaunchKernelGGL((metrics_kernel<true, false>), dim3(groups), dim3(256), 0, s, a, b, (double *)work, map, p->width, p->height, fa, fb, eps, c1, c2);
    else
        hipLaunchKernelGGL((metrics_kernel<true, true>), dim3(groups), dim3(256), 0, s, a, b, (double *)work, map, p->width, p->height, fa, fb, eps, c1, c2);
    MID_HIP(hipGetLastError());
    hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(kFinalChains * MID_METRICS_N), 0, s, (double *)work, groups);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

}  // namespace mid

using namespace mid;

extern "C" size_t mid_image_metrics_workspace(int width, int height)
{
    if (!size_ok(width, height)) return 0;
    return sizeof(double) * MID_METRICS_N * (1 + (size_t)metrics_groups(width, height));
}

extern "C" int mid_image_metrics(mid_ctx *ctx, const mid_image_metrics_params *p, const void *a, const void *b, void *work, float *map, void *stream)
{
    Bind bind(ctx, stream);
    if (bind.rc) return bind.rc;
    const char *who = "image_metrics";
    if (int rc = image_metrics_check(p, who)) return rc;
    MID_REQUIRE(a && b && work, "%s: NULL pointer", who);
    MID_REQUIRE(p->ssim || !map, "%s: a map needs ssim == 1", who);
    const int fa = fmt_frames(p->format_a), fb = fmt_frames(p->format_b);
    const size_t npix = (size_t)p->width * p->height, na = npix * fmt_bytes(fa), nb = npix * fmt_bytes(fb);
    const size_t nw = mid_image_metrics_workspace(p->width, p->height), nm = map ? npix * sizeof(float) : 0;
    MID_REQUIRE(((uintptr_t)a & (fmt_bytes(fa) - 1)) == 0, "%s: a is not %d-byte aligned", who, (int)fmt_bytes(fa));
    MID_REQUIRE(((uintptr_t)b & (fmt_bytes(fb) - 1)) == 0, "%s: b is not %d-byte aligned", who, (int)fmt_bytes(fb));
    MID_REQUIRE(((uintptr_t)work & 15) == 0, "%s: work is not 16-byte aligned", who);
    MID_REQUIRE(((uintptr_t)map & 3) == 0, "%s: map is not 4-byte aligned", who);
    MID_REQUIRE(!ranges_overlap(work, nw, a, na) && !ranges_overlap(work, nw, b, nb), "%s: work overlaps an input", who);
    MID_REQUIRE(!ranges_overlap(map, nm, a, na) && !ranges_overlap(map, nm, b, nb), "%s: map overlaps an input", who);
    MID_REQUIRE(!ranges_overlap(map, nm, work, nw), "%s: map overlaps work", who);
    return image_metrics_out(ctx, p, a, b, work, map, bind.s);
}

extern "C" int mid_image_metrics_derive(const double *sums, const mid_image_metrics_params *p, mid_image_metrics_result *out)
{
    const char *who = "image_metrics_derive";
    MID_REQUIRE(sums && p && out, "%s: NULL pointer", who);
    MID_REQUIRE(std::isfinite(p->peak) && p->peak > 0.f, "%s: peak %g must be finite and > 0", who, (double)p->peak);
    const double n = sums[MID_METRICS_N_VALID], nan = std::nan(""), peak = (double)p->peak;
    const bool some = n > 0.0;
    out->n_valid = n;
    out->n_invalid = sums[MID_METRICS_N_INVALID];
    out->mse = some ? (sums[MID_METRICS_SQ_R] + sums[MID_METRICS_SQ_G] + sums[MID_METRICS_SQ_B]) / (3.0 * n) : nan;
    out->mse_r = some ? sums[MID_METRICS_SQ_R] / n : nan;
    out->mse_g = some ? sums[MID_METRICS_SQ_G] / n : nan;
    out->mse_b = some ? sums[MID_METRICS_SQ_B] / n : nan;
    out->mae = some ? (sums[MID_METRICS_ABS_R] + sums[MID_METRICS_ABS_G] + sums[MID_METRICS_ABS_B]) / (3.0 * n) : nan;
    out->max_abs = sums[MID_METRICS_MAX_ABS];
    out->psnr = !some ? nan : out->mse == 0.0 ? (double)INFINITY : 10.0 * std::log10(peak * peak / out->mse);
    out->relmse = some ? (sums[MID_METRICS_REL_R] + sums[MID_METRICS_REL_G] + sums[MID_METRICS_REL_B]) / (3.0 * n) : nan;
    out->ssim = some && p->ssim ? sums[MID_METRICS_SSIM] / n : nan;
    return MID_OK;
}
