// guided.hip -- the guided filter (include/mi_denoise.h, section a4o; He, Sun, Tang 2010 with a colour guide): inside every window
// the frame is fitted as an affine function of the guide's colour, and the averaged fit is evaluated at the pixel's own guide texel.
//
// Kernel class: two launches that share one sliding box sum (csrc/guided_box.hpp has the geometry and its reasons).
//   guided_model_kernel   22 sums per window (n, 3 + 3 means, 6 + 9 products) over the VALID texels, in binary64, of values from
//                         which a reference texel of the tile has been subtracted; the 3 x 3 solve by the adjugate, in binary64;
//                         a (9), b (3) and the "has a model" flag rounded once to fp32 into thirteen planes of `work`.
//   guided_apply_kernel   13 sums per window over those planes, in binary64; the means rounded once to fp32; one fp32 fma chain.
// A workgroup of four waves holds 256 image columns, lanes along x, and walks down a segment of 32 output rows.  Each lane keeps
// the vertical sums of its column in registers: the row entering the window is added, the row leaving it subtracted.  Per output
// row the column sums become prefix sums along x -- a shuffle scan inside each wave, the three wave totals through LDS -- and
// cross LDS once; an output lane takes the difference of two slots.  Nothing in a row's work depends on the radius; the radius
// costs the 2 r + 1 warm-up rows of a segment and the 2 r columns of a strip that are held but not output.
// Workgroup g of min(tiles, kGuidedGroups) takes the tiles g, g + G, ...  Index arithmetic in size_t; formats are run-time,
// wave-uniform values.  No atomics: the bits depend on the inputs and the parameters alone.
#include "common.hpp"
#include "guided_box.hpp"
#include <cmath>

namespace mid {

namespace {

constexpr int kModelSums = 22, kApplySums = 13;

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

template <int N>
struct BoxLds {
    double tot[kGuidedLanes / 64][N];
    double pre[N][kGuidedLanes];
};

// v: the column sums of lane t on entry, the window sums of output lane t on return (other lanes: unspecified, finite).
// Two barriers; every thread of the workgroup must call it.
template <int N>
__device__ __forceinline__ void box_window(double (&v)[N], BoxLds<N> &s, int t, int r)
{
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double x = v[k];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        v[k] = x;
        if (lane == 63) s.tot[wave][k] = x;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double off = 0.0;
        for (int q = 0; q < wave; ++q) off += s.tot[q][k];
        s.pre[k][t] = v[k] + off;
    }
    __syncthreads();
    const int hi = guided_slot_hi(t, r) < kGuidedLanes ? guided_slot_hi(t, r) : kGuidedLanes - 1;   // (clamped for the lanes that output nothing)
    const int lo = guided_slot_lo(t, r);
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = s.pre[k][hi] - (lo >= 0 ? s.pre[k][lo] : 0.0);
}

// The 22 terms of one texel, 0 where it is not VALID: 1, dI (3), dp (3), dI dI^T (6: 00 01 02 11 12 22), dI dp^T (9: row = guide channel).
__device__ __forceinline__ void model_terms(float4 p, float4 g, const double (&sI)[3], const double (&sp)[3], double (&e)[kModelSums])
{
    const bool ok = valid_pair(p, g);
    const double I[3] = {ok ? (double)g.x - sI[0] : 0.0, ok ? (double)g.y - sI[1] : 0.0, ok ? (double)g.z - sI[2] : 0.0};
    const double P[3] = {ok ? (double)p.x - sp[0] : 0.0, ok ? (double)p.y - sp[1] : 0.0, ok ? (double)p.z - sp[2] : 0.0};
    e[0] = ok ? 1.0 : 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) { e[1 + j] = I[j]; e[4 + j] = P[j]; }
    e[7] = I[0] * I[0]; e[8] = I[0] * I[1]; e[9] = I[0] * I[2]; e[10] = I[1] * I[1]; e[11] = I[1] * I[2]; e[12] = I[2] * I[2];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) e[13 + 3 * j + c] = I[j] * P[c];
}

__global__ __launch_bounds__(kGuidedLanes) void guided_model_kernel(const void *in, const void *guide, float *work, int width, int height, int r,
                                                                    double eps, int fmt_in, int fmt_g)
{
    constexpr int N = kModelSums;
    __shared__ BoxLds<N> lds;
    const int t = threadIdx.x;
    const int strips = guided_strips(width, r);
    const unsigned tiles = guided_tiles(width, height, r);
    const size_t npix = (size_t)width * (size_t)height;

    for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int seg = (int)(tile / (unsigned)strips), strip = (int)(tile - (unsigned)seg * (unsigned)strips);
        const int cx = guided_col(strip, r, t);
        const bool col_in = cx >= 0 && cx < width;
        // the reference texel: the tile's first output pixel, which lies inside the image; a channel that is not finite shifts by 0
        double sI[3], sp[3];
        {
            const size_t at = guided_flat(strip * guided_strip_w(r), guided_seg_y0(seg), width);
            const float4 p = load_texel(in, fmt_in, at), g = load_texel(guide, fmt_g, at);
            sI[0] = finite_f(g.x) ? (double)g.x : 0.0; sI[1] = finite_f(g.y) ? (double)g.y : 0.0; sI[2] = finite_f(g.z) ? (double)g.z : 0.0;
            sp[0] = finite_f(p.x) ? (double)p.x : 0.0; sp[1] = finite_f(p.y) ? (double)p.y : 0.0; sp[2] = finite_f(p.z) ? (double)p.z : 0.0;
        }
        double vs[N];
#pragma unroll
        for (int k = 0; k < N; ++k) vs[k] = 0.0;

        const int y_end = guided_row_end(seg, r, height);
#pragma unroll 1
        for (int yy = guided_row_begin(seg, r); yy < y_end; ++yy) {
            double e[N];
            const int yl = guided_row_leaving(yy, r);
            const bool enters = col_in && yy >= 0 && yy < height, leaves = col_in && guided_row_left(yy, seg, r) && yl >= 0 && yl < height;
            // (both rows' texels are requested before either is used: one memory round trip per walked row, not two)
            float4 pe = make_float4(NAN, NAN, NAN, NAN), ge = pe, pl = pe, gl = pe;
            if (enters) { const size_t at = guided_flat(cx, yy, width); pe = load_texel(in, fmt_in, at); ge = load_texel(guide, fmt_g, at); }
            if (leaves) { const size_t at = guided_flat(cx, yl, width); pl = load_texel(in, fmt_in, at); gl = load_texel(guide, fmt_g, at); }
            if (enters) {
                model_terms(pe, ge, sI, sp, e);
#pragma unroll
                for (int k = 0; k < N; ++k) vs[k] += e[k];
            }
            if (leaves) {
                model_terms(pl, gl, sI, sp, e);
#pragma unroll
                for (int k = 0; k < N; ++k) vs[k] -= e[k];
            }
            if (!guided_row_is_out(yy, seg, r)) continue;       // (uniform: the barriers below are reached by all or by none)
            double v[N];
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = vs[k];
            box_window<N>(v, lds, t, r);
            if (!(guided_out_lane(r, t) && cx < width)) continue;
            const size_t at = guided_flat(cx, guided_row_out(yy, r), width);
            float m[kApplySums];
#pragma unroll
            for (int k = 0; k < kApplySums; ++k) m[k] = 0.f;
            const double n = v[0];
            if (n > 0.0) {
                double mu[3], nu[3], C[3][3];
#pragma unroll
                for (int j = 0; j < 3; ++j) { mu[j] = v[1 + j] / n; nu[j] = v[4 + j] / n; }
                const double A00 = v[7] / n - mu[0] * mu[0] + eps, A01 = v[8] / n - mu[0] * mu[1], A02 = v[9] / n - mu[0] * mu[2];
                const double A11 = v[10] / n - mu[1] * mu[1] + eps, A12 = v[11] / n - mu[1] * mu[2], A22 = v[12] / n - mu[2] * mu[2] + eps;
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int c = 0; c < 3; ++c) C[j][c] = v[13 + 3 * j + c] / n - mu[j] * nu[c];
                // (Sigma + eps U)^-1 by the adjugate: symmetric positive definite, so det > 0 and nothing pivots on data
                const double c00 = A11 * A22 - A12 * A12, c01 = A02 * A12 - A01 * A22, c02 = A01 * A12 - A02 * A11;
                const double c11 = A00 * A22 - A02 * A02, c12 = A01 * A02 - A00 * A12, c22 = A00 * A11 - A01 * A01;
                const double det = A00 * c00 + A01 * c01 + A02 * c02;
                const double inv[3][3] = {{c00 / det, c01 / det, c02 / det}, {c01 / det, c11 / det, c12 / det}, {c02 / det, c12 / det, c22 / det}};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double a[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) a[j] = inv[j][0] * C[0][c] + inv[j][1] * C[1][c] + inv[j][2] * C[2][c];
                    // b = nu - a^T mu in the unshifted units
                    const double b = (nu[c] + sp[c]) - (a[0] * (mu[0] + sI[0]) + a[1] * (mu[1] + sI[1]) + a[2] * (mu[2] + sI[2]));
#pragma unroll
                    for (int j = 0; j < 3; ++j) m[3 * j + c] = (float)a[j];
                    m[9 + c] = (float)b;
                }
                m[12] = 1.f;
            }
#pragma unroll
            for (int k = 0; k < kApplySums; ++k) work[(size_t)k * npix + at] = m[k];
        }
        __syncthreads();        // the next tile's first round writes lds.tot
    }
}

__global__ __launch_bounds__(kGuidedLanes) void guided_apply_kernel(const void *in, const void *guide, const float *work, void *out, int width,
                                                                    int height, int r, int fmt_in, int fmt_g, int fmt_out)
{
    constexpr int N = kApplySums;
    __shared__ BoxLds<N> lds;
    const int t = threadIdx.x;
    const int strips = guided_strips(width, r);
    const unsigned tiles = guided_tiles(width, height, r);
    const size_t npix = (size_t)width * (size_t)height;

    for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int seg = (int)(tile / (unsigned)strips), strip = (int)(tile - (unsigned)seg * (unsigned)strips);
        const int cx = guided_col(strip, r, t);
        const bool col_in = cx >= 0 && cx < width;
        double vs[N];
#pragma unroll
        for (int k = 0; k < N; ++k) vs[k] = 0.0;

        const int y_end = guided_row_end(seg, r, height);
#pragma unroll 1
        for (int yy = guided_row_begin(seg, r); yy < y_end; ++yy) {
            const int yl = guided_row_leaving(yy, r);
            const bool enters = col_in && yy >= 0 && yy < height, leaves = col_in && guided_row_left(yy, seg, r) && yl >= 0 && yl < height;
            float fe[N], fl[N];                                  // (both rows in flight together, as in the model kernel)
#pragma unroll
            for (int k = 0; k < N; ++k) { fe[k] = 0.f; fl[k] = 0.f; }
            if (enters) {
                const size_t at = guided_flat(cx, yy, width);
#pragma unroll
                for (int k = 0; k < N; ++k) fe[k] = work[(size_t)k * npix + at];
            }
            if (leaves) {
                const size_t at = guided_flat(cx, yl, width);
#pragma unroll
                for (int k = 0; k < N; ++k) fl[k] = work[(size_t)k * npix + at];
            }
            // (a row that does not enter or leave contributes zeros)
#pragma unroll
            for (int k = 0; k < N; ++k) vs[k] = (vs[k] + (double)fe[k]) - (double)fl[k];
            if (!guided_row_is_out(yy, seg, r)) continue;       // (uniform)
            double v[N];
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = vs[k];
            box_window<N>(v, lds, t, r);
            if (!(guided_out_lane(r, t) && cx < width)) continue;
            const size_t at = guided_flat(cx, guided_row_out(yy, r), width);
            const float4 p = load_texel(in, fmt_in, at), g = load_texel(guide, fmt_g, at);
            float4 o = p;
            const double m = v[12];
            if (valid_pair(p, g) && m > 0.0) {
                float a[12];
#pragma unroll
                for (int k = 0; k < 12; ++k) a[k] = (float)(v[k] / m);
                // a4o's chain: the guide channels 2, 1, 0 in that order onto b
                o.x = fmaf(a[0], g.x, fmaf(a[3], g.y, fmaf(a[6], g.z, a[9])));
                o.y = fmaf(a[1], g.x, fmaf(a[4], g.y, fmaf(a[7], g.z, a[10])));
                o.z = fmaf(a[2], g.x, fmaf(a[5], g.y, fmaf(a[8], g.z, a[11])));
            }
            store_out(out, at, fmt_out, o);
        }
        __syncthreads();
    }
}

bool ranges_overlap(const void *p, size_t np, const void *q, size_t nq)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return np && nq && a < b + nq && b < a + np;
}

}  // namespace

int guided_check(const mid_guided_params *p, const char *who)
{
    MID_REQUIRE(p != nullptr, "%s: params is NULL", who);
    MID_REQUIRE(p->width > 0 && p->height > 0, "%s: bad size %dx%d", who, p->width, p->height);
    MID_REQUIRE((long)p->width * p->height < (1l << 30), "%s: image too large", who);
    MID_REQUIRE(p->radius >= 1 && p->radius <= kGuidedMaxRadius, "%s: radius %d outside 1..%d", who, p->radius, kGuidedMaxRadius);
    MID_REQUIRE(std::isfinite(p->eps) && p->eps > 0.f, "%s: eps %g must be finite and > 0", who, (double)p->eps);
    MID_REQUIRE((p->format & ~0xffff) == 0 && fmt_known(fmt_frames(p->format)) && fmt_guide(p->format) >= 0, "%s: unknown format 0x%x", who, p->format);
    return MID_OK;
}

size_t guided_work_bytes(const mid_guided_params *p) { return sizeof(float) * kApplySums * (size_t)p->width * (size_t)p->height; }

int guided_out(mid_ctx *ctx, const mid_guided_params *p, const void *in, const void *guide, void *work, void *out, int out_fmt, hipStream_t s)
{
    (void)ctx;
    const int fi = fmt_frames(p->format), fg = guide && guide != in ? fmt_guide(p->format) : fi;
    const void *g = guide ? guide : in;
    const unsigned tiles = guided_tiles(p->width, p->height, p->radius), groups = tiles < kGuidedGroups ? tiles : kGuidedGroups;
    hipLaunchKernelGGL(guided_model_kernel, dim3(groups), dim3(kGuidedLanes), 0, s, in, g, (float *)work, p->width, p->height, p->radius, (double)p->eps, fi, fg);
    MID_HIP(hipGetLastError());
    hipLaunchKernelGGL(guided_apply_kernel, dim3(groups), dim3(kGuidedLanes), 0, s, in, g, (const float *)work, out, p->width, p->height, p->radius, fi, fg,
                       out_fmt);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

}  // namespace mid

using namespace mid;

extern "C" int mid_guided_workspace(const mid_guided_params *p, size_t *bytes)
{
    const char *who = "guided_workspace";
    MID_REQUIRE(bytes != nullptr, "%s: bytes is NULL", who);
    if (int rc = guided_check(p, who)) return rc;
    *bytes = guided_work_bytes(p);
    return MID_OK;
}

extern "C" int mid_guided_filter(mid_ctx *ctx, const mid_guided_params *p, const void *in, const void *guide, void *work, void *out, int out_format,
                                 void *stream)
{
    Bind bind(ctx, stream);
    if (bind.rc) return bind.rc;
    const char *who = "guided_filter";
    if (int rc = guided_check(p, who)) return rc;
    MID_REQUIRE(in && work && out, "%s: NULL pointer", who);
    MID_REQUIRE(fmt_known(out_format), "%s: unknown out_format %d", who, out_format);
    const int fi = fmt_frames(p->format), fg = fmt_guide(p->format);
    MID_REQUIRE(guide != in || fg == fi, "%s: guide == in, but the format word 0x%x names another guide format", who, p->format);
    const bool self = guide == nullptr || guide == in;
    const size_t npix = (size_t)p->width * p->height, ni = npix * fmt_bytes(fi), ng = self ? 0 : npix * fmt_bytes(fg);
    const size_t no = npix * fmt_bytes(out_format), nw = guided_work_bytes(p);
    MID_REQUIRE(((uintptr_t)in & (fmt_bytes(fi) - 1)) == 0, "%s: in is not %d-byte aligned", who, (int)fmt_bytes(fi));
    MID_REQUIRE(self || ((uintptr_t)guide & (fmt_bytes(fg) - 1)) == 0, "%s: guide is not %d-byte aligned", who, (int)fmt_bytes(fg));
    MID_REQUIRE(((uintptr_t)out & (fmt_bytes(out_format) - 1)) == 0, "%s: out is not %d-byte aligned", who, (int)fmt_bytes(out_format));
    MID_REQUIRE(((uintptr_t)work & 15) == 0, "%s: work is not 16-byte aligned", who);
    MID_REQUIRE(!ranges_overlap(out, no, in, ni) && !ranges_overlap(out, no, guide, ng), "%s: out overlaps an input (the pass is a stencil: not in place)", who);
    MID_REQUIRE(!ranges_overlap(work, nw, in, ni) && !ranges_overlap(work, nw, guide, ng), "%s: work overlaps an input", who);
    MID_REQUIRE(!ranges_overlap(out, no, work, nw), "%s: out overlaps work", who);
    return guided_out(ctx, p, in, guide, work, out, out_format, bind.s);
}
