// median.hip -- the median and the layer-weighted median (include/mi_denoise.h, section a4p).
//
// Per pixel p and channel c of r, g, b, C the widened texel, the taps q of the (2 R + 1)^2 window cut at the image:
//   w(q) = 1 (no layers), or 2^arg with arg the FMA chain of a4g over the layers (no colour term, no K(o)); not finite or arg < -126: 0
//   V_c = the taps with C_c(q) finite and w(q) > 0;  W = sum_{V_c} w;  S(v) = sum_{q in V_c, C_c(q) <= v} w(q)
//   out_c = min { C_c(q) : q in V_c, 2 S(C_c(q)) >= W }      (V_c empty: C_c(p));      out.a = in.a
// Every class forms the SAME fp32 sums: a tap's place in them is its place in the window, rows top to bottom, a row left to right,
// and a tap that takes no part (outside the image, not finite, weight 0) adds an exact 0 there -- so the bits do not depend on the
// class.  The selection is rank counting: the window's values and weights of one channel sit in registers under constant indices,
// S_i = sum_j w_j [v_j <= v_i] for every candidate i, and the answer is the smallest v_i with 2 S_i >= W.  A tap that takes no part
// is carried as (v, w) = (+Inf, 0): it neither adds to a sum nor wins the minimum, and the tap loop has no edge branch.
//
// Kernel classes:
//   * median_tiled_kernel<R> (n_layers <= 4): four waves, a 64 x 16 tile, lanes along x, a lane owning the four pixels of rows
//     4 wave .. 4 wave + 3 of its column one after the other.  The LDS tile (csrc/median_tile.hpp) holds the colour as three float
//     planes -- NaN outside the image, so "outside" and "not valid" are one case -- and three already-scaled planes per layer, decoded
//     from the guide format at the fill.  Per pixel the weights are computed once, per channel the window is read from LDS once.
//   * the plain selection class, inside the tiled kernels: with no layers, and a workgroup's vote saying that every texel of its
//     tile is inside the image with finite r, g, b, the taps go through a min / max / v_med3_f32 selection network instead: the
//     9-input median network at radius 1, forgetful selection (select_median) over 25 and 49 inputs at radius 2 and 3.  A median
//     is a selection, so the values are the general class's.
//   * median_global_kernel<R> (n_layers 5..16, or a device whose LDS does not hold the tile): one pixel per lane, 64 x 4 pixels per
//     workgroup, taps from global memory (a tap outside the image reads the centre's address and takes no part), same arithmetic.
// Tiles are dealt to at most kMedianGroupsPerCu workgroups per CU; a workgroup strides.  No scratch memory, no atomics.
#include "common.hpp"
#include "median_tile.hpp"
#include <cmath>

namespace mid {

namespace {

constexpr int kMedianGroupsPerCu = 4;

struct MedianArgs {
    int w, h;
    int fmt, gfmt;                      // MID_FMT_* of the frame / of the guide layers
    int n_layers;
    int out_fmt;
    const void *in;
    void *out;
    float scl[kMaxLayers];              // per layer: sqrt(.5 log2 e) / sigma_l, what a guide value is multiplied by
    const void *layer[kMaxLayers];
};

__device__ __forceinline__ float4 load_texel(const void *img, int fmt, size_t idx)
{
    if (fmt == MID_FMT_RGBA8) return decode_rgba8(((const uint32_t *)img)[idx]);
    if (fmt == MID_FMT_RGBA16F) return decode_rgba16f(((const uint2 *)img)[idx]);
    return ((const float4 *)img)[idx];
}

__device__ __forceinline__ float channel(float4 c, int k) { return k == 0 ? c.x : k == 1 ? c.y : c.z; }

// 2^arg; 0 below the normal range (v_exp_f32 is not asked for a subnormal) and where arg is NaN (a NaN guide texel at p or q, or
// Inf against Inf; one Inf alone gives arg = -Inf)
__device__ __forceinline__ float weight_of(float arg)
{
    return arg >= -126.f ? __builtin_amdgcn_exp2f(arg) : 0.f;
}

// The lower weighted median of one channel's window: v[i] = +Inf and w[i] = 0 where tap i takes no part.
template <int T>
__device__ __forceinline__ float rank_select(const float (&v)[T], const float (&w)[T], float centre)
{
    float W = 0.f;
#pragma unroll
    for (int j = 0; j < T; ++j) W += w[j];
    float best = INFINITY;
#pragma unroll
    for (int i = 0; i < T; ++i) {
        float S = 0.f;
#pragma unroll
        for (int j = 0; j < T; ++j) S += v[j] <= v[i] ? w[j] : 0.f;
        best = fminf(best, S + S >= W ? v[i] : INFINITY);
    }
    return W > 0.f ? best : centre;
}

__device__ __forceinline__ float min3(float a, float b, float c) { return fminf(fminf(a, b), c); }
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
__device__ __forceinline__ float med3(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }

// The median of nine finite values: every column of three sorted, then the largest of the minima, the median of the medians and
// the smallest of the maxima, and the median of those three.
__device__ __forceinline__ float median9(const float (&v)[9])
{
    const float lo = max3(min3(v[0], v[3], v[6]), min3(v[1], v[4], v[7]), min3(v[2], v[5], v[8]));
    const float mi = med3(med3(v[0], v[3], v[6]), med3(v[1], v[4], v[7]), med3(v[2], v[5], v[8]));
    const float hi = min3(max3(v[0], v[3], v[6]), max3(v[1], v[4], v[7]), max3(v[2], v[5], v[8]));
    return med3(lo, mi, hi);
}

__device__ __forceinline__ void sort2(float &a, float &b)
{
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo; b = hi;
}

// The median of T finite values (T odd) by forgetful selection: of any (T + 3) / 2 values of the T the smallest has at least
// (T + 1) / 2 values above or equal and the largest as many below or equal, so neither is the median unless it equals it; both are
// dropped, which leaves the median of the rest where it was, one unread value joins, and the window is one shorter.  Three values are
// left at the end.  A round moves the smallest of the window e[lo .. K) to e[lo] and the largest to e[K - 1] with about 1.5 n
// exchanges: every value against its mirror, then the lower half against e[lo] and the upper half against e[K - 1].
// 99 + 49 exchanges at T = 25 and 345 + 172 at T = 49, two operations each, against 3 T^2 of counting ranks.
template <int T>
__device__ __forceinline__ float select_median(float (&e)[T])
{
    constexpr int K = (T + 3) / 2;
#pragma unroll
    for (int lo = 0; lo + 3 < K; ++lo) {
        const int n = K - lo;
#pragma unroll
        for (int i = 0; i < n / 2; ++i) sort2(e[lo + i], e[K - 1 - i]);
#pragma unroll
        for (int i = 1; i <= (n - 1) / 2; ++i) sort2(e[lo], e[lo + i]);
#pragma unroll
        for (int i = n / 2; i < n - 1; ++i) sort2(e[lo + i], e[K - 1]);
        e[K - 1] = e[K + lo];                                   // the largest is dropped for the next unread value; lo + 1 drops the smallest
    }
    return med3(e[K - 3], e[K - 2], e[K - 1]);
}

// The weights of a pixel's window from the tile's guide planes (layer l: planes 3 l .. 3 l + 2 of N floats each at g): a4g's chain.
template <int R, int NL>
__device__ __forceinline__ void tile_weights(const float *g, int N, int TW, int base, float (&wt)[(2 * R + 1) * (2 * R + 1)])
{
    constexpr int D = 2 * R + 1;
    float cx[NL], cy[NL], cz[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const float *gp = g + 3 * l * N + base + R * TW + R;
        cx[l] = gp[0]; cy[l] = gp[N]; cz[l] = gp[2 * N];
    }
#pragma unroll
    for (int k = 0; k < D * D; ++k) {
        float arg = 0.f;
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const float *gp = g + 3 * l * N + base + (k / D) * TW + k % D;
            const float dx = cx[l] - gp[0], dy = cy[l] - gp[N], dz = cz[l] - gp[2 * N];
            arg = fmaf(-dz, dz, fmaf(-dy, dy, fmaf(-dx, dx, arg)));
        }
        wt[k] = weight_of(arg);
    }
}

template <int R>
__global__ __launch_bounds__(256) void median_tiled_kernel(const MedianArgs a)
{
    constexpr int TW = kMedianTileW + 2 * R, TH = kMedianTileH + 2 * R, N = TW * TH, D = 2 * R + 1, T = D * D;
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = a.w, h = a.h, L = a.n_layers;
    const unsigned tiles_x = (unsigned)median_tiles_x(w), tiles = tiles_x * (unsigned)median_tiles_y(h);
    float *guide = lds + 3 * N;
    unsigned *vote = (unsigned *)(lds + (3 + 3 * L) * N);

    for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int tile_y = (int)(t / tiles_x), tile_x = (int)(t - (unsigned)tile_y * tiles_x);
        if (tid == 0) vote[0] = 1u;
        bool mine = true;               // every texel THIS thread stored is inside the image with finite r, g, b
        for (int f = tid; f < N; f += 256) {
            const MedianSlot s = median_fill_slot(R, tile_x, tile_y, f, w, h);
            const size_t at = s.inside ? median_flat(s.x, s.y, w) : 0;
            float4 c = make_float4(NAN, NAN, NAN, NAN);
            if (s.inside) c = load_texel(a.in, a.fmt, at);
            lds[f] = c.x; lds[N + f] = c.y; lds[2 * N + f] = c.z;
            mine = mine && fabsf(c.x) < INFINITY && fabsf(c.y) < INFINITY && fabsf(c.z) < INFINITY;
            for (int l = 0; l < L; ++l) {
                float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
                if (s.inside) g = load_texel(a.layer[l], a.gfmt, at);
                const float sc = a.scl[l];
                float *gp = guide + 3 * l * N + f;
                gp[0] = g.x * sc; gp[N] = g.y * sc; gp[2 * N] = g.z * sc;
            }
        }
        __syncthreads();
        if (!mine) vote[0] = 0u;
        __syncthreads();
        const bool all_finite = __builtin_amdgcn_readfirstlane((int)vote[0]) != 0;

#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const int row = 4 * wave + j;
            const int x = tile_x * kMedianTileW + lane, y = tile_y * kMedianTileH + row;
            if (x >= w || y >= h) continue;
            const int base = row * TW + lane;                   // the window's top-left slot; the centre is base + R TW + R
            const size_t at = median_flat(x, y, w);
            const float4 cen = load_texel(a.in, a.fmt, at);
            float o0 = cen.x, o1 = cen.y, o2 = cen.z;
            if (L == 0 && all_finite) {                         // the plain selection class (wave-uniform)
#pragma unroll 1
                for (int c = 0; c < 3; ++c) {
                    float v[T];
#pragma unroll
                    for (int k = 0; k < T; ++k) v[k] = lds[c * N + base + (k / D) * TW + k % D];
                    float m;
                    if constexpr (R == 1) m = median9(v); else m = select_median<T>(v);
                    if (c == 0) o0 = m; else if (c == 1) o1 = m; else o2 = m;
                }
            } else {
                float wt[T];
                switch (L) {
                case 0:
#pragma unroll
                    for (int k = 0; k < T; ++k) wt[k] = 1.f;
                    break;
                case 1: tile_weights<R, 1>(guide, N, TW, base, wt); break;
                case 2: tile_weights<R, 2>(guide, N, TW, base, wt); break;
                case 3: tile_weights<R, 3>(guide, N, TW, base, wt); break;
                default: tile_weights<R, 4>(guide, N, TW, base, wt); break;
                }
                static_assert(kMedianTiledLayers == 4, "one weight loop per layer count");
#pragma unroll 1
                for (int c = 0; c < 3; ++c) {
                    float v[T], ww[T];
#pragma unroll
                    for (int k = 0; k < T; ++k) {
                        const float val = lds[c * N + base + (k / D) * TW + k % D];
                        const bool valid = fabsf(val) < INFINITY && wt[k] > 0.f;
                        v[k] = valid ? val : INFINITY;
                        ww[k] = valid ? wt[k] : 0.f;
                    }
                    const float m = rank_select<T>(v, ww, channel(cen, c));
                    if (c == 0) o0 = m; else if (c == 1) o1 = m; else o2 = m;
                }
            }
            store_out(a.out, at, a.out_fmt, make_float4(o0, o1, o2, cen.w));
        }
        __syncthreads();                                        // the tile is filled again
    }
}

template <int R>
__global__ __launch_bounds__(256) void median_global_kernel(const MedianArgs a)
{
    constexpr int D = 2 * R + 1, T = D * D;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int w = a.w, h = a.h, L = a.n_layers;
    if (x >= w || y >= h) return;
    const size_t ci = median_flat(x, y, w);
    size_t at[T];                                               // a tap outside the image: the centre's address, and `in` says so
    bool in[T];
#pragma unroll
    for (int k = 0; k < T; ++k) {
        const int xx = x + k % D - R, yy = y + k / D - R;
        in[k] = xx >= 0 && xx < w && yy >= 0 && yy < h;
        at[k] = in[k] ? median_flat(xx, yy, w) : ci;
    }
    float arg[T];
#pragma unroll
    for (int k = 0; k < T; ++k) arg[k] = 0.f;
#pragma unroll 1
    for (int l = 0; l < L; ++l) {                               // layer by layer: every tap's chain still runs layer 0, 1, ...
        const void *layer = a.layer[l];
        const float sc = a.scl[l];
        const float4 g0 = load_texel(layer, a.gfmt, ci);
        const float cx = g0.x * sc, cy = g0.y * sc, cz = g0.z * sc;
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const float4 g = load_texel(layer, a.gfmt, at[k]);
            const float dx = cx - g.x * sc, dy = cy - g.y * sc, dz = cz - g.z * sc;
            arg[k] = fmaf(-dz, dz, fmaf(-dy, dy, fmaf(-dx, dx, arg[k])));
        }
    }
    float wt[T];
#pragma unroll
    for (int k = 0; k < T; ++k) wt[k] = in[k] ? (L ? weight_of(arg[k]) : 1.f) : 0.f;
    const float4 cen = load_texel(a.in, a.fmt, ci);
    float o0 = cen.x, o1 = cen.y, o2 = cen.z;
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        float v[T], ww[T];
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const float val = channel(load_texel(a.in, a.fmt, at[k]), c);
            const bool valid = fabsf(val) < INFINITY && wt[k] > 0.f;
            v[k] = valid ? val : INFINITY;
            ww[k] = valid ? wt[k] : 0.f;
        }
        const float m = rank_select<T>(v, ww, channel(cen, c));
        if (c == 0) o0 = m; else if (c == 1) o1 = m; else o2 = m;
    }
    store_out(a.out, ci, a.out_fmt, make_float4(o0, o1, o2, cen.w));
}

template <int R>
int launch_median(mid_ctx *ctx, const MedianArgs &a, hipStream_t s)
{
    const size_t lds_bytes = median_lds_bytes(R, a.n_layers);
    if (a.n_layers <= kMedianTiledLayers && lds_bytes <= (size_t)ctx->lds_max) {
        auto kern = median_tiled_kernel<R>;
        if (int rc = ensure_lds(ctx, (const void *)kern, (size_t)ctx->lds_max)) return rc;
        const size_t tiles = (size_t)median_tiles_x(a.w) * median_tiles_y(a.h), cap = (size_t)ctx->cu_count * kMedianGroupsPerCu;
        hipLaunchKernelGGL(kern, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(256), lds_bytes, s, a);
    } else {
        hipLaunchKernelGGL(median_global_kernel<R>, dim3(cdiv(a.w, 64), cdiv(a.h, 4)), dim3(256), 0, s, a);
    }
    MID_HIP(hipGetLastError());
    return MID_OK;
}

bool ranges_overlap(const void *p, size_t np, const void *q, size_t nq)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return np && nq && a < b + nq && b < a + np;
}

}  // namespace

// What the entry point and the sequence check before their pointers.
int median_check(const mid_median_params *p, const char *who, const float *layer_sigma, bool have_layers, int n_layers)
{
    MID_REQUIRE(p != nullptr, "%s: params is NULL", who);
    MID_REQUIRE(p->width > 0 && p->height > 0, "%s: bad size %dx%d", who, p->width, p->height);
    MID_REQUIRE((long)p->width * p->height < (1l << 30), "%s: image too large", who);
    MID_REQUIRE(p->radius >= 1 && p->radius <= kMedianMaxRadius, "%s: radius %d outside 1..%d", who, p->radius, kMedianMaxRadius);
    MID_REQUIRE((p->format & ~0xffff) == 0 && fmt_known(fmt_frames(p->format)), "%s: unknown format 0x%x", who, p->format);
    MID_REQUIRE(fmt_guide(p->format) >= 0, "%s: unknown guide-layer format code %d in format 0x%x", who, p->format >> 8, p->format);
    MID_REQUIRE(n_layers >= 0 && n_layers <= kMaxLayers, "%s: n_layers %d outside 0..16", who, n_layers);
    if (n_layers == 0) {
        MID_REQUIRE(!have_layers && layer_sigma == nullptr, "%s: a layer table or sigma table with n_layers == 0 (the plain median takes NULL for both)", who);
        MID_REQUIRE((p->format >> 8) == 0, "%s: guide bits set in format 0x%x, but the plain median reads no guide layer", who, p->format);
        return MID_OK;
    }
    MID_REQUIRE(have_layers, "%s: the layer table is NULL", who);
    MID_REQUIRE(layer_sigma != nullptr, "%s: layer_sigma is NULL", who);
    for (int l = 0; l < n_layers; ++l)
        MID_REQUIRE(std::isfinite(layer_sigma[l]) && layer_sigma[l] > 0.f, "%s: sigmas must be finite and > 0 (layer_sigma[%d] = %g)", who, l, (double)layer_sigma[l]);
    return MID_OK;
}

int median_out(mid_ctx *ctx, const mid_median_params *p, const float *layer_sigma, const void *in, const uint32_t *const *layers, int n_layers,
               void *out, int out_fmt, hipStream_t s)
{
    MedianArgs a{};
    a.w = p->width; a.h = p->height;
    a.fmt = fmt_frames(p->format); a.gfmt = fmt_guide(p->format);
    a.n_layers = n_layers;
    a.out_fmt = out_fmt;
    a.in = in; a.out = out;
    const double c = sqrt(0.5 * 1.4426950408889634);
    for (int l = 0; l < n_layers; ++l) {
        a.scl[l] = (float)(c / (double)layer_sigma[l]);
        a.layer[l] = layers[l];
    }
    switch (p->radius) {
    case 1: return launch_median<1>(ctx, a, s);
    case 2: return launch_median<2>(ctx, a, s);
    default: return launch_median<3>(ctx, a, s);
    }
}

}  // namespace mid

using namespace mid;

extern "C" int mid_median_filter(mid_ctx *ctx, const mid_median_params *p, const float *layer_sigma, const void *in,
                                 const uint32_t *const *layers, int n_layers, void *out, int out_format, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    const char *who = "median_filter";
    if (int rc = median_check(p, who, layer_sigma, layers != nullptr, n_layers)) return rc;
    MID_REQUIRE(in && out, "%s: NULL image", who);
    MID_REQUIRE(fmt_known(out_format), "%s: unknown output format %d", who, out_format);
    const int fmt = fmt_frames(p->format), gfmt = fmt_guide(p->format);
    const size_t npix = (size_t)p->width * p->height;
    MID_REQUIRE(((uintptr_t)in & (fmt_bytes(fmt) - 1)) == 0, "%s: in is not %d-byte aligned", who, (int)fmt_bytes(fmt));
    MID_REQUIRE(((uintptr_t)out & (fmt_bytes(out_format) - 1)) == 0, "%s: out is not %d-byte aligned", who, (int)fmt_bytes(out_format));
    const size_t in_bytes = npix * fmt_bytes(fmt), out_bytes = npix * fmt_bytes(out_format), layer_bytes = npix * fmt_bytes(gfmt);
    MID_REQUIRE(!ranges_overlap(out, out_bytes, in, in_bytes), "%s: out overlaps in (the filter is a stencil: not even exactly in place)", who);
    for (int l = 0; l < n_layers; ++l) {
        MID_REQUIRE(layers[l] != nullptr, "%s: layer %d is NULL", who, l);
        MID_REQUIRE(((uintptr_t)layers[l] & (fmt_bytes(gfmt) - 1)) == 0, "%s: layer %d is not %d-byte aligned", who, l, (int)fmt_bytes(gfmt));
        MID_REQUIRE(!ranges_overlap(out, out_bytes, layers[l], layer_bytes), "%s: out overlaps layer %d", who, l);
    }
    return median_out(ctx, p, layer_sigma, in, layers, n_layers, out, out_format, b.s);
}
