// atrous_variance.hip -- the variance-guided a-trous filter (include/mi_denoise.h, section a4i): the luminance moments that
// estimate a per-pixel variance, and the a-trous passes whose colour term is steered by that variance and that filter it along
// with the colour.
//
// Luminance everywhere: l(C) = fmaf(0.0722f, b, fmaf(0.7152f, g, 0.2126f * r)) of the widened fp32 texel.
//
// 1. mid_atrous_moments.  Output frame t, window f = max(0, t-k) .. min(n-1, t+k), a 7 x 7 neighbourhood in every frame:
//     w = 2^arg, arg = a4g's layer chain between G[t][l](p) and G[f][l](q) (no spatial kernel), 0 for q outside the image
//     d = l(C[f](q)) - l(C[t](p));   W += w;  wd = w d;  s1 += wd;  s2 = fmaf(wd, d, s2)
//     frames ascending, inside a frame j = -3 .. 3, then i = -3 .. 3
//     m = s1 / W;  v = fmaf(-m, m, s2 / W);  V_0(p) = v < 0 ? 0 : v
//   * moments_tiled_kernel (n_layers <= 4): 64 x 16 pixels per workgroup of eight waves, two rows per wave.  Per neighbour frame
//     a 70 x 22 tile is refilled: ONE plane of luminances and 3 L planes of scaled guide values (the colour itself is never
//     needed again).  The centres and the three sums of both rows stay in registers across the neighbours; two barriers per
//     neighbour, lanes right of the image and rows below it stay in the loop and skip their work.
//   * moments_global_kernel (n_layers 5 .. 16, and a device whose LDS does not hold the tile): one pixel per lane, global taps.
//
// 2. mid_atrous_variance.  Pass i at step s = 2^i over the colour level C_i and the variance plane V_i:
//     vt(p)  = sum g(i) g(j) V_i(p + (i, j)) / sum g(i) g(j),  g = (1, 2, 1) / 4, |i|, |j| <= 1 at step 1, in-image taps, j then i,
//              num = fmaf(g g, V, num), den += g g, one IEEE division
//     scv(p) = (float)log2(e) / fmaf(sigmaLum, sqrtf(vt(p)), epsilon)
//     arg    = a4g's layer chain from 0, then arg = fmaf(-|l(C_i(p)) - l(C_i(q))|, scv(p), arg)
//     w      = K(o) 2^arg, 0 outside;  acc = fmaf(C_i(q), w, acc), accw += w, accv = fmaf(w w, V_i(q), accv)
//     C_{i+1}(p) = acc / accw per channel,  V_{i+1}(p) = accv / (accw accw)
//   sigmaLum == 0: no luminance term, vt is not loaded, and the colour chain is atrous.hip's with colorSigma = 0, bit for bit.
//   * variance_comb_kernel<P> (steps 1 .. 32, n_layers <= 4): atrous.hip's row comb with one more plane in the tile -- float4
//     colour, one float of V, 3 L floats of scaled guides per texel.  vt(p) comes from global memory (nine loads over three image
//     rows: in a comb tile the rows y +- 1 belong to other residue classes).
//   * variance_global_kernel (steps 64 and 128, n_layers 5 .. 16, and whatever does not fit LDS): one pixel per lane.
// A launch knows its step and nothing of n_passes: passes [0, N) in one call are N one-pass calls, bit for bit.
//
// The few device helpers shared with atrous.hip (b3, load_texel, the LDS byte formula) are restated here, as in
// atrous_temporal.hip: atrous.hip keeps its text and its code object.
#include "common.hpp"
#include <cmath>

namespace mid {

namespace {

constexpr int kMaxPtrs = MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS;
constexpr int kAVTiledLayers = 4;       // layers the LDS kernels keep resident
constexpr int kAVCuLds = 163840;        // LDS of one CU: what two workgroups must share to be resident together
constexpr int kAVNW = 8;                // waves per workgroup
constexpr int kAVCombMaxStep = 32;      // the row comb takes the steps up to this one; beyond it: global taps
constexpr int kAVMaxPasses = 8;
constexpr int kMomR = 3;                // the moments' neighbourhood: 7 x 7
constexpr int kMomP = 2;                // rows per wave of the moments' tiled kernel: a 64 x 16 tile

// One texel at flat index idx, the format a run-time (wave-uniform) value; the caller keeps idx inside the image.
__device__ __forceinline__ float4 load_texel(const void *img, int fmt, size_t idx)
{
    if (fmt == MID_FMT_RGBA8) return decode_rgba8(((const uint32_t *)img)[idx]);
    if (fmt == MID_FMT_RGBA16F) return decode_rgba16f(((const uint2 *)img)[idx]);
    return ((const float4 *)img)[idx];
}

// the B3-spline factor (1, 4, 6, 4, 1) / 16 of offset d = -2 .. 2
__device__ __forceinline__ constexpr float b3(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// Rec. 709 luminance of a widened texel: the one formula of section a4i
__device__ __forceinline__ float lum(float4 c) { return fmaf(0.0722f, c.z, fmaf(0.7152f, c.y, 0.2126f * c.x)); }

template <int N> struct LayerCount { static constexpr int value = N; };

bool ranges_overlap(const void *p, size_t np, const void *q, size_t nq)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return np && nq && a < b + nq && b < a + np;
}

// ---- 1. the moments ---------------------------------------------------------------------------------------------------------------

struct MomentsArgs {
    int w, h;
    int fmt, gfmt;                      // MID_FMT_* of the frames, of the layers
    int tiles_x, tiles_y;
    int n_nb;                           // frames of the window: slots [0, n_nb)
    int n_layers;
    int t_slot;                         // the window slot that is the output frame itself
    float *var_out;
    float scl[kMaxLayers];              // per layer: sqrt(.5 log2 e) / sigma_l
    const void *p[kMaxPtrs];            // slot j: p[j * (n_layers + 1)] = frame, then its n_layers guide layers
};
static_assert(sizeof(MomentsArgs) <= 4096, "one kernel argument block");

__device__ __forceinline__ const void *nb_frame(const MomentsArgs &a, int f) { return a.p[f * (a.n_layers + 1)]; }
__device__ __forceinline__ const void *nb_layer(const MomentsArgs &a, int f, int l) { return a.p[f * (a.n_layers + 1) + 1 + l]; }

constexpr int kMomLW = 64 + 2 * kMomR, kMomLH = kAVNW * kMomP + 2 * kMomR;          // the 70 x 22 tile
constexpr size_t moments_lds_bytes(int n_layers) { return (size_t)kMomLW * kMomLH * sizeof(float) * (1 + 3 * (size_t)n_layers); }
static_assert(moments_lds_bytes(1) == 24640 && moments_lds_bytes(4) == 80080 && 2 * moments_lds_bytes(4) <= kAVCuLds, "a4i's class table");
inline bool moments_tiled(int lds_max, int n_layers) { return n_layers <= kAVTiledLayers && (int)moments_lds_bytes(n_layers) <= lds_max; }

__device__ __forceinline__ void put_moments(float *out, size_t idx, float W, float s1, float s2)
{
    const float m = s1 / W;
    const float v = fmaf(-m, m, s2 / W);
    out[idx] = v < 0.f ? 0.f : v;                          // (a NaN stays a NaN)
}

__global__ __launch_bounds__(kAVNW * 64) void moments_tiled_kernel(const MomentsArgs a)
{
    constexpr int MAXL = kAVTiledLayers, P = kMomP, R = kMomR, TR = kAVNW * P, LW = kMomLW, LH = kMomLH, N = LW * LH;
    extern __shared__ float lds_f[];
    float *lum_t = lds_f;                                  // luminance tile of the neighbour
    float *gde_t = lds_f + N;                              // its layer l: planes x, y, z at gde_t + (3 l + {0, 1, 2}) * N

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
    const int w = a.w, h = a.h, L = a.n_layers;
    const int X0 = tx * 64, Y0 = ty * TR;
    const int gx = X0 + lane, yb = Y0 + wv * P;

    // the centres: l(C[t](p)) and G[t][l](p) sc_l of this thread's P pixels, with a tile texel's decode, luminance and multiply; a
    // lane right of the image or a row below it holds zeros and stores nothing
    float lc[P];
    float cx[MAXL][P], cy[MAXL][P], cz[MAXL][P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const bool inside = gx < w && yb + k < h;
        const size_t ci = inside ? (size_t)(yb + k) * w + gx : 0;
        lc[k] = 0.f;
        if (inside) lc[k] = lum(load_texel(nb_frame(a, a.t_slot), a.fmt, ci));
#pragma unroll
        for (int l = 0; l < MAXL; ++l) {
            cx[l][k] = cy[l][k] = cz[l][k] = 0.f;
            if (l < L && inside) {
                const float4 g = load_texel(nb_layer(a, a.t_slot, l), a.gfmt, ci);
                const float sc = a.scl[l];
                cx[l][k] = g.x * sc; cy[l][k] = g.y * sc; cz[l][k] = g.z * sc;
            }
        }
    }

    float sW[P], s1[P], s2[P];
#pragma unroll
    for (int k = 0; k < P; ++k) sW[k] = s1[k] = s2[k] = 0.f;

    for (int f = 0; f < a.n_nb; ++f) {
        __syncthreads();                                   // every wave has left the previous neighbour's tap loop
        // fill: a texel's luminance and its L guide texels are loaded together; out-of-image texels are zero (their taps weigh 0)
        const void *frame = nb_frame(a, f);
        for (int t = tid; t < N; t += kAVNW * 64) {
            const int r = t / LW, c = t - r * LW;
            const int x = X0 - R + c, y = Y0 - R + r;
            const bool inside = (unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h;
            const size_t idx = inside ? (size_t)y * w + x : 0;
            float lq = 0.f;
            if (inside) lq = lum(load_texel(frame, a.fmt, idx));
            lum_t[t] = lq;
            for (int l = 0; l < L; ++l) {
                float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
                if (inside) g = load_texel(nb_layer(a, f, l), a.gfmt, idx);
                const float sc = a.scl[l];
                float *gp = gde_t + 3 * l * N + t;
                gp[0] = g.x * sc; gp[N] = g.y * sc; gp[2 * N] = g.z * sc;
            }
        }
        __syncthreads();

        auto taps = [&](auto nl_tag) {
            constexpr int NL = decltype(nl_tag)::value;
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const int gy = yb + k;
                if (gy >= h) continue;                      // (wave-uniform, and no barrier inside: the wave rejoins below)
                const int ct = (wv * P + k + R) * LW + lane + R;
#pragma unroll 1
                for (int j = -R; j <= R; ++j) {             // a tap row at a time
                    const bool row_in = (unsigned)(gy + j) < (unsigned)h;
#pragma unroll
                    for (int i = -R; i <= R; ++i) {
                        const bool valid = row_in && (unsigned)(gx + i) < (unsigned)w;
                        const int t = ct + j * LW + i;
                        float arg = 0.f;
#pragma unroll
                        for (int l = 0; l < NL; ++l) {
                            const float *gp = gde_t + 3 * l * N + t;
                            const float dx = cx[l][k] - gp[0], dy = cy[l][k] - gp[N], dz = cz[l][k] - gp[2 * N];
                            arg = fmaf(-dz, dz, fmaf(-dy, dy, fmaf(-dx, dx, arg)));
                        }
                        float wt = __builtin_amdgcn_exp2f(arg);
                        wt = valid ? wt : 0.f;
                        const float d = lum_t[t] - lc[k];
                        const float wd = wt * d;
                        sW[k] += wt;
                        s1[k] += wd;
                        s2[k] = fmaf(wd, d, s2[k]);
                    }
                }
            }
        };
        static_assert(kAVTiledLayers == 4, "one tap loop per layer count");
        switch (L) {
        case 1: taps(LayerCount<1>{}); break;
        case 2: taps(LayerCount<2>{}); break;
        case 3: taps(LayerCount<3>{}); break;
        default: taps(LayerCount<4>{}); break;
        }
    }

    if (gx >= w) return;                                   // after the last barrier
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int gy = yb + k;
        if (gy < h) put_moments(a.var_out, (size_t)gy * w + gx, sW[k], s1[k], s2[k]);
    }
}

// Every n_layers > 4 (and what does not fit LDS): one pixel per lane, the taps of every neighbour from global memory.  A tap
// outside the image reads the centre's address instead (a valid one), counts as luminance 0 as a tile texel would, and weighs 0.
__global__ __launch_bounds__(256) void moments_global_kernel(const MomentsArgs a)
{
    constexpr int R = kMomR;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int w = a.w, h = a.h, L = a.n_layers;
    if (x >= w || y >= h) return;                          // (no barrier in this kernel)
    const size_t ci = (size_t)y * w + x;
    float cx[kMaxLayers], cy[kMaxLayers], cz[kMaxLayers];       // G[t][l](p) sc_l of every layer (constant indices: registers)
#pragma unroll
    for (int l = 0; l < kMaxLayers; ++l) {
        cx[l] = cy[l] = cz[l] = 0.f;
        if (l < L) {
            const float4 g = load_texel(nb_layer(a, a.t_slot, l), a.gfmt, ci);
            const float sc = a.scl[l];
            cx[l] = g.x * sc; cy[l] = g.y * sc; cz[l] = g.z * sc;
        }
    }
    const float lc = lum(load_texel(nb_frame(a, a.t_slot), a.fmt, ci));
    float sW = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll 1
    for (int f = 0; f < a.n_nb; ++f) {
        const void *frame = nb_frame(a, f);
#pragma unroll 1
        for (int j = -R; j <= R; ++j) {
            const int yy = y + j;
            const bool row_in = yy >= 0 && yy < h;
#pragma unroll 1
            for (int i = -R; i <= R; ++i) {
                const int xx = x + i;
                const bool valid = row_in && xx >= 0 && xx < w;
                const size_t t = valid ? (size_t)yy * w + (size_t)xx : ci;
                float lq = lum(load_texel(frame, a.fmt, t));
                if (!valid) lq = 0.f;                       // what the tiled kernel's tile holds there
                float arg = 0.f;
#pragma unroll
                for (int l = 0; l < kMaxLayers; ++l) {
                    if (l < L) {            // (wave-uniform; an unrolled body per layer keeps cx[l] a register)
                        const float4 g = load_texel(nb_layer(a, f, l), a.gfmt, t);
                        const float sc = a.scl[l];
                        const float dx = cx[l] - g.x * sc, dy = cy[l] - g.y * sc, dz = cz[l] - g.z * sc;
                        arg = fmaf(-dz, dz, fmaf(-dy, dy, fmaf(-dx, dx, arg)));
                    }
                }
                float wt = __builtin_amdgcn_exp2f(arg);
                wt = valid ? wt : 0.f;
                const float d = lq - lc;
                const float wd = wt * d;
                sW += wt;
                s1 += wd;
                s2 = fmaf(wd, d, s2);
            }
        }
    }
    put_moments(a.var_out, ci, sW, s1, s2);
}

// The moments of one output.  The class depends on n_layers and the device's LDS only.
int dispatch_moments(mid_ctx *ctx, MomentsArgs &a, hipStream_t s)
{
    if (moments_tiled(ctx->lds_max, a.n_layers)) {
        auto kern = moments_tiled_kernel;
        if (int rc = ensure_lds(ctx, (const void *)kern, (size_t)ctx->lds_max)) return rc;
        a.tiles_x = (int)cdiv(a.w, 64);
        a.tiles_y = (int)cdiv(a.h, kAVNW * kMomP);
        hipLaunchKernelGGL(kern, dim3((unsigned)a.tiles_x * a.tiles_y), dim3(kAVNW * 64), moments_lds_bytes(a.n_layers), s, a);
        MID_HIP(hipGetLastError());
        return MID_OK;
    }
    hipLaunchKernelGGL(moments_global_kernel, dim3(cdiv(a.w, 64), cdiv(a.h, 4)), dim3(256), 0, s, a);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

// ---- 2. the variance-guided passes ------------------------------------------------------------------------------------------------

struct VarianceArgs {
    int w, h;
    int step;                           // 2^i of this pass
    int fmt, gfmt, out_fmt;             // MID_FMT_* of `in` (the frame's format in the first pass, RGBA32F afterwards), of the layers, of `out`
    int n_layers;
    int use_lum;                        // the luminance term is on (sigmaLum > 0)
    int store_var;                      // this pass stores its variance plane (off only in a last pass with var_out == NULL)
    float sigma_lum, epsilon;
    int tiles_x, tiles_y;
    const void *in;
    const float *var_in;
    void *out;
    float *var_out;
    float scl[kMaxLayers];              // per layer: sqrt(.5 log2 e) / sigma_l
    const void *layer[kMaxLayers];
};

// The row comb of atrous.hip with one float more per texel: bytes of LDS of one workgroup with P rows per wave, and the P a
// (step, n_layers) runs with: two rows per wave while two such workgroups fit one CU's 160 KB, else one.
constexpr size_t variance_comb_lds_bytes(int step, int n_layers, int rows_per_wave)
{
    return (size_t)(64 + 4 * step) * (kAVNW * rows_per_wave + 4) * (sizeof(float4) + sizeof(float) + 3 * sizeof(float) * (size_t)n_layers);
}
constexpr int variance_comb_rows(int step, int n_layers) { return 2 * variance_comb_lds_bytes(step, n_layers, 2) <= kAVCuLds ? 2 : 1; }
inline bool variance_comb(int lds_max, int step, int n_layers)
{
    return step <= kAVCombMaxStep && n_layers <= kAVTiledLayers &&
           (int)variance_comb_lds_bytes(step, n_layers, variance_comb_rows(step, n_layers)) <= lds_max;
}
static_assert(variance_comb_lds_bytes(1, 1, 2) == 43520 && variance_comb_lds_bytes(32, 4, 1) == 156672 && variance_comb_rows(32, 1) == 1,
              "a4i's class table");

// scv(p): the nine variance texels around p (in-image ones), a 3 x 3 Gaussian, and the luminance scale of this pixel
__device__ __forceinline__ float lum_scale(const VarianceArgs &a, int x, long y)
{
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int j = -1; j <= 1; ++j) {
        const long yy = y + j;
        const bool row_in = yy >= 0 && yy < a.h;
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
            const int xx = x + i;
            const bool valid = row_in && xx >= 0 && xx < a.w;
            const float g = (j == 0 ? 0.5f : 0.25f) * (i == 0 ? 0.5f : 0.25f);
            if (valid) {
                num = fmaf(g, a.var_in[(size_t)yy * a.w + (size_t)xx], num);
                den += g;
            }
        }
    }
    const float vt = num / den;
    return 1.44269504088896340736f / fmaf(a.sigma_lum, sqrtf(vt), a.epsilon);
}

__device__ __forceinline__ void put_variance(const VarianceArgs &a, size_t idx, float4 acc, float accw, float accv)
{
    store_out(a.out, idx, a.out_fmt, make_float4(acc.x / accw, acc.y / accw, acc.z / accw, acc.w / accw));
    if (a.store_var) a.var_out[idx] = accv / (accw * accw);
}

template <int P>
__global__ __launch_bounds__(kAVNW * 64) void variance_comb_kernel(const VarianceArgs a)
{
    constexpr int TR = kAVNW * P, LH = TR + 4;
    const int S = a.step, H = 2 * S, LW = 64 + 2 * H, N = LW * LH;
    extern __shared__ float4 lds[];
    float4 *img_t = lds;                                  // colour tile
    float *var_t = (float *)(lds + N);                    // variance tile
    float *gde_t = var_t + N;                             // layer l: planes x, y, z at gde_t + (3 l + {0, 1, 2}) * N

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int by = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - by * a.tiles_x;
    const int y0 = by % S, chunk = by / S;                // the residue class and the run of TR of its rows
    const int w = a.w, h = a.h, L = a.n_layers;
    const int X0 = tx * 64;
    const int Yfirst = y0 + S * chunk * TR;               // image row of tile row 0 of the outputs
    if (Yfirst >= h) return;                              // (a short residue class: the whole workgroup, before any barrier)

    // fill: a texel's colour, its variance and its L guide texels are loaded together; out-of-image texels are zero
    for (int t = tid; t < N; t += kAVNW * 64) {
        const int r = t / LW, c = t - r * LW;
        const int x = X0 - H + c;
        const long y = (long)Yfirst + (long)S * (r - 2);
        const bool inside = (unsigned)x < (unsigned)w && y >= 0 && y < h;
        const size_t idx = inside ? (size_t)y * w + x : 0;
        float4 col = make_float4(0.f, 0.f, 0.f, 0.f);
        float vq = 0.f;
        if (inside) { col = load_texel(a.in, a.fmt, idx); vq = a.var_in[idx]; }
        img_t[t] = col;
        var_t[t] = vq;
        for (int l = 0; l < L; ++l) {
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
            if (inside) g = load_texel(a.layer[l], a.gfmt, idx);
            const float sc = a.scl[l];
            float *gp = gde_t + 3 * l * N + t;
            gp[0] = g.x * sc; gp[N] = g.y * sc; gp[2 * N] = g.z * sc;
        }
    }
    __syncthreads();

    const int gx = X0 + lane;
    if (gx >= w) return;
    const bool use_lum = a.use_lum != 0;

    auto taps = [&](auto nl_tag) {
        constexpr int NL = decltype(nl_tag)::value;
#pragma unroll 1
        for (int k = 0; k < P; ++k) {
            const int rr = wv * P + k;
            const long gy = (long)Yfirst + (long)S * rr;
            if (gy >= h) break;
            const int ct = (rr + 2) * LW + lane + H;
            float cx[NL], cy[NL], cz[NL];
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const float *gp = gde_t + 3 * l * N + ct;
                cx[l] = gp[0]; cy[l] = gp[N]; cz[l] = gp[2 * N];
            }
            const float lc = lum(img_t[ct]);
            const float scv = use_lum ? lum_scale(a, gx, gy) : 0.f;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            float accw = 0.f, accv = 0.f;
#pragma unroll 1
            for (int j = -2; j <= 2; ++j) {     // a tap row at a time
                const long yy = gy + (long)j * S;
                const bool row_in = yy >= 0 && yy < h;
                const float kj = b3(j);
#pragma unroll
                for (int i = -2; i <= 2; ++i) {
                    const long xx = (long)gx + (long)i * S;
                    const bool valid = row_in && xx >= 0 && xx < w;
                    const int t = ct + j * LW + i * S;
                    const float4 q = img_t[t];
                    const float vq = var_t[t];
                    float arg = 0.f;
#pragma unroll
                    for (int l = 0; l < NL; ++l) {
                        const float *gp = gde_t + 3 * l * N + t;
                        const float dx = cx[l] - gp[0], dy = cy[l] - gp[N], dz = cz[l] - gp[2 * N];
                        arg = fmaf(-dz, dz, fmaf(-dy, dy, fmaf(-dx, dx, arg)));
                    }
                    if (use_lum) arg = fmaf(-fabsf(lc - lum(q)), scv, arg);
                    float wt = (b3(i) * kj) * __builtin_amdgcn_exp2f(arg);
                    wt = valid ? wt : 0.f;
                    acc.x = fmaf(q.x, wt, acc.x); acc.y = fmaf(q.y, wt, acc.y);
                    acc.z = fmaf(q.z, wt, acc.z); acc.w = fmaf(q.w, wt, acc.w);
                    accw += wt;
                    accv = fmaf(wt * wt, vq, accv);
                }
            }
            put_variance(a, (size_t)gy * w + gx, acc, accw, accv);
        }
    };
    static_assert(kAVTiledLayers == 4, "one tap loop per layer count");
    switch (L) {
    case 1: taps(LayerCount<1>{}); break;
    case 2: taps(LayerCount<2>{}); break;
    case 3: taps(LayerCount<3>{}); break;
    default: taps(LayerCount<4>{}); break;
    }
}

// Every other (step, n_layers): one pixel per lane, the taps from global memory.  A tap outside the image reads the centre's
// address instead (a valid one), counts as a zero texel with zero variance as a tile texel would, and weighs 0.
__global__ __launch_bounds__(256) void variance_global_kernel(const VarianceArgs a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int w = a.w, h = a.h, L = a.n_layers, s = a.step;
    if (x >= w || y >= h) return;
    const size_t ci = (size_t)y * w + x;
    float cx[kMaxLayers], cy[kMaxLayers], cz[kMaxLayers];       // G_l(p) sc_l of every layer (constant indices: registers)
#pragma unroll
    for (int l = 0; l < kMaxLayers; ++l) {
        cx[l] = cy[l] = cz[l] = 0.f;
        if (l < L) {
            const float4 g = load_texel(a.layer[l], a.gfmt, ci);
            const float sc = a.scl[l];
            cx[l] = g.x * sc; cy[l] = g.y * sc; cz[l] = g.z * sc;
        }
    }
    const float lc = lum(load_texel(a.in, a.fmt, ci));
    const bool use_lum = a.use_lum != 0;
    const float scv = use_lum ? lum_scale(a, x, y) : 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float accw = 0.f, accv = 0.f;
#pragma unroll 1
    for (int j = -2; j <= 2; ++j) {
        const long yy = (long)y + (long)j * s;
        const bool row_in = yy >= 0 && yy < h;
        const float kj = b3(j);
#pragma unroll 1
        for (int i = -2; i <= 2; ++i) {
            const long xx = (long)x + (long)i * s;
            const bool valid = row_in && xx >= 0 && xx < w;
            const size_t t = valid ? (size_t)yy * w + (size_t)xx : ci;
            float4 q = load_texel(a.in, a.fmt, t);
            float vq = a.var_in[t];
            if (!valid) { q = make_float4(0.f, 0.f, 0.f, 0.f); vq = 0.f; }      // what the comb kernel's tile holds there
            float arg = 0.f;
#pragma unroll
            for (int l = 0; l < kMaxLayers; ++l) {
                if (l < L) {                // (wave-uniform; an unrolled body per layer keeps cx[l] a register)
                    const float4 g = load_texel(a.layer[l], a.gfmt, t);
                    const float sc = a.scl[l];
                    const float dx = cx[l] - g.x * sc, dy = cy[l] - g.y * sc, dz = cz[l] - g.z * sc;
                    arg = fmaf(-dz, dz, fmaf(-dy, dy, fmaf(-dx, dx, arg)));
                }
            }
            if (use_lum) arg = fmaf(-fabsf(lc - lum(q)), scv, arg);
            float wt = (b3(i) * kj) * __builtin_amdgcn_exp2f(arg);
            wt = valid ? wt : 0.f;
            acc.x = fmaf(q.x, wt, acc.x); acc.y = fmaf(q.y, wt, acc.y);
            acc.z = fmaf(q.z, wt, acc.z); acc.w = fmaf(q.w, wt, acc.w);
            accw += wt;
            accv = fmaf(wt * wt, vq, accv);
        }
    }
    put_variance(a, ci, acc, accw, accv);
}

template <int P>
int launch_variance_comb(mid_ctx *ctx, VarianceArgs &a, hipStream_t s)
{
    auto kern = variance_comb_kernel<P>;
    if (int rc = ensure_lds(ctx, (const void *)kern, (size_t)ctx->lds_max)) return rc;
    a.tiles_x = (int)cdiv(a.w, 64);
    a.tiles_y = a.step * (int)cdiv(cdiv(a.h, a.step), kAVNW * P);      // per residue class: its ceil(h / step) rows at most, in runs of 8 P
    hipLaunchKernelGGL(kern, dim3((unsigned)a.tiles_x * a.tiles_y), dim3(kAVNW * 64), variance_comb_lds_bytes(a.step, a.n_layers, P), s, a);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

// One pass.  The class depends on (step, n_layers) and the device's LDS only.
int dispatch_variance(mid_ctx *ctx, VarianceArgs &a, hipStream_t s)
{
    if (variance_comb(ctx->lds_max, a.step, a.n_layers))
        return variance_comb_rows(a.step, a.n_layers) == 2 ? launch_variance_comb<2>(ctx, a, s) : launch_variance_comb<1>(ctx, a, s);
    hipLaunchKernelGGL(variance_global_kernel, dim3(cdiv(a.w, 64), cdiv(a.h, 4)), dim3(256), 0, s, a);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

size_t variance_sets(int n_passes) { return n_passes <= 1 ? 0 : n_passes == 2 ? 1 : 2; }      // atrous_scratch_frames

// What both entry points of the family check about layers and sigmas (a4g's rules).
int layers_check(const char *who, const float *layer_sigma, bool have_layers, int n_layers)
{
    MID_REQUIRE(n_layers >= 1 && n_layers <= kMaxLayers, "%s: n_layers %d outside 1..16", who, n_layers);
    MID_REQUIRE(have_layers, "%s: the layer table is NULL", who);
    MID_REQUIRE(layer_sigma != nullptr, "%s: layer_sigma is NULL (there is no sigma to fall back on)", who);
    for (int l = 0; l < n_layers; ++l)
        MID_REQUIRE(std::isfinite(layer_sigma[l]) && layer_sigma[l] > 0.f, "%s: sigmas must be finite and > 0 (layer_sigma[%d] = %g)", who, l, (double)layer_sigma[l]);
    return MID_OK;
}

int format_check(const char *who, int width, int height, int format)
{
    MID_REQUIRE(width > 0 && height > 0, "%s: bad size %dx%d", who, width, height);
    MID_REQUIRE((long)width * height < (1l << 30), "%s: image too large", who);
    MID_REQUIRE((format & ~0xffff) == 0 && fmt_known(fmt_frames(format)), "%s: unknown format %d", who, format);
    MID_REQUIRE(fmt_guide(format) >= 0, "%s: unknown guide-layer format code %d in format 0x%x", who, format >> 8, format);
    return MID_OK;
}

}  // namespace

// What mid_atrous_moments and the frame pipeline check before their own tables: size, the format word, n_layers in 1..16, a layer
// table, every sigma finite and > 0, n_frames >= 1, k >= 0 and the pointer limit of one launch.
int atrous_moments_check(const mid_atrous_moments_params *p, const char *who, const float *layer_sigma, bool have_layers, int n_layers,
                         int n_frames, int k)
{
    MID_REQUIRE(p != nullptr, "%s: params is NULL", who);
    if (int rc = format_check(who, p->width, p->height, p->format)) return rc;
    if (int rc = layers_check(who, layer_sigma, have_layers, n_layers)) return rc;
    MID_REQUIRE(n_frames >= 1 && k >= 0, "%s: bad n_frames=%d k=%d", who, n_frames, k);
    const long window = (long)(2l * k + 1 < n_frames ? 2l * k + 1 : n_frames);
    MID_REQUIRE(window * (n_layers + 1) <= kMaxPtrs, "%s: a window of %ld frames with %d layers each needs %ld pointers per launch, the limit is "
                "min(2k+1, n_frames) * (n_layers + 1) <= %d", who, window, n_layers, window * (n_layers + 1), kMaxPtrs);
    return MID_OK;
}

// What mid_atrous_variance and the frame pipeline check before their own tables: size, pass range, sigmaLum and epsilon, the
// format word, n_layers in 1..16, a layer table, every sigma finite and > 0.
int atrous_variance_check(const mid_atrous_variance_params *p, const char *who, const float *layer_sigma, bool have_layers, int n_layers)
{
    MID_REQUIRE(p != nullptr, "%s: params is NULL", who);
    if (int rc = format_check(who, p->width, p->height, p->format)) return rc;
    MID_REQUIRE(p->first_pass >= 0 && p->n_passes >= 1 && (long)p->first_pass + p->n_passes <= kAVMaxPasses,
                "%s: passes [%d, %d + %d) outside 0..8", who, p->first_pass, p->first_pass, p->n_passes);
    MID_REQUIRE(std::isfinite(p->sigmaLum) && p->sigmaLum >= 0.f, "%s: sigmaLum %g must be 0 (no luminance term) or > 0 and finite", who, (double)p->sigmaLum);
    MID_REQUIRE(p->sigmaLum == 0.f || (std::isfinite(p->epsilon) && p->epsilon > 0.f), "%s: epsilon %g must be > 0 and finite", who, (double)p->epsilon);
    return layers_check(who, layer_sigma, have_layers, n_layers);
}

// mid_atrous_moments without its checks (the caller has made them), one launch on `s`.
int atrous_moments_out(mid_ctx *ctx, const mid_atrous_moments_params *p, const float *layer_sigma, const void *const *frames,
                       const uint32_t *const *layers, int n_layers, int n_frames, int k, int t, float *var_out, hipStream_t s)
{
    const double c = sqrt(0.5 * 1.4426950408889634);
    MomentsArgs a{};
    a.w = p->width; a.h = p->height;
    a.fmt = fmt_frames(p->format); a.gfmt = fmt_guide(p->format);
    for (int l = 0; l < n_layers; ++l) a.scl[l] = (float)(c / (double)layer_sigma[l]);
    pack_temporal_window(a, frames, layers, n_layers, n_frames, k, t);
    a.var_out = var_out;
    return dispatch_moments(ctx, a, s);
}

// mid_atrous_variance without its checks, one launch per pass on `s`.  level[i] / vlevel[i]: the RGBA32F colour levels and the
// float variance levels between passes (the first pair needed from two passes on, the second from three).
int atrous_variance_out(mid_ctx *ctx, const mid_atrous_variance_params *p, const float *layer_sigma, const void *in, const float *var_in,
                        const uint32_t *const *layers, int n_layers, void *out, int out_fmt, float *var_out, void *const level[2],
                        float *const vlevel[2], hipStream_t s)
{
    VarianceArgs a{};
    a.w = p->width; a.h = p->height;
    a.gfmt = fmt_guide(p->format);
    a.n_layers = n_layers;
    const double c = sqrt(0.5 * 1.4426950408889634);
    for (int l = 0; l < n_layers; ++l) {
        a.scl[l] = (float)(c / (double)layer_sigma[l]);
        a.layer[l] = layers[l];
    }
    a.use_lum = p->sigmaLum > 0.f;
    a.sigma_lum = p->sigmaLum; a.epsilon = p->epsilon;
    const void *src = in;
    const float *vsrc = var_in;
    int src_fmt = fmt_frames(p->format);
    for (int i = 0; i < p->n_passes; ++i) {
        const bool last = i == p->n_passes - 1;
        a.step = 1 << (p->first_pass + i);
        a.in = src; a.fmt = src_fmt; a.var_in = vsrc;
        a.out = last ? out : level[i & 1];
        a.out_fmt = last ? out_fmt : MID_FMT_RGBA32F;
        a.var_out = last ? var_out : vlevel[i & 1];
        a.store_var = a.var_out != nullptr;
        if (int rc = dispatch_variance(ctx, a, s)) return rc;
        src = a.out; src_fmt = MID_FMT_RGBA32F; vsrc = a.var_out;
    }
    return MID_OK;
}

}  // namespace mid

using namespace mid;

extern "C" int mid_atrous_moments(mid_ctx *ctx, const mid_atrous_moments_params *p, const float *layer_sigma, const void *const *frames,
                                  const uint32_t *const *layers, int n_layers, int n_frames, int k, int t, float *var_out, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    const char *who = "atrous_moments";
    if (int rc = atrous_moments_check(p, who, layer_sigma, layers != nullptr, n_layers, n_frames, k)) return rc;
    MID_REQUIRE(frames && var_out, "%s: NULL table or output", who);
    MID_REQUIRE(t >= 0 && t < n_frames, "%s: frame t=%d outside the sequence of %d", who, t, n_frames);
    MID_REQUIRE(((uintptr_t)var_out & 15u) == 0, "%s: var_out is not 16-byte aligned", who);
    const int fmt = fmt_frames(p->format), gfmt = fmt_guide(p->format);
    const size_t npix = (size_t)p->width * p->height;
    const size_t in_bytes = npix * fmt_bytes(fmt), layer_bytes = npix * fmt_bytes(gfmt), var_bytes = npix * sizeof(float);
    const int lo = t - k < 0 ? 0 : t - k, hi = (long)t + k > n_frames - 1 ? n_frames - 1 : t + k;
    for (int f = lo; f <= hi; ++f) {
        MID_REQUIRE(frames[f] != nullptr, "%s: frame %d is NULL", who, f);
        MID_REQUIRE(fmt_aligned(fmt, frames[f]), "%s: frame %d is not 8-byte aligned (RGBA16F)", who, f);
        MID_REQUIRE(!ranges_overlap(var_out, var_bytes, frames[f], in_bytes), "%s: var_out overlaps frame %d", who, f);
        for (int l = 0; l < n_layers; ++l) {
            const void *ly = layers[(size_t)f * n_layers + l];
            MID_REQUIRE(ly != nullptr, "%s: layer %d of frame %d is NULL", who, l, f);
            MID_REQUIRE(guide_aligned(gfmt, ly), "%s: layer %d of frame %d is not %d-byte aligned (%s guide)", who, l, f,
                        gfmt == MID_FMT_RGBA16F ? 8 : 16, gfmt == MID_FMT_RGBA16F ? "RGBA16F" : "RGBA32F");
            MID_REQUIRE(!ranges_overlap(var_out, var_bytes, ly, layer_bytes), "%s: var_out overlaps layer %d of frame %d", who, l, f);
        }
    }
    return atrous_moments_out(ctx, p, layer_sigma, frames, layers, n_layers, n_frames, k, t, var_out, b.s);
}

extern "C" size_t mid_atrous_variance_scratch_bytes(const mid_atrous_variance_params *p)
{
    if (!p || p->width <= 0 || p->height <= 0) return 0;
    return variance_sets(p->n_passes) * (size_t)p->width * p->height * (sizeof(float4) + sizeof(float));
}

extern "C" int mid_atrous_variance(mid_ctx *ctx, const mid_atrous_variance_params *p, const float *layer_sigma, const void *in,
                                   const float *var_in, const uint32_t *const *layers, int n_layers, void *out, int out_format,
                                   float *var_out, void *scratch, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    const char *who = "atrous_variance";
    if (int rc = atrous_variance_check(p, who, layer_sigma, layers != nullptr, n_layers)) return rc;
    MID_REQUIRE(in && out, "%s: NULL image", who);
    MID_REQUIRE(var_in != nullptr, "%s: var_in is NULL", who);
    MID_REQUIRE(fmt_known(out_format), "%s: unknown output format %d", who, out_format);
    const int fmt = fmt_frames(p->format), gfmt = fmt_guide(p->format);
    const size_t npix = (size_t)p->width * p->height;
    const size_t scratch_bytes = mid_atrous_variance_scratch_bytes(p);
    MID_REQUIRE(scratch || scratch_bytes == 0, "%s: scratch is NULL and %d passes need %zu bytes", who, p->n_passes, scratch_bytes);
    if (scratch_bytes == 0) scratch = nullptr;
    MID_REQUIRE(fmt_aligned(fmt, in), "%s: the frame is not 8-byte aligned (RGBA16F)", who);
    MID_REQUIRE(fmt_aligned(out_format, out), "%s: out is not 8-byte aligned (RGBA16F)", who);
    MID_REQUIRE(((uintptr_t)scratch & 15u) == 0, "%s: scratch is not 16-byte aligned", who);
    MID_REQUIRE(((uintptr_t)var_in & 15u) == 0 && ((uintptr_t)var_out & 15u) == 0, "%s: a variance plane is not 16-byte aligned", who);
    const size_t in_bytes = npix * fmt_bytes(fmt), out_bytes = npix * fmt_bytes(out_format), layer_bytes = npix * fmt_bytes(gfmt);
    const size_t var_bytes = npix * sizeof(float), vo_bytes = var_out ? var_bytes : 0;       // var_out == NULL: nothing is stored
    for (int l = 0; l < n_layers; ++l) {
        MID_REQUIRE(layers[l] != nullptr, "%s: layer %d is NULL", who, l);
        MID_REQUIRE(guide_aligned(gfmt, layers[l]), "%s: layer %d is not %d-byte aligned (%s guide)", who, l, gfmt == MID_FMT_RGBA16F ? 8 : 16,
                    gfmt == MID_FMT_RGBA16F ? "RGBA16F" : "RGBA32F");
        MID_REQUIRE(!ranges_overlap(out, out_bytes, layers[l], layer_bytes), "%s: out overlaps layer %d", who, l);
        MID_REQUIRE(!ranges_overlap(var_out, vo_bytes, layers[l], layer_bytes), "%s: var_out overlaps layer %d", who, l);
        MID_REQUIRE(!ranges_overlap(scratch, scratch_bytes, layers[l], layer_bytes), "%s: scratch overlaps layer %d", who, l);
    }
    MID_REQUIRE(!ranges_overlap(out, out_bytes, in, in_bytes), "%s: out overlaps the frame (in-place filtering is not supported)", who);
    MID_REQUIRE(!ranges_overlap(out, out_bytes, var_in, var_bytes), "%s: out overlaps var_in", who);
    MID_REQUIRE(!ranges_overlap(var_out, vo_bytes, in, in_bytes), "%s: var_out overlaps the frame", who);
    MID_REQUIRE(!ranges_overlap(var_out, vo_bytes, var_in, var_bytes), "%s: var_out overlaps var_in (in-place filtering is not supported)", who);
    MID_REQUIRE(!ranges_overlap(var_out, vo_bytes, out, out_bytes), "%s: var_out overlaps out", who);
    MID_REQUIRE(!ranges_overlap(scratch, scratch_bytes, in, in_bytes), "%s: scratch overlaps the frame", who);
    MID_REQUIRE(!ranges_overlap(scratch, scratch_bytes, var_in, var_bytes), "%s: scratch overlaps var_in", who);
    MID_REQUIRE(!ranges_overlap(scratch, scratch_bytes, out, out_bytes), "%s: scratch overlaps out", who);
    MID_REQUIRE(!ranges_overlap(scratch, scratch_bytes, var_out, vo_bytes), "%s: scratch overlaps var_out", who);
    // the colour levels first, then the variance levels
    const size_t sets = variance_sets(p->n_passes);
    char *base = (char *)scratch;
    void *level[2] = {sets >= 1 ? base : nullptr, sets >= 2 ? base + npix * sizeof(float4) : nullptr};
    char *vbase = base ? base + sets * npix * sizeof(float4) : nullptr;
    float *vlevel[2] = {sets >= 1 ? (float *)vbase : nullptr, sets >= 2 ? (float *)(vbase + npix * sizeof(float)) : nullptr};
    return atrous_variance_out(ctx, p, layer_sigma, in, var_in, layers, n_layers, out, out_format, var_out, level, vlevel, b.s);
}
