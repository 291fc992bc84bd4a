// atrous.hip -- the edge-avoiding a-trous wavelet filter guided by render layers (include/mi_denoise.h, section a4g).
//
// N passes of a 5x5 B3-spline kernel, pass i sampling with holes at step s = 2^i.  For q = p + s o, o = (i, j), |i|, |j| <= 2:
//     w(p, o)    = K(o) * prod_l exp(-.5 |G_l(p) - G_l(q)|^2_rgb / sigma_l^2) * [exp(-.5 |C_i(p) - C_i(q)|^2_rgb / (colorSigma 2^-i)^2)]
//     C_{i+1}(p) = sum_o w C_i(q) / sum_o w                      over the taps whose q lies inside the image
// One launch per pass; the levels between passes are RGBA32F frames in the caller's scratch, the first pass decodes the frame's
// format and the last one packs the output format.  A pass never looks at n_passes or first_pass: the class of a launch follows
// from (step, n_layers, the device's LDS) alone, so a call over passes [0, N) is N one-pass calls, bit for bit.
//
// Arithmetic of one tap, the same in all three kernels (so a pixel has the same bits whichever of them computes it):
//     arg = 0;  per layer l = 0 .. L-1:  d = G_l(p) sc_l - G_l(q) sc_l (x, then y, then z),  arg = fmaf(-d, d, arg)
//     colour term:                       d = (C(p) - C(q)) scc         (r, then g, then b),  arg = fmaf(-d, d, arg)
//     w = K(o) * 2^arg    (K(o) = k1[i] k1[j], products of 1/16, 4/16, 6/16: exact),  0 for a tap outside the image
//     acc = fmaf(C(q), w, acc) per channel, accw += w;   taps in the order j = -2 .. 2 (rows), inside it i = -2 .. 2
//     out = acc / accw per channel (IEEE division; the centre tap always counts, so accw > 0 for finite inputs)
// sc_l = (float)(sqrt(.5 log2 e) / sigma_l) as in bilateral_joint.hip: a guide value is carried as the fp32 product g * sc_l, an
// all-zero layer adds fmaf(-0, 0, arg) = arg, and a layer in any slot gives the chain of that layer alone.
//
// Lanes run along x in every kernel: a tap row of a wave is one contiguous segment of 64 texels at every step.
//   * atrous_tiled_kernel<S> (steps 1 and 2, n_layers <= 4, where two workgroups fit a CU): 64 x 16 pixels per workgroup of eight
//     waves from LDS tiles of (64 + 4 S) x (16 + 4 S) texels -- the colour tile as float4, three planes of floats per layer, already
//     scaled, decoded from the guide format when the tile is filled.  The tap loop exists once per layer count 1 .. 4 (a
//     wave-uniform switch picks it): the centres of all layers stay in registers, no register array is indexed by a run-time
//     layer number.
//   * atrous_comb_kernel<P> (the other (step, n_layers) up to step 32 and four layers): the same tiles for the rows of ONE residue
//     class y == y0 (mod step), so that the vertical halo is 4 rows at every step; the step is a kernel argument.
//   * atrous_global_kernel (steps 64 and 128, and every n_layers > 4): one pixel per lane, 64 x 4 pixels per workgroup, taps read
//     from global memory.  The layer loop is unrolled over the 16 possible layers with constant indices; a body is skipped
//     where l >= n_layers.
#include "common.hpp"
#include <cmath>

namespace mid {

namespace {

constexpr int kAtrousTiledLayers = 4;           // layers the tiled kernel keeps resident
// Development switches (tools/atrous_joint_rate.py --alt times such builds beside the shipped one): the largest step of the
// fixed-step tiled kernel and of the row-comb kernel; 0 takes the class out.
#ifndef MID_ATROUS_TILED_MAX_STEP
#define MID_ATROUS_TILED_MAX_STEP 2
#endif
#ifndef MID_ATROUS_COMB_MAX_STEP
#define MID_ATROUS_COMB_MAX_STEP 32
#endif
constexpr int kAtrousTiledMaxStep = MID_ATROUS_TILED_MAX_STEP;      // the fixed-step tiled kernel exists for steps 1 and 2
constexpr int kAtrousCombMaxStep = MID_ATROUS_COMB_MAX_STEP;        // the row-comb kernel takes the steps up to this one; beyond it: global taps
constexpr int kAtrousCuLds = 163840;            // LDS of one CU: what two workgroups must share to be resident together
constexpr int kANW = 8, kAP = 2;                // tiled kernel: eight waves, two rows per wave: a 64 x 16 tile
constexpr int kAtrousMaxPasses = 8;

struct AtrousArgs {
    int w, h;
    int step;                           // 2^i of this pass
    int fmt, gfmt, out_fmt;             // MID_FMT_* of `in` (the frame's format in the first pass, RGBA32F afterwards), of the layers, of `out`
    int n_layers;
    int use_colour;                     // the colour term is on (colorSigma > 0)
    float scc;                          // sqrt(.5 log2 e) / (colorSigma 2^-i)
    int tiles_x, tiles_y;
    const void *in;
    void *out;
    float scl[kMaxLayers];              // per layer: sqrt(.5 log2 e) / sigma_l
    const void *layer[kMaxLayers];
};

// bytes of LDS of one workgroup of the tiled kernel
constexpr size_t atrous_lds_bytes(int step, int n_layers)
{
    return (size_t)(64 + 4 * step) * (kANW * kAP + 4 * step) * (sizeof(float4) + 3 * sizeof(float) * (size_t)n_layers);
}
// The fixed-step kernel runs where two of its workgroups fit one CU (measured: with one workgroup per CU it loses 1.5 x to the comb).
inline bool atrous_tiled(int lds_max, int step, int n_layers)
{
    return step <= kAtrousTiledMaxStep && n_layers <= kAtrousTiledLayers && 2 * atrous_lds_bytes(step, n_layers) <= kAtrousCuLds &&
           (int)atrous_lds_bytes(step, n_layers) <= lds_max;
}

// The row-comb kernel: bytes of LDS of one workgroup with P rows per wave, and the P a (step, n_layers) runs with: two rows per
// wave while two such workgroups fit one CU's 160 KB, else one.
constexpr size_t atrous_comb_lds_bytes(int step, int n_layers, int rows_per_wave)
{
    return (size_t)(64 + 4 * step) * (kANW * rows_per_wave + 4) * (sizeof(float4) + 3 * sizeof(float) * (size_t)n_layers);
}
constexpr int atrous_comb_rows(int step, int n_layers) { return 2 * atrous_comb_lds_bytes(step, n_layers, 2) <= kAtrousCuLds ? 2 : 1; }
inline bool atrous_comb(int lds_max, int step, int n_layers)
{
    return step <= kAtrousCombMaxStep && n_layers <= kAtrousTiledLayers &&
           (int)atrous_comb_lds_bytes(step, n_layers, atrous_comb_rows(step, n_layers)) <= lds_max;
}

// the B3-spline factor (1, 4, 6, 4, 1) / 16 of offset d = -2 .. 2
__device__ __forceinline__ constexpr float b3(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// One texel at flat index idx, the format a run-time (wave-uniform) value; the caller keeps idx inside the image.
__device__ __forceinline__ float4 load_texel(const void *img, int fmt, size_t idx)
{
    if (fmt == MID_FMT_RGBA8) return decode_rgba8(((const uint32_t *)img)[idx]);
    if (fmt == MID_FMT_RGBA16F) return decode_rgba16f(((const uint2 *)img)[idx]);
    return ((const float4 *)img)[idx];
}

__device__ __forceinline__ void put(const AtrousArgs &a, size_t idx, float4 acc, float accw)
{
    store_out(a.out, idx, a.out_fmt, make_float4(acc.x / accw, acc.y / accw, acc.z / accw, acc.w / accw));
}

template <int N> struct LayerCount { static constexpr int value = N; };

template <int S>
__global__ __launch_bounds__(kANW * 64) void atrous_tiled_kernel(const AtrousArgs a)
{
    constexpr int H = 2 * S, LW = 64 + 2 * H, LH = kANW * kAP + 2 * H, N = LW * LH;
    extern __shared__ float4 lds[];
    float4 *img_t = lds;                                  // colour tile
    float *gde_t = (float *)(lds + N);                    // layer l: planes x, y, z at gde_t + (3 l + {0, 1, 2}) * N

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
    const int w = a.w, h = a.h, L = a.n_layers;
    const int X0 = tx * 64, Y0 = ty * (kANW * kAP);

    // fill: a texel's colour and its L guide texels are loaded together; out-of-image texels are zero (their taps weigh 0)
    for (int t = tid; t < N; t += kANW * 64) {
        const int r = t / LW, c = t - r * LW;
        const int x = X0 - H + c, y = Y0 - H + r;
        const bool inside = (unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h;
        const size_t idx = inside ? (size_t)y * w + x : 0;
        float4 col = make_float4(0.f, 0.f, 0.f, 0.f);
        if (inside) col = load_texel(a.in, a.fmt, idx);
        img_t[t] = col;
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
    const bool colour = a.use_colour != 0;
    const float scc = a.scc;

    auto taps = [&](auto nl_tag) {
        constexpr int NL = decltype(nl_tag)::value;
#pragma unroll 1
        for (int k = 0; k < kAP; ++k) {
            const int gy = Y0 + wv * kAP + k;
            if (gy >= h) break;
            const int ct = (wv * kAP + k + H) * LW + lane + H;
            float cx[NL], cy[NL], cz[NL];
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const float *gp = gde_t + 3 * l * N + ct;
                cx[l] = gp[0]; cy[l] = gp[N]; cz[l] = gp[2 * N];
            }
            const float4 cc = img_t[ct];
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            float accw = 0.f;
#pragma unroll 1
            for (int j = -2; j <= 2; ++j) {     // a tap row at a time: five taps' tile reads in flight, not twenty-five
                const bool row_in = (unsigned)(gy + j * S) < (unsigned)h;
                const float kj = b3(j);
#pragma unroll
                for (int i = -2; i <= 2; ++i) {
                    const bool valid = row_in && (unsigned)(gx + i * S) < (unsigned)w;
                    const int t = ct + j * S * LW + i * S;
                    const float4 q = img_t[t];
                    float arg = 0.f;
#pragma unroll
                    for (int l = 0; l < NL; ++l) {
                        const float *gp = gde_t + 3 * l * N + t;
                        const float dx = cx[l] - gp[0], dy = cy[l] - gp[N], dz = cz[l] - gp[2 * N];
                        arg = fmaf(-dz, dz, fmaf(-dy, dy, fmaf(-dx, dx, arg)));
                    }
                    if (colour) {
                        const float dr = (cc.x - q.x) * scc, dg = (cc.y - q.y) * scc, db = (cc.z - q.z) * scc;
                        arg = fmaf(-db, db, fmaf(-dg, dg, fmaf(-dr, dr, arg)));
                    }
                    float wt = (b3(i) * kj) * __builtin_amdgcn_exp2f(arg);
                    wt = valid ? wt : 0.f;
                    acc.x = fmaf(q.x, wt, acc.x); acc.y = fmaf(q.y, wt, acc.y);
                    acc.z = fmaf(q.z, wt, acc.z); acc.w = fmaf(q.w, wt, acc.w);
                    accw += wt;
                }
            }
            put(a, (size_t)gy * w + gx, acc, accw);
        }
    };
    static_assert(kAtrousTiledLayers == 4, "one tap loop per layer count");
    switch (L) {
    case 1: taps(LayerCount<1>{}); break;
    case 2: taps(LayerCount<2>{}); break;
    case 3: taps(LayerCount<3>{}); break;
    default: taps(LayerCount<4>{}); break;
    }
}

// Every step up to 32 from LDS tiles (steps 1 and 2: where the fixed-step kernel would be alone on its CU): the row comb.  At step s the rows y == y0 (mod s) form an independent problem, so a workgroup
// owns TR = 8 P rows y0 + s r of ONE residue class: the vertical taps are neighbouring TILE rows (a halo of 4 rows at every step)
// and only the horizontal halo grows, 2 s columns on either side of the 64.  Same fill, same tap arithmetic, same tap order as
// atrous_tiled_kernel; the step is a kernel argument.  P rows per wave: 2, or 1 where two would not leave room for two workgroups
// per CU (atrous_comb_rows).
template <int P>
__global__ __launch_bounds__(kANW * 64) void atrous_comb_kernel(const AtrousArgs a)
{
    constexpr int TR = kANW * P, LH = TR + 4;
    const int S = a.step, H = 2 * S, LW = 64 + 2 * H, N = LW * LH;
    extern __shared__ float4 lds[];
    float4 *img_t = lds;
    float *gde_t = (float *)(lds + N);

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int by = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - by * a.tiles_x;
    const int y0 = by % S, chunk = by / S;                // the residue class and the run of TR of its rows
    const int w = a.w, h = a.h, L = a.n_layers;
    const int X0 = tx * 64;
    const int Yfirst = y0 + S * chunk * TR;               // image row of tile row 0 of the outputs
    if (Yfirst >= h) return;                              // (a short residue class: the whole workgroup, before any barrier)

    for (int t = tid; t < N; t += kANW * 64) {
        const int r = t / LW, c = t - r * LW;
        const int x = X0 - H + c;
        const long y = (long)Yfirst + (long)S * (r - 2);
        const bool inside = (unsigned)x < (unsigned)w && y >= 0 && y < h;
        const size_t idx = inside ? (size_t)y * w + x : 0;
        float4 col = make_float4(0.f, 0.f, 0.f, 0.f);
        if (inside) col = load_texel(a.in, a.fmt, idx);
        img_t[t] = col;
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
    const bool colour = a.use_colour != 0;
    const float scc = a.scc;

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
            const float4 cc = img_t[ct];
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            float accw = 0.f;
#pragma unroll 1
            for (int j = -2; j <= 2; ++j) {
                const long yy = gy + (long)j * S;
                const bool row_in = yy >= 0 && yy < h;
                const float kj = b3(j);
#pragma unroll
                for (int i = -2; i <= 2; ++i) {
                    const long xx = (long)gx + (long)i * S;
                    const bool valid = row_in && xx >= 0 && xx < w;
                    const int t = ct + j * LW + i * S;
                    const float4 q = img_t[t];
                    float arg = 0.f;
#pragma unroll
                    for (int l = 0; l < NL; ++l) {
                        const float *gp = gde_t + 3 * l * N + t;
                        const float dx = cx[l] - gp[0], dy = cy[l] - gp[N], dz = cz[l] - gp[2 * N];
                        arg = fmaf(-dz, dz, fmaf(-dy, dy, fmaf(-dx, dx, arg)));
                    }
                    if (colour) {
                        const float dr = (cc.x - q.x) * scc, dg = (cc.y - q.y) * scc, db = (cc.z - q.z) * scc;
                        arg = fmaf(-db, db, fmaf(-dg, dg, fmaf(-dr, dr, arg)));
                    }
                    float wt = (b3(i) * kj) * __builtin_amdgcn_exp2f(arg);
                    wt = valid ? wt : 0.f;
                    acc.x = fmaf(q.x, wt, acc.x); acc.y = fmaf(q.y, wt, acc.y);
                    acc.z = fmaf(q.z, wt, acc.z); acc.w = fmaf(q.w, wt, acc.w);
                    accw += wt;
                }
            }
            put(a, (size_t)gy * w + gx, acc, accw);
        }
    };
    switch (L) {
    case 1: taps(LayerCount<1>{}); break;
    case 2: taps(LayerCount<2>{}); break;
    case 3: taps(LayerCount<3>{}); break;
    default: taps(LayerCount<4>{}); break;
    }
}

// Every other (step, n_layers): one pixel per lane, the taps from global memory.  A tap outside the image reads the centre's
// address instead (a valid one) and weighs 0.
__global__ __launch_bounds__(256) void atrous_global_kernel(const AtrousArgs a)
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
    const float4 cc = load_texel(a.in, a.fmt, ci);
    const bool colour = a.use_colour != 0;
    const float scc = a.scc;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float accw = 0.f;
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
            if (!valid) q = make_float4(0.f, 0.f, 0.f, 0.f);      // what the tiled kernel's tile holds there: 0 * w, never the centre's NaN or Inf
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
            if (colour) {
                const float dr = (cc.x - q.x) * scc, dg = (cc.y - q.y) * scc, db = (cc.z - q.z) * scc;
                arg = fmaf(-db, db, fmaf(-dg, dg, fmaf(-dr, dr, arg)));
            }
            float wt = (b3(i) * kj) * __builtin_amdgcn_exp2f(arg);
            wt = valid ? wt : 0.f;
            acc.x = fmaf(q.x, wt, acc.x); acc.y = fmaf(q.y, wt, acc.y);
            acc.z = fmaf(q.z, wt, acc.z); acc.w = fmaf(q.w, wt, acc.w);
            accw += wt;
        }
    }
    put(a, ci, acc, accw);
}

template <int S>
int launch_atrous_tiled(mid_ctx *ctx, AtrousArgs &a, hipStream_t s)
{
    auto kern = atrous_tiled_kernel<S>;
    if (int rc = ensure_lds(ctx, (const void *)kern, (size_t)ctx->lds_max)) return rc;
    a.tiles_x = (int)cdiv(a.w, 64);
    a.tiles_y = (int)cdiv(a.h, kANW * kAP);
    hipLaunchKernelGGL(kern, dim3((unsigned)a.tiles_x * a.tiles_y), dim3(kANW * 64), atrous_lds_bytes(S, a.n_layers), s, a);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

template <int P>
int launch_atrous_comb(mid_ctx *ctx, AtrousArgs &a, hipStream_t s)
{
    auto kern = atrous_comb_kernel<P>;
    if (int rc = ensure_lds(ctx, (const void *)kern, (size_t)ctx->lds_max)) return rc;
    a.tiles_x = (int)cdiv(a.w, 64);
    a.tiles_y = a.step * (int)cdiv(cdiv(a.h, a.step), kANW * P);      // per residue class: its ceil(h / step) rows at most, in runs of 8 P
    hipLaunchKernelGGL(kern, dim3((unsigned)a.tiles_x * a.tiles_y), dim3(kANW * 64), atrous_comb_lds_bytes(a.step, a.n_layers, P), s, a);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

// One pass.  The class depends on (step, n_layers) and the device's LDS only.
int dispatch_atrous(mid_ctx *ctx, AtrousArgs &a, hipStream_t s)
{
    if (atrous_tiled(ctx->lds_max, a.step, a.n_layers)) {
        switch (a.step) {
        case 1: return launch_atrous_tiled<1>(ctx, a, s);
        case 2: return launch_atrous_tiled<2>(ctx, a, s);
        }
    }
    if (atrous_comb(ctx->lds_max, a.step, a.n_layers))
        return atrous_comb_rows(a.step, a.n_layers) == 2 ? launch_atrous_comb<2>(ctx, a, s) : launch_atrous_comb<1>(ctx, a, s);
    hipLaunchKernelGGL(atrous_global_kernel, dim3(cdiv(a.w, 64), cdiv(a.h, 4)), dim3(256), 0, s, a);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

bool ranges_overlap(const void *p, size_t np, const void *q, size_t nq)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return np && nq && a < b + nq && b < a + np;
}

}  // namespace

int atrous_check(const mid_atrous_params *p, const char *who, const float *layer_sigma, bool have_layers, int n_layers)
{
    MID_REQUIRE(p != nullptr, "%s: params is NULL", who);
    MID_REQUIRE(p->width > 0 && p->height > 0, "%s: bad size %dx%d", who, p->width, p->height);
    MID_REQUIRE((long)p->width * p->height < (1l << 30), "%s: image too large", who);
    MID_REQUIRE(p->first_pass >= 0 && p->n_passes >= 1 && (long)p->first_pass + p->n_passes <= kAtrousMaxPasses,
                "%s: passes [%d, %d + %d) outside 0..8", who, p->first_pass, p->first_pass, p->n_passes);
    MID_REQUIRE(std::isfinite(p->colorSigma) && p->colorSigma >= 0.f, "%s: colorSigma %g must be 0 (no colour term) or > 0 and finite", who, (double)p->colorSigma);
    MID_REQUIRE((p->format & ~0xffff) == 0 && fmt_known(fmt_frames(p->format)), "%s: unknown format %d", who, p->format);
    MID_REQUIRE(fmt_guide(p->format) >= 0, "%s: unknown guide-layer format code %d in format 0x%x", who, p->format >> 8, p->format);
    MID_REQUIRE(n_layers >= 1 && n_layers <= kMaxLayers, "%s: n_layers %d outside 1..16", who, n_layers);
    MID_REQUIRE(have_layers, "%s: the layer table is NULL", who);
    MID_REQUIRE(layer_sigma != nullptr, "%s: layer_sigma is NULL (there is no sigma to fall back on)", who);
    for (int l = 0; l < n_layers; ++l)
        MID_REQUIRE(std::isfinite(layer_sigma[l]) && layer_sigma[l] > 0.f, "%s: sigmas must be finite and > 0 (layer_sigma[%d] = %g)", who, l, (double)layer_sigma[l]);
    return MID_OK;
}

int atrous_joint_out(mid_ctx *ctx, const mid_atrous_params *p, const float *layer_sigma, const void *in, const uint32_t *const *layers,
                     int n_layers, void *out, int out_fmt, void *scratch0, void *scratch1, hipStream_t s)
{
    AtrousArgs a{};
    a.w = p->width; a.h = p->height;
    a.gfmt = fmt_guide(p->format);
    a.n_layers = n_layers;
    const double c = sqrt(0.5 * 1.4426950408889634);
    for (int l = 0; l < n_layers; ++l) {
        a.scl[l] = (float)(c / (double)layer_sigma[l]);
        a.layer[l] = layers[l];
    }
    a.use_colour = p->colorSigma > 0.f;
    const void *src = in;
    int src_fmt = fmt_frames(p->format);
    void *level[2] = {scratch0, scratch1};
    for (int i = 0; i < p->n_passes; ++i) {
        const int pass = p->first_pass + i;
        const bool last = i == p->n_passes - 1;
        a.step = 1 << pass;
        a.scc = a.use_colour ? (float)(c / ((double)p->colorSigma * ldexp(1.0, -pass))) : 0.f;
        a.in = src; a.fmt = src_fmt;
        a.out = last ? out : level[i & 1];
        a.out_fmt = last ? out_fmt : MID_FMT_RGBA32F;
        if (int rc = dispatch_atrous(ctx, a, s)) return rc;
        src = a.out; src_fmt = MID_FMT_RGBA32F;
    }
    return MID_OK;
}

size_t atrous_scratch_frames(int n_passes) { return n_passes <= 1 ? 0 : n_passes == 2 ? 1 : 2; }

}  // namespace mid

using namespace mid;

extern "C" size_t mid_atrous_scratch_bytes(const mid_atrous_params *p)
{
    if (!p || p->width <= 0 || p->height <= 0) return 0;
    return atrous_scratch_frames(p->n_passes) * (size_t)p->width * p->height * sizeof(float4);
}

extern "C" int mid_atrous_joint(mid_ctx *ctx, const mid_atrous_params *p, const float *layer_sigma, const void *in,
                                const uint32_t *const *layers, int n_layers, void *out, int out_format, void *scratch, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    const char *who = "atrous_joint";
    if (int rc = atrous_check(p, who, layer_sigma, layers != nullptr, n_layers)) return rc;
    MID_REQUIRE(in && out, "%s: NULL image", who);
    MID_REQUIRE(fmt_known(out_format), "%s: unknown output format %d", who, out_format);
    const int fmt = fmt_frames(p->format), gfmt = fmt_guide(p->format);
    const size_t npix = (size_t)p->width * p->height;
    const size_t scratch_bytes = mid_atrous_scratch_bytes(p);
    MID_REQUIRE(scratch || scratch_bytes == 0, "%s: scratch is NULL and %d passes need %zu bytes", who, p->n_passes, scratch_bytes);
    if (scratch_bytes == 0) scratch = nullptr;
    MID_REQUIRE(fmt_aligned(fmt, in), "%s: the frame is not 8-byte aligned (RGBA16F)", who);
    MID_REQUIRE(fmt_aligned(out_format, out), "%s: out is not 8-byte aligned (RGBA16F)", who);
    MID_REQUIRE(((uintptr_t)scratch & 15u) == 0, "%s: scratch is not 16-byte aligned", who);
    const size_t in_bytes = npix * fmt_bytes(fmt), out_bytes = npix * fmt_bytes(out_format), layer_bytes = npix * fmt_bytes(gfmt);
    for (int l = 0; l < n_layers; ++l) {
        MID_REQUIRE(layers[l] != nullptr, "%s: layer %d is NULL", who, l);
        MID_REQUIRE(guide_aligned(gfmt, layers[l]), "%s: layer %d is not %d-byte aligned (%s guide)", who, l, gfmt == MID_FMT_RGBA16F ? 8 : 16,
                    gfmt == MID_FMT_RGBA16F ? "RGBA16F" : "RGBA32F");
        MID_REQUIRE(!ranges_overlap(out, out_bytes, layers[l], layer_bytes), "%s: out overlaps layer %d", who, l);
        MID_REQUIRE(!ranges_overlap(scratch, scratch_bytes, layers[l], layer_bytes), "%s: scratch overlaps layer %d", who, l);
    }
    MID_REQUIRE(!ranges_overlap(out, out_bytes, in, in_bytes), "%s: out overlaps the frame (in-place filtering is not supported)", who);
    MID_REQUIRE(!ranges_overlap(scratch, scratch_bytes, in, in_bytes), "%s: scratch overlaps the frame", who);
    MID_REQUIRE(!ranges_overlap(scratch, scratch_bytes, out, out_bytes), "%s: scratch overlaps out", who);
    return atrous_joint_out(ctx, p, layer_sigma, in, layers, n_layers, out, out_format, scratch,
                            scratch ? (char *)scratch + npix * sizeof(float4) : nullptr, b.s);
}
