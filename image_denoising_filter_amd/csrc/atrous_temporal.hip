// atrous_temporal.hip -- the edge-avoiding a-trous filter over neighbouring frames (include/mi_denoise.h, section a4h).
//
// Pass 0 (step 1) of output frame t takes its taps from every frame f of the window lo = max(0, t-k) .. hi = min(n-1, t+k); the
// centre always comes from frame t.  For q = p + o, o = (i, j), |i|, |j| <= 2:
//     w(p, f, o) = K(o) * prod_l exp(-.5 |G[t][l](p) - G[f][l](q)|^2_rgb / sigma_l^2) * [exp(-.5 |C[t](p) - C[f](q)|^2_rgb / colorSigma^2)]
//     C_1(p)     = sum_f sum_o w C[f](q) / sum_f sum_o w                  over the taps whose q lies inside the image
// Passes 1 .. N-1 are atrous.hip's, unchanged, on C_1 with frame t's layers (atrous_joint_out with first_pass = 1): the temporal
// samples enter once, the later passes filter the accumulated estimate.
//
// Arithmetic of one tap: atrous.hip's, with G[t][l](p) sc_l and C[t](p) as the centre and frame f's texels as the tap --
//     arg = 0;  per layer:  d = G[t][l](p) sc_l - G[f][l](q) sc_l (x, y, z),  arg = fmaf(-d, d, arg);  colour: d = (C[t](p) - C[f](q)) scc_0
//     w = K(o) * 2^arg,  0 for a tap outside the image;  acc = fmaf(C[f](q), w, acc) per channel, accw += w
// ONE pair (acc, accw) per pixel runs across the whole window: frames ascending lo .. hi, inside a frame j = -2 .. 2, then i = -2 .. 2;
// one IEEE division per channel at the end.  Both kernels compute exactly this, and with a window of one frame it is the chain
// of mid_atrous_joint's step-1 pass: the same bits.
//
//   * atrous_temporal_tiled_kernel<P> (n_layers <= 4): atrous.hip's step-1 shapes -- eight waves, P rows per wave, 64 x 8 P pixels from
//     LDS tiles of 68 x (8 P + 4) texels; P = 2 while two workgroups fit a CU (n_layers <= 3: 68 x 20), else 1 (n_layers = 4: the
//     68 x 12 comb shape).  One neighbour's tiles are resident at a time, so the LDS bytes are those of a4g's table.  The centres
//     C[t](p) and G[t][l](p) sc_l are loaded once, from global memory, decoded and scaled as a tile texel is; the accumulators of
//     the P rows stay in registers across the neighbours.  Two barriers per neighbour (readers done / tile filled): lanes right of
//     the image and rows below it stay in the loop and only skip their work and their stores.  The tap loop exists once per layer
//     count 1 .. 4 behind a wave-uniform switch; no register array is indexed by a run-time value.
//   * atrous_temporal_global_kernel (n_layers 5 .. 16, and a device whose LDS does not hold the tiles): atrous_global_kernel's scheme,
//     one pixel per lane and global taps, with the frame loop around the tap loops.
//
// The compiler's report for gfx950 (-Rpass-analysis=kernel-resource-usage):
//     kernel                               VGPRs  SGPRs  scratch  occupancy (waves per SIMD)
//     atrous_temporal_tiled_kernel<2>      105    66     0        4
//     atrous_temporal_tiled_kernel<1>      70     68     0        7
//     atrous_temporal_global_kernel        80     85     0        6
// (no spills; at 105 VGPRs two workgroups of the 68 x 20 shape share a CU, which is also what their LDS allows at three layers)
#include "nlm_strip.hpp"
#include <cmath>

namespace mid {

namespace {

constexpr int kMaxPtrs = MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS;
constexpr int kATTiledLayers = 4;       // layers the tiled kernel keeps resident
constexpr int kATCuLds = 163840;        // LDS of one CU: what two workgroups must share to be resident together
constexpr int kATNW = 8;                // waves per workgroup

struct AtrousTemporalArgs {
    int w, h;
    int fmt, gfmt, out_fmt;             // MID_FMT_* of the frames, of the layers, of `out`
    int use_colour;                     // the colour term is on (colorSigma > 0)
    float scc;                          // sqrt(.5 log2 e) / colorSigma
    int tiles_x, tiles_y;
    int n_nb;                           // neighbours of this output: window slots [0, n_nb)
    int n_layers;
    int t_slot;                         // the window slot that is the output frame itself
    void *out;
    float scl[kMaxLayers];              // per layer: sqrt(.5 log2 e) / sigma_l
    const void *p[kMaxPtrs];            // slot j: p[j * (n_layers + 1)] = frame, then its n_layers guide layers
};
static_assert(sizeof(AtrousTemporalArgs) <= sizeof(NlmArgs), "no larger than the temporal NLM kernels' argument block");

// Bytes of LDS of one workgroup with P rows per wave: a4g's step-1 rows (68 x 20: tiled and comb alike; 68 x 12: comb).
constexpr size_t atrous_temporal_lds_bytes(int n_layers, int rows_per_wave)
{
    return (size_t)68 * (kATNW * rows_per_wave + 4) * (sizeof(float4) + 3 * sizeof(float) * (size_t)n_layers);
}
constexpr int atrous_temporal_rows(int n_layers) { return 2 * atrous_temporal_lds_bytes(n_layers, 2) <= kATCuLds ? 2 : 1; }
static_assert(atrous_temporal_rows(3) == 2 && atrous_temporal_lds_bytes(3, 2) == 70720 && atrous_temporal_rows(4) == 1 &&
              atrous_temporal_lds_bytes(4, 1) == 52224, "the step-1 rows of a4g's class table");
inline bool atrous_temporal_tiled(int lds_max, int n_layers)
{
    return n_layers <= kATTiledLayers && (int)atrous_temporal_lds_bytes(n_layers, atrous_temporal_rows(n_layers)) <= lds_max;
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

__device__ __forceinline__ const void *nb_frame(const AtrousTemporalArgs &a, int f) { return a.p[f * (a.n_layers + 1)]; }
__device__ __forceinline__ const void *nb_layer(const AtrousTemporalArgs &a, int f, int l) { return a.p[f * (a.n_layers + 1) + 1 + l]; }

__device__ __forceinline__ void put(const AtrousTemporalArgs &a, size_t idx, float4 acc, float accw)
{
    store_out(a.out, idx, a.out_fmt, make_float4(acc.x / accw, acc.y / accw, acc.z / accw, acc.w / accw));
}

template <int N> struct LayerCount { static constexpr int value = N; };

template <int P>
__global__ __launch_bounds__(kATNW * 64) void atrous_temporal_tiled_kernel(const AtrousTemporalArgs a)
{
    constexpr int MAXL = kATTiledLayers, TR = kATNW * P, LW = 68, LH = TR + 4, N = LW * LH;
    extern __shared__ float4 lds[];
    float4 *img_t = lds;                                  // colour tile of the neighbour
    float *gde_t = (float *)(lds + N);                    // its layer l: planes x, y, z at gde_t + (3 l + {0, 1, 2}) * N

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
    const int w = a.w, h = a.h, L = a.n_layers;
    const int X0 = tx * 64, Y0 = ty * TR;
    const int gx = X0 + lane, yb = Y0 + wv * P;
    const bool colour = a.use_colour != 0;
    const float scc = a.scc;

    // the centres: C[t](p) and G[t][l](p) sc_l of this thread's P pixels, with a tile texel's decode and multiply; a lane right of
    // the image or a row below it holds zeros and stores nothing
    float4 cc[P];
    float cx[MAXL][P], cy[MAXL][P], cz[MAXL][P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const bool inside = gx < w && yb + k < h;
        const size_t ci = inside ? (size_t)(yb + k) * w + gx : 0;
        cc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (inside) cc[k] = load_texel(nb_frame(a, a.t_slot), a.fmt, ci);
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

    float4 acc[P];
    float accw[P];
#pragma unroll
    for (int k = 0; k < P; ++k) { acc[k] = make_float4(0.f, 0.f, 0.f, 0.f); accw[k] = 0.f; }

    for (int f = 0; f < a.n_nb; ++f) {
        __syncthreads();                                   // every wave has left the previous neighbour's tap loop
        // fill: a texel's colour and its L guide texels are loaded together; out-of-image texels are zero (their taps weigh 0)
        const void *frame = nb_frame(a, f);
        for (int t = tid; t < N; t += kATNW * 64) {
            const int r = t / LW, c = t - r * LW;
            const int x = X0 - 2 + c, y = Y0 - 2 + r;
            const bool inside = (unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h;
            const size_t idx = inside ? (size_t)y * w + x : 0;
            float4 col = make_float4(0.f, 0.f, 0.f, 0.f);
            if (inside) col = load_texel(frame, a.fmt, idx);
            img_t[t] = col;
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
                const int ct = (wv * P + k + 2) * LW + lane + 2;
#pragma unroll 1
                for (int j = -2; j <= 2; ++j) {             // a tap row at a time, as in atrous_tiled_kernel
                    const bool row_in = (unsigned)(gy + j) < (unsigned)h;
                    const float kj = b3(j);
#pragma unroll
                    for (int i = -2; i <= 2; ++i) {
                        const bool valid = row_in && (unsigned)(gx + i) < (unsigned)w;
                        const int t = ct + j * LW + i;
                        const float4 q = img_t[t];
                        float arg = 0.f;
#pragma unroll
                        for (int l = 0; l < NL; ++l) {
                            const float *gp = gde_t + 3 * l * N + t;
                            const float dx = cx[l][k] - gp[0], dy = cy[l][k] - gp[N], dz = cz[l][k] - gp[2 * N];
                            arg = fmaf(-dz, dz, fmaf(-dy, dy, fmaf(-dx, dx, arg)));
                        }
                        if (colour) {
                            const float dr = (cc[k].x - q.x) * scc, dg = (cc[k].y - q.y) * scc, db = (cc[k].z - q.z) * scc;
                            arg = fmaf(-db, db, fmaf(-dg, dg, fmaf(-dr, dr, arg)));
                        }
                        float wt = (b3(i) * kj) * __builtin_amdgcn_exp2f(arg);
                        wt = valid ? wt : 0.f;
                        acc[k].x = fmaf(q.x, wt, acc[k].x); acc[k].y = fmaf(q.y, wt, acc[k].y);
                        acc[k].z = fmaf(q.z, wt, acc[k].z); acc[k].w = fmaf(q.w, wt, acc[k].w);
                        accw[k] += wt;
                    }
                }
            }
        };
        static_assert(kATTiledLayers == 4, "one tap loop per layer count");
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
        if (gy < h) put(a, (size_t)gy * w + gx, acc[k], accw[k]);
    }
}

// Every n_layers > 4 (and what does not fit LDS): one pixel per lane, the taps of every neighbour from global memory.  A tap
// outside the image reads the centre's address instead (a valid one) and weighs 0.
__global__ __launch_bounds__(256) void atrous_temporal_global_kernel(const AtrousTemporalArgs a)
{
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
    const float4 cc = load_texel(nb_frame(a, a.t_slot), a.fmt, ci);
    const bool colour = a.use_colour != 0;
    const float scc = a.scc;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float accw = 0.f;
#pragma unroll 1
    for (int f = 0; f < a.n_nb; ++f) {
        const void *frame = nb_frame(a, f);
#pragma unroll 1
        for (int j = -2; j <= 2; ++j) {
            const int yy = y + j;
            const bool row_in = yy >= 0 && yy < h;
            const float kj = b3(j);
#pragma unroll 1
            for (int i = -2; i <= 2; ++i) {
                const int xx = x + i;
                const bool valid = row_in && xx >= 0 && xx < w;
                const size_t t = valid ? (size_t)yy * w + (size_t)xx : ci;
                float4 q = load_texel(frame, a.fmt, t);
                if (!valid) q = make_float4(0.f, 0.f, 0.f, 0.f);      // what the tiled kernel's tile holds there
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
    }
    put(a, ci, acc, accw);
}

template <int P>
int launch_atrous_temporal_tiled(mid_ctx *ctx, AtrousTemporalArgs &a, hipStream_t s)
{
    auto kern = atrous_temporal_tiled_kernel<P>;
    if (int rc = ensure_lds(ctx, (const void *)kern, (size_t)ctx->lds_max)) return rc;
    a.tiles_x = (int)cdiv(a.w, 64);
    a.tiles_y = (int)cdiv(a.h, kATNW * P);
    hipLaunchKernelGGL(kern, dim3((unsigned)a.tiles_x * a.tiles_y), dim3(kATNW * 64), atrous_temporal_lds_bytes(a.n_layers, P), s, a);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

// The temporal pass of one output.  The class depends on n_layers and the device's LDS only.
int dispatch_atrous_temporal(mid_ctx *ctx, AtrousTemporalArgs &a, hipStream_t s)
{
    if (atrous_temporal_tiled(ctx->lds_max, a.n_layers))
        return atrous_temporal_rows(a.n_layers) == 2 ? launch_atrous_temporal_tiled<2>(ctx, a, s) : launch_atrous_temporal_tiled<1>(ctx, a, s);
    hipLaunchKernelGGL(atrous_temporal_global_kernel, dim3(cdiv(a.w, 64), cdiv(a.h, 4)), dim3(256), 0, s, a);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

bool ranges_overlap(const void *p, size_t np, const void *q, size_t nq)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return np && nq && a < b + nq && b < a + np;
}

}  // namespace

int atrous_temporal_check(const mid_atrous_params *p, const char *who, const float *layer_sigma, bool have_layers, int n_layers,
                          int n_frames, int k)
{
    if (int rc = atrous_check(p, who, layer_sigma, have_layers, n_layers)) return rc;
    MID_REQUIRE(p->first_pass == 0, "%s: first_pass %d: the temporal pass is pass 0 (continue a filter with mid_atrous_joint)", who, p->first_pass);
    MID_REQUIRE(n_frames >= 1 && k >= 0, "%s: bad n_frames=%d k=%d", who, n_frames, k);
    return nlm_layers_temporal_fits(who, n_layers, n_frames, k);
}

int atrous_temporal_out(mid_ctx *ctx, const mid_atrous_params *p, const float *layer_sigma, const void *const *frames,
                        const uint32_t *const *layers, int n_layers, int n_frames, int k, int first, int count, void *const *out,
                        int out_fmt, void *scratch0, void *scratch1, hipStream_t s)
{
    const double c = sqrt(0.5 * 1.4426950408889634);
    const bool last = p->n_passes == 1;
    mid_atrous_params rest = *p;                            // passes 1 .. N-1: mid_atrous_joint's, from the first level
    rest.first_pass = 1; rest.n_passes = p->n_passes - 1;
    rest.format = MID_FMT_RGBA32F | (p->format & ~0xff);
    for (int t = first; t < first + count; ++t) {
        AtrousTemporalArgs a{};
        a.w = p->width; a.h = p->height;
        a.fmt = fmt_frames(p->format); a.gfmt = fmt_guide(p->format);
        for (int l = 0; l < n_layers; ++l) a.scl[l] = (float)(c / (double)layer_sigma[l]);
        a.use_colour = p->colorSigma > 0.f;
        a.scc = a.use_colour ? (float)(c / (double)p->colorSigma) : 0.f;     // scc_0: pass 0's colour sigma is colorSigma itself
        pack_temporal_window(a, frames, layers, n_layers, n_frames, k, t);
        a.out = last ? out[t - first] : scratch0;
        a.out_fmt = last ? out_fmt : MID_FMT_RGBA32F;
        if (int rc = dispatch_atrous_temporal(ctx, a, s)) return rc;
        // the first of the remaining passes reads scratch0, so the levels are handed over swapped: it writes scratch1
        if (!last)
            if (int rc = atrous_joint_out(ctx, &rest, layer_sigma, scratch0, layers + (size_t)t * n_layers, n_layers, out[t - first], out_fmt,
                                          scratch1, scratch0, s)) return rc;
    }
    return MID_OK;
}

}  // namespace mid

using namespace mid;

extern "C" int mid_atrous_joint_temporal(mid_ctx *ctx, const mid_atrous_params *p, const float *layer_sigma, const void *const *frames,
                                         const uint32_t *const *layers, int n_layers, int n_frames, int k, int first, int count,
                                         void *const *out, int out_format, void *scratch, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    const char *who = "atrous_joint_temporal";
    if (int rc = atrous_temporal_check(p, who, layer_sigma, layers != nullptr, n_layers, n_frames, k)) return rc;
    MID_REQUIRE(frames && out, "%s: NULL table", who);
    MID_REQUIRE(fmt_known(out_format), "%s: unknown output format %d", who, out_format);
    const int fmt = fmt_frames(p->format), gfmt = fmt_guide(p->format);
    const size_t npix = (size_t)p->width * p->height;
    const size_t scratch_bytes = mid_atrous_scratch_bytes(p);
    MID_REQUIRE(scratch || scratch_bytes == 0, "%s: scratch is NULL and %d passes need %zu bytes", who, p->n_passes, scratch_bytes);
    if (scratch_bytes == 0) scratch = nullptr;
    MID_REQUIRE(((uintptr_t)scratch & 15u) == 0, "%s: scratch is not 16-byte aligned", who);
    if (int rc = check_temporal_window(who, fmt, frames, layers, n_layers, n_frames, k, first, count, out, out_format, gfmt)) return rc;
    // scratch against every frame and layer of the call's windows and against every output
    const size_t in_bytes = npix * fmt_bytes(fmt), out_bytes = npix * fmt_bytes(out_format), layer_bytes = npix * fmt_bytes(gfmt);
    const int lo = first - k < 0 ? 0 : first - k;
    const int hi = (long)first + count - 1 + k > n_frames - 1 ? n_frames - 1 : first + count - 1 + k;
    for (int f = lo; f <= hi; ++f) {
        MID_REQUIRE(!ranges_overlap(scratch, scratch_bytes, frames[f], in_bytes), "%s: scratch overlaps frame %d", who, f);
        for (int l = 0; l < n_layers; ++l)
            MID_REQUIRE(!ranges_overlap(scratch, scratch_bytes, layers[(size_t)f * n_layers + l], layer_bytes), "%s: scratch overlaps layer %d of frame %d", who, l, f);
    }
    for (int i = 0; i < count; ++i)
        MID_REQUIRE(!ranges_overlap(scratch, scratch_bytes, out[i], out_bytes), "%s: scratch overlaps out %d", who, i);
    return atrous_temporal_out(ctx, p, layer_sigma, frames, layers, n_layers, n_frames, k, first, count, out, out_format, scratch,
                               scratch ? (char *)scratch + npix * sizeof(float4) : nullptr, b.s);
}
