// temporal_accumulate.hip -- recursive temporal accumulation with motion vectors (include/mi_denoise.h, section a4j): a history of
// the colour and of the luminance moments that lives from frame to frame, reprojected by per-pixel motion and blended with the new
// frame as lerp(history, frame, max(1 / N, alpha)) with a per-pixel history length N.
//
// Per pixel p = (x, y), C = the widened texel of `cur`, l = l(C) (a4i's luminance):
//   taps     reproject_taps.hpp: pp = p + motion(p), the four bilinear taps q around pp in the order b = 0, 1, inside it a = 0, 1; a
//            tap outside the image or with bw == 0 is skipped (never read); a pp outside (-1, width) x (-1, height), NaN or Inf: none
//   weights  arg = a4g's layer chain from 0 between cur_layers[l](p) and prev_layers[l](q), layers ascending;  w = bw 2^arg
//   sums     S += w;  hc = fmaf(Hc(q), w, hc) per channel;  h1, h2, hn = fmaf(Hs(q).{x, y, z}, w, .)
//   S > 0:   hc /= S, h1 /= S, h2 /= S (IEEE divisions); else all 0.  hn stays the UNNORMALISED sum
//   N' = fminf(historyMax, hn + 1);  a = fmaxf(1 / N', alpha);  am = fmaxf(1 / N', alphaMoments)
//   color_out = fmaf(a, C - hc, hc);  m1' = fmaf(am, l - h1, h1);  m2' = fmaf(am, l l - h2, h2);  state_out = (m1', m2', N', 0)
//   v = fmaf(-m1', m1', m2');  Vt = v < 0 ? 0 : v;  var_out = Vs given ? fmaf(fminf(1, (N' - 1) / (historyFull - 1)), Vt - Vs, Vs) : Vt
//
// With a clip box (section a4m, mid_temporal_accumulate_clip), after the normalisation and where S > 0, per colour channel:
//   hc' = hc < lo ? lo : (hc > hi ? hi : hc);  d = l(hc') - l(hc);  h1' = h1 + d;  h2' = fmaf(d, fmaf(2, h1, d), h2)
// and everything below reads hc', h1', h2'.  A compile-time variant (accumulate_pixel<CLIP>): the unclipped kernel has no trace of it.
//
// One kernel: one pixel per lane, 64 x 4 pixels per workgroup, no LDS -- the tap addresses depend on the data.  Motion is locally
// coherent, so the four taps of neighbouring lanes share cache lines.  The layer loop is wave-uniform and runs OUTSIDE the taps: per
// layer the centre texel and the (up to) four previous texels are loaded and the four exponents advance together, so no centre
// table is kept and every per-tap array is indexed by unrolled constants only.
//
// The device helpers shared with atrous_variance.hip (load_texel, lum) are restated here, as there: that file keeps its text and
// its code object.
#include "common.hpp"
#include "reproject_taps.hpp"
#include <cmath>

namespace mid {

namespace {

// One texel at flat index idx, the format a run-time (wave-uniform) value; the caller keeps idx inside the image.
__device__ __forceinline__ float4 load_texel(const void *img, int fmt, size_t idx)
{
    if (fmt == MID_FMT_RGBA8) return decode_rgba8(((const uint32_t *)img)[idx]);
    if (fmt == MID_FMT_RGBA16F) return decode_rgba16f(((const uint2 *)img)[idx]);
    return ((const float4 *)img)[idx];
}

// Rec. 709 luminance of a widened texel: the one formula of section a4i
__device__ __forceinline__ float lum(float4 c) { return fmaf(0.0722f, c.z, fmaf(0.7152f, c.y, 0.2126f * c.x)); }

struct AccumArgs {
    int w, h;
    int fmt, gfmt;                      // MID_FMT_* of `cur`, of the layers
    int n_layers;
    float alpha, alpha_m, hist_max, hist_full;
    const void *cur;
    const float2 *motion;               // or nullptr: zero motion
    const float4 *hist_color;           // both nullptr: no history
    const float4 *hist_state;
    const float *var_spatial;           // or nullptr
    float4 *color_out;
    float4 *state_out;
    float *var_out;                     // or nullptr
    float scl[kMaxLayers];              // per layer: sqrt(.5 log2 e) / sigma_l
    const void *cur_layer[kMaxLayers];
    const void *prev_layer[kMaxLayers];
};
static_assert(2 * kMaxLayers + 10 <= MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS, "the pointer table of one launch");
static_assert(sizeof(AccumArgs) <= 4096, "one kernel argument block");

// The whole pixel; CLIP: the normalised history is clipped to [clip_lo(p), clip_hi(p)] per colour channel and the moments move with it
// (section a4m).  Without it no instruction of the unclipped kernel changes.
template <bool CLIP>
__device__ __forceinline__ void accumulate_pixel(const AccumArgs &a, const float4 *clip_lo, const float4 *clip_hi)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int w = a.w, h = a.h, L = a.n_layers;
    if (x >= w || y >= h) return;                          // (no barrier in this kernel)
    const size_t ci = (size_t)y * w + x;
    const float4 C = load_texel(a.cur, a.fmt, ci);
    const float l = lum(C);

    float4 hc = make_float4(0.f, 0.f, 0.f, 0.f);
    float h1 = 0.f, h2 = 0.f, hn = 0.f, S = 0.f;
    if (a.hist_color) {                                    // (wave-uniform)
        float mx = 0.f, my = 0.f;
        if (a.motion) { const float2 m = a.motion[ci]; mx = m.x; my = m.y; }
        const ReprojectTaps tp = reproject_taps(x, y, mx, my, w, h);
        size_t qi[4];
        float arg[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // a slot that is not taken keeps the centre's index (a valid one) and is never dereferenced
            qi[i] = tp.take[i] ? (size_t)(tp.y0 + (i >> 1)) * w + (size_t)(tp.x0 + (i & 1)) : ci;
            arg[i] = 0.f;
        }
        for (int ly = 0; ly < L; ++ly) {                   // wave-uniform
            const float sc = a.scl[ly];
            const void *gc = a.cur_layer[ly], *gp = a.prev_layer[ly];
            const float4 g = load_texel(gc, a.gfmt, ci);
            const float cx = g.x * sc, cy = g.y * sc, cz = g.z * sc;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (tp.take[i]) {
                    const float4 q = load_texel(gp, a.gfmt, qi[i]);
                    const float dx = cx - q.x * sc, dy = cy - q.y * sc, dz = cz - q.z * sc;
                    arg[i] = fmaf(-dz, dz, fmaf(-dy, dy, fmaf(-dx, dx, arg[i])));
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (tp.take[i]) {
                const float wt = tp.bw[i] * __builtin_amdgcn_exp2f(arg[i]);
                const float4 Hc = a.hist_color[qi[i]];
                const float4 Hs = a.hist_state[qi[i]];
                S += wt;
                hc.x = fmaf(Hc.x, wt, hc.x); hc.y = fmaf(Hc.y, wt, hc.y);
                hc.z = fmaf(Hc.z, wt, hc.z); hc.w = fmaf(Hc.w, wt, hc.w);
                h1 = fmaf(Hs.x, wt, h1); h2 = fmaf(Hs.y, wt, h2); hn = fmaf(Hs.z, wt, hn);
            }
        }
    }
    if (S > 0.f) {
        hc.x /= S; hc.y /= S; hc.z /= S; hc.w /= S;
        h1 /= S; h2 /= S;
    } else {
        hc = make_float4(0.f, 0.f, 0.f, 0.f);
        h1 = h2 = 0.f;
    }
    if (CLIP && S > 0.f) {
        const float4 lo = clip_lo[ci], hi = clip_hi[ci];
        float4 hk = hc;                                    // (a NaN hc stays NaN; a NaN bound clips nothing)
        hk.x = hc.x < lo.x ? lo.x : (hc.x > hi.x ? hi.x : hc.x);
        hk.y = hc.y < lo.y ? lo.y : (hc.y > hi.y ? hi.y : hc.y);
        hk.z = hc.z < lo.z ? lo.z : (hc.z > hi.z ? hi.z : hc.z);
        const float d = lum(hk) - lum(hc);
        h2 = fmaf(d, fmaf(2.0f, h1, d), h2);               // the mean moves by d, the variance h2 - h1^2 stays
        h1 = h1 + d;
        hc = hk;
    }
    const float N = fminf(a.hist_max, hn + 1.0f);
    const float inv = 1.0f / N;
    const float al = fmaxf(inv, a.alpha), am = fmaxf(inv, a.alpha_m);
    a.color_out[ci] = make_float4(fmaf(al, C.x - hc.x, hc.x), fmaf(al, C.y - hc.y, hc.y), fmaf(al, C.z - hc.z, hc.z), fmaf(al, C.w - hc.w, hc.w));
    const float m1 = fmaf(am, l - h1, h1);
    const float m2 = fmaf(am, l * l - h2, h2);
    a.state_out[ci] = make_float4(m1, m2, N, 0.f);
    if (a.var_out) {                                       // (wave-uniform)
        const float v = fmaf(-m1, m1, m2);
        const float Vt = v < 0.f ? 0.f : v;                // (a NaN stays a NaN)
        float vo = Vt;
        if (a.var_spatial) {
            const float Vs = a.var_spatial[ci];
            const float tt = fminf(1.0f, (N - 1.0f) / (a.hist_full - 1.0f));
            vo = fmaf(tt, Vt - Vs, Vs);
        }
        a.var_out[ci] = vo;
    }
}

__global__ __launch_bounds__(256) void temporal_accumulate_kernel(const AccumArgs a) { accumulate_pixel<false>(a, nullptr, nullptr); }

struct AccumClipArgs {
    AccumArgs a;
    const float4 *clip_lo, *clip_hi;
};
static_assert(sizeof(AccumClipArgs) <= 4096, "one kernel argument block");

__global__ __launch_bounds__(256) void temporal_accumulate_clip_kernel(const AccumClipArgs c) { accumulate_pixel<true>(c.a, c.clip_lo, c.clip_hi); }

bool ranges_overlap(const void *p, size_t np, const void *q, size_t nq)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && np && nq && a < b + nq && b < a + np;
}

}  // namespace

// What mid_temporal_accumulate checks before its tables: the parameters, the format word, n_layers in 0..16 and, with layers, both
// tables and every sigma finite and > 0.
int temporal_accumulate_check(const mid_temporal_accum_params *p, const char *who, const float *layer_sigma, bool have_layers, int n_layers)
{
    MID_REQUIRE(p != nullptr, "%s: params is NULL", who);
    MID_REQUIRE(p->width > 0 && p->height > 0, "%s: bad size %dx%d", who, p->width, p->height);
    MID_REQUIRE((long)p->width * p->height < (1l << 30), "%s: image too large", who);
    MID_REQUIRE((p->format & ~0xffff) == 0 && fmt_known(fmt_frames(p->format)), "%s: unknown format %d", who, p->format);
    MID_REQUIRE(fmt_guide(p->format) >= 0, "%s: unknown guide-layer format code %d in format 0x%x", who, p->format >> 8, p->format);
    MID_REQUIRE(std::isfinite(p->alpha) && p->alpha > 0.f && p->alpha <= 1.f, "%s: alpha %g outside (0, 1]", who, (double)p->alpha);
    MID_REQUIRE(std::isfinite(p->alphaMoments) && p->alphaMoments > 0.f && p->alphaMoments <= 1.f, "%s: alphaMoments %g outside (0, 1]", who,
                (double)p->alphaMoments);
    MID_REQUIRE(std::isfinite(p->historyMax) && p->historyMax >= 1.f, "%s: historyMax %g must be >= 1 and finite", who, (double)p->historyMax);
    MID_REQUIRE(std::isfinite(p->historyFull) && p->historyFull > 1.f, "%s: historyFull %g must be > 1 and finite", who, (double)p->historyFull);
    MID_REQUIRE(n_layers >= 0 && n_layers <= kMaxLayers, "%s: n_layers %d outside 0..16", who, n_layers);
    if (n_layers) {
        MID_REQUIRE(have_layers, "%s: a layer table is NULL", who);
        MID_REQUIRE(layer_sigma != nullptr, "%s: layer_sigma is NULL (there is no sigma to fall back on)", who);
        for (int l = 0; l < n_layers; ++l)
            MID_REQUIRE(std::isfinite(layer_sigma[l]) && layer_sigma[l] > 0.f, "%s: sigmas must be finite and > 0 (layer_sigma[%d] = %g)", who, l,
                        (double)layer_sigma[l]);
    }
    return MID_OK;
}

// mid_temporal_accumulate_clip without its checks (the caller has made them), one launch on `s`; without clip planes the unclipped kernel.
int temporal_accumulate_out(mid_ctx *ctx, const mid_temporal_accum_params *p, const float *layer_sigma, const void *cur,
                            const uint32_t *const *cur_layers, const uint32_t *const *prev_layers, int n_layers, const float *motion,
                            const mid_pixel *hist_color_in, const mid_pixel *hist_state_in, const float *var_spatial,
                            const mid_pixel *clip_lo, const mid_pixel *clip_hi, mid_pixel *color_out, mid_pixel *state_out, float *var_out,
                            hipStream_t s)
{
    (void)ctx;
    AccumArgs a{};
    a.w = p->width; a.h = p->height;
    a.fmt = fmt_frames(p->format); a.gfmt = fmt_guide(p->format);
    a.n_layers = n_layers;
    a.alpha = p->alpha; a.alpha_m = p->alphaMoments; a.hist_max = p->historyMax; a.hist_full = p->historyFull;
    a.cur = cur;
    a.motion = (const float2 *)motion;
    a.hist_color = (const float4 *)hist_color_in; a.hist_state = (const float4 *)hist_state_in;
    a.var_spatial = var_spatial;
    a.color_out = (float4 *)color_out; a.state_out = (float4 *)state_out; a.var_out = var_out;
    const double c = sqrt(0.5 * 1.4426950408889634);
    for (int l = 0; l < n_layers; ++l) {
        a.scl[l] = (float)(c / (double)layer_sigma[l]);
        a.cur_layer[l] = cur_layers[l];
        a.prev_layer[l] = prev_layers[l];
    }
    if (clip_lo) {
        const AccumClipArgs c{a, (const float4 *)clip_lo, (const float4 *)clip_hi};
        hipLaunchKernelGGL(temporal_accumulate_clip_kernel, dim3(cdiv(a.w, 64), cdiv(a.h, 4)), dim3(256), 0, s, c);
    } else
        hipLaunchKernelGGL(temporal_accumulate_kernel, dim3(cdiv(a.w, 64), cdiv(a.h, 4)), dim3(256), 0, s, a);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

}  // namespace mid

using namespace mid;

extern "C" int mid_temporal_accumulate_clip(mid_ctx *ctx, const mid_temporal_accum_params *p, const float *layer_sigma, const void *cur,
                                            const uint32_t *const *cur_layers, const uint32_t *const *prev_layers, int n_layers,
                                            const float *motion, const mid_pixel *hist_color_in, const mid_pixel *hist_state_in,
                                            const float *var_spatial, const mid_pixel *clip_lo, const mid_pixel *clip_hi, mid_pixel *color_out,
                                            mid_pixel *state_out, float *var_out, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    const char *who = clip_lo || clip_hi ? "temporal_accumulate_clip" : "temporal_accumulate";
    if (int rc = temporal_accumulate_check(p, who, layer_sigma, cur_layers != nullptr && prev_layers != nullptr, n_layers)) return rc;
    MID_REQUIRE(cur && color_out && state_out, "%s: NULL frame or output", who);
    MID_REQUIRE((hist_color_in == nullptr) == (hist_state_in == nullptr), "%s: the history is its colour AND its state: both or neither", who);
    const int fmt = fmt_frames(p->format), gfmt = fmt_guide(p->format);
    const size_t npix = (size_t)p->width * p->height;
    const size_t in_bytes = npix * fmt_bytes(fmt), layer_bytes = npix * fmt_bytes(gfmt);
    const size_t px_bytes = npix * sizeof(mid_pixel), var_bytes = npix * sizeof(float), mv_bytes = npix * 2 * sizeof(float);
    MID_REQUIRE(fmt_aligned(fmt, cur), "%s: the frame is not 8-byte aligned (RGBA16F)", who);
    MID_REQUIRE(((uintptr_t)motion & 7u) == 0, "%s: motion is not 8-byte aligned", who);
    MID_REQUIRE(((uintptr_t)hist_color_in & 15u) == 0 && ((uintptr_t)hist_state_in & 15u) == 0, "%s: a history plane is not 16-byte aligned", who);
    MID_REQUIRE(((uintptr_t)color_out & 15u) == 0 && ((uintptr_t)state_out & 15u) == 0, "%s: color_out or state_out is not 16-byte aligned", who);
    MID_REQUIRE(((uintptr_t)var_spatial & 15u) == 0 && ((uintptr_t)var_out & 15u) == 0, "%s: a variance plane is not 16-byte aligned", who);
    MID_REQUIRE((clip_lo == nullptr) == (clip_hi == nullptr), "%s: the clip box is its lower AND its upper plane: both or neither", who);
    MID_REQUIRE(((uintptr_t)clip_lo & 15u) == 0 && ((uintptr_t)clip_hi & 15u) == 0, "%s: a clip plane is not 16-byte aligned", who);
    // every output against every input and against the other outputs: the gather reads neighbours, so nothing works in place
    struct Plane { const void *p; size_t n; const char *name; };
    const Plane outs[3] = {{color_out, px_bytes, "color_out"}, {state_out, px_bytes, "state_out"}, {var_out, var_bytes, "var_out"}};
    const Plane ins[7] = {{cur, in_bytes, "the frame"}, {motion, mv_bytes, "motion"}, {hist_color_in, px_bytes, "hist_color_in"},
                          {hist_state_in, px_bytes, "hist_state_in"}, {var_spatial, var_bytes, "var_spatial"},
                          {clip_lo, px_bytes, "clip_lo"}, {clip_hi, px_bytes, "clip_hi"}};
    for (int l = 0; l < n_layers; ++l) {
        MID_REQUIRE(cur_layers[l] != nullptr && prev_layers[l] != nullptr, "%s: layer %d is NULL", who, l);
        MID_REQUIRE(guide_aligned(gfmt, cur_layers[l]) && guide_aligned(gfmt, prev_layers[l]), "%s: layer %d is not %d-byte aligned (%s guide)", who, l,
                    gfmt == MID_FMT_RGBA16F ? 8 : 16, gfmt == MID_FMT_RGBA16F ? "RGBA16F" : "RGBA32F");
        for (const Plane &o : outs)
            MID_REQUIRE(!ranges_overlap(o.p, o.n, cur_layers[l], layer_bytes) && !ranges_overlap(o.p, o.n, prev_layers[l], layer_bytes),
                        "%s: %s overlaps layer %d", who, o.name, l);
    }
    for (int i = 0; i < 3; ++i) {
        for (const Plane &in : ins)
            MID_REQUIRE(!ranges_overlap(outs[i].p, outs[i].n, in.p, in.n), "%s: %s overlaps %s (nothing is accumulated in place: the gather reads neighbours)",
                        who, outs[i].name, in.name);
        for (int j = i + 1; j < 3; ++j)
            MID_REQUIRE(!ranges_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n), "%s: %s overlaps %s", who, outs[i].name, outs[j].name);
    }
    return temporal_accumulate_out(ctx, p, layer_sigma, cur, cur_layers, prev_layers, n_layers, motion, hist_color_in, hist_state_in,
                                   var_spatial, clip_lo, clip_hi, color_out, state_out, var_out, b.s);
}

extern "C" int mid_temporal_accumulate(mid_ctx *ctx, const mid_temporal_accum_params *p, const float *layer_sigma, const void *cur,
                                       const uint32_t *const *cur_layers, const uint32_t *const *prev_layers, int n_layers,
                                       const float *motion, const mid_pixel *hist_color_in, const mid_pixel *hist_state_in,
                                       const float *var_spatial, mid_pixel *color_out, mid_pixel *state_out, float *var_out, void *stream)
{
    return mid_temporal_accumulate_clip(ctx, p, layer_sigma, cur, cur_layers, prev_layers, n_layers, motion, hist_color_in, hist_state_in, var_spatial,
                                        nullptr, nullptr, color_out, state_out, var_out, stream);
}
