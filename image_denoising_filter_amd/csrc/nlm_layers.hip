// nlm_layers.hip -- non-local means guided by RGBA8 layers: nonlocal.comp with the patch distance taken on a guide layer and the
// colour taken from the input, fed layers the way src/main.cpp:1610-1623 feeds them to bialteral_layers.comp.
//
// One accumulate dispatch for layer l (mid_nlm_layers_accum):
//     d(p,s) = sum_{q in patch} |G_l(p+q) - G_l(p+s+q)|^2_rgb,   w = exp(-d/h^2)
//     W[p].weightColor += w * I(p+s),   W[p].normWeight += 0.001 + sum of w      (nonlocal.comp:32-33, :55-62)
// and mid_nlm_layers = L such dispatches into a zeroed W followed by normalize.comp, fused in one kernel: the accumulators stay in
// registers across the layers and the epilogue normalizes (float4, pack_rgba8 or pack_rgba16f).  Out-of-image texels are 0.
//
// The strip kernel (tuned windows) is nlm_strip.hpp's decomposition -- a wave owns 64 columns x R rows, the guide column strip
// stays in registers, search rows are walked innermost with a ring of window rows, vertical block sums, horizontal DPP sums --
// with two tiles in LDS instead of one:
//   * the INPUT tile (float4 colours, centre positions only: no patch halo) is filled once and stays resident for every layer;
//     the centre colours of a wave's R output rows walk down it with the search rows in a second register ring (R float4): one
//     ds_read_b128 per offset, not one per output and offset (measured: 2.1-2.2x a one-frame NLM launch per layer with the
//     latter, the LDS port binds);
//   * the GUIDE tile holds the packed RGBA8 texels (4 B, a quarter of a float4 tile), refilled per layer.  Texels are widened to
//     their byte values 0..255 when they enter the register ring, so every per-texel difference, square and patch sum is an
//     exact integer in fp32 (a 9x9 patch sums to at most 81 * 3 * 255^2 < 2^24) and the scale 1/(255^2 h^2) is applied once,
//     in the exponent.  The order of the additions does not change a patch distance's bits.
// Eight waves per workgroup (both tiles of the 21x21 / 7x7 window: 140 KB of LDS, one workgroup per CU, two waves per SIMD).
// Any other window runs on a per-pixel kernel with the same arithmetic.
#include "nlm_guide.hpp"

namespace mid {

namespace {

constexpr int kLR = 8, kLNW = 8;        // strip kernel: rows per wave, waves per workgroup

struct NlmLayerArgs {
    int w, h;
    float kd;                           // log2(e) / (255^2 h^2): exp2 scale of an integer patch distance
    int fmt;                            // MID_FMT_* of the input
    int tiles_x, tiles_y;
    const void *in;
    int n_layers;                       // fused form: layers [0, n_layers); the accumulate form reads layer[0]
    const uint32_t *layer[kMaxLayers];
    mid_weightinfo *W;                  // accumulate form
    void *out;                          // fused form, in out_fmt
    int out_fmt;
};

// Output pixel (x,y) of both kernels' epilogues: W += the sums (accumulate form) or the normalized pixel (fused form,
// normalize.comp:36-42 as in pointwise.hip's normalize_kernel, then packed like nlm_strip_kernel's epilogue).
template <bool FUSED>
__device__ __forceinline__ void put(const NlmLayerArgs &a, size_t idx, float4 tot, float totw)
{
    if (FUSED) put_normalized(a.out, idx, a.out_fmt, tot, totw);
    else put_accumulated(a.W, idx, tot, totw);
}

template <int SLO, int SHI, int PLO, int PHI, bool FUSED>
__global__ __launch_bounds__(kLNW * 64) void nlm_layers_strip_kernel(const NlmLayerArgs a)
{
    using T = GuideTile<SLO, SHI, PLO, PHI, kLR, kLNW>;     // LHC: the input tile's rows, LHG: the guide tile's
    constexpr int R = T::R, NW = T::NW, PW = T::PW, DR = T::DR, NL = T::NL, NR = T::NR, VW = T::VW, TILE_H = T::TILE_H;
    constexpr int SW = T::SW, LW = T::LW, LHC = T::LHC, LHG = T::LHG;

    extern __shared__ float4 lds[];
    float4 *ctile = lds;
    uint32_t *gtile = (uint32_t *)(lds + LW * LHC);

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned trem = xcd_remap_in_frame(blockIdx.x, (unsigned)(a.tiles_x * a.tiles_y), 0u);
    const int ty = (int)(trem / (unsigned)a.tiles_x), tx = (int)(trem - (unsigned)ty * a.tiles_x);
    const int w = a.w, h = a.h;
    const int X0 = tx * VW, Y0 = ty * TILE_H;
    const int gx = X0 + PLO + lane;                  // column owned by this lane
    const int yb = Y0 + wv * R;                      // first output row of this wave
    const bool wave_active = yb < h;

    // The input tile, and from its CONTENT the form of the weight sums for every layer (nlm_strip_kernel's opaque form: all
    // alphas 1.0f, so sum(w * alpha) is sum(w) and normWeight = 0.001 + weightColor.w).  Both kernels decide it here, from
    // the same tile, so a fused call and its chain of accumulate dispatches add the same terms in the same order.
    bool mine = true;
    if (a.fmt == MID_FMT_RGBA8) fill_tile<MID_FMT_RGBA8, false>(ctile, LW, LHC, a.in, w, h, X0 + PLO + SLO, Y0 + SLO, tid, NW * 64, 1.0f, &mine);
    else if (a.fmt == MID_FMT_RGBA16F) fill_tile<MID_FMT_RGBA16F, false>(ctile, LW, LHC, a.in, w, h, X0 + PLO + SLO, Y0 + SLO, tid, NW * 64, 1.0f, &mine);
    else fill_tile<MID_FMT_RGBA32F, false>(ctile, LW, LHC, a.in, w, h, X0 + PLO + SLO, Y0 + SLO, tid, NW * 64, 1.0f, &mine);
    const bool opaque = __syncthreads_and(mine) != 0;

    float4 tot[R];
    float totw[R];
#pragma unroll
    for (int k = 0; k < R; ++k) { tot[k] = make_float4(0.f, 0.f, 0.f, 0.f); totw[k] = 0.f; }

    const int n_layers = FUSED ? a.n_layers : 1;
    for (int l = 0; l < n_layers; ++l) {
        __syncthreads();   // the previous layer's readers are done with the guide tile
        fill_guide(gtile, LW, LHG, a.layer[l], w, h, X0 + PLO + SLO, Y0 + PLO + SLO, tid, NW * 64);
        __syncthreads();
        if (!wave_active) continue;

        // the guide's column strip at this lane (offset 0 in the tile), kept in registers for every offset
        float Tr[DR], Tg[DR], Tb[DR];
#pragma unroll
        for (int m = 0; m < DR; ++m) {
            const float3 t = bytes_rgb(gtile[(wv * R + m - SLO) * LW + lane - SLO]);
            Tr[m] = t.x; Tg[m] = t.y; Tb[m] = t.z;
        }

        float4 acc[R];
        float accw[R];
#pragma unroll
        for (int k = 0; k < R; ++k) { acc[k] = make_float4(0.f, 0.f, 0.f, 0.f); accw[k] = 0.001f; }   // nonlocal.comp:32-33

        const float kd = a.kd;

        // one offset: guide window row r lives in ring slot (j + r) % DR, the centre colour of output row k in slot (j + k) % R of
        // the colour ring; `cnext` is the input-tile texel that enters the colour ring after this offset
        auto step = [&](auto A1, int j, float3 (&n)[DR], const uint32_t *nextp, bool more, float4 (&c)[R], const float4 *cnext) {
            float D[DR];
#pragma unroll
            for (int m = 0; m < DR; ++m) {
                const float3 &t = n[(j + m) % DR];
                const float dx = Tr[m] - t.x, dy = Tg[m] - t.y, dz = Tb[m] - t.z;
                D[m] = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            }
            if (more) n[j % DR] = bytes_rgb(nextp[0]);      // the row that leaves the window makes room for the one that enters
            float4 cn;
            if (more) cn = cnext[0];
            raise_priority();
            float V[R];
            vertical_box<PW, R>(D, V);
            float ww[R];
#pragma unroll
            for (int k = 0; k < R; ++k) ww[k] = horizontal_box<PLO, PHI>(V[k]) * kd;
#pragma unroll
            for (int k = 0; k < R; ++k) ww[k] = __builtin_amdgcn_exp2f(-ww[k]);    // exp(-d/h^2), nonlocal.comp:55
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const float wt = ww[k];
                const float4 &ck = c[(j + k) % R];                                // I(p+s) of output row k
                acc[k].x = fmaf(ck.x, wt, acc[k].x); acc[k].y = fmaf(ck.y, wt, acc[k].y);   // :56
                acc[k].z = fmaf(ck.z, wt, acc[k].z); acc[k].w = fmaf(ck.w, wt, acc[k].w);
                if constexpr (!decltype(A1)::value) accw[k] += wt;                // :57
            }
            if (more) c[j % R] = cn;                        // output row 0's centre leaves, row R's enters
            drop_priority();
        };
        // one search column: its SW search rows as one run through the ring
        auto run = [&](auto A1, int sx) __attribute__((always_inline)) {
            const uint32_t *gp = gtile + (wv * R) * LW + lane + sx;
            const float4 *cp = ctile + (wv * R) * LW + lane + sx;
            float3 n[DR];
            float4 c[R];
#pragma unroll
            for (int m = 0; m < DR; ++m) n[m] = bytes_rgb(gp[m * LW]);
#pragma unroll
            for (int k = 0; k < R; ++k) c[k] = cp[k * LW];
#pragma unroll
            for (int j = 0; j < SW; ++j) step(A1, j, n, gp + (DR + j) * LW, j + 1 < SW, c, cp + (R + j) * LW);
        };
        if (opaque) {
            for (int sx = 0; sx < SW; ++sx) run(std::true_type{}, sx);
#pragma unroll
            for (int k = 0; k < R; ++k) accw[k] = 0.001f + acc[k].w;
        } else {
            for (int sx = 0; sx < SW; ++sx) run(std::false_type{}, sx);
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {   // W += this layer's sums (the fused form: the registers that stand for W)
            tot[k].x += acc[k].x; tot[k].y += acc[k].y; tot[k].z += acc[k].z; tot[k].w += acc[k].w;
            totw[k] += accw[k];
        }
    }

    if (wave_active && lane >= NL && lane <= 63 - NR && gx < w) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int gy = yb + k;
            if (gy >= h) break;
            put<FUSED>(a, (size_t)gy * w + gx, tot[k], totw[k]);
        }
    }
}

// Every other window: one thread per pixel, nonlocal.comp:36-59 with the distance on the guide (integer byte differences as in
// the strip kernel) and global-memory fetches.  Correct for every legal parameter set; not a tuned path.
template <int FMT, bool FUSED>
__global__ __launch_bounds__(256) void nlm_layers_generic_kernel(const NlmLayerArgs a, int slo, int shi, int plo, int phi)
{
    const int px = blockIdx.x * 16 + (threadIdx.x & 15), py = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (px >= a.w || py >= a.h) return;
    float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
    float totw = 0.f;
    const int n_layers = FUSED ? a.n_layers : 1;
    for (int l = 0; l < n_layers; ++l) {
        const uint32_t *g = a.layer[l];
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        float accw = 0.001f;
        for (int y = py + slo; y < py + shi; ++y)
            for (int x = px + slo; x < px + shi; ++x) {
                float d = 0.f;
                for (int j = plo; j < phi; ++j)
                    for (int i = plo; i < phi; ++i) {
                        const float3 t = bytes_rgb(guide_at(g, a.w, a.h, px + i, py + j));
                        const float3 n = bytes_rgb(guide_at(g, a.w, a.h, x + i, y + j));
                        const float dx = t.x - n.x, dy = t.y - n.y, dz = t.z - n.z;
                        d += fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                    }
                const float wt = __builtin_amdgcn_exp2f(-(d * a.kd));
                const float4 c = fetch_texture<FMT>(a.in, a.w, a.h, x, y);
                acc.x = fmaf(c.x, wt, acc.x); acc.y = fmaf(c.y, wt, acc.y);
                acc.z = fmaf(c.z, wt, acc.z); acc.w = fmaf(c.w, wt, acc.w);
                accw += wt;
            }
        tot.x += acc.x; tot.y += acc.y; tot.z += acc.z; tot.w += acc.w;
        totw += accw;
    }
    put<FUSED>(a, (size_t)py * a.w + px, tot, totw);
}

template <bool FUSED>
int dispatch_layers(mid_ctx *ctx, const mid_nlm_params *p, NlmLayerArgs &a, hipStream_t s)
{
    int rc;
    if (nlm_guide_for_window(p, &rc, [&](auto win) {
            using W = decltype(win);
            return launch_guide_strip<GuideTile<W::SLO, W::SHI, W::PLO, W::PHI, kLR, kLNW>>(
                ctx, "nlm_layers", nlm_layers_strip_kernel<W::SLO, W::SHI, W::PLO, W::PHI, FUSED>, 1, a, s);
        }))
        return rc;
    return launch_guide_per_pixel([](auto fmt) { return nlm_layers_generic_kernel<decltype(fmt)::value, FUSED>; }, p, a, s);
}

void init_args(NlmLayerArgs &a, const mid_nlm_params *p, const void *in)
{
    a.w = p->width; a.h = p->height; a.fmt = p->format; a.in = in;
    a.kd = nlm_guide_kd((double)p->filteringParameter);
}

}  // namespace

int nlm_layers_out(mid_ctx *ctx, const mid_nlm_params *p, const void *in, const uint32_t *const *layers, int n_layers, void *out,
                   int out_fmt, hipStream_t s)
{
    NlmLayerArgs a{};
    init_args(a, p, in);
    a.n_layers = n_layers;
    for (int l = 0; l < n_layers; ++l) a.layer[l] = layers[l];
    a.out = out; a.out_fmt = out_fmt;
    return dispatch_layers<true>(ctx, p, a, s);
}

}  // namespace mid

using namespace mid;

extern "C" int mid_nlm_layers_accum(mid_ctx *ctx, const mid_nlm_params *p, const void *in, const uint32_t *layer_rgba8,
                                    mid_weightinfo *W, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    if (int rc = nlm_check_params(p)) return rc;
    MID_REQUIRE(in && layer_rgba8 && W, "nlm_layers_accum: NULL pointer");
    MID_REQUIRE(fmt_aligned(p->format, in), "nlm_layers_accum: RGBA16F input must be 8-byte aligned");
    NlmLayerArgs a{};
    init_args(a, p, in);
    a.n_layers = 1;
    a.layer[0] = layer_rgba8;
    a.W = W;
    return dispatch_layers<false>(ctx, p, a, b.s);
}

extern "C" int mid_nlm_layers(mid_ctx *ctx, const mid_nlm_params *p, const void *in, const uint32_t *const *layers, int n_layers,
                              mid_pixel *out, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    if (int rc = nlm_check_params(p)) return rc;
    MID_REQUIRE(in && layers && out, "nlm_layers: NULL pointer");
    MID_REQUIRE(fmt_aligned(p->format, in), "nlm_layers: RGBA16F input must be 8-byte aligned");
    MID_REQUIRE(n_layers >= 0 && n_layers <= kMaxLayers, "nlm_layers: n_layers %d outside 0..16", n_layers);
    const void *inputs[1 + kMaxLayers] = {in};
    for (int i = 0; i < n_layers; ++i) {
        MID_REQUIRE(layers[i] != nullptr, "nlm_layers: layer %d is NULL", i);
        inputs[1 + i] = layers[i];
    }
    const void *outs[1] = {out};
    if (int rc = check_no_alias("nlm_layers", "the input or one of its layers", inputs, 1 + n_layers, outs, 1)) return rc;
    return nlm_layers_out(ctx, p, in, layers, n_layers, out, MID_FMT_RGBA32F, b.s);
}
