// nlm_layers_temporal.hip -- layer-guided non-local means over neighbouring frames: nlm_layers.hip's dispatch with the patch
// distance taken between TWO guide images -- the target frame's layer and the neighbour frame's layer -- and the colour taken
// from a third, the neighbour frame.
//
// One accumulate dispatch (mid_nlm_layers_pair_accum), target guide Gt, neighbour guide Gn, neighbour colour In:
//     d(p,s) = sum_{q in patch} |Gt(p+q) - Gn(p+s+q)|^2_rgb,   w = exp(-d/h^2)
//     W[p].weightColor += w * In(p+s),   W[p].normWeight += 0.001 + sum of w
// Output t of mid_nlm_layers_temporal = for each neighbour f = max(0,t-k) .. min(n-1,t+k) and, inside it, each layer l:
// one such dispatch with Gt = layer[t][l], Gn = layer[f][l], In = frame[f], into a zeroed W; then normalize.comp.  Fused in one
// kernel per output frame: the accumulators stay in registers across every (f, l) and the epilogue normalizes and packs.
//
// The strip kernel (tuned windows) is nlm_layers_strip_kernel with one more loop around it.  LDS holds the same two tiles:
//   * the COLOUR tile of neighbour frame f (float4, centre positions only), filled once per neighbour and resident for all of
//     its layers -- neighbour outside, layer inside is the order of the contract for exactly this reason; the opaque form of the
//     weight sums is decided from it, per neighbour, so that the fused call and its chain of dispatches add the same terms;
//   * the packed GUIDE tile of layer[f][l] (4 B texels, centres + patch halo + search halo), refilled per (f, l).
// The TARGET guide needs no search halo and each wave reads its own column strip of it exactly once per (f, l), into registers:
// it comes straight from global memory (DR coalesced 256 B rows per wave), not from a third tile.  21x21 / 7x7: 84 x 84 x 16 B +
// 84 x 90 x 4 B = 143136 B, what nlm_layers_strip_kernel uses: one workgroup per CU, eight waves, two per SIMD.
// Texels enter the arithmetic as their byte values, so every patch distance is an exact integer in fp32 and with Gt == Gn the
// kernels give the bits of nlm_layers.hip's.  Any other window runs on a per-pixel kernel with the same arithmetic.
//
// Kernel arguments: one launch per output frame carries that output's window only -- for each neighbour its frame pointer and
// its L layer pointers, (L + 1) per neighbour, the target's layers being those of the neighbour f == t -- at most
// MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS of them, so the block stays smaller than the by-value tables of the temporal NLM kernels.
#include "nlm_guide.hpp"

namespace mid {

namespace {

constexpr int kLR = 8, kLNW = 8;        // strip kernel: rows per wave, waves per workgroup (as nlm_layers.hip)

struct NlmLayerPairArgs {
    int w, h;
    float kd;                           // log2(e) / (255^2 h^2): exp2 scale of an integer patch distance
    int fmt;                            // MID_FMT_* of the frames
    int tiles_x, tiles_y;
    int n_nb;                           // neighbours of this output: window slots [0, n_nb)
    int n_layers;                       // layers per frame
    int t_slot;                         // fused form: the window slot that is the output frame itself (its layers are the targets)
    int out_fmt;
    const uint32_t *target;             // accumulate form: the target guide
    mid_weightinfo *W;                  // accumulate form
    void *out;                          // fused form, in out_fmt
    const void *p[kMaxPtrs];            // slot j: p[j * (n_layers + 1)] = frame, then its n_layers guide layers
};
static_assert(sizeof(NlmLayerPairArgs) <= sizeof(NlmArgs), "no larger than the temporal NLM kernels' argument block");

template <bool FUSED>
__device__ __forceinline__ const uint32_t *target_layer(const NlmLayerPairArgs &a, int l)
{
    return FUSED ? (const uint32_t *)a.p[a.t_slot * (a.n_layers + 1) + 1 + l] : a.target;
}

// Output pixel of both kernels' epilogues, as nlm_layers.hip's put().
template <bool FUSED>
__device__ __forceinline__ void put(const NlmLayerPairArgs &a, size_t idx, float4 tot, float totw)
{
    if (FUSED) put_normalized(a.out, idx, a.out_fmt, tot, totw);
    else put_accumulated(a.W, idx, tot, totw);
}

template <int SLO, int SHI, int PLO, int PHI, bool FUSED>
__global__ __launch_bounds__(kLNW * 64) void nlm_layers_pair_strip_kernel(const NlmLayerPairArgs a)
{
    using T = GuideTile<SLO, SHI, PLO, PHI, kLR, kLNW>;
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

    float4 tot[R];
    float totw[R];
#pragma unroll
    for (int k = 0; k < R; ++k) { tot[k] = make_float4(0.f, 0.f, 0.f, 0.f); totw[k] = 0.f; }

    const int n_nb = FUSED ? a.n_nb : 1, n_layers = FUSED ? a.n_layers : 1;
    for (int f = 0; f < n_nb; ++f) {
        __syncthreads();   // the previous neighbour's readers are done with the colour tile
        // The neighbour's colour tile, and from its CONTENT the form of the weight sums for each of its layers (all alphas 1.0f:
        // sum(w * alpha) is sum(w) and normWeight = 0.001 + weightColor.w), as nlm_layers_strip_kernel decides it from its input
        // tile: the fused call and its chain of accumulate dispatches see the same tile and add the same terms in the same order.
        const void *nb = nb_frame(a, f);
        bool mine = true;
        if (a.fmt == MID_FMT_RGBA8) fill_tile<MID_FMT_RGBA8, false>(ctile, LW, LHC, nb, w, h, X0 + PLO + SLO, Y0 + SLO, tid, NW * 64, 1.0f, &mine);
        else if (a.fmt == MID_FMT_RGBA16F) fill_tile<MID_FMT_RGBA16F, false>(ctile, LW, LHC, nb, w, h, X0 + PLO + SLO, Y0 + SLO, tid, NW * 64, 1.0f, &mine);
        else fill_tile<MID_FMT_RGBA32F, false>(ctile, LW, LHC, nb, w, h, X0 + PLO + SLO, Y0 + SLO, tid, NW * 64, 1.0f, &mine);
        const bool opaque = __syncthreads_and(mine) != 0;

        for (int l = 0; l < n_layers; ++l) {
            __syncthreads();   // the previous layer's readers are done with the guide tile
            fill_guide(gtile, LW, LHG, nb_layer(a, f, l), w, h, X0 + PLO + SLO, Y0 + PLO + SLO, tid, NW * 64);
            __syncthreads();
            if (!wave_active) continue;

            // the TARGET guide's column strip at this lane, from global memory (bounds-checked: out-of-image texels are 0),
            // kept in registers for every offset of this (neighbour, layer)
            const uint32_t *tg = target_layer<FUSED>(a, l);
            float Tr[DR], Tg[DR], Tb[DR];
#pragma unroll
            for (int m = 0; m < DR; ++m) {
                const float3 t = bytes_rgb(guide_at(tg, w, h, gx, yb + PLO + m));
                Tr[m] = t.x; Tg[m] = t.y; Tb[m] = t.z;
            }

            float4 acc[R];
            float accw[R];
#pragma unroll
            for (int k = 0; k < R; ++k) { acc[k] = make_float4(0.f, 0.f, 0.f, 0.f); accw[k] = 0.001f; }   // nonlocal.comp:32-33

            const float kd = a.kd;

            // one offset: neighbour guide window row r lives in ring slot (j + r) % DR, the centre colour of output row k in slot
            // (j + k) % R of the colour ring; `cnext` is the colour-tile texel that enters the colour ring after this offset
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
                    const float4 &ck = c[(j + k) % R];                                // In(p+s) of output row k
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
            for (int k = 0; k < R; ++k) {   // W += this dispatch's sums (the fused form: the registers that stand for W)
                tot[k].x += acc[k].x; tot[k].y += acc[k].y; tot[k].z += acc[k].z; tot[k].w += acc[k].w;
                totw[k] += accw[k];
            }
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

// Every other window: one thread per pixel with global-memory fetches, nlm_layers_generic_kernel's arithmetic.
template <int FMT, bool FUSED>
__global__ __launch_bounds__(256) void nlm_layers_pair_generic_kernel(const NlmLayerPairArgs a, int slo, int shi, int plo, int phi)
{
    const int px = blockIdx.x * 16 + (threadIdx.x & 15), py = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (px >= a.w || py >= a.h) return;
    float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
    float totw = 0.f;
    const int n_nb = FUSED ? a.n_nb : 1, n_layers = FUSED ? a.n_layers : 1;
    for (int f = 0; f < n_nb; ++f) {
        const void *in = nb_frame(a, f);
        for (int l = 0; l < n_layers; ++l) {
            const uint32_t *gt = target_layer<FUSED>(a, l), *gn = nb_layer(a, f, l);
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            float accw = 0.001f;
            for (int y = py + slo; y < py + shi; ++y)
                for (int x = px + slo; x < px + shi; ++x) {
                    float d = 0.f;
                    for (int j = plo; j < phi; ++j)
                        for (int i = plo; i < phi; ++i) {
                            const float3 t = bytes_rgb(guide_at(gt, a.w, a.h, px + i, py + j));
                            const float3 n = bytes_rgb(guide_at(gn, a.w, a.h, x + i, y + j));
                            const float dx = t.x - n.x, dy = t.y - n.y, dz = t.z - n.z;
                            d += fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                        }
                    const float wt = __builtin_amdgcn_exp2f(-(d * a.kd));
                    const float4 c = fetch_texture<FMT>(in, a.w, a.h, x, y);
                    acc.x = fmaf(c.x, wt, acc.x); acc.y = fmaf(c.y, wt, acc.y);
                    acc.z = fmaf(c.z, wt, acc.z); acc.w = fmaf(c.w, wt, acc.w);
                    accw += wt;
                }
            tot.x += acc.x; tot.y += acc.y; tot.z += acc.z; tot.w += acc.w;
            totw += accw;
        }
    }
    put<FUSED>(a, (size_t)py * a.w + px, tot, totw);
}

template <bool FUSED>
int dispatch_pair(mid_ctx *ctx, const mid_nlm_params *p, NlmLayerPairArgs &a, hipStream_t s)
{
    int rc;
    if (nlm_guide_for_window(p, &rc, [&](auto win) {
            using W = decltype(win);
            return launch_guide_strip<GuideTile<W::SLO, W::SHI, W::PLO, W::PHI, kLR, kLNW>>(
                ctx, "nlm_layers_temporal", nlm_layers_pair_strip_kernel<W::SLO, W::SHI, W::PLO, W::PHI, FUSED>, 1, a, s);
        }))
        return rc;
    return launch_guide_per_pixel([](auto fmt) { return nlm_layers_pair_generic_kernel<decltype(fmt)::value, FUSED>; }, p, a, s);
}

void init_args(NlmLayerPairArgs &a, const mid_nlm_params *p)
{
    a.w = p->width; a.h = p->height; a.fmt = p->format;
    a.kd = nlm_guide_kd((double)p->filteringParameter);
}

}  // namespace

int nlm_layers_temporal_fits(const char *who, int n_layers, int n_frames, int k)
{
    const long window = (long)(2l * k + 1 < n_frames ? 2l * k + 1 : n_frames);
    if (window * (n_layers + 1) > kMaxPtrs)
        return set_error(MID_ERR_INVALID, "%s: a window of %ld frames with %d layers each needs %ld pointers per launch, the limit is "
                         "min(2k+1, n_frames) * (n_layers + 1) <= %d", who, window, n_layers, window * (n_layers + 1), kMaxPtrs);
    return MID_OK;
}

int nlm_layers_temporal_out(mid_ctx *ctx, const mid_nlm_params *p, const void *const *frames, const uint32_t *const *layers,
                            int n_layers, int n_frames, int k, int first, int count, void *const *out, int out_fmt, hipStream_t s)
{
    for (int t = first; t < first + count; ++t) {
        NlmLayerPairArgs a{};
        init_args(a, p);
        pack_temporal_window(a, frames, layers, n_layers, n_frames, k, t);
        a.out = out[t - first]; a.out_fmt = out_fmt;
        if (int rc = dispatch_pair<true>(ctx, p, a, s)) return rc;
    }
    return MID_OK;
}

}  // namespace mid

using namespace mid;

extern "C" int mid_nlm_layers_pair_accum(mid_ctx *ctx, const mid_nlm_params *p, const uint32_t *target_layer_rgba8,
                                         const uint32_t *neighbour_layer_rgba8, const void *neighbour_in, mid_weightinfo *W, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    if (int rc = nlm_check_params(p)) return rc;
    MID_REQUIRE(target_layer_rgba8 && neighbour_layer_rgba8 && neighbour_in && W, "nlm_layers_pair_accum: NULL pointer");
    MID_REQUIRE(fmt_aligned(p->format, neighbour_in), "nlm_layers_pair_accum: RGBA16F input must be 8-byte aligned");
    NlmLayerPairArgs a{};
    init_args(a, p);
    a.n_nb = 1; a.n_layers = 1; a.t_slot = 0;
    a.target = target_layer_rgba8;
    a.p[0] = neighbour_in;
    a.p[1] = neighbour_layer_rgba8;
    a.W = W;
    return dispatch_pair<false>(ctx, p, a, b.s);
}

extern "C" int mid_nlm_layers_temporal(mid_ctx *ctx, const mid_nlm_params *p, const void *const *frames,
                                       const uint32_t *const *layers_rgba8, int n_layers, int n_frames, int k, int first, int count,
                                       void *const *out, int out_format, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    if (int rc = nlm_check_params(p)) return rc;
    MID_REQUIRE(frames && out, "nlm_layers_temporal: NULL table");
    MID_REQUIRE(fmt_known(out_format), "nlm_layers_temporal: unknown output format %d", out_format);
    MID_REQUIRE(n_layers >= 0 && n_layers <= kMaxLayers, "nlm_layers_temporal: n_layers %d outside 0..16", n_layers);
    MID_REQUIRE(layers_rgba8 || n_layers == 0, "nlm_layers_temporal: layers is NULL");
    MID_REQUIRE(n_frames >= 1 && k >= 0,
                "nlm_layers_temporal: bad frame range (n=%d k=%d first=%d count=%d)", n_frames, k, first, count);
    if (int rc = nlm_layers_temporal_fits("nlm_layers_temporal", n_layers, n_frames, k)) return rc;
    if (int rc = check_temporal_window("nlm_layers_temporal", p->format, frames, layers_rgba8, n_layers, n_frames, k, first, count, out, out_format)) return rc;
    return nlm_layers_temporal_out(ctx, p, frames, layers_rgba8, n_layers, n_frames, k, first, count, out, out_format, b.s);
}
