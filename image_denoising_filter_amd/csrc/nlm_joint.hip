// nlm_joint.hip -- joint layer-guided non-local means: ONE patch weight from all guide layers (include/mi_denoise.h, section a4f).
//
//     d_l(p,f,s) = sum_{q in patch} |G[t][l](p+q) - G[f][l](p+s+q)|^2_rgb
//     w(p,f,s)   = exp(-sum_l d_l / h_l^2),     out_t(p) = sum_{f,s} w * In_f(p+s) / sum_f (0.001 + sum_s w)
//
// nlm_layers_temporal.hip runs one complete NLM pass per (neighbour, layer) and adds the passes.  Here the patch distance of an
// offset is formed once from all layers: a box sum is linear, so the weighted squared differences of the L layers are summed per
// TEXEL,  D[m] = D_0[m] + sum_{l >= 1} (h_0/h_l)^2 D_l[m],  and everything behind that stage -- the vertical block sums, the
// horizontal DPP sums, the scale log2(e) / (255^2 h_0^2), the exp2 and the colour accumulation -- runs once per offset instead of
// L times.  Texels enter as their byte values, so every D_l[m] is an exact integer in fp32; with one layer the factor of layer 0
// is never applied and the kernels perform nlm_layers_temporal.hip's operations on the same operands: the same bits.
//
// The strip kernel (tuned windows, n_layers <= kJointTiledLayers) is nlm_layers_pair_strip_kernel with all L neighbour guide
// tiles resident at once beside the neighbour's colour tile -- the exponent needs every layer of an offset before the exp2:
//   * the COLOUR tile of neighbour frame f (float4, centre positions only), filled once per neighbour; the opaque form of the
//     weight sums is voted from it per neighbour, exactly as the layered kernel votes;
//   * L packed GUIDE tiles of layer[f][0..L) (4 B texels, centres + patch halo + search halo);
//   * the TARGET column strips of the L layers come straight from global memory into registers, once per launch.
// Shapes (joint_rows, joint_packed, joint_packed_targets; the table of section a4f): one layer keeps the layered kernel's shape --
// eight waves of eight rows, 64-row tiles -- which the bit identity with it needs (the opaque vote is per tile).  Two to four
// layers run eight waves of FOUR rows on 32-row tiles: the tiles of four layers then fit the LDS (21x21 / 7x7: 69888 + 4 x 19488
// = 147840 B), a wave's target strips and neighbour rings are DR = R + PW - 1 = 10 rows per layer instead of 14, and the kernel
// stays under 256 VGPRs, so that two waves share a SIMD (one wave alone issues VALU at half rate).  With three or four layers
// the neighbour rings stay packed (one register per row and layer) and are widened per use, with four layers one target strip
// as well.  Compiler's report for gfx950, 21x21 / 7x7 | 14x14 / 6x6: 230 | 228 VGPRs at one layer, 211 | 200 at two, 215 | 203 at
// three, 236 | 222 at four; no kernel uses scratch.
// Every other window, and more than four layers, runs on a per-pixel kernel with the same arithmetic.
#include "nlm_guide.hpp"

namespace mid {

namespace {

constexpr int kJointTiledLayers = 4;    // layers the strip kernels are built for
constexpr int kJNW = 8;                 // waves per workgroup, every shape

// rows per wave / neighbour rings packed, by layer count
constexpr int joint_rows(int n_layers) { return n_layers == 1 ? 8 : 4; }
constexpr bool joint_packed(int n_layers) { return n_layers >= 3; }
// layers (the last ones) whose TARGET strips stay packed as well: what keeps the four-layer kernel of the 7x7 patch under 256 VGPRs
constexpr int joint_packed_targets(int n_layers) { return n_layers >= 4 ? 1 : 0; }

// geometry and LDS bytes of a strip launch with L layers: the colour tile and L guide tiles
template <int SLO, int SHI, int PLO, int PHI, int L> using JointTile = GuideTile<SLO, SHI, PLO, PHI, joint_rows(L), kJNW>;
static_assert(JointTile<-10, 11, -3, 4, 1>::lds_bytes(1) == 143136 && JointTile<-10, 11, -3, 4, 4>::lds_bytes(4) == 147840, "21x21 / 7x7");
static_assert(JointTile<-7, 7, -3, 3, 1>::lds_bytes(1) == 120120 && JointTile<-7, 7, -3, 3, 4>::lds_bytes(4) == 117040, "14x14 / 6x6");

struct NlmJointArgs {
    int w, h;
    float kd;                           // log2(e) / (255^2 h_0^2): exp2 scale of the summed patch distance
    int fmt;                            // MID_FMT_* of the frames
    int tiles_x, tiles_y;
    int n_nb;                           // neighbours of this output: window slots [0, n_nb)
    int n_layers;                       // layers per frame
    int t_slot;                         // the window slot that is the output frame itself (its layers are the targets)
    int out_fmt;
    void *out;
    float rel[kMaxLayers];              // (h_0 / h_l)^2: weight of layer l's squared differences (rel[0] = 1 is never applied)
    const void *p[kMaxPtrs];            // slot j: p[j * (n_layers + 1)] = frame, then its n_layers guide layers
};
static_assert(sizeof(NlmJointArgs) <= sizeof(NlmArgs), "no larger than the temporal NLM kernels' argument block");

// A neighbour guide texel in a wave's ring: widened to its byte values when it enters (float3), or kept packed and widened per use.
template <bool PACKED> struct RingTexel { using type = float3; };
template <> struct RingTexel<true> { using type = uint32_t; };
__device__ __forceinline__ float3 ring_in(uint32_t v, float3 *) { return bytes_rgb(v); }
__device__ __forceinline__ uint32_t ring_in(uint32_t v, uint32_t *) { return v; }
__device__ __forceinline__ float3 ring_rgb(const float3 &v) { return v; }
// (the empty asm hides the value's origin: without it the compiler widens a packed texel once for all the offsets that use it
// and keeps the three floats live, which is the unpacked ring again)
__device__ __forceinline__ float3 ring_rgb(uint32_t v) { asm volatile("" : "+v"(v)); return bytes_rgb(v); }

// L: the layer count (a.n_layers == L); R rows per wave, kJNW waves; TP: layers [L - TP, L) keep their target strips packed.
template <int SLO, int SHI, int PLO, int PHI, int R, int L, bool PACKED, int TP>
__global__ __launch_bounds__(kJNW * 64) void nlm_joint_strip_kernel(const NlmJointArgs a)
{
    using T = GuideTile<SLO, SHI, PLO, PHI, R, kJNW>;
    constexpr int NW = T::NW, PW = T::PW, DR = T::DR, NL = T::NL, NR = T::NR, VW = T::VW, TILE_H = T::TILE_H;
    constexpr int SW = T::SW, LW = T::LW, LHC = T::LHC, LHG = T::LHG;
    static_assert(L >= 1 && L <= kJointTiledLayers, "layers of the strip kernels");
    using Ring = typename RingTexel<PACKED>::type;

    extern __shared__ float4 lds[];
    float4 *ctile = lds;
    uint32_t *gtile = (uint32_t *)(lds + LW * LHC);  // layer l: gtile + l * LW * LHG

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

    // the TARGET guides' column strips at this lane, from global memory (bounds-checked: out-of-image texels are 0), kept in
    // registers for every neighbour and offset
    float Tr[L][DR], Tg[L][DR], Tb[L][DR];
    uint32_t Tp[L][DR];                              // (the packed ones; of either set only the entries of its layers are ever used)
    if (wave_active) {
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const uint32_t *tg = nb_layer(a, a.t_slot, l);
#pragma unroll
            for (int m = 0; m < DR; ++m) {
                const uint32_t v = guide_at(tg, w, h, gx, yb + PLO + m);
                if (l >= L - TP) { Tp[l][m] = v; continue; }
                const float3 t = bytes_rgb(v);
                Tr[l][m] = t.x; Tg[l][m] = t.y; Tb[l][m] = t.z;
            }
        }
    }
    float rel[L];
#pragma unroll
    for (int l = 0; l < L; ++l) rel[l] = a.rel[l];

    for (int f = 0; f < a.n_nb; ++f) {
        __syncthreads();   // the previous neighbour's readers are done with the tiles
        // The neighbour's colour tile, and from its CONTENT the form of the weight sums (all alphas 1.0f: sum(w * alpha) is sum(w)
        // and normWeight = 0.001 + weightColor.w), as nlm_layers_pair_strip_kernel decides it.
        const void *nb = nb_frame(a, f);
        bool mine = true;
        if (a.fmt == MID_FMT_RGBA8) fill_tile<MID_FMT_RGBA8, false>(ctile, LW, LHC, nb, w, h, X0 + PLO + SLO, Y0 + SLO, tid, NW * 64, 1.0f, &mine);
        else if (a.fmt == MID_FMT_RGBA16F) fill_tile<MID_FMT_RGBA16F, false>(ctile, LW, LHC, nb, w, h, X0 + PLO + SLO, Y0 + SLO, tid, NW * 64, 1.0f, &mine);
        else fill_tile<MID_FMT_RGBA32F, false>(ctile, LW, LHC, nb, w, h, X0 + PLO + SLO, Y0 + SLO, tid, NW * 64, 1.0f, &mine);
        const bool opaque = __syncthreads_and(mine) != 0;
#pragma unroll
        for (int l = 0; l < L; ++l)
            fill_guide(gtile + l * (LW * LHG), LW, LHG, nb_layer(a, f, l), w, h, X0 + PLO + SLO, Y0 + PLO + SLO, tid, NW * 64);
        __syncthreads();
        if (!wave_active) continue;

        float4 acc[R];
        float accw[R];
#pragma unroll
        for (int k = 0; k < R; ++k) { acc[k] = make_float4(0.f, 0.f, 0.f, 0.f); accw[k] = 0.001f; }   // nonlocal.comp:32-33, once per neighbour

        const float kd = a.kd;

        // one offset: neighbour guide window row r of layer l lives in ring slot n[l][(j + r) % DR], the centre colour of output row
        // k in slot (j + k) % R of the colour ring; `cnext` is the colour-tile texel that enters the colour ring after this offset
        auto step = [&](auto A1, int j, Ring (&n)[L][DR], const uint32_t *nextp, bool more, float4 (&c)[R], const float4 *cnext) {
            float D[DR];
#pragma unroll
            for (int m = 0; m < DR; ++m) {
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    const float3 t = ring_rgb(n[l][(j + m) % DR]);
                    const float3 g = l >= L - TP ? ring_rgb(Tp[l][m]) : make_float3(Tr[l][m], Tg[l][m], Tb[l][m]);
                    const float dx = g.x - t.x, dy = g.y - t.y, dz = g.z - t.z;
                    const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                    D[m] = l == 0 ? d : fmaf(rel[l], d, D[m]);
                }
            }
            if (more) {                                     // the rows that leave the window make room for the ones that enter
#pragma unroll
                for (int l = 0; l < L; ++l) n[l][j % DR] = ring_in(nextp[l * (LW * LHG)], (Ring *)nullptr);
            }
            float4 cn;
            if (more) cn = cnext[0];
            raise_priority();
            float V[R];
            vertical_box<PW, R>(D, V);
            float ww[R];
#pragma unroll
            for (int k = 0; k < R; ++k) ww[k] = horizontal_box<PLO, PHI>(V[k]) * kd;
#pragma unroll
            for (int k = 0; k < R; ++k) ww[k] = __builtin_amdgcn_exp2f(-ww[k]);    // exp(-sum_l d_l/h_l^2)
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const float wt = ww[k];
                const float4 &ck = c[(j + k) % R];                                // In(p+s) of output row k
                acc[k].x = fmaf(ck.x, wt, acc[k].x); acc[k].y = fmaf(ck.y, wt, acc[k].y);
                acc[k].z = fmaf(ck.z, wt, acc[k].z); acc[k].w = fmaf(ck.w, wt, acc[k].w);
                if constexpr (!decltype(A1)::value) accw[k] += wt;
            }
            if (more) c[j % R] = cn;                        // output row 0's centre leaves, row R's enters
            drop_priority();
        };
        // one search column: its SW search rows as one run through the rings
        auto run = [&](auto A1, int sx) __attribute__((always_inline)) {
            const uint32_t *gp = gtile + (wv * R) * LW + lane + sx;
            const float4 *cp = ctile + (wv * R) * LW + lane + sx;
            Ring n[L][DR];
            float4 c[R];
#pragma unroll
            for (int l = 0; l < L; ++l) {
#pragma unroll
                for (int m = 0; m < DR; ++m) n[l][m] = ring_in(gp[l * (LW * LHG) + m * LW], (Ring *)nullptr);
            }
#pragma unroll
            for (int k = 0; k < R; ++k) c[k] = cp[k * LW];
            // (static_for, not an unrolled loop: with four layers the run is longer than the compiler's limit for `#pragma unroll`,
            // and a ring indexed by a run-time j would live in scratch)
            static_for<SW>([&](auto J) {
                constexpr int j = decltype(J)::value;
                step(A1, j, n, gp + (DR + j) * LW, j + 1 < SW, c, cp + (R + j) * LW);
            });
        };
        if (opaque) {
            for (int sx = 0; sx < SW; ++sx) run(std::true_type{}, sx);
#pragma unroll
            for (int k = 0; k < R; ++k) accw[k] = 0.001f + acc[k].w;
        } else {
            for (int sx = 0; sx < SW; ++sx) run(std::false_type{}, sx);
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {   // this neighbour's sums
            tot[k].x += acc[k].x; tot[k].y += acc[k].y; tot[k].z += acc[k].z; tot[k].w += acc[k].w;
            totw[k] += accw[k];
        }
    }

    if (wave_active && lane >= NL && lane <= 63 - NR && gx < w) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int gy = yb + k;
            if (gy >= h) break;
            put_normalized(a.out, (size_t)gy * w + gx, a.out_fmt, tot[k], totw[k]);
        }
    }
}

// Every other window and layer count: one thread per pixel with global-memory fetches, nlm_layers_pair_generic_kernel's arithmetic
// with the layers inside the offset.  A layer's patch distance is an exact integer; the layers are combined per offset,
// d = d_0 + sum_{l >= 1} rel[l] * d_l.
template <int FMT>
__global__ __launch_bounds__(256) void nlm_joint_generic_kernel(const NlmJointArgs a, int slo, int shi, int plo, int phi)
{
    const int px = blockIdx.x * 16 + (threadIdx.x & 15), py = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (px >= a.w || py >= a.h) return;
    float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
    float totw = 0.f;
    for (int f = 0; f < a.n_nb; ++f) {
        const void *in = nb_frame(a, f);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        float accw = 0.001f;
        for (int y = py + slo; y < py + shi; ++y)
            for (int x = px + slo; x < px + shi; ++x) {
                float d = 0.f;
                for (int l = 0; l < a.n_layers; ++l) {
                    const uint32_t *gt = nb_layer(a, a.t_slot, l), *gn = nb_layer(a, f, l);
                    float dl = 0.f;
                    for (int j = plo; j < phi; ++j)
                        for (int i = plo; i < phi; ++i) {
                            const float3 t = bytes_rgb(guide_at(gt, a.w, a.h, px + i, py + j));
                            const float3 n = bytes_rgb(guide_at(gn, a.w, a.h, x + i, y + j));
                            const float dx = t.x - n.x, dy = t.y - n.y, dz = t.z - n.z;
                            dl += fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                        }
                    d = l == 0 ? dl : fmaf(a.rel[l], dl, d);
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
    put_normalized(a.out, (size_t)py * a.w + px, a.out_fmt, tot, totw);
}

int launch_joint_generic(const mid_nlm_params *p, NlmJointArgs &a, hipStream_t s)
{
    return launch_guide_per_pixel([](auto fmt) { return nlm_joint_generic_kernel<decltype(fmt)::value>; }, p, a, s);
}

template <int SLO, int SHI, int PLO, int PHI, int L>
int launch_joint_strip(mid_ctx *ctx, const mid_nlm_params *p, NlmJointArgs &a, hipStream_t s)
{
    using T = JointTile<SLO, SHI, PLO, PHI, L>;
    if ((int)T::lds_bytes(L) > ctx->lds_max) {
        // the tiles do not fit this device: the per-pixel kernel, as the header says -- under a named range, so that a trace of a
        // device on which this happens shows why its launches are slow (no gfx950 class comes here: all fit 160 KB)
        Range r("nlm_joint: tiles need %zu B of LDS, device offers %d: per-pixel kernel", T::lds_bytes(L), ctx->lds_max);
        return launch_joint_generic(p, a, s);
    }
    return launch_guide_strip<T>(ctx, "nlm_joint", nlm_joint_strip_kernel<SLO, SHI, PLO, PHI, T::R, L, joint_packed(L), joint_packed_targets(L)>, L, a, s);
}

template <int SLO, int SHI, int PLO, int PHI>
int launch_joint_window(mid_ctx *ctx, const mid_nlm_params *p, NlmJointArgs &a, hipStream_t s)
{
    switch (a.n_layers) {
    case 1: return launch_joint_strip<SLO, SHI, PLO, PHI, 1>(ctx, p, a, s);
    case 2: return launch_joint_strip<SLO, SHI, PLO, PHI, 2>(ctx, p, a, s);
    case 3: return launch_joint_strip<SLO, SHI, PLO, PHI, 3>(ctx, p, a, s);
    case 4: return launch_joint_strip<SLO, SHI, PLO, PHI, 4>(ctx, p, a, s);
    default: return launch_joint_generic(p, a, s);                               // n_layers > kJointTiledLayers
    }
}

int dispatch_joint(mid_ctx *ctx, const mid_nlm_params *p, NlmJointArgs &a, hipStream_t s)
{
    // (the list of nlm_guide_for_window, written out: this dispatcher's window and layer classes are read off its text by
    // tests/test_nlm_joint_args.py)
    if (p->search_lo == -10 && p->search_hi == 11 && p->patch_lo == -3 && p->patch_hi == 4)    // 21x21 / 7x7 (benchmark)
        return launch_joint_window<-10, 11, -3, 4>(ctx, p, a, s);
    if (p->search_lo == -7 && p->search_hi == 7 && p->patch_lo == -3 && p->patch_hi == 3)      // nonlocal.comp:5-6 as shipped
        return launch_joint_window<-7, 7, -3, 3>(ctx, p, a, s);
    return launch_joint_generic(p, a, s);
}

}  // namespace

int nlm_joint_check(const mid_nlm_params *p, const char *who, const float *layer_h, bool have_layers, int n_layers, int n_frames, int k)
{
    if (int rc = nlm_check_params(p)) return rc;
    MID_REQUIRE(n_layers >= 1 && n_layers <= kMaxLayers, "%s: n_layers %d outside 1..16 (a weight from no layers is no joint filter)", who, n_layers);
    MID_REQUIRE(have_layers, "%s: the layer table is NULL", who);
    MID_REQUIRE(n_frames >= 1 && k >= 0, "%s: bad frame range (n=%d k=%d)", who, n_frames, k);
    if (int rc = nlm_layers_temporal_fits(who, n_layers, n_frames, k)) return rc;
    // every h finite and > 0, and the two factors it becomes finite and > 0 in fp32: kd = log2(e) / (255^2 h_0^2) and
    // r_l = h_0^2 / h_l^2 (an infinite or zero factor would turn matching patches, 0 * inf, into NaN)
    for (int l = 0; layer_h && l < n_layers; ++l) {
        MID_REQUIRE(layer_h[l] > 0.f && std::isfinite(layer_h[l]), "%s: every h must be finite and > 0 (layer_h[%d] = %g)", who, l, (double)layer_h[l]);
        const double h0 = (double)layer_h[0], hl = (double)layer_h[l];
        const float kd = nlm_guide_kd(h0), rel = (float)((h0 * h0) / (hl * hl));
        MID_REQUIRE(std::isfinite(kd) && kd > 0.f && std::isfinite(rel) && rel > 0.f,
                    "%s: layer_h[%d] = %g beside layer_h[0] = %g leaves fp32 (log2(e) / (255^2 h_0^2) and h_0^2 / h_l^2 must be finite and > 0)",
                    who, l, hl, h0);
    }
    return MID_OK;
}

int nlm_joint_out(mid_ctx *ctx, const mid_nlm_params *p, const float *layer_h, const void *const *frames, const uint32_t *const *layers,
                  int n_layers, int n_frames, int k, int first, int count, void *const *out, int out_fmt, hipStream_t s)
{
    for (int t = first; t < first + count; ++t) {
        NlmJointArgs a{};
        a.w = p->width; a.h = p->height; a.fmt = p->format;
        const double h0 = layer_h ? (double)layer_h[0] : (double)p->filteringParameter;
        a.kd = nlm_guide_kd(h0);                                              // nlm_layers_temporal.hip's init_args with h = h_0
        for (int l = 0; l < n_layers; ++l) {
            const double hl = layer_h ? (double)layer_h[l] : (double)p->filteringParameter;
            a.rel[l] = (float)((h0 * h0) / (hl * hl));
        }
        pack_temporal_window(a, frames, layers, n_layers, n_frames, k, t);
        a.out = out[t - first]; a.out_fmt = out_fmt;
        if (int rc = dispatch_joint(ctx, p, a, s)) return rc;
    }
    return MID_OK;
}

}  // namespace mid

using namespace mid;

extern "C" int mid_nlm_joint(mid_ctx *ctx, const mid_nlm_params *p, const float *layer_h, const void *const *frames,
                             const uint32_t *const *layers_rgba8, int n_layers, int n_frames, int k, int first, int count,
                             void *const *out, int out_format, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    MID_REQUIRE(p, "nlm_joint: NULL argument");
    MID_REQUIRE(frames && out, "nlm_joint: NULL table");
    MID_REQUIRE(fmt_known(out_format), "nlm_joint: unknown output format %d", out_format);
    if (int rc = nlm_joint_check(p, "nlm_joint", layer_h, layers_rgba8 != nullptr, n_layers, n_frames, k)) return rc;
    if (int rc = check_temporal_window("nlm_joint", p->format, frames, layers_rgba8, n_layers, n_frames, k, first, count, out, out_format)) return rc;
    return nlm_joint_out(ctx, p, layer_h, frames, layers_rgba8, n_layers, n_frames, k, first, count, out, out_format, b.s);
}
