// bilateral_temporal.hip -- the bilateral filter over neighbouring frames: bilateral.hip's dispatch with the range weight taken
// between TWO guide images -- the target frame's and the neighbour frame's -- and the colour taken from the neighbour frame.
//
// One accumulate dispatch, target guide Gt, neighbour guide Gn, neighbour colour In, taps o = (i, j), |i|, |j| <= radius:
//     w = exp(-.5 |o|^2 / ss^2) * exp(-.5 |Gt(p) - Gn(p+o)|^2_rgb / sc^2)
//     W[p].weightColor += w * In(p+o),   W[p].normWeight += w
// Only the centre comes from the target; everything under the taps comes from the neighbour.  The plain form
// (mid_bilateral_pair_accum) has Gt = target frame, Gn = In = neighbour frame; the layered form
// (mid_bilateral_layers_pair_accum) has guide layers for Gt and Gn: RGBA8, or RGBA16F / RGBA32F when the format word says so.  Output t of mid_bilateral_temporal = for each
// neighbour f = max(0,t-k) .. min(n-1,t+k) and, in the layered form, inside it each layer l: one such dispatch into a zeroed W;
// then normalize.comp.  Fused in one kernel per output frame: the accumulators stay in registers across every (f, l) and the
// epilogue normalizes and packs.
//
// The tiled kernels are bilateral_kernel (bilateral.hip) with one more loop around it and the same LDS tiles, nothing else:
//   * plain: ONE float4 tile of the neighbour frame, pre-multiplied by sqrt(-kc) like MODE 0, refilled per neighbour;
//   * layered: the COLOUR tile of neighbour frame f, refilled per neighbour and resident across its layers, plus the GUIDE tile
//     of layer[f][l], refilled per (f, l) through the register-staged prefetch of bilateral_kernel's MODE 2 (the next guide is
//     (f, l+1) or (f+1, 0)); the opaque form of the tap loop is voted per neighbour tile in the first word of the guide tile,
//     which is unused while the colour tile is being filled -- not one static word of LDS more than bilateral_kernel.
// The TARGET centre Gt(p) needs no halo: each lane reads its own P centre texels straight from global memory, coalesced and
// bounds-checked, once per (f, l), and scales them by the multiply that fill_tile / commit apply to a tile texel: the bits of a
// centre read from a tile, which is what makes "target == neighbour" give the bits of bilateral.hip's kernels.
// The tap loop -- arithmetic, order, paired-row exp bursts, priority phases -- is bilateral_kernel's; per dispatch the taps go
// into `acc` and then tot += acc (the plain form applies inv_sc before the add), the order of the chain of dispatches.
//
// Guide texel format (the guide field of mid_bilateral_params.format): a TEMPLATE axis of the layered kernels.  It changes how a
// guide texel reaches a register -- 4, 8 or 16 bytes per texel in the register-staged prefetch, the target-centre load and the
// per-pixel kernel's fetches -- and nothing after that: every format ends as the fp32 value times sc in the same float4 tile.
// The RGBA8 instantiations keep their code (a float4 prefetch slot is four registers where RGBA8 needs one, so a run-time format
// would have charged them for it).  The
// single-frame calls with such guides run here as well: mid_bilateral_layers as the k = 0 window of one frame,
// mid_bilateral_layers_accum as the pair dispatch with target guide == neighbour guide.
//
// Kernel arguments: as nlm_layers_temporal.hip, one launch per output frame carries that output's window by value -- for each
// neighbour its frame pointer and its L layer pointers -- at most MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS of them.
#include "bilateral_shapes.hpp"

namespace mid {

namespace {

constexpr int kMaxPtrs = MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS;

struct BilPairArgs {
    int w, h;
    float ks, kc;                       // exponent scales (log2 domain)
    float sc, inv_sc;                   // sqrt(-kc) and its reciprocal, as BilArgs
    int tiles_x, tiles_y;
    int fmt;                            // MID_FMT_* of the frames
    int n_nb;                           // neighbours of this output: window slots [0, n_nb)
    int n_layers;                       // layers per frame (plain form: 0)
    int t_slot;                         // fused form: the window slot that is the output frame itself
    int out_fmt;
    const void *target;                 // accumulate form: the target guide (plain: a frame in fmt; layered: a layer in the kernel's guide format)
    mid_weightinfo *W;                  // accumulate form
    void *out;                          // fused form, in out_fmt
    const void *p[kMaxPtrs];            // slot j: p[j * (n_layers + 1)] = frame, then its n_layers guide layers
};

__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nwg)
{
    const unsigned q = nwg >> 3, r = nwg & 7u, x = bid & 7u, i = bid >> 3;
    return x * q + (x < r ? x : r) + i;
}

__device__ __forceinline__ const void *nb_frame(const BilPairArgs &a, int j) { return a.p[j * (a.n_layers + 1)]; }
__device__ __forceinline__ const void *nb_layer(const BilPairArgs &a, int j, int l) { return a.p[j * (a.n_layers + 1) + 1 + l]; }
// the target guide of pass l: the output frame itself (plain) or its layer l; the accumulate form carries it on its own
template <bool LAYERED, bool FUSED>
__device__ __forceinline__ const void *target_guide(const BilPairArgs &a, int l)
{
    if (!FUSED) return a.target;
    return LAYERED ? a.p[a.t_slot * (a.n_layers + 1) + 1 + l] : a.p[a.t_slot * (a.n_layers + 1)];
}

// One guide texel as it is loaded (one global_load_dword / dwordx2 / dwordx4) and staged in registers, and its decode to the
// float4 every format shares.  All-zero bits decode to vec4(0) in each format: the out-of-image texel.
template <int GF> struct GuideRaw { using type = float4; };
template <> struct GuideRaw<MID_FMT_RGBA8> { using type = uint32_t; };
template <> struct GuideRaw<MID_FMT_RGBA16F> { using type = uint2; };
template <int GF> __device__ __forceinline__ typename GuideRaw<GF>::type guide_zero()
{
    if constexpr (GF == MID_FMT_RGBA8) return 0u;
    else if constexpr (GF == MID_FMT_RGBA16F) return make_uint2(0u, 0u);
    else return make_float4(0.f, 0.f, 0.f, 0.f);
}
template <int GF> __device__ __forceinline__ typename GuideRaw<GF>::type guide_load(const void *layer, size_t idx)
{
    return ((const typename GuideRaw<GF>::type *)layer)[idx];
}
template <int GF> __device__ __forceinline__ float4 guide_decode(typename GuideRaw<GF>::type v)
{
    if constexpr (GF == MID_FMT_RGBA8) return decode_rgba8(v);
    else if constexpr (GF == MID_FMT_RGBA16F) return decode_rgba16f(v);
    else return v;
}

// One texel with the format as a run-time (wave-uniform) value: the frames' format is a kernarg here, not a template axis.
__device__ __forceinline__ float4 fetch_any(const void *img, int fmt, int w, int h, int x, int y)
{
    if (fmt == MID_FMT_RGBA8) return fetch_texture<MID_FMT_RGBA8>(img, w, h, x, y);
    if (fmt == MID_FMT_RGBA16F) return fetch_texture<MID_FMT_RGBA16F>(img, w, h, x, y);
    return fetch_texture<MID_FMT_RGBA32F>(img, w, h, x, y);
}

__device__ __forceinline__ void fill_any(float4 *lds, int tw, int th, const void *img, int fmt, int w, int h, int x0, int y0, int tid,
                                         int nthreads, float rgb_scale, bool *opaque)
{
    if (fmt == MID_FMT_RGBA8) fill_tile<MID_FMT_RGBA8, false>(lds, tw, th, img, w, h, x0, y0, tid, nthreads, rgb_scale, opaque);
    else if (fmt == MID_FMT_RGBA16F) fill_tile<MID_FMT_RGBA16F, false>(lds, tw, th, img, w, h, x0, y0, tid, nthreads, rgb_scale, opaque);
    else fill_tile<MID_FMT_RGBA32F, false>(lds, tw, th, img, w, h, x0, y0, tid, nthreads, rgb_scale, opaque);
}

// Gt(p) of one lane, scaled like a tile texel (fill_tile / commit: rgb * sc): out-of-image centres are vec4(0), never stored.
template <bool LAYERED, int GF>
__device__ __forceinline__ float4 centre(const void *tg, const BilPairArgs &a, int x, int y)
{
    const float4 c = LAYERED ? fetch_texture<GF>(tg, a.w, a.h, x, y) : fetch_any(tg, a.fmt, a.w, a.h, x, y);
    return make_float4(c.x * a.sc, c.y * a.sc, c.z * a.sc, c.w);
}

// Epilogue of every kernel: the fused form normalizes (normalize.comp, magenta where the weights sum to 0) and packs, the
// accumulate form adds to W.
template <bool FUSED>
__device__ __forceinline__ void put(const BilPairArgs &a, size_t idx, float4 tot, float totw)
{
    if (FUSED) {
        float4 o;
        if (totw == 0.0f) o = make_float4(1.f, 0.f, 1.f, 1.f);
        else o = make_float4(tot.x / totw, tot.y / totw, tot.z / totw, tot.w / totw);
        store_out(a.out, idx, a.out_fmt, o);
    } else {
        float4 *wp = (float4 *)(a.W + idx);
        float4 wc = wp[0], nw = wp[1];
        wc.x += tot.x; wc.y += tot.y; wc.z += tot.z; wc.w += tot.w;
        nw.x += totw;
        wp[0] = wc; wp[1] = nw;
    }
}

// Tuned radii: bilateral_kernel's tile, tap loop and epilogue with the neighbour loop around the pass loop.  GF: the guide
// layers' texel format (layered form); PREFETCH: the guide tile is filled through the register-staged prefetch, or (false) by a
// plain fill_tile at the point of the commit -- same texels, same decode, same scale, so the same bits either way.
// (GF and PREFETCH are trailing arguments with the values of the RGBA8 kernels: those instantiations are the ones that were
// always here, argument for argument.)
// A float4 prefetch slot is four registers: the tuned fused kernels stay at 128 VGPRs or fewer (four waves per SIMD) with it,
// but r = 20 with RGBA32F guides would stage 10 slots = 40 VGPRs on top of the RGBA8 kernel's 176 and spill, so that one fills
// the guide tile without the prefetch (guide_prefetch); LDS holds r = 20 at two waves per SIMD either way.
template <int R, int P, int NW, int GF> constexpr bool guide_prefetch() { return !(GF == MID_FMT_RGBA32F && R == 20); }
template <int R, int P, int NW, bool LAYERED, bool FUSED, int GF = MID_FMT_RGBA8, bool PREFETCH = guide_prefetch<R, P, NW, GF>()>
__global__ __launch_bounds__(NW * 64) void bilateral_pair_kernel(const BilPairArgs a)
{
    static_assert(LAYERED || GF == MID_FMT_RGBA8, "the plain form has no guide layers");
    constexpr int TILE_W = 64, TILE_H = NW * P;
    constexpr int LW = TILE_W + 2 * R, LH = TILE_H + 2 * R;
    constexpr int MR = P + 2 * R;   // tile rows a lane walks per column offset

    extern __shared__ float4 lds[];
    float4 *img_t = lds;                                  // colour source: the neighbour frame
    float4 *gde_t = LAYERED ? lds + LW * LH : lds;        // range-weight source: the neighbour's guide

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned flat = xcd_remap(blockIdx.x, gridDim.x);
    const int ty = (int)(flat / (unsigned)a.tiles_x), tx = (int)(flat - (unsigned)ty * a.tiles_x);
    const int w = a.w, h = a.h;
    const int X0 = tx * TILE_W, Y0 = ty * TILE_H;
    const int gx = X0 + lane, yb = Y0 + wv * P;
    const bool wave_active = yb < h;

    // Register-staged double buffer for the guide tile, as bilateral_kernel's MODE 2: the NEXT guide's texels are requested
    // before the current tap loop and decoded into LDS after it.  Same texels, same decode, same scale as fill_tile: same bits.
    constexpr int PF = LAYERED && PREFETCH ? (LW * LH + NW * 64 - 1) / (NW * 64) : 1;
    typename GuideRaw<GF>::type pf[PF];
    auto prefetch = [&](const void *layer) {
        if constexpr (!PREFETCH) return;
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int t = tid + j * NW * 64;
            const int ty_ = t / LW, tx_ = t - ty_ * LW;
            const int x = X0 - R + tx_, y = Y0 - R + ty_;
            pf[j] = guide_zero<GF>();                      // decodes to vec4(0): the out-of-image texel
            if (t < LW * LH && (unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h) pf[j] = guide_load<GF>(layer, (size_t)y * w + x);
        }
    };
    auto commit = [&](const void *layer) {
        if constexpr (!PREFETCH) {
            fill_tile<GF, false>(gde_t, LW, LH, layer, w, h, X0 - R, Y0 - R, tid, NW * 64, a.sc);
            return;
        }
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int t = tid + j * NW * 64;
            const float4 v = guide_decode<GF>(pf[j]);
            if (t < LW * LH) gde_t[t] = make_float4(v.x * a.sc, v.y * a.sc, v.z * a.sc, v.w);
        }
    };

    const int n_nb = FUSED ? a.n_nb : 1;
    const int n_pass = LAYERED ? (FUSED ? a.n_layers : 1) : 1;    // dispatches per neighbour (no layers: none, the output is magenta)
    if (LAYERED && n_pass > 0) prefetch(nb_layer(a, 0, 0));

    // spatial exponent by |j|: ks * j^2 (wave-uniform)
    float sj[R + 1];
#pragma unroll
    for (int j = 0; j <= R; ++j) sj[j] = a.ks * (float)(j * j);

    float4 tot[P];
    float totw[P];
#pragma unroll
    for (int k = 0; k < P; ++k) { tot[k] = make_float4(0.f, 0.f, 0.f, 0.f); totw[k] = 0.f; }

    for (int f = 0; f < n_nb; ++f) {
        __syncthreads();                                   // every wave has left the previous neighbour's last tap loop
        bool mine = true;                                  // every texel THIS thread stored in the colour tile has alpha == 1.0f
        fill_any(img_t, LW, LH, nb_frame(a, f), a.fmt, w, h, X0 - R, Y0 - R, tid, NW * 64, LAYERED ? 1.0f : a.sc, &mine);
        // The opaque form of the tap loop (bilateral_kernel explains it) is decided from the CONTENT of this neighbour's colour
        // tile, as a dispatch of its own would decide it: the fused call and its chain add the same terms in the same order.
        bool alpha_one = false;
        if constexpr (!LAYERED) {
            alpha_one = __syncthreads_and(mine) != 0;
        } else {
            unsigned *vote = (unsigned *)gde_t;            // the guide tile is free here: its readers passed the barrier above
            if (tid == 0) vote[0] = 1u;
            __syncthreads();
            if (!mine) vote[0] = 0u;
            __syncthreads();
            alpha_one = __builtin_amdgcn_readfirstlane((int)vote[0]) != 0;      // (the pass loop's first barrier comes before the guide tile is written)
        }

        for (int pass = 0; pass < n_pass; ++pass) {
            if constexpr (LAYERED) {
                __syncthreads();                           // every wave has left the previous pass's tap loop (and read the vote)
                commit(nb_layer(a, f, pass));
                if (pass + 1 < n_pass) prefetch(nb_layer(a, f, pass + 1));
                else if (f + 1 < n_nb) prefetch(nb_layer(a, f + 1, 0));
                __syncthreads();
            }
            if (!wave_active) continue;

            float cr[P], cg[P], cb[P];   // centre guide colour Gt(p), from global memory
            const void *tg = target_guide<LAYERED, FUSED>(a, pass);
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const float4 c = centre<LAYERED, GF>(tg, a, gx, yb + k);
                cr[k] = c.x; cg[k] = c.y; cb[k] = c.z;
            }
            float4 acc[P];
            float accw[P];
#pragma unroll
            for (int k = 0; k < P; ++k) { acc[k] = make_float4(0.f, 0.f, 0.f, 0.f); accw[k] = 0.f; }

            auto taps = [&](auto a1_tag) {
            constexpr bool A1 = decltype(a1_tag)::value;
            for (int i = -R; i <= R; ++i) {
                const float si = a.ks * (float)(i * i);
                float sij[R + 1];
#pragma unroll
                for (int j = 0; j <= R; ++j) sij[j] = si + sj[j];
                const int base = (wv * P) * LW + lane + R + i;
                // rows in groups of two: exponent arguments, then all v_exp_f32 of the group in one burst at raised issue
                // priority, then the accumulates -- bilateral_kernel's phases, instruction for instruction
                constexpr int RG = 2;
#pragma unroll
                for (int m0 = 0; m0 < MR; m0 += RG) {
                    float4 cc[RG];
                    float ar[RG][P];
#pragma unroll
                    for (int r = 0; r < RG; ++r) {
                        const int m = m0 + r;
                        if (m >= MR) continue;
                        const float4 g = gde_t[base + m * LW];
                        cc[r] = g;
                        if (LAYERED) cc[r] = img_t[base + m * LW];
#pragma unroll
                        for (int k = 0; k < P; ++k) {
                            const int j = m - R - k;
                            if (j < -R || j > R) continue;
                            const float dx = cr[k] - g.x, dy = cg[k] - g.y, dz = cb[k] - g.z;
                            ar[r][k] = fmaf(-dz, dz, fmaf(-dy, dy, fmaf(-dx, dx, sij[j < 0 ? -j : j])));
                        }
                        if (LAYERED) asm volatile("" ::"v"(g.w), "v"(accw[P - 1]));
                        // opaque form: the colour texel's alpha is kept formally live so that the tile read stays a ds_read_b128
                        if constexpr (A1) asm volatile("" ::"v"(cc[r].w));
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_setprio(1);
#pragma unroll
                    for (int r = 0; r < RG; ++r)
#pragma unroll
                        for (int k = 0; k < P; ++k) {
                            const int j = m0 + r - R - k;
                            if (m0 + r >= MR || j < -R || j > R) continue;
                            ar[r][k] = __builtin_amdgcn_exp2f(ar[r][k]);
                        }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int r = 0; r < RG; ++r)
#pragma unroll
                        for (int k = 0; k < P; ++k) {
                            const int j = m0 + r - R - k;
                            if (m0 + r >= MR || j < -R || j > R) continue;
                            const float wt = ar[r][k];
                            const float4 c = cc[r];
                            acc[k].x = fmaf(c.x, wt, acc[k].x); acc[k].y = fmaf(c.y, wt, acc[k].y);
                            acc[k].z = fmaf(c.z, wt, acc[k].z);
                            if constexpr (!A1) acc[k].w = fmaf(c.w, wt, acc[k].w);
                            accw[k] += wt;
                        }
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_setprio(0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if constexpr (A1) {
#pragma unroll
                for (int k = 0; k < P; ++k) acc[k].w = accw[k];
            }
            };
            if (alpha_one) taps(std::true_type{}); else taps(std::false_type{});
#pragma unroll
            for (int k = 0; k < P; ++k) {   // W += this dispatch's sums (the fused form: the registers that stand for W)
                if (!LAYERED) { acc[k].x *= a.inv_sc; acc[k].y *= a.inv_sc; acc[k].z *= a.inv_sc; }   // back to unscaled colours
                tot[k].x += acc[k].x; tot[k].y += acc[k].y; tot[k].z += acc[k].z; tot[k].w += acc[k].w;
                totw[k] += accw[k];
            }
        }
    }

    if (!wave_active || gx >= w) return;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int gy = yb + k;
        if (gy >= h) break;
        put<FUSED>(a, (size_t)gy * w + gx, tot[k], totw[k]);
    }
}

// Any other radius whose tiles fit LDS: bilateral_rt_kernel's run-time-radius scheme (8 waves x 2 rows, taps in row pairs) with
// the neighbour loop around it.
template <bool LAYERED, bool FUSED, int GF = MID_FMT_RGBA8>
__global__ __launch_bounds__(512) void bilateral_pair_rt_kernel(const BilPairArgs a, const int R)
{
    static_assert(LAYERED || GF == MID_FMT_RGBA8, "the plain form has no guide layers");
    constexpr int NW = 8, P = 2, TILE_W = 64, TILE_H = NW * P;
    const int LW = TILE_W + 2 * R, LH = TILE_H + 2 * R;
    extern __shared__ float4 lds[];
    float4 *img_t = lds;
    float4 *gde_t = LAYERED ? lds + LW * LH : lds;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned flat = xcd_remap(blockIdx.x, gridDim.x);
    const int ty = (int)(flat / (unsigned)a.tiles_x), tx = (int)(flat - (unsigned)ty * a.tiles_x);
    const int w = a.w, h = a.h;
    const int X0 = tx * TILE_W, Y0 = ty * TILE_H;
    const int gx = X0 + lane, yb = Y0 + wv * P;
    const bool wave_active = yb < h;

    float4 tot[P];
    float totw[P];
#pragma unroll
    for (int k = 0; k < P; ++k) { tot[k] = make_float4(0.f, 0.f, 0.f, 0.f); totw[k] = 0.f; }
    const int n_nb = FUSED ? a.n_nb : 1;
    const int n_pass = LAYERED ? (FUSED ? a.n_layers : 1) : 1;
    for (int f = 0; f < n_nb; ++f) {
        __syncthreads();                                   // the previous neighbour's readers are done with the colour tile
        fill_any(img_t, LW, LH, nb_frame(a, f), a.fmt, w, h, X0 - R, Y0 - R, tid, NW * 64, LAYERED ? 1.0f : a.sc, nullptr);
        for (int pass = 0; pass < n_pass; ++pass) {
            if (LAYERED) {
                __syncthreads();
                fill_tile<GF, false>(gde_t, LW, LH, nb_layer(a, f, pass), w, h, X0 - R, Y0 - R, tid, NW * 64, a.sc);
            }
            __syncthreads();
            if (!wave_active) continue;
            float cr[P], cg[P], cb[P];
            const void *tg = target_guide<LAYERED, FUSED>(a, pass);
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const float4 c = centre<LAYERED, GF>(tg, a, gx, yb + k);
                cr[k] = c.x; cg[k] = c.y; cb[k] = c.z;
            }
            float4 acc[P];
            float accw[P];
#pragma unroll
            for (int k = 0; k < P; ++k) { acc[k] = make_float4(0.f, 0.f, 0.f, 0.f); accw[k] = 0.f; }
            for (int i = -R; i <= R; ++i) {
                const float si = a.ks * (float)(i * i);
                const int base = (wv * P) * LW + lane + R + i;
                // tile row m feeds output k = 0 with j = m - R and output k = 1 with j = m - R - 1: first and last row alone, the
                // 2R rows between them in pairs with their four exps as one burst (bilateral_rt_kernel)
                auto arg_of = [&](const float4 &g, int k, int j) {
                    const float dx = cr[k] - g.x, dy = cg[k] - g.y, dz = cb[k] - g.z;
                    return fmaf(-dz, dz, fmaf(-dy, dy, fmaf(-dx, dx, fmaf(a.ks, (float)(j * j), si))));
                };
                auto add_tap = [&](const float4 &c, int k, float wt) {
                    acc[k].x = fmaf(c.x, wt, acc[k].x); acc[k].y = fmaf(c.y, wt, acc[k].y);
                    acc[k].z = fmaf(c.z, wt, acc[k].z); acc[k].w = fmaf(c.w, wt, acc[k].w);
                    accw[k] += wt;
                };
                {
                    const float4 g = gde_t[base];
                    add_tap(LAYERED ? img_t[base] : g, 0, exp2_hw(arg_of(g, 0, -R)));
                }
                for (int m = 1; m < 2 * R; m += 2) {
                    const float4 g0 = gde_t[base + m * LW], g1 = gde_t[base + (m + 1) * LW];
                    const float4 c0 = LAYERED ? img_t[base + m * LW] : g0, c1 = LAYERED ? img_t[base + (m + 1) * LW] : g1;
                    float w00 = arg_of(g0, 0, m - R), w01 = arg_of(g0, 1, m - R - 1), w10 = arg_of(g1, 0, m + 1 - R), w11 = arg_of(g1, 1, m - R);
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_setprio(1);
                    w00 = __builtin_amdgcn_exp2f(w00); w01 = __builtin_amdgcn_exp2f(w01);
                    w10 = __builtin_amdgcn_exp2f(w10); w11 = __builtin_amdgcn_exp2f(w11);
                    __builtin_amdgcn_sched_barrier(0);
                    add_tap(c0, 0, w00); add_tap(c0, 1, w01); add_tap(c1, 0, w10); add_tap(c1, 1, w11);
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_setprio(0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                {
                    const int m = 2 * R + 1;
                    const float4 g = gde_t[base + m * LW];
                    add_tap(LAYERED ? img_t[base + m * LW] : g, 1, exp2_hw(arg_of(g, 1, R)));
                }
            }
#pragma unroll
            for (int k = 0; k < P; ++k) {
                if (!LAYERED) { acc[k].x *= a.inv_sc; acc[k].y *= a.inv_sc; acc[k].z *= a.inv_sc; }
                tot[k].x += acc[k].x; tot[k].y += acc[k].y; tot[k].z += acc[k].z; tot[k].w += acc[k].w;
                totw[k] += accw[k];
            }
        }
    }
    if (!wave_active || gx >= w) return;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int gy = yb + k;
        if (gy >= h) break;
        put<FUSED>(a, (size_t)gy * w + gx, tot[k], totw[k]);
    }
}

// Last resort (the layered form's two tiles do not fit LDS): one thread per pixel with global fetches,
// bilateral_generic_kernel's arithmetic.
template <bool FUSED, int GF = MID_FMT_RGBA8>
__global__ __launch_bounds__(256) void bilateral_pair_generic_kernel(const BilPairArgs a, int R)
{
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= a.w || y >= a.h) return;
    float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
    float totw = 0.f;
    const int n_nb = FUSED ? a.n_nb : 1, n_pass = FUSED ? a.n_layers : 1;
    for (int f = 0; f < n_nb; ++f) {
        const void *in = nb_frame(a, f);
        for (int pass = 0; pass < n_pass; ++pass) {
            const void *gn = nb_layer(a, f, pass);
            const float4 ctr = fetch_texture<GF>(target_guide<true, FUSED>(a, pass), a.w, a.h, x, y);
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            float accw = 0.f;
            for (int j = -R; j <= R; ++j)
                for (int i = -R; i <= R; ++i) {
                    const float4 g = fetch_texture<GF>(gn, a.w, a.h, x + i, y + j);
                    const float4 c = fetch_any(in, a.fmt, a.w, a.h, x + i, y + j);
                    const float dx = ctr.x - g.x, dy = ctr.y - g.y, dz = ctr.z - g.z;
                    const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                    const float wt = exp2_hw(fmaf(d2, a.kc, a.ks * (float)(i * i + j * j)));
                    acc.x = fmaf(c.x, wt, acc.x); acc.y = fmaf(c.y, wt, acc.y);
                    acc.z = fmaf(c.z, wt, acc.z); acc.w = fmaf(c.w, wt, acc.w);
                    accw += wt;
                }
            tot.x += acc.x; tot.y += acc.y; tot.z += acc.z; tot.w += acc.w;
            totw += accw;
        }
    }
    put<FUSED>(a, (size_t)y * a.w + x, tot, totw);
}

template <int R, int P, int NW, bool LAYERED, bool FUSED, int GF>
int launch_pair_tiled(mid_ctx *ctx, BilPairArgs &a, hipStream_t s)
{
    constexpr size_t lds_bytes = bil_lds_bytes(R, NW * P, LAYERED);
    auto kern = bilateral_pair_kernel<R, P, NW, LAYERED, FUSED, GF>;
    if ((int)lds_bytes > ctx->lds_max)
        return set_error(MID_ERR_UNSUPPORTED, "bilateral_temporal tile needs %zu B of LDS, device offers %d", lds_bytes, ctx->lds_max);
    if (int rc = ensure_lds(ctx, (const void *)kern, lds_bytes)) return rc;
    a.tiles_x = (int)cdiv(a.w, 64);
    a.tiles_y = (int)cdiv(a.h, NW * P);
    hipLaunchKernelGGL(kern, dim3((unsigned)a.tiles_x * a.tiles_y), dim3(NW * 64), lds_bytes, s, a);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

template <bool LAYERED, bool FUSED, int GF>
int dispatch_pair_radius(mid_ctx *ctx, int radius, BilPairArgs &a, hipStream_t s)
{
    static_assert(LAYERED || GF == MID_FMT_RGBA8, "the plain form has no guide layers");
    return bil_for_radius(radius,
        [&](auto sh) { return launch_pair_tiled<decltype(sh)::R, decltype(sh)::P, decltype(sh)::NW, LAYERED, FUSED, GF>(ctx, a, s); },
        [&]() -> int {
            const size_t lds_bytes = bil_lds_bytes(radius, kBilRtNW * kBilRtP, LAYERED);
            if ((int)lds_bytes <= ctx->lds_max) {
                auto kern = bilateral_pair_rt_kernel<LAYERED, FUSED, GF>;
                if (int rc = ensure_lds(ctx, (const void *)kern, (size_t)ctx->lds_max)) return rc;
                a.tiles_x = (int)cdiv(a.w, 64);
                a.tiles_y = (int)cdiv(a.h, kBilRtNW * kBilRtP);
                hipLaunchKernelGGL(kern, dim3((unsigned)a.tiles_x * a.tiles_y), dim3(kBilRtNW * 64), lds_bytes, s, a, radius);
                MID_HIP(hipGetLastError());
                return MID_OK;
            }
            // (only the two-tile layered form at r > 17 gets here: the plain form's single tile fits LDS for every legal radius)
            if constexpr (LAYERED) {
                const dim3 grid(cdiv(a.w, 16), cdiv(a.h, 16));
                hipLaunchKernelGGL((bilateral_pair_generic_kernel<FUSED, GF>), grid, dim3(256), 0, s, a, radius);
                MID_HIP(hipGetLastError());
                return MID_OK;
            } else {
                return set_error(MID_ERR_UNSUPPORTED, "bilateral_temporal: the tile of radius %d does not fit %d B of LDS", radius, ctx->lds_max);
            }
        });
}

// guide_fmt: the guide layers' MID_FMT_* (fmt_guide of the format word); the plain form passes MID_FMT_RGBA8.
template <bool LAYERED, bool FUSED>
int dispatch_pair(mid_ctx *ctx, int radius, int guide_fmt, BilPairArgs &a, hipStream_t s)
{
    if constexpr (LAYERED) {
        if (guide_fmt == MID_FMT_RGBA16F) return dispatch_pair_radius<true, FUSED, MID_FMT_RGBA16F>(ctx, radius, a, s);
        if (guide_fmt == MID_FMT_RGBA32F) return dispatch_pair_radius<true, FUSED, MID_FMT_RGBA32F>(ctx, radius, a, s);
    }
    return dispatch_pair_radius<LAYERED, FUSED, MID_FMT_RGBA8>(ctx, radius, a, s);
}

void init_args(BilPairArgs &a, const mid_bilateral_params *p)
{
    bil_fill_scales(p, a);
    a.fmt = fmt_frames(p->format);
}

// mid_bilateral's parameter checks and "no temporal form for the linear layout".  guide_ok: the call reads guide layers.
int check_pair_params(const mid_bilateral_params *p, const char *who, bool guide_ok)
{
    if (int rc = bilateral_check_params(p, who, guide_ok)) return rc;
    MID_REQUIRE(p->layout == MID_LAYOUT_TEXTURE, "%s: neighbouring frames exist for the texture layout only", who);
    return MID_OK;
}

}  // namespace

int bilateral_temporal_check(const mid_bilateral_params *p, const char *who, bool layered, int n_layers, int n_frames, int k)
{
    if (int rc = check_pair_params(p, who, layered)) return rc;
    MID_REQUIRE(n_layers >= 0 && n_layers <= kMaxLayers, "%s: n_layers %d outside 0..16", who, n_layers);
    MID_REQUIRE(layered || n_layers == 0, "%s: n_layers is %d without a layer table (the plain form takes 0)", who, n_layers);
    MID_REQUIRE(n_frames >= 1 && k >= 0, "%s: bad n_frames=%d k=%d", who, n_frames, k);
    return nlm_layers_temporal_fits(who, n_layers, n_frames, k);
}

int bilateral_temporal_out(mid_ctx *ctx, const mid_bilateral_params *p, const void *const *frames, const uint32_t *const *layers,
                           int n_layers, int n_frames, int k, int first, int count, void *const *out, int out_fmt, hipStream_t s)
{
    for (int t = first; t < first + count; ++t) {
        BilPairArgs a{};
        init_args(a, p);
        pack_temporal_window(a, frames, layers, layers ? n_layers : 0, n_frames, k, t);
        a.out = out[t - first]; a.out_fmt = out_fmt;
        const int rc = layers ? dispatch_pair<true, true>(ctx, p->radius, fmt_guide(p->format), a, s)
                              : dispatch_pair<false, true>(ctx, p->radius, MID_FMT_RGBA8, a, s);
        if (rc) return rc;
    }
    return MID_OK;
}

int bilateral_layers_pair_out(mid_ctx *ctx, const mid_bilateral_params *p, const void *target_layer, const void *neighbour_layer,
                              const void *neighbour_in, mid_weightinfo *W, hipStream_t s)
{
    BilPairArgs a{};
    init_args(a, p);
    a.n_nb = 1; a.n_layers = 1; a.t_slot = 0;
    a.target = target_layer;
    a.p[0] = neighbour_in;
    a.p[1] = neighbour_layer;
    a.W = W;
    return dispatch_pair<true, false>(ctx, p->radius, fmt_guide(p->format), a, s);
}

}  // namespace mid

using namespace mid;

extern "C" int mid_bilateral_pair_accum(mid_ctx *ctx, const mid_bilateral_params *p, const void *target, const void *neighbour,
                                        mid_weightinfo *W, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    if (int rc = check_pair_params(p, "bilateral_pair_accum", false)) return rc;
    MID_REQUIRE(target && neighbour && W, "bilateral_pair_accum: NULL pointer");
    MID_REQUIRE(fmt_aligned(p->format, target) && fmt_aligned(p->format, neighbour), "bilateral_pair_accum: RGBA16F frames must be 8-byte aligned");
    BilPairArgs a{};
    init_args(a, p);
    a.n_nb = 1; a.n_layers = 0; a.t_slot = 0;
    a.target = target;
    a.p[0] = neighbour;
    a.W = W;
    return dispatch_pair<false, false>(ctx, p->radius, MID_FMT_RGBA8, a, b.s);
}

extern "C" int mid_bilateral_layers_pair_accum(mid_ctx *ctx, const mid_bilateral_params *p, const uint32_t *target_layer_rgba8,
                                               const uint32_t *neighbour_layer_rgba8, const void *neighbour_in, mid_weightinfo *W,
                                               void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    if (int rc = check_pair_params(p, "bilateral_layers_pair_accum", true)) return rc;
    MID_REQUIRE(target_layer_rgba8 && neighbour_layer_rgba8 && neighbour_in && W, "bilateral_layers_pair_accum: NULL pointer");
    MID_REQUIRE(fmt_aligned(fmt_frames(p->format), neighbour_in), "bilateral_layers_pair_accum: RGBA16F input must be 8-byte aligned");
    MID_REQUIRE(guide_aligned(fmt_guide(p->format), target_layer_rgba8) && guide_aligned(fmt_guide(p->format), neighbour_layer_rgba8),
                "bilateral_layers_pair_accum: RGBA16F guide layers must be 8-byte aligned, RGBA32F ones 16-byte aligned");
    return bilateral_layers_pair_out(ctx, p, target_layer_rgba8, neighbour_layer_rgba8, neighbour_in, W, b.s);
}

extern "C" int mid_bilateral_temporal(mid_ctx *ctx, const mid_bilateral_params *p, const void *const *frames,
                                      const uint32_t *const *layers_rgba8, int n_layers, int n_frames, int k, int first, int count,
                                      void *const *out, int out_format, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    MID_REQUIRE(frames && out, "bilateral_temporal: NULL table");
    MID_REQUIRE(fmt_known(out_format), "bilateral_temporal: unknown output format %d", out_format);
    if (int rc = bilateral_temporal_check(p, "bilateral_temporal", layers_rgba8 != nullptr, n_layers, n_frames, k)) return rc;
    if (int rc = check_temporal_window("bilateral_temporal", fmt_frames(p->format), frames, layers_rgba8, n_layers, n_frames, k, first, count, out, out_format,
                                       fmt_guide(p->format))) return rc;
    return bilateral_temporal_out(ctx, p, frames, layers_rgba8, n_layers, n_frames, k, first, count, out, out_format, b.s);
}
