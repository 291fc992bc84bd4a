// bilateral.hip -- bilateral filters for gfx950 (replaces shaders/bialteral.comp,
// bialteral_linear.comp and bialteral_layers.comp).
//
// Design.  A workgroup stages its output tile plus a `radius` halo in LDS as float4 texels
// (coalesced 16 B/lane HBM reads, halo zero-filled per the reference's out-of-image policy).
// A wave owns 64 adjacent columns x P rows: lane l owns one column and P vertically adjacent
// outputs, so each LDS texel it reads (one conflict-free ds_read_b128) feeds up to P taps.
// Per tap: 3 sub, 3 mul/fma (colour distance), 1 fma folding the colour and the spatial
// exponent, 1 v_exp_f32, 4 fma + 1 add.  The two exp() of the shader become one:
//     exp(-.5 (sd/ss)^2) * exp(-.5 (cd/sc)^2) = exp2(ks*(i^2+j^2) + kc*cd^2)
// with ks = -.5*log2(e)/ss^2, kc = -.5*log2(e)/sc^2; the spatial term is wave-uniform.
//
// The texture and linear variants differ only in how the tile is addressed when it is filled
// (2-D zero border vs flat index with row wrap-around), exactly the difference between
// bialteral.comp:58-59 and bialteral_linear.comp:58.
//
// The tap loops, the guide prefetch, the opaque vote and the epilogue below are restated in bilateral_temporal.hip, whose kernels
// put a loop over neighbouring frames around them.  The copies are deliberate.  With both files calling one set of
// __forceinline__ function templates the instruction mix, LDS and occupancy classes stayed the same but register allocation
// did not, and on an MI355X (profiles/r10_ab_shared_filter_bodies.txt; medians in ms, parent -> shared, parent-against-parent
// spread 0.0000-0.0012) r = 20 went 0.9281 -> 0.9390 (+1.2 %), r = 4 0.0495 -> 0.0497, layers fused r = 8 L = 1 0.1648 -> 0.1671
// (+1.4 %), r = 10 L = 4 1.0021 -> 1.0096, run-time radius r = 3 / 12 / 16 +0.3-3 %; only r = 8 and r = 10 held.  These are the
// bench paths.  A change to the tap arithmetic has to be made in both files; the k = 0 identities of
// tests/test_gpu_bilateral_temporal.py fail when only one is changed, tests/test_gpu_kernel_bits.py when the bits move at all.
// Shared with that file: the scales and the table of tuned radii and tile shapes (bilateral_shapes.hpp), store_out (common.hpp).
#include "bilateral_shapes.hpp"
#include <cstdlib>

namespace mid {

struct BilArgs {
    int w, h;
    float ks, kc;          // exponent scales (log2 domain)
    float sc, inv_sc;      // sqrt(-kc) and its reciprocal: the tiled kernels carry the range scale in the guide colours
    int tiles_x, tiles_y;
    const void *in;
    void *out;             // plain / fused-layers output, written as out_fmt
    mid_weightinfo *W;     // layers accumulate mode
    int n_layers;
    int out_fmt;           // MID_FMT_* of `out`: float4, RGBA8 (pack_rgba8) or RGBA16F (pack_rgba16f); a kernarg, so wave-uniform
    const uint32_t *layers[kMaxLayers];
};

// Frame tables of the batched plain bilateral (mid_bilateral_batch): passed by value in kernarg space like the NLM
// kernels' tables.  Single-frame launches pass the empty BilOne instead, so their kernarg block stays small.
struct BilBatch { FrameTable in; OutTable out; };
struct BilOne {};

__device__ __forceinline__ unsigned xcd_remap_b(unsigned bid, unsigned nwg)
{
    const unsigned q = nwg >> 3, r = nwg & 7u, x = bid & 7u, i = bid >> 3;
    return x * q + (x < r ? x : r) + i;
}

// MODE 0: plain bilateral (range weight and colour from `in`)
// MODE 1: layers, accumulate one layer into W      (one dispatch of bialteral_layers.comp)
// MODE 2: layers, all layers fused + normalize     (loop src/main.cpp:1610-1623 + normalize.comp)
template <int R, int P, int NW, int FMT, bool LINEAR, int MODE, typename BT>
__global__ __launch_bounds__(NW * 64) void bilateral_kernel(const BilArgs a, const BT bt)
{
    constexpr bool BATCH = std::is_same<BT, BilBatch>::value;
    constexpr int TILE_W = 64, TILE_H = NW * P;
    constexpr int LW = TILE_W + 2 * R, LH = TILE_H + 2 * R;
    constexpr int MR = P + 2 * R;   // tile rows a lane walks per column offset

    extern __shared__ float4 lds[];
    float4 *img_t = lds;                                  // colour source
    float4 *gde_t = (MODE == 0) ? lds : lds + LW * LH;    // range-weight source (guide)

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned flat;
    const void *in = a.in;
    void *out = a.out;
    if constexpr (BATCH) {
        // frames in launch order, tiles remapped inside their frame (every XCD gets a contiguous run of each frame)
        const unsigned tiles = (unsigned)(a.tiles_x * a.tiles_y);
        const unsigned fz = blockIdx.x / tiles;
        flat = xcd_remap_in_frame(blockIdx.x - fz * tiles, tiles, fz);
        in = bt.in.p[fz];
        out = bt.out.p[fz];
    } else {
        flat = xcd_remap_b(blockIdx.x, gridDim.x);
    }
    const int ty = (int)(flat / (unsigned)a.tiles_x), tx = (int)(flat - (unsigned)ty * a.tiles_x);
    const int w = a.w, h = a.h;
    const int X0 = tx * TILE_W, Y0 = ty * TILE_H;
    const int gx = X0 + lane, yb = Y0 + wv * P;
    const bool wave_active = yb < h;

    // Register-staged double buffer for the guide tile (MODE 2): the NEXT layer's RGBA8 texels -- PF u32 per thread -- are
    // requested from HBM before the current layer's tap loop and only decoded into LDS after it, between the two barriers
    // that already separate the passes (the first layer's request goes out ahead of the image tile's fill).  Same texels,
    // same decode, same scale as fill_tile ==> the same bits in LDS; not a byte more LDS.  Measured: 4 layers at r = 8
    // 0.702 -> 0.689 ms, r = 4 0.207 -> 0.203, r = 10 1.083 -> 1.061, outputs bit-identical (LABNOTES R5.2).
    constexpr int PF = (LW * LH + NW * 64 - 1) / (NW * 64);
    uint32_t pf[PF];
    auto prefetch = [&](const uint32_t *layer) {
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int t = tid + j * NW * 64;
            const int ty_ = t / LW, tx_ = t - ty_ * LW;
            const int x = X0 - R + tx_, y = Y0 - R + ty_;
            pf[j] = 0u;                                    // decode_rgba8(0) == vec4(0): the out-of-image texel
            if (t < LW * LH && (unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h) pf[j] = layer[(size_t)y * w + x];
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int t = tid + j * NW * 64;
            const float4 v = decode_rgba8(pf[j]);
            if (t < LW * LH) gde_t[t] = make_float4(v.x * a.sc, v.y * a.sc, v.z * a.sc, v.w);
        }
    };
    if (MODE == 2 && a.n_layers > 0) prefetch(a.layers[0]);      // (no layers: the loop below does not run, the output is the magenta sentinel)
    // The guide colours (the image itself in MODE 0) are pre-multiplied by sqrt(-kc), so -|dc|^2 is already the
    // colour part of the exp2 argument and the FMA chain can start from the spatial term: 12 ops per tap, not 13.
    bool mine = true;                                     // every texel THIS thread stored in the colour tile has alpha == 1.0f
    fill_tile<FMT, LINEAR>(img_t, LW, LH, in, w, h, X0 - R, Y0 - R, tid, NW * 64, MODE == 0 ? a.sc : 1.0f, &mine);

    // Is every texel of the colour tile opaque (alpha == 1.0f, the usual case away from the image border, where out-of-image
    // texels are vec4(0))?  Then the alpha accumulator repeats the weight accumulator operation for operation --
    // fma(1.0f, wt, acc.w) and accw + wt round alike, both start at 0 -- and the tap loop need not carry it: one FMA of 13
    // instructions per tap less, the same bits.  Round 6: r = 8 0.1541 -> 0.1490 ms (-3.3 %), r = 10 / 20 -3 %, r = 4 -1 %, every
    // output's sha equal; 4 layers fused at r = 8 0.6443 -> 0.6225 ms (-3.4 %), r = 10 -3.7 %, r = 4 -2 %
    // (profiles/r06_ab_bilateral_opaque_alpha.txt, LABNOTES R6.7).
    // How the workgroup agrees.  Plain bilateral: __syncthreads_and (4 B of static LDS: the 40 KB tile then fits three times per
    // CU instead of four, which this kernel does not notice -- 0.1547-0.1553 against 0.1552-0.1554 ms).  Layer modes: their two
    // tiles are EXACTLY half the CU's LDS, and one static word would halve the occupancy (+20 %, measured); the guide tile is
    // still unused at this point, so its first word carries the vote.
    bool alpha_one = false;
    if constexpr (MODE == 0) {
        alpha_one = __syncthreads_and(mine) != 0;
    } else {
        unsigned *vote = (unsigned *)gde_t;
        if (tid == 0) vote[0] = 1u;
        __syncthreads();
        if (!mine) vote[0] = 0u;
        __syncthreads();
        alpha_one = __builtin_amdgcn_readfirstlane((int)vote[0]) != 0;      // (the pass loop's first barrier comes before the guide tile is written)
    }

    // spatial exponent by |j|: ks * j^2 (wave-uniform)
    float sj[R + 1];
#pragma unroll
    for (int j = 0; j <= R; ++j) sj[j] = a.ks * (float)(j * j);

    float4 tot[P];
    float totw[P];
#pragma unroll
    for (int k = 0; k < P; ++k) { tot[k] = make_float4(0.f, 0.f, 0.f, 0.f); totw[k] = 0.f; }

    const int n_pass = (MODE == 2) ? a.n_layers : 1;
    for (int pass = 0; pass < n_pass; ++pass) {
        if (MODE == 2) {
            __syncthreads();                               // every wave has left the previous pass's tap loop
            commit();
            if (pass + 1 < n_pass) prefetch(a.layers[pass + 1]);
        } else if (MODE != 0) {
            __syncthreads();
            fill_tile<MID_FMT_RGBA8, false>(gde_t, LW, LH, a.layers[pass], w, h, X0 - R, Y0 - R, tid, NW * 64, a.sc);
        }
        __syncthreads();
        if (!wave_active) continue;

        float cr[P], cg[P], cb[P];   // centre guide colour (texColor / layerColor)
#pragma unroll
        for (int k = 0; k < P; ++k) {
            const float4 c = gde_t[(wv * P + k + R) * LW + lane + R];
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
            // Rows in groups of RG = 2 (measured against 0/3/4/6/9/18: profiles/r03_ab_bilateral_exp_bursts.txt): exponent arguments
            // of the group (plain VALU), then ALL its v_exp_f32 in one burst at raised issue priority, then the accumulates, still
            // at raised priority.  A transcendental mixed into other waves' plain instructions costs far more than its own 8
            // cycles (tools/microbench10/11.hip: 8 exps + 88 FMAs 357 cycles per group per SIMD against 67 + 211 alone; 274
            // with s_setprio around the exp burst); scheduling barriers keep the three phases apart.
            // Same instructions per tap, same accumulation order: identical output bits.
            // (Each group's two ds_read_b128 are followed directly by their first use.  Issuing them one group ahead was measured in
            // round 6 and buys nothing -- 8 waves per SIMD cover the LDS latency already; profiles/r06_ab_bilateral_readahead.txt.)
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
                    if (MODE != 0) cc[r] = img_t[base + m * LW];
#pragma unroll
                    for (int k = 0; k < P; ++k) {
                        const int j = m - R - k;
                        if (j < -R || j > R) continue;
                        const float dx = cr[k] - g.x, dy = cg[k] - g.y, dz = cb[k] - g.z;
                        ar[r][k] = fmaf(-dz, dz, fmaf(-dy, dy, fmaf(-dx, dx, sij[j < 0 ? -j : j])));
                    }
                    if (MODE != 0) asm volatile("" ::"v"(g.w), "v"(accw[P - 1]));
                    // opaque form: the colour texel's alpha is not used any more; kept formally live so that the tile read stays a
                    // ds_read_b128 (4 LDS cycles; the ds_read_b96 the compiler would shrink it to takes 8: LDS utilisation 0.45 against 0.22)
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
        for (int k = 0; k < P; ++k) {
            if (MODE == 0) { acc[k].x *= a.inv_sc; acc[k].y *= a.inv_sc; acc[k].z *= a.inv_sc; }   // back to unscaled colours
            tot[k].x += acc[k].x; tot[k].y += acc[k].y; tot[k].z += acc[k].z; tot[k].w += acc[k].w;
            totw[k] += accw[k];
        }
    }

    if (!wave_active || gx >= w) return;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int gy = yb + k;
        if (gy >= h) break;
        const size_t idx = (size_t)gy * w + gx;
        if (MODE == 0) {
            store_out(out, idx, a.out_fmt, make_float4(tot[k].x / totw[k], tot[k].y / totw[k], tot[k].z / totw[k], tot[k].w / totw[k]));
        } else if (MODE == 2) {
            float4 o;
            if (totw[k] == 0.0f) o = make_float4(1.f, 0.f, 1.f, 1.f);
            else o = make_float4(tot[k].x / totw[k], tot[k].y / totw[k], tot[k].z / totw[k], tot[k].w / totw[k]);
            store_out(out, idx, a.out_fmt, o);
        } else {
            float4 *wp = (float4 *)(a.W + idx);
            float4 wc = wp[0], nw = wp[1];
            wc.x += tot[k].x; wc.y += tot[k].y; wc.z += tot[k].z; wc.w += tot[k].w;
            nw.x += totw[k];
            wp[0] = wc; wp[1] = nw;
        }
    }
}

// Any radius without a tuned instantiation: the same LDS-tiled scheme with the radius as a run-time
// value (loops not unrolled, spatial exponent computed per tap row).  8 waves x 2 rows per workgroup.
template <int FMT, bool LINEAR, int MODE, typename BT>
__global__ __launch_bounds__(512) void bilateral_rt_kernel(const BilArgs a, const int R, const BT bt)
{
    constexpr bool BATCH = std::is_same<BT, BilBatch>::value;
    constexpr int NW = 8, P = 2, TILE_W = 64, TILE_H = NW * P;
    const int LW = TILE_W + 2 * R, LH = TILE_H + 2 * R;
    extern __shared__ float4 lds[];
    float4 *img_t = lds;
    float4 *gde_t = (MODE == 0) ? lds : lds + LW * LH;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned flat;
    const void *in = a.in;
    void *out = a.out;
    if constexpr (BATCH) {
        const unsigned tiles = (unsigned)(a.tiles_x * a.tiles_y);
        const unsigned fz = blockIdx.x / tiles;
        flat = xcd_remap_in_frame(blockIdx.x - fz * tiles, tiles, fz);
        in = bt.in.p[fz];
        out = bt.out.p[fz];
    } else {
        flat = xcd_remap_b(blockIdx.x, gridDim.x);
    }
    const int ty = (int)(flat / (unsigned)a.tiles_x), tx = (int)(flat - (unsigned)ty * a.tiles_x);
    const int w = a.w, h = a.h;
    const int X0 = tx * TILE_W, Y0 = ty * TILE_H;
    const int gx = X0 + lane, yb = Y0 + wv * P;
    const bool wave_active = yb < h;

    fill_tile<FMT, LINEAR>(img_t, LW, LH, in, w, h, X0 - R, Y0 - R, tid, NW * 64, MODE == 0 ? a.sc : 1.0f);
    float4 tot[P];
    float totw[P];
#pragma unroll
    for (int k = 0; k < P; ++k) { tot[k] = make_float4(0.f, 0.f, 0.f, 0.f); totw[k] = 0.f; }
    const int n_pass = (MODE == 2) ? a.n_layers : 1;
    for (int pass = 0; pass < n_pass; ++pass) {
        if (MODE != 0) {
            __syncthreads();
            fill_tile<MID_FMT_RGBA8, false>(gde_t, LW, LH, a.layers[pass], w, h, X0 - R, Y0 - R, tid, NW * 64, a.sc);
        }
        __syncthreads();
        if (!wave_active) continue;
        float cr[P], cg[P], cb[P];
#pragma unroll
        for (int k = 0; k < P; ++k) {
            const float4 c = gde_t[(wv * P + k + R) * LW + lane + R];
            cr[k] = c.x; cg[k] = c.y; cb[k] = c.z;
        }
        float4 acc[P];
        float accw[P];
#pragma unroll
        for (int k = 0; k < P; ++k) { acc[k] = make_float4(0.f, 0.f, 0.f, 0.f); accw[k] = 0.f; }
        for (int i = -R; i <= R; ++i) {
            const float si = a.ks * (float)(i * i);
            const int base = (wv * P) * LW + lane + R + i;
            // Tile row m feeds output k = 0 with row offset j = m - R and output k = 1 with j = m - R - 1; the first row has only the
            // k = 0 tap, the last only the k = 1 tap, and the 2R rows between them go in PAIRS with their four exps as one burst at
            // raised issue priority, like the tuned kernel (per output the taps are still added in row order: same bits).
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
                add_tap(MODE != 0 ? img_t[base] : g, 0, exp2_hw(arg_of(g, 0, -R)));
            }
            for (int m = 1; m < 2 * R; m += 2) {
                const float4 g0 = gde_t[base + m * LW], g1 = gde_t[base + (m + 1) * LW];
                const float4 c0 = MODE != 0 ? img_t[base + m * LW] : g0, c1 = MODE != 0 ? img_t[base + (m + 1) * LW] : g1;
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
                add_tap(MODE != 0 ? img_t[base + m * LW] : g, 1, exp2_hw(arg_of(g, 1, R)));
            }
        }
#pragma unroll
        for (int k = 0; k < P; ++k) {
            if (MODE == 0) { acc[k].x *= a.inv_sc; acc[k].y *= a.inv_sc; acc[k].z *= a.inv_sc; }
            tot[k].x += acc[k].x; tot[k].y += acc[k].y; tot[k].z += acc[k].z; tot[k].w += acc[k].w;
            totw[k] += accw[k];
        }
    }
    if (!wave_active || gx >= w) return;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int gy = yb + k;
        if (gy >= h) break;
        const size_t idx = (size_t)gy * w + gx;
        if (MODE == 1) {
            float4 *wp = (float4 *)(a.W + idx);
            float4 wc = wp[0], nw = wp[1];
            wc.x += tot[k].x; wc.y += tot[k].y; wc.z += tot[k].z; wc.w += tot[k].w;
            nw.x += totw[k];
            wp[0] = wc; wp[1] = nw;
        } else {
            float4 o;
            if (MODE == 2 && totw[k] == 0.0f) o = make_float4(1.f, 0.f, 1.f, 1.f);
            else o = make_float4(tot[k].x / totw[k], tot[k].y / totw[k], tot[k].z / totw[k], tot[k].w / totw[k]);
            store_out(out, idx, a.out_fmt, o);
        }
    }
}

// Last resort (tile does not fit LDS): one thread per pixel, global fetches.
template <int FMT, bool LINEAR, int MODE>
__global__ __launch_bounds__(256) void bilateral_generic_kernel(const BilArgs a, int R)
{
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= a.w || y >= a.h) return;
    float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
    float totw = 0.f;
    const int n_pass = (MODE == 2) ? a.n_layers : 1;
    for (int pass = 0; pass < n_pass; ++pass) {
        float4 ctr;
        if (MODE != 0) ctr = fetch_texture<MID_FMT_RGBA8>(a.layers[pass], a.w, a.h, x, y);
        else ctr = LINEAR ? fetch_linear<FMT>(a.in, a.w, a.h, x, y) : fetch_texture<FMT>(a.in, a.w, a.h, x, y);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        float accw = 0.f;
        for (int j = -R; j <= R; ++j)
            for (int i = -R; i <= R; ++i) {
                float4 g, c;
                if (MODE != 0) {
                    g = fetch_texture<MID_FMT_RGBA8>(a.layers[pass], a.w, a.h, x + i, y + j);
                    c = fetch_texture<FMT>(a.in, a.w, a.h, x + i, y + j);
                } else {
                    g = LINEAR ? fetch_linear<FMT>(a.in, a.w, a.h, x + i, y + j) : fetch_texture<FMT>(a.in, a.w, a.h, x + i, y + j);
                    c = g;
                }
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
    const size_t idx = (size_t)y * a.w + x;
    if (MODE == 1) {
        float4 *wp = (float4 *)(a.W + idx);
        float4 wc = wp[0], nw = wp[1];
        wc.x += tot.x; wc.y += tot.y; wc.z += tot.z; wc.w += tot.w;
        nw.x += totw;
        wp[0] = wc; wp[1] = nw;
    } else {
        float4 o;
        if (MODE == 2 && totw == 0.0f) o = make_float4(1.f, 0.f, 1.f, 1.f);
        else o = make_float4(tot.x / totw, tot.y / totw, tot.z / totw, tot.w / totw);
        store_out(a.out, idx, a.out_fmt, o);
    }
}

template <int R, int P, int NW, int FMT, bool LINEAR, int MODE, typename BT>
static int launch_tiled(mid_ctx *ctx, BilArgs &a, const BT &bt, int n_frames, hipStream_t s)
{
    constexpr size_t lds_bytes = bil_lds_bytes(R, NW * P, MODE != 0);
    auto kern = bilateral_kernel<R, P, NW, FMT, LINEAR, MODE, BT>;
    if ((int)lds_bytes > ctx->lds_max)
        return set_error(MID_ERR_UNSUPPORTED, "bilateral tile needs %zu B of LDS, device offers %d", lds_bytes, ctx->lds_max);
    if (int rc = ensure_lds(ctx, (const void *)kern, lds_bytes)) return rc;
    a.tiles_x = (int)cdiv(a.w, 64);
    a.tiles_y = (int)cdiv(a.h, NW * P);
    hipLaunchKernelGGL(kern, dim3((unsigned)a.tiles_x * a.tiles_y * (unsigned)n_frames), dim3(NW * 64), lds_bytes, s, a, bt);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

// n_frames > 1 only with BT = BilBatch (plain bilateral, MODE 0): grid = tiles x frames.
template <int FMT, bool LINEAR, int MODE, typename BT = BilOne>
static int dispatch_radius(mid_ctx *ctx, int radius, BilArgs &a, hipStream_t s, const BT &bt = BT{}, int n_frames = 1)
{
    return bil_for_radius(radius,
        [&](auto sh) { return launch_tiled<decltype(sh)::R, decltype(sh)::P, decltype(sh)::NW, FMT, LINEAR, MODE, BT>(ctx, a, bt, n_frames, s); },
        [&]() -> int {
            const size_t lds_bytes = bil_lds_bytes(radius, kBilRtNW * kBilRtP, MODE != 0);
            if ((int)lds_bytes <= ctx->lds_max) {    // run-time radius, LDS tiled
                auto kern = bilateral_rt_kernel<FMT, LINEAR, MODE, BT>;
                if (int rc = ensure_lds(ctx, (const void *)kern, (size_t)ctx->lds_max)) return rc;
                a.tiles_x = (int)cdiv(a.w, 64);
                a.tiles_y = (int)cdiv(a.h, kBilRtNW * kBilRtP);
                hipLaunchKernelGGL(kern, dim3((unsigned)a.tiles_x * a.tiles_y * (unsigned)n_frames), dim3(kBilRtNW * 64), lds_bytes, s, a, radius, bt);
                MID_HIP(hipGetLastError());
                return MID_OK;
            }
            // (unreachable for the plain bilateral: its single tile fits LDS for every legal radius; only the two-tile
            // layer modes at r > 17 get here, and those are never batched)
            if (n_frames != 1) return set_error(MID_ERR_UNSUPPORTED, "bilateral: no batched kernel for radius %d", radius);
            dim3 grid(cdiv(a.w, 16), cdiv(a.h, 16));
            hipLaunchKernelGGL((bilateral_generic_kernel<FMT, LINEAR, MODE>), grid, dim3(256), 0, s, a, radius);
            MID_HIP(hipGetLastError());
            return MID_OK;
        });
}

static int check_params(const mid_bilateral_params *p, const char *who, bool guide_ok = false)
{
    MID_REQUIRE(p != nullptr, "%s: params is NULL", who);
    MID_REQUIRE(p->width > 0 && p->height > 0, "%s: bad size %dx%d", who, p->width, p->height);
    MID_REQUIRE((long)p->width * p->height < (1l << 30), "%s: image too large", who);
    MID_REQUIRE(p->spatialSigma > 0.f && p->colorSigma > 0.f, "%s: sigmas must be > 0", who);
    MID_REQUIRE(p->radius >= 1 && p->radius <= 24, "%s: radius %d outside 1..24", who, p->radius);
    // the format word: the frames' format in bits 0..7, the guide layers' in bits 8..15 (MID_FMT_WITH_GUIDE), nothing above
    MID_REQUIRE((p->format & ~0xffff) == 0 && fmt_known(fmt_frames(p->format)), "%s: unknown format %d", who, p->format);
    if ((p->format >> 8) != 0) {
        MID_REQUIRE(guide_ok, "%s: format 0x%x names a guide-layer format, and this call reads no guide layers of the bilateral family", who, p->format);
        MID_REQUIRE(fmt_guide(p->format) >= 0, "%s: unknown guide-layer format code %d in format 0x%x", who, p->format >> 8, p->format);
    }
    MID_REQUIRE(p->layout == MID_LAYOUT_TEXTURE || p->layout == MID_LAYOUT_LINEAR, "%s: unknown layout %d", who, p->layout);
    return MID_OK;
}

int bilateral_check_params(const mid_bilateral_params *p, const char *who, bool guide_ok) { return check_params(p, who, guide_ok); }

// The input's texel format as a template argument: one switch for every entry point (the guide layers of these kernels are
// always RGBA8: RGBA16F / RGBA32F guides run on bilateral_temporal.hip's kernels, see bilateral_out).
template <bool LINEAR, int MODE, typename BT = BilOne>
static int dispatch_format(mid_ctx *ctx, int format, int radius, BilArgs &a, hipStream_t s, const BT &bt = BT{}, int n_frames = 1)
{
    if (format == MID_FMT_RGBA8) return dispatch_radius<MID_FMT_RGBA8, LINEAR, MODE, BT>(ctx, radius, a, s, bt, n_frames);
    if (format == MID_FMT_RGBA16F) return dispatch_radius<MID_FMT_RGBA16F, LINEAR, MODE, BT>(ctx, radius, a, s, bt, n_frames);
    return dispatch_radius<MID_FMT_RGBA32F, LINEAR, MODE, BT>(ctx, radius, a, s, bt, n_frames);
}

int bilateral_out(mid_ctx *ctx, const mid_bilateral_params *p, const void *in, const uint32_t *const *layers, int n_layers,
                  void *out, int out_fmt, hipStream_t s)
{
    BilArgs a{};
    bil_fill_scales(p, a);
    a.in = in; a.out = out; a.out_fmt = out_fmt;
    if (layers && fmt_guide(p->format) != MID_FMT_RGBA8)     // the k = 0 window of one frame: the identity DESIGN 3.7 pins bit for bit
        return bilateral_temporal_out(ctx, p, &in, layers, n_layers, 1, 0, 0, 1, &out, out_fmt, s);
    if (!layers) {
        if (p->layout == MID_LAYOUT_LINEAR) return dispatch_format<true, 0>(ctx, p->format, p->radius, a, s);
        return dispatch_format<false, 0>(ctx, p->format, p->radius, a, s);
    }
    a.n_layers = n_layers;
    for (int i = 0; i < n_layers; ++i) a.layers[i] = layers[i];
    return dispatch_format<false, 2>(ctx, fmt_frames(p->format), p->radius, a, s);
}

}  // namespace mid

using namespace mid;

extern "C" int mid_bilateral(mid_ctx *ctx, const mid_bilateral_params *p, const void *in,
                             mid_pixel *out, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    if (int rc = check_params(p, "bilateral")) return rc;
    MID_REQUIRE(in && out, "bilateral: NULL image pointer");
    MID_REQUIRE((const void *)in != (const void *)out, "bilateral: in-place filtering is not supported");
    MID_REQUIRE(fmt_aligned(p->format, in), "bilateral: RGBA16F input must be 8-byte aligned");
    return bilateral_out(ctx, p, in, nullptr, 0, out, MID_FMT_RGBA32F, b.s);
}

extern "C" int mid_bilateral_layers_accum(mid_ctx *ctx, const mid_bilateral_params *p, const void *in,
                                          const uint32_t *layer, mid_weightinfo *W, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    if (int rc = check_params(p, "bilateral_layers_accum", true)) return rc;
    MID_REQUIRE(in && layer && W, "bilateral_layers_accum: NULL pointer");
    MID_REQUIRE(fmt_aligned(fmt_frames(p->format), in), "bilateral_layers_accum: RGBA16F input must be 8-byte aligned");
    MID_REQUIRE(guide_aligned(fmt_guide(p->format), layer), "bilateral_layers_accum: an RGBA16F guide layer must be 8-byte aligned, an RGBA32F one 16-byte aligned");
    // NLM/layers are only ever bound to textures in the reference (src/main.cpp:1406-1428).
    MID_REQUIRE(p->layout == MID_LAYOUT_TEXTURE, "bilateral_layers_accum: layers exist for the texture layout only");
    if (fmt_guide(p->format) != MID_FMT_RGBA8)              // the pair dispatch with target guide == neighbour guide: the same bits
        return bilateral_layers_pair_out(ctx, p, layer, layer, in, W, b.s);
    BilArgs a{};
    bil_fill_scales(p, a);
    a.in = in; a.W = W; a.n_layers = 1; a.layers[0] = layer;
    return dispatch_format<false, 1>(ctx, fmt_frames(p->format), p->radius, a, b.s);
}

extern "C" int mid_bilateral_layers(mid_ctx *ctx, const mid_bilateral_params *p, const void *in,
                                    const uint32_t *const *layers, int n_layers, mid_pixel *out, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    if (int rc = check_params(p, "bilateral_layers", true)) return rc;
    MID_REQUIRE(in && layers && out, "bilateral_layers: NULL pointer");
    MID_REQUIRE(fmt_aligned(fmt_frames(p->format), in), "bilateral_layers: RGBA16F input must be 8-byte aligned");
    MID_REQUIRE((const void *)out != in, "bilateral_layers: out is the input image (in-place filtering is not supported)");
    MID_REQUIRE(p->layout == MID_LAYOUT_TEXTURE, "bilateral_layers: layers exist for the texture layout only");
    MID_REQUIRE(n_layers >= 0 && n_layers <= kMaxLayers, "bilateral_layers: n_layers %d outside 0..16", n_layers);
    for (int i = 0; i < n_layers; ++i) MID_REQUIRE(layers[i] != nullptr, "bilateral_layers: layer %d is NULL", i);
    for (int i = 0; i < n_layers; ++i)
        MID_REQUIRE(guide_aligned(fmt_guide(p->format), layers[i]), "bilateral_layers: layer %d is not aligned for its format (RGBA16F: 8 bytes, RGBA32F: 16)", i);
    return bilateral_out(ctx, p, in, layers, n_layers, out, MID_FMT_RGBA32F, b.s);
}

extern "C" int mid_bilateral_batch(mid_ctx *ctx, const mid_bilateral_params *p, const void *const *in,
                                   mid_pixel *const *out, int n_frames, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    if (int rc = check_params(p, "bilateral_batch")) return rc;
    MID_REQUIRE(in && out, "bilateral_batch: NULL table");
    MID_REQUIRE(n_frames >= 1, "bilateral_batch: n_frames %d < 1", n_frames);
    for (int i = 0; i < n_frames; ++i) MID_REQUIRE(in[i] && out[i], "bilateral_batch: frame %d is NULL", i);
    for (int i = 0; i < n_frames; ++i) MID_REQUIRE(fmt_aligned(p->format, in[i]), "bilateral_batch: RGBA16F frame %d is not 8-byte aligned", i);
    // All frames of a launch run concurrently: an output that is ANY frame's input (not only its own) would be written while
    // other workgroups still read it -- ping-pong tables shifted by one slot, say.
    if (int rc = check_no_alias("bilateral_batch", "an input frame of this call", in, n_frames, (const void *const *)out, n_frames)) return rc;
    const bool lin = p->layout == MID_LAYOUT_LINEAR;
    for (int c0 = 0; c0 < n_frames; c0 += kMaxFrames) {          // one launch per kMaxFrames frames
        const int cn = n_frames - c0 < kMaxFrames ? n_frames - c0 : kMaxFrames;
        BilArgs a{};
        bil_fill_scales(p, a);
        BilBatch bt{};
        for (int i = 0; i < cn; ++i) { bt.in.p[i] = in[c0 + i]; bt.out.p[i] = out[c0 + i]; }
        int rc;
        if (lin) rc = dispatch_format<true, 0, BilBatch>(ctx, p->format, p->radius, a, b.s, bt, cn);
        else rc = dispatch_format<false, 0, BilBatch>(ctx, p->format, p->radius, a, b.s, bt, cn);
        if (rc) return rc;
    }
    return MID_OK;
}
