// bilateral_joint.hip -- the joint (cross) bilateral filter: ONE weight per tap from all guide layers, each with its own sigma.
//
// Output t, pixel p, neighbours f = max(0,t-k) .. min(n-1,t+k), taps o = (i, j), |i|, |j| <= radius, layers l = 0 .. L-1:
//     w(p, f, o) = exp(-.5 |o|^2 / ss^2) * prod_l exp(-.5 |G[t][l](p) - G[f][l](p+o)|^2_rgb / sigma_l^2)
//     out_t(p)   = sum_{f,o} w * In_f(p+o) / sum_{f,o} w                  (magenta where the denominator is 0)
// Where mid_bilateral_temporal's layered form runs one complete filter per layer and adds them (L exps per tap, one sigma), this
// one multiplies the range terms: the exponent of a tap is ONE chain of FMAs -- spatial term, then layer 0's x, y, z, then layer
// 1's, ... -- and one v_exp_f32 follows.  Each layer is pre-multiplied by its own sc_l = sqrt(.5 log2 e) / sigma_l when it enters
// LDS (and the target centre by the same multiply), so a layer costs three subtracts and three FMAs per tap and no sigma
// appears in the tap loop.
//
// The tiled kernels are bilateral_pair_kernel / bilateral_pair_rt_kernel (bilateral_temporal.hip) with all L neighbour guide
// tiles resident beside the colour tile: same tile shapes (bilateral_shapes.hpp), same spatial term per class, same paired-row
// exp bursts, priority phases and opaque-tile vote, per neighbour `acc` and then tot += acc.  With L = 1 the chain is the layered
// kernel's chain: the bits of mid_bilateral_temporal with that layer.
//   * Guide tiles hold what the arithmetic reads, three floats per texel, as three planes of floats per layer (x, y, z; alpha is
//     never read): 12 B per texel against a float4's 16 is what lets four layers sit beside the colour tile of radius 8 in
//     exactly 160 KB, and consecutive lanes read consecutive words of a plane (no bank conflicts, ds_read_b32).
//   * The guide format is decoded when a tile is filled (a wave-uniform branch per fill): every format ends as the fp32 value
//     times sc_l in the same planes, so it is no template axis.
//     The colour tile and layer 0 are filled in one trip loop (their loads in flight together), further layers one by one.
//   * The layer count is a kernel argument.  The target centres of all layers live in registers across the tap loop, and a
//     register array indexed by a run-time layer number would go to scratch, so the tap loop exists once per layer count
//     1 .. kJointTiledLayers inside the one kernel and a wave-uniform switch picks it: no scratch, no branch inside the loop.
// What does not fit LDS, and every L > kJointTiledLayers, runs one thread per pixel with bilateral_pair_generic_kernel's
// arithmetic: arg = ks*(i^2+j^2), then arg = fmaf(d2_l, kc_l, arg) per layer.  With one layer the class is the one the layered
// form of mid_bilateral_temporal runs at that radius (joint_tiled): a radius runs the same arithmetic in every form.
#include "bilateral_shapes.hpp"

namespace mid {

namespace {

constexpr int kMaxPtrs = MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS;
constexpr int kJointTiledLayers = 4;    // layers the tiled kernels keep resident (radius 8: 40 KB + 4 * 30 KB = 160 KB)

struct BilJointArgs {
    int w, h;
    float ks, kc;                       // spatial exponent scale (log2 domain); kc, sc, inv_sc: of p->colorSigma, unused
    float sc, inv_sc;
    int tiles_x, tiles_y;
    int fmt, gfmt;                      // MID_FMT_* of the frames / of the guide layers
    int n_nb;                           // neighbours of this output: window slots [0, n_nb)
    int n_layers;
    int t_slot;                         // the window slot that is the output frame itself
    int out_fmt;
    void *out;
    float scl[kMaxLayers];              // per layer: sqrt(.5 log2 e) / sigma_l, what a guide value is multiplied by (tiled kernels)
    float kcl[kMaxLayers];              // per layer: -.5 log2 e / sigma_l^2 (per-pixel kernel)
    const void *p[kMaxPtrs];            // slot j: p[j * (n_layers + 1)] = frame, then its n_layers guide layers
};

// bytes of LDS of one workgroup: the colour tile (float4) and L guide tiles of three floats per texel
constexpr size_t joint_lds_bytes(int radius, int tile_h, int n_layers)
{
    return (size_t)(64 + 2 * radius) * (tile_h + 2 * radius) * (sizeof(float4) + 3 * sizeof(float) * (size_t)n_layers);
}
// Tiled or per pixel.  One layer: the LDS test of the layered form (two float4 tiles), so that L = 1 runs in the class that
// mid_bilateral_temporal's layered form runs in -- this kernel's own tiles are smaller than those.
inline bool joint_tiled(int lds_max, int radius, int tile_h, int n_layers)
{
    if (n_layers > kJointTiledLayers) return false;
    if (n_layers == 1) return (int)bil_lds_bytes(radius, tile_h, true) <= lds_max;
    return (int)joint_lds_bytes(radius, tile_h, n_layers) <= lds_max;
}

__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nwg)
{
    const unsigned q = nwg >> 3, r = nwg & 7u, x = bid & 7u, i = bid >> 3;
    return x * q + (x < r ? x : r) + i;
}

__device__ __forceinline__ const void *nb_frame(const BilJointArgs &a, int j) { return a.p[j * (a.n_layers + 1)]; }
__device__ __forceinline__ const void *nb_layer(const BilJointArgs &a, int j, int l) { return a.p[j * (a.n_layers + 1) + 1 + l]; }

// One texel with the format as a run-time (wave-uniform) value.
__device__ __forceinline__ float4 fetch_any(const void *img, int fmt, int w, int h, int x, int y)
{
    if (fmt == MID_FMT_RGBA8) return fetch_texture<MID_FMT_RGBA8>(img, w, h, x, y);
    if (fmt == MID_FMT_RGBA16F) return fetch_texture<MID_FMT_RGBA16F>(img, w, h, x, y);
    return fetch_texture<MID_FMT_RGBA32F>(img, w, h, x, y);
}

// Cooperative fill of one layer's three planes (x at g, y at g + n, z at g + 2n; n = tw * th), each value times sc: fill_tile's
// trip -- four texels per thread in flight -- and fill_tile's multiply, so a plane value has the bits of a float4 tile's.
template <int GF>
__device__ __forceinline__ void fill_planes(float *g, int tw, int th, const void *layer, int w, int h, int x0, int y0, int tid,
                                            int nthreads, float sc)
{
    const int n = tw * th;
    for (int t0 = tid; t0 < n; t0 += 4 * nthreads) {
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + j * nthreads;
            const int ty = t / tw, tx = t - ty * tw;
            v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < n) v[j] = fetch_texture<GF>(layer, w, h, x0 + tx, y0 + ty);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + j * nthreads;
            if (t < n) { g[t] = v[j].x * sc; g[n + t] = v[j].y * sc; g[2 * n + t] = v[j].z * sc; }
        }
    }
}
__device__ __forceinline__ void fill_planes_any(float *g, int tw, int th, const void *layer, int gfmt, int w, int h, int x0, int y0,
                                                int tid, int nthreads, float sc)
{
    if (gfmt == MID_FMT_RGBA8) fill_planes<MID_FMT_RGBA8>(g, tw, th, layer, w, h, x0, y0, tid, nthreads, sc);
    else if (gfmt == MID_FMT_RGBA16F) fill_planes<MID_FMT_RGBA16F>(g, tw, th, layer, w, h, x0, y0, tid, nthreads, sc);
    else fill_planes<MID_FMT_RGBA32F>(g, tw, th, layer, w, h, x0, y0, tid, nthreads, sc);
}

// The colour tile and layer 0's planes in ONE trip loop: the eight global loads of a trip -- four colour texels, four guide
// texels -- are in flight together, so a neighbour with one layer costs the memory latencies of one tile, not of two.  Same
// texels, same decode, same multiply as fill_tile / fill_planes: the same bits.  `held` (optional): the x value of guide texel 0
// is handed back instead of stored, so that g[0] stays free for the opaque-tile vote; the caller stores it afterwards.
template <int FF, int GF>
__device__ __forceinline__ void fill_colour_and_planes(float4 *img, float *g, int tw, int th, const void *frame, const void *layer, int w,
                                                       int h, int x0, int y0, int tid, int nthreads, float sc, bool *opaque, float *held)
{
    const int n = tw * th;
    for (int t0 = tid; t0 < n; t0 += 4 * nthreads) {
        float4 c[4], v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + j * nthreads;
            const int ty = t / tw, tx = t - ty * tw;
            c[j] = v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < n) {
                c[j] = fetch_texture<FF>(frame, w, h, x0 + tx, y0 + ty);
                v[j] = fetch_texture<GF>(layer, w, h, x0 + tx, y0 + ty);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + j * nthreads;
            if (t < n) {
                img[t] = c[j];
                if (held && t == 0) *held = v[j].x * sc; else g[t] = v[j].x * sc;
                g[n + t] = v[j].y * sc; g[2 * n + t] = v[j].z * sc;
            }
            if (opaque && t < n) *opaque = *opaque && c[j].w == 1.0f;
        }
    }
}
template <int FF>
__device__ __forceinline__ void fill_colour_and_planes_g(float4 *img, float *g, int tw, int th, const void *frame, const void *layer,
                                                         int gfmt, int w, int h, int x0, int y0, int tid, int nthreads, float sc,
                                                         bool *opaque, float *held)
{
    if (gfmt == MID_FMT_RGBA8) fill_colour_and_planes<FF, MID_FMT_RGBA8>(img, g, tw, th, frame, layer, w, h, x0, y0, tid, nthreads, sc, opaque, held);
    else if (gfmt == MID_FMT_RGBA16F) fill_colour_and_planes<FF, MID_FMT_RGBA16F>(img, g, tw, th, frame, layer, w, h, x0, y0, tid, nthreads, sc, opaque, held);
    else fill_colour_and_planes<FF, MID_FMT_RGBA32F>(img, g, tw, th, frame, layer, w, h, x0, y0, tid, nthreads, sc, opaque, held);
}
__device__ __forceinline__ void fill_colour_and_planes_any(float4 *img, float *g, int tw, int th, const void *frame, int fmt,
                                                           const void *layer, int gfmt, int w, int h, int x0, int y0, int tid,
                                                           int nthreads, float sc, bool *opaque, float *held)
{
    if (fmt == MID_FMT_RGBA8) fill_colour_and_planes_g<MID_FMT_RGBA8>(img, g, tw, th, frame, layer, gfmt, w, h, x0, y0, tid, nthreads, sc, opaque, held);
    else if (fmt == MID_FMT_RGBA16F) fill_colour_and_planes_g<MID_FMT_RGBA16F>(img, g, tw, th, frame, layer, gfmt, w, h, x0, y0, tid, nthreads, sc, opaque, held);
    else fill_colour_and_planes_g<MID_FMT_RGBA32F>(img, g, tw, th, frame, layer, gfmt, w, h, x0, y0, tid, nthreads, sc, opaque, held);
}

// normalize.comp and the pack of the output format
__device__ __forceinline__ void put(const BilJointArgs &a, size_t idx, float4 tot, float totw)
{
    float4 o;
    if (totw == 0.0f) o = make_float4(1.f, 0.f, 1.f, 1.f);
    else o = make_float4(tot.x / totw, tot.y / totw, tot.z / totw, tot.w / totw);
    store_out(a.out, idx, a.out_fmt, o);
}

template <int N> struct LayerCount { static constexpr int value = N; };

// Tuned radii (bilateral_shapes.hpp): bilateral_pair_kernel's tile and tap loop, the exponent chain running through MAXL >= L
// resident layers.  MAXL: the largest layer count whose tiles fit 160 KB at this shape (more tap loops would never run).
template <int R, int P, int NW, int MAXL>
__global__ __launch_bounds__(NW * 64) void bilateral_joint_kernel(const BilJointArgs a)
{
    constexpr int TILE_W = 64, TILE_H = NW * P;
    constexpr int LW = TILE_W + 2 * R, LH = TILE_H + 2 * R, N = LW * LH;
    constexpr int MR = P + 2 * R;   // tile rows a lane walks per column offset

    extern __shared__ float4 lds[];
    float4 *img_t = lds;                                  // colour source: the neighbour frame
    float *gde_t = (float *)(lds + N);                    // layer l: planes x, y, z at gde_t + (3 l + {0, 1, 2}) * N

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned flat = xcd_remap(blockIdx.x, gridDim.x);
    const int ty = (int)(flat / (unsigned)a.tiles_x), tx = (int)(flat - (unsigned)ty * a.tiles_x);
    const int w = a.w, h = a.h;
    const int X0 = tx * TILE_W, Y0 = ty * TILE_H;
    const int gx = X0 + lane, yb = Y0 + wv * P;
    const bool wave_active = yb < h;
    const int L = a.n_layers;                             // 1 .. MAXL (the dispatcher's promise)

    // spatial exponent by |j|: ks * j^2 (wave-uniform)
    float sj[R + 1];
#pragma unroll
    for (int j = 0; j <= R; ++j) sj[j] = a.ks * (float)(j * j);

    // Gt(p) of every layer, from global memory, scaled as a tile texel is (fill_planes: value * sc_l): the centres do not
    // change with the neighbour
    float cr[MAXL][P], cg[MAXL][P], cb[MAXL][P];
#pragma unroll
    for (int l = 0; l < MAXL; ++l)
#pragma unroll
        for (int k = 0; k < P; ++k) {
            cr[l][k] = cg[l][k] = cb[l][k] = 0.f;
            if (l < L && wave_active) {
                const float4 c = fetch_any(a.p[a.t_slot * (L + 1) + 1 + l], a.gfmt, w, h, gx, yb + k);
                const float sc = a.scl[l];
                cr[l][k] = c.x * sc; cg[l][k] = c.y * sc; cb[l][k] = c.z * sc;
            }
        }

    float4 tot[P];
    float totw[P];
#pragma unroll
    for (int k = 0; k < P; ++k) { tot[k] = make_float4(0.f, 0.f, 0.f, 0.f); totw[k] = 0.f; }

    for (int f = 0; f < a.n_nb; ++f) {
        __syncthreads();                                   // every wave has left the previous neighbour's tap loop
        bool mine = true;                                  // every texel THIS thread stored in the colour tile has alpha == 1.0f
        float held = 0.f;                                  // thread 0: the x value of layer 0's texel 0, whose word carries the vote
        fill_colour_and_planes_any(img_t, gde_t, LW, LH, nb_frame(a, f), a.fmt, nb_layer(a, f, 0), a.gfmt, w, h, X0 - R, Y0 - R, tid, NW * 64,
                                   a.scl[0], &mine, &held);
        for (int l = 1; l < L; ++l)
            fill_planes_any(gde_t + (size_t)3 * l * N, LW, LH, nb_layer(a, f, l), a.gfmt, w, h, X0 - R, Y0 - R, tid, NW * 64, a.scl[l]);
        // The opaque form of the tap loop is decided from the content of this neighbour's colour tile, voted in the first word
        // of the guide tiles, which the fill left free; thread 0 stores that word's texel once every thread has read the vote.
        unsigned *vote = (unsigned *)gde_t;
        if (tid == 0) vote[0] = 1u;
        __syncthreads();
        if (!mine) vote[0] = 0u;
        __syncthreads();
        const bool alpha_one = __builtin_amdgcn_readfirstlane((int)vote[0]) != 0;
        __syncthreads();
        if (tid == 0) gde_t[0] = held;
        __syncthreads();
        if (!wave_active) continue;

        float4 acc[P];
        float accw[P];
#pragma unroll
        for (int k = 0; k < P; ++k) { acc[k] = make_float4(0.f, 0.f, 0.f, 0.f); accw[k] = 0.f; }

        auto taps = [&](auto a1_tag, auto nl_tag) {
        constexpr bool A1 = decltype(a1_tag)::value;
        constexpr int NL = decltype(nl_tag)::value;
        if constexpr (NL <= MAXL) {
        for (int i = -R; i <= R; ++i) {
            const float si = a.ks * (float)(i * i);
            float sij[R + 1];
#pragma unroll
            for (int j = 0; j <= R; ++j) sij[j] = si + sj[j];
            const int base = (wv * P) * LW + lane + R + i;
            // rows in groups of two: exponent arguments, then all v_exp_f32 of the group in one burst at raised issue
            // priority, then the accumulates -- bilateral_pair_kernel's phases
            constexpr int RG = 2;
#pragma unroll
            for (int m0 = 0; m0 < MR; m0 += RG) {
                float4 cc[RG];
                float ar[RG][P];
#pragma unroll
                for (int r = 0; r < RG; ++r) {
                    const int m = m0 + r;
                    if (m >= MR) continue;
                    cc[r] = img_t[base + m * LW];
#pragma unroll
                    for (int k = 0; k < P; ++k) {
                        const int j = m - R - k;
                        if (j < -R || j > R) continue;
                        ar[r][k] = sij[j < 0 ? -j : j];
                    }
#pragma unroll
                    for (int l = 0; l < NL; ++l) {
                        const float *gp = gde_t + 3 * l * N + base + m * LW;
                        const float g_x = gp[0], g_y = gp[N], g_z = gp[2 * N];
#pragma unroll
                        for (int k = 0; k < P; ++k) {
                            const int j = m - R - k;
                            if (j < -R || j > R) continue;
                            const float dx = cr[l][k] - g_x, dy = cg[l][k] - g_y, dz = cb[l][k] - g_z;
                            ar[r][k] = fmaf(-dz, dz, fmaf(-dy, dy, fmaf(-dx, dx, ar[r][k])));
                        }
                    }
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
        }
        };
        auto taps_of = [&](auto a1_tag) {
            switch (L) {
            case 1: taps(a1_tag, LayerCount<1>{}); break;
            case 2: taps(a1_tag, LayerCount<2>{}); break;
            case 3: taps(a1_tag, LayerCount<3>{}); break;
            default: taps(a1_tag, LayerCount<4>{}); break;
            }
        };
        static_assert(MAXL <= 4 && kJointTiledLayers == 4, "one tap loop per layer count");
        if (alpha_one) taps_of(std::true_type{}); else taps_of(std::false_type{});
#pragma unroll
        for (int k = 0; k < P; ++k) {
            tot[k].x += acc[k].x; tot[k].y += acc[k].y; tot[k].z += acc[k].z; tot[k].w += acc[k].w;
            totw[k] += accw[k];
        }
    }

    if (!wave_active || gx >= w) return;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int gy = yb + k;
        if (gy >= h) break;
        put(a, (size_t)gy * w + gx, tot[k], totw[k]);
    }
}

// Any other radius whose tiles fit LDS: bilateral_pair_rt_kernel's run-time-radius scheme (8 waves x 2 rows, taps in row pairs,
// spatial term fma(ks, j^2, si)) with the layers resident.
__global__ __launch_bounds__(512) void bilateral_joint_rt_kernel(const BilJointArgs a, const int R)
{
    constexpr int NW = 8, P = 2, TILE_W = 64, TILE_H = NW * P, MAXL = kJointTiledLayers;
    const int LW = TILE_W + 2 * R, LH = TILE_H + 2 * R, N = LW * LH;
    extern __shared__ float4 lds[];
    float4 *img_t = lds;
    float *gde_t = (float *)(lds + N);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned flat = xcd_remap(blockIdx.x, gridDim.x);
    const int ty = (int)(flat / (unsigned)a.tiles_x), tx = (int)(flat - (unsigned)ty * a.tiles_x);
    const int w = a.w, h = a.h;
    const int X0 = tx * TILE_W, Y0 = ty * TILE_H;
    const int gx = X0 + lane, yb = Y0 + wv * P;
    const bool wave_active = yb < h;
    const int L = a.n_layers;

    float cr[MAXL][P], cg[MAXL][P], cb[MAXL][P];
#pragma unroll
    for (int l = 0; l < MAXL; ++l)
#pragma unroll
        for (int k = 0; k < P; ++k) {
            cr[l][k] = cg[l][k] = cb[l][k] = 0.f;
            if (l < L && wave_active) {
                const float4 c = fetch_any(a.p[a.t_slot * (L + 1) + 1 + l], a.gfmt, w, h, gx, yb + k);
                const float sc = a.scl[l];
                cr[l][k] = c.x * sc; cg[l][k] = c.y * sc; cb[l][k] = c.z * sc;
            }
        }

    float4 tot[P];
    float totw[P];
#pragma unroll
    for (int k = 0; k < P; ++k) { tot[k] = make_float4(0.f, 0.f, 0.f, 0.f); totw[k] = 0.f; }
    for (int f = 0; f < a.n_nb; ++f) {
        __syncthreads();                                   // the previous neighbour's readers are done with the tiles
        fill_colour_and_planes_any(img_t, gde_t, LW, LH, nb_frame(a, f), a.fmt, nb_layer(a, f, 0), a.gfmt, w, h, X0 - R, Y0 - R, tid, NW * 64,
                                   a.scl[0], nullptr, nullptr);
        for (int l = 1; l < L; ++l)
            fill_planes_any(gde_t + (size_t)3 * l * N, LW, LH, nb_layer(a, f, l), a.gfmt, w, h, X0 - R, Y0 - R, tid, NW * 64, a.scl[l]);
        __syncthreads();
        if (!wave_active) continue;
        float4 acc[P];
        float accw[P];
#pragma unroll
        for (int k = 0; k < P; ++k) { acc[k] = make_float4(0.f, 0.f, 0.f, 0.f); accw[k] = 0.f; }
        auto taps = [&](auto nl_tag) {
        constexpr int NL = decltype(nl_tag)::value;
        for (int i = -R; i <= R; ++i) {
            const float si = a.ks * (float)(i * i);
            const int base = (wv * P) * LW + lane + R + i;
            // tile row m feeds output k = 0 with j = m - R and output k = 1 with j = m - R - 1: first and last row alone, the
            // 2R rows between them in pairs with their four exps as one burst (bilateral_pair_rt_kernel)
            auto arg_of = [&](int t, int k, int j) {
                float arg = fmaf(a.ks, (float)(j * j), si);
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    const float *gp = gde_t + 3 * l * N + t;
                    const float dx = cr[l][k] - gp[0], dy = cg[l][k] - gp[N], dz = cb[l][k] - gp[2 * N];
                    arg = fmaf(-dz, dz, fmaf(-dy, dy, fmaf(-dx, dx, arg)));
                }
                return arg;
            };
            auto add_tap = [&](const float4 &c, int k, float wt) {
                acc[k].x = fmaf(c.x, wt, acc[k].x); acc[k].y = fmaf(c.y, wt, acc[k].y);
                acc[k].z = fmaf(c.z, wt, acc[k].z); acc[k].w = fmaf(c.w, wt, acc[k].w);
                accw[k] += wt;
            };
            add_tap(img_t[base], 0, exp2_hw(arg_of(base, 0, -R)));
            for (int m = 1; m < 2 * R; m += 2) {
                const int t0 = base + m * LW, t1 = t0 + LW;
                const float4 c0 = img_t[t0], c1 = img_t[t1];
                float w00 = arg_of(t0, 0, m - R), w01 = arg_of(t0, 1, m - R - 1), w10 = arg_of(t1, 0, m + 1 - R), w11 = arg_of(t1, 1, m - R);
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
                const int t = base + (2 * R + 1) * LW;
                add_tap(img_t[t], 1, exp2_hw(arg_of(t, 1, R)));
            }
        }
        };
        switch (L) {
        case 1: taps(LayerCount<1>{}); break;
        case 2: taps(LayerCount<2>{}); break;
        case 3: taps(LayerCount<3>{}); break;
        default: taps(LayerCount<4>{}); break;
        }
#pragma unroll
        for (int k = 0; k < P; ++k) {
            tot[k].x += acc[k].x; tot[k].y += acc[k].y; tot[k].z += acc[k].z; tot[k].w += acc[k].w;
            totw[k] += accw[k];
        }
    }
    if (!wave_active || gx >= w) return;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int gy = yb + k;
        if (gy >= h) break;
        put(a, (size_t)gy * w + gx, tot[k], totw[k]);
    }
}

// Everything else: one thread per pixel with global fetches, bilateral_pair_generic_kernel's arithmetic with the exponent
// carried through the layers.
template <int GF>
__global__ __launch_bounds__(256) void bilateral_joint_generic_kernel(const BilJointArgs a, int R)
{
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= a.w || y >= a.h) return;
    const int L = a.n_layers;
    float cr[kMaxLayers], cg[kMaxLayers], cb[kMaxLayers];      // Gt(p) of every layer (constant indices: registers)
#pragma unroll
    for (int l = 0; l < kMaxLayers; ++l) {
        cr[l] = cg[l] = cb[l] = 0.f;
        if (l < L) {
            const float4 c = fetch_texture<GF>(a.p[a.t_slot * (L + 1) + 1 + l], a.w, a.h, x, y);
            cr[l] = c.x; cg[l] = c.y; cb[l] = c.z;
        }
    }
    float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
    float totw = 0.f;
    for (int f = 0; f < a.n_nb; ++f) {
        const void *in = nb_frame(a, f);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        float accw = 0.f;
        for (int j = -R; j <= R; ++j)
            for (int i = -R; i <= R; ++i) {
                const float4 c = fetch_any(in, a.fmt, a.w, a.h, x + i, y + j);
                float arg = a.ks * (float)(i * i + j * j);
#pragma unroll
                for (int l = 0; l < kMaxLayers; ++l) {
                    if (l >= L) break;
                    const float4 g = fetch_texture<GF>(nb_layer(a, f, l), a.w, a.h, x + i, y + j);
                    const float dx = cr[l] - g.x, dy = cg[l] - g.y, dz = cb[l] - g.z;
                    const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                    arg = fmaf(d2, a.kcl[l], arg);
                }
                const float wt = exp2_hw(arg);
                acc.x = fmaf(c.x, wt, acc.x); acc.y = fmaf(c.y, wt, acc.y);
                acc.z = fmaf(c.z, wt, acc.z); acc.w = fmaf(c.w, wt, acc.w);
                accw += wt;
            }
        tot.x += acc.x; tot.y += acc.y; tot.z += acc.z; tot.w += acc.w;
        totw += accw;
    }
    put(a, (size_t)y * a.w + x, tot, totw);
}

int launch_generic(BilJointArgs &a, int radius, hipStream_t s)
{
    const dim3 grid(cdiv(a.w, 16), cdiv(a.h, 16));
    if (a.gfmt == MID_FMT_RGBA8) hipLaunchKernelGGL((bilateral_joint_generic_kernel<MID_FMT_RGBA8>), grid, dim3(256), 0, s, a, radius);
    else if (a.gfmt == MID_FMT_RGBA16F) hipLaunchKernelGGL((bilateral_joint_generic_kernel<MID_FMT_RGBA16F>), grid, dim3(256), 0, s, a, radius);
    else hipLaunchKernelGGL((bilateral_joint_generic_kernel<MID_FMT_RGBA32F>), grid, dim3(256), 0, s, a, radius);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

// layers a tuned shape can ever hold beside its colour tile in 160 KB: the tap loops the kernel is built with
template <int R, int P, int NW> constexpr int joint_max_layers()
{
    int l = 1;
    while (l < kJointTiledLayers && joint_lds_bytes(R, NW * P, l + 1) <= 160 * 1024) ++l;
    return l;
}

template <int R, int P, int NW>
int launch_joint_tiled(mid_ctx *ctx, BilJointArgs &a, hipStream_t s)
{
    constexpr int MAXL = joint_max_layers<R, P, NW>();
    if (a.n_layers > MAXL || !joint_tiled(ctx->lds_max, R, NW * P, a.n_layers)) return launch_generic(a, R, s);
    const size_t lds_bytes = joint_lds_bytes(R, NW * P, a.n_layers);
    auto kern = bilateral_joint_kernel<R, P, NW, MAXL>;
    if (int rc = ensure_lds(ctx, (const void *)kern, (size_t)ctx->lds_max)) return rc;
    a.tiles_x = (int)cdiv(a.w, 64);
    a.tiles_y = (int)cdiv(a.h, NW * P);
    hipLaunchKernelGGL(kern, dim3((unsigned)a.tiles_x * a.tiles_y), dim3(NW * 64), lds_bytes, s, a);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

int dispatch_joint(mid_ctx *ctx, int radius, BilJointArgs &a, hipStream_t s)
{
    return bil_for_radius(radius,
        [&](auto sh) { return launch_joint_tiled<decltype(sh)::R, decltype(sh)::P, decltype(sh)::NW>(ctx, a, s); },
        [&]() -> int {
            if (!joint_tiled(ctx->lds_max, radius, kBilRtNW * kBilRtP, a.n_layers)) return launch_generic(a, radius, s);
            const size_t lds_bytes = joint_lds_bytes(radius, kBilRtNW * kBilRtP, a.n_layers);
            auto kern = bilateral_joint_rt_kernel;
            if (int rc = ensure_lds(ctx, (const void *)kern, (size_t)ctx->lds_max)) return rc;
            a.tiles_x = (int)cdiv(a.w, 64);
            a.tiles_y = (int)cdiv(a.h, kBilRtNW * kBilRtP);
            hipLaunchKernelGGL(kern, dim3((unsigned)a.tiles_x * a.tiles_y), dim3(kBilRtNW * 64), lds_bytes, s, a, radius);
            MID_HIP(hipGetLastError());
            return MID_OK;
        });
}

}  // namespace

int bilateral_joint_check(const mid_bilateral_params *p, const char *who, const float *layer_sigma, bool have_layers, int n_layers,
                          int n_frames, int k)
{
    MID_REQUIRE(n_layers >= 1 && n_layers <= kMaxLayers, "%s: n_layers %d outside 1..16 (the product of no range terms is no joint filter)", who, n_layers);
    MID_REQUIRE(have_layers, "%s: the layer table is NULL", who);
    if (int rc = bilateral_temporal_check(p, who, true, n_layers, n_frames, k)) return rc;
    for (int l = 0; layer_sigma && l < n_layers; ++l)
        MID_REQUIRE(layer_sigma[l] > 0.f, "%s: sigmas must be > 0 (layer_sigma[%d] = %g)", who, l, (double)layer_sigma[l]);
    return MID_OK;
}

int bilateral_joint_out(mid_ctx *ctx, const mid_bilateral_params *p, const float *layer_sigma, const void *const *frames,
                        const uint32_t *const *layers, int n_layers, int n_frames, int k, int first, int count, void *const *out,
                        int out_fmt, hipStream_t s)
{
    for (int t = first; t < first + count; ++t) {
        BilJointArgs a{};
        bil_fill_scales(p, a);
        a.fmt = fmt_frames(p->format);
        a.gfmt = fmt_guide(p->format);
        for (int l = 0; l < n_layers; ++l) {
            const double sigma = layer_sigma ? (double)layer_sigma[l] : (double)p->colorSigma;
            a.scl[l] = (float)(sqrt(0.5 * 1.4426950408889634) / sigma);       // bil_fill_scales' sc
            a.kcl[l] = (float)(-0.5 * 1.4426950408889634 / (sigma * sigma));  // and kc
        }
        pack_temporal_window(a, frames, layers, n_layers, n_frames, k, t);
        a.out = out[t - first]; a.out_fmt = out_fmt;
        if (int rc = dispatch_joint(ctx, p->radius, a, s)) return rc;
    }
    return MID_OK;
}

}  // namespace mid

using namespace mid;

extern "C" int mid_bilateral_joint(mid_ctx *ctx, const mid_bilateral_params *p, const float *layer_sigma, const void *const *frames,
                                   const uint32_t *const *layers, int n_layers, int n_frames, int k, int first, int count,
                                   void *const *out, int out_format, void *stream)
{
    Bind b(ctx, stream);
    if (b.rc) return b.rc;
    MID_REQUIRE(frames && out, "bilateral_joint: NULL table");
    MID_REQUIRE(fmt_known(out_format), "bilateral_joint: unknown output format %d", out_format);
    if (int rc = bilateral_joint_check(p, "bilateral_joint", layer_sigma, layers != nullptr, n_layers, n_frames, k)) return rc;
    if (int rc = check_temporal_window("bilateral_joint", fmt_frames(p->format), frames, layers, n_layers, n_frames, k, first, count, out,
                                       out_format, fmt_guide(p->format))) return rc;
    return bilateral_joint_out(ctx, p, layer_sigma, frames, layers, n_layers, n_frames, k, first, count, out, out_format, b.s);
}
