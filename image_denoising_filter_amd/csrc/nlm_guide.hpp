// nlm_guide.hpp -- what the guide-driven NLM files (nlm_layers.hip, nlm_layers_temporal.hip, nlm_joint.hip) take from one place: the guide texel
// and tile helpers, the two epilogues, the geometry of a strip launch, and on the host side the exp2 scale, the table of tuned
// windows and the two launch functions.  The kernel bodies -- the offset loops with their rings -- are NOT shared: each file keeps
// its own text, for the reason in LABNOTES R10.1 (an inlined common body moves the register allocation).
#pragma once
#include "nlm_strip.hpp"

namespace mid {

constexpr int kMaxPtrs = MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS;

// ---- geometry ------------------------------------------------------------------------------------------------------------------
// A strip launch for the search range [SLO, SHI), the patch range [PLO, PHI): NW waves of R rows per workgroup, a wave owns 64
// columns of which VW carry finished patch sums.  LDS holds the colour tile (float4, centre positions only: no patch halo) and
// n guide tiles behind it (packed RGBA8, centres + patch halo), both with the search halo.
template <int SLO_, int SHI_, int PLO_, int PHI_, int R_, int NW_>
struct GuideTile {
    static constexpr int SLO = SLO_, SHI = SHI_, PLO = PLO_, PHI = PHI_, R = R_, NW = NW_;
    static_assert(PLO <= 0 && PHI >= 1 && SLO <= 0 && SHI >= 1, "ranges must contain 0");
    static constexpr int PW = PHI - PLO, DR = R + PW - 1, NL = -PLO, NR = PHI - 1, VW = 64 - (PW - 1), TILE_H = NW * R;
    static constexpr int SW = SHI - SLO, LW = 64 + SW - 1;
    static constexpr int LHC = TILE_H + SW - 1;             // colour tile rows: centres only
    static constexpr int LHG = TILE_H + PW - 1 + SW - 1;    // guide tile rows: centres + patch halo
    static_assert(SW <= kNlmWalk, "one run of search rows per search column");
    static constexpr size_t lds_bytes(int n_guide_tiles) { return (size_t)LW * LHC * sizeof(float4) + (size_t)n_guide_tiles * LW * LHG * 4; }
};

// The tuned windows, as a type: true and *rc = tuned(NlmWindow<...>{}) for a window of the list, false for every other one.
template <int SLO_, int SHI_, int PLO_, int PHI_> struct NlmWindow { static constexpr int SLO = SLO_, SHI = SHI_, PLO = PLO_, PHI = PHI_; };
template <typename Tuned>
inline bool nlm_guide_for_window(const mid_nlm_params *p, int *rc, Tuned &&tuned)
{
    if (p->search_lo == -10 && p->search_hi == 11 && p->patch_lo == -3 && p->patch_hi == 4) { *rc = tuned(NlmWindow<-10, 11, -3, 4>{}); return true; }   // 21x21 / 7x7 (benchmark)
    if (p->search_lo == -7 && p->search_hi == 7 && p->patch_lo == -3 && p->patch_hi == 3) { *rc = tuned(NlmWindow<-7, 7, -3, 3>{}); return true; }       // nonlocal.comp:5-6 as shipped
    return false;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// log2(e) / (255^2 h^2): the exp2 scale of a patch distance summed over byte values
inline float nlm_guide_kd(double h) { return (float)(1.4426950408889634 / (h * h * 255.0 * 255.0)); }

// The per-pixel kernel of the frames' format: kern(std::integral_constant<int, MID_FMT_*>{}) names the instantiation.
template <typename Kern, typename Args>
inline int launch_guide_per_pixel(Kern &&kern, const mid_nlm_params *p, const Args &a, hipStream_t s)
{
    const dim3 grid(cdiv(a.w, 16), cdiv(a.h, 16));
    auto go = [&](auto fmt) { hipLaunchKernelGGL(kern(fmt), grid, dim3(256), 0, s, a, p->search_lo, p->search_hi, p->patch_lo, p->patch_hi); };
    if (a.fmt == MID_FMT_RGBA8) go(std::integral_constant<int, MID_FMT_RGBA8>{});
    else if (a.fmt == MID_FMT_RGBA16F) go(std::integral_constant<int, MID_FMT_RGBA16F>{});
    else go(std::integral_constant<int, MID_FMT_RGBA32F>{});
    MID_HIP(hipGetLastError());
    return MID_OK;
}

// A strip kernel of geometry T with n_guide_tiles guide tiles; `who` names the caller in the message.
template <typename T, typename Args>
inline int launch_guide_strip(mid_ctx *ctx, const char *who, void (*kern)(const Args), int n_guide_tiles, Args &a, hipStream_t s)
{
    const size_t lds_bytes = T::lds_bytes(n_guide_tiles);
    if ((int)lds_bytes > ctx->lds_max)
        return set_error(MID_ERR_UNSUPPORTED, "%s tile needs %zu B of LDS, device offers %d", who, lds_bytes, ctx->lds_max);
    if (int rc = ensure_lds(ctx, (const void *)kern, lds_bytes)) return rc;
    a.tiles_x = (int)cdiv(a.w, T::VW);
    a.tiles_y = (int)cdiv(a.h, T::TILE_H);
    hipLaunchKernelGGL(kern, dim3((unsigned)a.tiles_x * a.tiles_y), dim3(T::NW * 64), lds_bytes, s, a);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

// ---- device side ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float3 bytes_rgb(uint32_t v)
{
    return make_float3((float)(v & 0xffu), (float)((v >> 8) & 0xffu), (float)((v >> 16) & 0xffu));
}

__device__ __forceinline__ uint32_t guide_at(const uint32_t *g, int w, int h, int x, int y)
{
    return ((unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h) ? g[(size_t)y * w + x] : 0u;
}

// Guide tile of tw x th packed texels whose top-left texel is image (x0,y0); four loads in flight per thread and trip.
__device__ __forceinline__ void fill_guide(uint32_t *t, int tw, int th, const uint32_t *g, int w, int h, int x0, int y0, int tid, int nthreads)
{
    const int n = tw * th;
    for (int t0 = tid; t0 < n; t0 += 4 * nthreads) {
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = t0 + j * nthreads;
            const int ty = i / tw, tx = i - ty * tw;
            v[j] = i < n ? guide_at(g, w, h, x0 + tx, y0 + ty) : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (t0 + j * nthreads < n) t[t0 + j * nthreads] = v[j];
    }
}

// Window slot j of an argument block packed by pack_temporal_window: its frame, and layer l of it.
template <typename Args>
__device__ __forceinline__ const void *nb_frame(const Args &a, int j) { return a.p[j * (a.n_layers + 1)]; }
template <typename Args>
__device__ __forceinline__ const uint32_t *nb_layer(const Args &a, int j, int l) { return (const uint32_t *)a.p[j * (a.n_layers + 1) + 1 + l]; }

// Issue priority by phase, as in nlm_strip_kernel: raised from the vertical sums to the end of the accumulation.
__device__ __forceinline__ void raise_priority() { __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_setprio(1); __builtin_amdgcn_sched_barrier(0); }
__device__ __forceinline__ void drop_priority() { __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_setprio(0); __builtin_amdgcn_sched_barrier(0); }

// The two epilogues of an output pixel.  Fused form: normalize.comp:36-42 as in pointwise.hip's normalize_kernel, stored in the
// launch's output format.  Accumulate form: W += the sums (nonlocal.comp:61-62).
__device__ __forceinline__ void put_normalized(void *out, size_t idx, int out_fmt, float4 tot, float totw)
{
    float4 o;
    if (totw == 0.0f) o = make_float4(1.f, 0.f, 1.f, 1.f);
    else o = make_float4(tot.x / totw, tot.y / totw, tot.z / totw, tot.w / totw);
    store_out(out, idx, out_fmt, o);
}
__device__ __forceinline__ void put_accumulated(mid_weightinfo *W, size_t idx, float4 tot, float totw)
{
    float4 *wp = (float4 *)(W + idx);
    float4 wc = wp[0], nw = wp[1];
    wc.x += tot.x; wc.y += tot.y; wc.z += tot.z; wc.w += tot.w;
    nw.x += totw;
    wp[0] = wc;
    wp[1] = nw;
}

}  // namespace mid
