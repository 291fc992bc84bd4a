// common.hpp -- context, error plumbing and device helpers shared by the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <unordered_set>
#include <vector>
#include "../../include/mi_denoise.h"

// Device buffers and events of the frame pipeline (csrc/pipeline.cpp), kept from call to call so that a steady stream of
// sequences pays for hipMalloc / hipEventCreate once: grown on demand, released by mid_ctx_release_cached and mid_ctx_destroy.
struct mid_pipe_set { std::vector<void *> p; size_t bytes = 0; };
struct mid_pipe_last {                  // event layout of the last mid_sequence_nlm* / mid_sequence_bilateral call
    int n_up = 0, nb = 0, f_lo = 0, first = 0, batch = 1; bool direct = false;
    std::vector<float> up_ms, out_ms;   // its timeline, kept from the first mid_pipe_last_timeline on: every later read gives these numbers
};
struct mid_pipe_cache {
    std::mutex mu;                      // one pipeline call per context at a time: the calls share the context's four streams
    mid_pipe_set ring, out;             // mid_sequence_nlm* / mid_sequence_bilateral: uploaded frames (2k + 4), output slots (4)
    mid_pipe_set layers;                // mid_sequence_bilateral with guide layers: n_layers per ring slot
    mid_pipe_set atrous;                // mid_sequence_atrous_joint: the RGBA32F levels between passes, two per kernel stream
                                        // (mid_sequence_atrous_variance: one block per kernel stream -- colour levels, variance levels, V_0)
    mid_pipe_set target, slots, weights, result;   // mid_nlm_multiframe
    std::vector<hipEvent_t> ev;
    mid_pipe_last last;                 // mid_pipe_last_timeline reads the events of the last call back
};

// Page-locked bounce buffers for host memory the caller did NOT pin (csrc/hostcopy.cpp): two halves used alternately, each
// guarded by the event of the last DMA that read or wrote it.  One set per direction, so the frame pipeline's upload and
// download streams never wait on each other's chunks.  Allocated on the first pageable copy, freed with the context.
struct mid_bounce {
    std::mutex mu;                      // one pageable copy per direction at a time
    void *buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool busy[2] = {false, false};      // ev[i] has been recorded and not yet waited for
    size_t chunk = 0;
};

// The stream a long NLM launch runs its packed right-edge launch on, beside the main launch (csrc/nlm_edge.hip): the device's LOWEST
// priority, as the sharded call's boundary streams and for their reason (sharded.cpp) -- a pool of hardware queues of the library's own,
// and workgroups that are dispatched where no workgroup of the main launch waits.  Created by the first launch that packs, freed with
// the context.  fork / join order it behind and before the caller's stream; mu is held from the fork's record to the join's wait.
struct mid_edge {
    std::mutex mu;
    hipStream_t s = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    bool failed = false;                // the stream or an event could not be created: launches stay whole from then on
};

struct mid_ctx {
    int device;
    // The four streams are created together, in this order, by mid_ctx_create (capi.cpp explains why and at which priorities).
    hipStream_t compute = nullptr;   // default stream for kernels
    hipStream_t compute2 = nullptr;  // second kernel stream of the frame pipeline (consecutive frames alternate)
    hipStream_t upload = nullptr;    // H2D stream of the frame pipeline    -- device's highest stream priority
    hipStream_t download = nullptr;  // D2H stream of the frame pipeline    -- device's highest stream priority
    int copy_priority = 0;           // what upload / download were created with
    int lds_max;           // max dynamic LDS per workgroup (bytes)
    int cu_count;
    char name[128];
    // kernels whose dynamic-LDS limit has been raised on THIS context's device (the attribute is per
    // device, so it is tracked per context; contexts may be used from different threads)
    std::mutex mu;
    std::unordered_set<const void *> lds_configured;
    mid_edge edge;
    mid_pipe_cache pipe;
    mid_bounce bounce_up, bounce_down;  // pageable host memory never reaches hipMemcpyAsync: see csrc/hostcopy.cpp
};

namespace mid {

int set_error(int code, const char *fmt, ...);

// (a failed call is reported once: the runtime's per-thread last error is cleared, so that the NEXT entry point's
// hipGetLastError after its launch does not report this failure again as its own)
#define MID_HIP(call)                                                                   \
    do {                                                                                \
        hipError_t e__ = (call);                                                        \
        if (e__ != hipSuccess) {                                                        \
            (void)hipGetLastError();                                                    \
            return mid::set_error(MID_ERR_HIP, "%s failed: %s (%s:%d)", #call,          \
                                  hipGetErrorString(e__), __FILE__, __LINE__);          \
        }                                                                               \
    } while (0)

#define MID_REQUIRE(cond, ...)                                                          \
    do {                                                                                \
        if (!(cond)) return mid::set_error(MID_ERR_INVALID, __VA_ARGS__);               \
    } while (0)

// The outputs of one launch are written while every workgroup of it still reads its inputs, so no output may be one of the
// call's inputs nor be given twice.  Reports the first out[t] (t ascending; an input before a repeat) as MID_ERR_INVALID:
// "<who>: out[t] is also <input_is> (...)" / "<who>: out[t] appears twice".  NULL outputs are skipped (the caller reports
// them).  Sorted copies, no hash sets; a failed allocation is an error code too, never an exception through the C-ABI.
int check_no_alias(const char *who, const char *input_is, const void *const *in, int n_in, const void *const *out, int n_out);

// Guide layers per frame that one call may pass: the "n_layers ... outside 0..16" limit of every layer-guided entry point.
constexpr int kMaxLayers = 16;

// What mid_nlm_layers_temporal and mid_bilateral_temporal check between their parameters and their launches, `who` being the
// name in the messages: the output range [first, first + count) inside n_frames, every frame and layer of its window
// [first - k, first + count - 1 + k] non-NULL (frames aligned for `fmt`), every output non-NULL and aligned for `out_fmt`, and
// no output among the window's frames and layers (all outputs of the call may be in flight beside launches that still read
// them).  layers[f * n_layers + l]; n_layers == 0 reads no layer table.  capi.cpp.
// guide_fmt: the layers' MID_FMT_* -- RGBA16F layers must be 8-byte aligned, RGBA32F ones 16-byte aligned (guide_aligned).
int check_temporal_window(const char *who, int fmt, const void *const *frames, const uint32_t *const *layers, int n_layers,
                          int n_frames, int k, int first, int count, void *const *out, int out_fmt, int guide_fmt = MID_FMT_RGBA8);

// The window of output frame t in the argument block of a kernel over neighbouring frames (NlmLayerPairArgs, BilPairArgs):
// slot j holds frame max(0, t - k) + j followed by its n_layers guide layers, t_slot is the output frame's own slot.
template <typename Args>
inline void pack_temporal_window(Args &a, const void *const *frames, const uint32_t *const *layers, int n_layers, int n_frames, int k, int t)
{
    const int lo = t - k < 0 ? 0 : t - k, hi = t + k > n_frames - 1 ? n_frames - 1 : t + k;
    a.n_nb = hi - lo + 1; a.n_layers = n_layers; a.t_slot = t - lo;
    for (int f = lo; f <= hi; ++f) {
        a.p[(f - lo) * (n_layers + 1)] = frames[f];
        for (int l = 0; l < n_layers; ++l) a.p[(f - lo) * (n_layers + 1) + 1 + l] = layers[(size_t)f * n_layers + l];
    }
}

// Binds the calling thread to the context's device and resolves the stream argument.
struct Bind {
    int rc;
    hipStream_t s;
    Bind(mid_ctx *ctx, void *stream);
};

inline unsigned cdiv(unsigned a, unsigned b) { return (a + b - 1) / b; }

// Entry points that wait on the host, allocate, or drive several streams cannot be part of a recording (csrc/recording.cpp: a stream
// between mid_record_begin and mid_record_end is in HIP's capture mode): they refuse with a message instead of leaving an invalidated
// capture behind.
inline int refuse_if_recording(hipStream_t s, const char *what)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return MID_OK; }
    if (st != hipStreamCaptureStatusNone)
        return set_error(MID_ERR_INVALID, "%s cannot be part of a recording (mid_record_begin is open on this stream): only the calls that "
                         "enqueue on ONE stream without waiting can -- kernels, mid_memset, copies from / to page-locked memory", what);
    return MID_OK;
}

// Frees what the frame pipeline keeps in the context (pipeline.cpp); the context's streams must be idle.
void pipe_cache_release(mid_ctx *ctx);

// Host <-> device copies that never hand the runtime pageable memory (csrc/hostcopy.cpp).  Pinned host memory
// (hipHostMalloc / hipHostRegister: mid_alloc_host, mid_host_register, mid_image_load_pinned) is DMA'd in place and the
// call is asynchronous on `s`; anything else goes through the context's page-locked bounce buffers in chunks: copy_h2d
// returns when the source has been consumed (the last DMAs may still be in flight on `s`), copy_d2h when the data is in dst.
bool host_is_pinned(const void *p, size_t bytes);
// Stronger than host_is_pinned, for memory the GPU will STORE into directly: [p, p+bytes) is mapped into the current device's
// address space as ONE contiguous range that lies inside ONE allocation or registration (hipHostGetDevicePointer of both ends,
// hipMemGetAddressRange of both mappings).  Any failed query answers false: the caller then takes a copy path instead.
bool host_range_in_one_mapping(const void *p, size_t bytes);
int copy_h2d(mid_ctx *ctx, void *dst, const void *src, size_t bytes, hipStream_t s);
// bounce = true: through the bounce buffers even when both ends of dst are page-locked (a range that spans two registrations,
// which the runtime's DMA refuses).
int copy_d2h(mid_ctx *ctx, void *dst, const void *src, size_t bytes, hipStream_t s, bool bounce = false);
void bounce_release(mid_ctx *ctx);     // waits for the last chunks and frees both bounce sets

// memset as a kernel launch (pointwise.hip): what mid_memset enqueues while its stream records -- see there why.
int fill_bytes(mid_ctx *ctx, void *dst, int value, size_t bytes, hipStream_t s);
inline bool stream_is_recording(hipStream_t s)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
    return st != hipStreamCaptureStatusNone;
}

// mid_nlm_temporal with the output format as an argument: out_fmt = MID_FMT_RGBA8 writes RGBA8 frames (pack_rgba8 of the
// normalized pixel), MID_FMT_RGBA16F half frames (pack_rgba16f), MID_FMT_RGBA32F float4 ones -- used by the frame pipeline's
// u8 / f16 variants, not exported.
// `corunning` != 0: the caller keeps launches on two streams in flight (the frame pipeline), so the last round of one launch
// overlaps the first of the next -- the HALF launch shape for a small launch's last round (nlm.hip, tail_split) is not used.
int nlm_temporal_out(mid_ctx *ctx, const mid_nlm_params *p, const void *const *frames, int n_frames, int k,
                     int first, int count, void *const *out, int out_fmt, void *stream, int corunning = 0);

// mid_bilateral (layers == nullptr) / mid_bilateral_layers (layers: n_layers guides in fmt_guide(p->format), texture layout) with the output format as
// an argument, as nlm_temporal_out: out_fmt = MID_FMT_RGBA8 / MID_FMT_RGBA16F writes pack_rgba8 / pack_rgba16f of the float4 result.
// No checks: the caller has made those of the public entry points.  Used by the frame pipeline (mid_sequence_bilateral), not exported.
// RGBA16F / RGBA32F guides run as the k = 0 window of one frame on bilateral_temporal.hip's kernels (bilateral_temporal_out).
int bilateral_out(mid_ctx *ctx, const mid_bilateral_params *p, const void *in, const uint32_t *const *layers, int n_layers,
                  void *out, int out_fmt, hipStream_t s);

// The parameter checks of mid_nlm_accum (size, filteringParameter, window limits, format): nlm.hip, shared with nlm_layers.hip.
int nlm_check_params(const mid_nlm_params *p);

// mid_nlm_layers with the output format as an argument (MID_FMT_RGBA8 / MID_FMT_RGBA16F: pack_rgba8 / pack_rgba16f of the float4
// result), as bilateral_out.  No checks: the caller has made those of the public entry points.  nlm_layers.hip; used by the frame
// pipeline (mid_sequence_nlm_layers), not exported.
int nlm_layers_out(mid_ctx *ctx, const mid_nlm_params *p, const void *in, const uint32_t *const *layers, int n_layers, void *out,
                   int out_fmt, hipStream_t s);

// mid_nlm_layers_temporal without its checks (the caller has made them), one launch per output frame on `s`:
// nlm_layers_temporal.hip; used by the frame pipeline (mid_sequence_nlm_layers_temporal), not exported.
// nlm_layers_temporal_fits: the pointer limit of one launch (MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS), MID_ERR_INVALID beyond it.
int nlm_layers_temporal_out(mid_ctx *ctx, const mid_nlm_params *p, const void *const *frames, const uint32_t *const *layers,
                            int n_layers, int n_frames, int k, int first, int count, void *const *out, int out_fmt, hipStream_t s);
int nlm_layers_temporal_fits(const char *who, int n_layers, int n_frames, int k);

// mid_nlm_joint without its checks (the caller has made them), one launch per output frame on `s`: nlm_joint.hip; used by the
// frame pipeline (mid_sequence_nlm_joint), not exported.  layer_h: n_layers host floats, or NULL for p->filteringParameter in
// every layer.  nlm_joint_check: what both entry points check after their own tables -- nlm_check_params, n_layers in 1..16, a
// layer table, n_frames >= 1, k >= 0, the pointer limit of one launch (nlm_layers_temporal_fits), every h > 0.
int nlm_joint_out(mid_ctx *ctx, const mid_nlm_params *p, const float *layer_h, const void *const *frames, const uint32_t *const *layers,
                  int n_layers, int n_frames, int k, int first, int count, void *const *out, int out_fmt, hipStream_t s);
int nlm_joint_check(const mid_nlm_params *p, const char *who, const float *layer_h, bool have_layers, int n_layers, int n_frames, int k);

// The parameter checks of mid_bilateral (size, sigmas, radius, format, layout): bilateral.hip, shared with bilateral_temporal.hip.
// guide_ok: the entry point reads guide layers of the bilateral family, so the format word may carry their format
// (MID_FMT_WITH_GUIDE); everywhere else a non-zero guide field is refused.
int bilateral_check_params(const mid_bilateral_params *p, const char *who, bool guide_ok = false);

// mid_bilateral_temporal without its checks (the caller has made them), one launch per output frame on `s`; layers == nullptr is
// the plain form: bilateral_temporal.hip; used by the frame pipeline (mid_sequence_bilateral_temporal), not exported.
// bilateral_temporal_check: the checks both entry points share -- bilateral_check_params, the texture layout, n_layers in 0..16
// (0 in the plain form), n_frames >= 1, k >= 0 and the pointer limit of one launch (nlm_layers_temporal_fits).
int bilateral_temporal_out(mid_ctx *ctx, const mid_bilateral_params *p, const void *const *frames, const uint32_t *const *layers,
                           int n_layers, int n_frames, int k, int first, int count, void *const *out, int out_fmt, hipStream_t s);
int bilateral_temporal_check(const mid_bilateral_params *p, const char *who, bool layered, int n_layers, int n_frames, int k);
// mid_bilateral_layers_pair_accum without its checks; mid_bilateral_layers_accum with RGBA16F / RGBA32F guides is this dispatch
// with target_layer == neighbour_layer.  bilateral_temporal.hip.
int bilateral_layers_pair_out(mid_ctx *ctx, const mid_bilateral_params *p, const void *target_layer, const void *neighbour_layer,
                              const void *neighbour_in, mid_weightinfo *W, hipStream_t s);

// mid_bilateral_joint without its checks (the caller has made them), one launch per output frame on `s`: bilateral_joint.hip;
// used by the frame pipeline (mid_sequence_bilateral_joint), not exported.  layer_sigma: n_layers host floats, or NULL for
// p->colorSigma in every layer.  bilateral_joint_check: what both entry points check after their own tables -- n_layers in
// 1..16, a layer table, bilateral_temporal_check, every sigma > 0.
int bilateral_joint_out(mid_ctx *ctx, const mid_bilateral_params *p, const float *layer_sigma, const void *const *frames,
                        const uint32_t *const *layers, int n_layers, int n_frames, int k, int first, int count, void *const *out,
                        int out_fmt, hipStream_t s);
int bilateral_joint_check(const mid_bilateral_params *p, const char *who, const float *layer_sigma, bool have_layers, int n_layers,
                          int n_frames, int k);

// mid_atrous_joint without its checks (the caller has made them), one launch per pass on `s`: atrous.hip; used by the frame
// pipeline (mid_sequence_atrous_joint), not exported.  scratch0 / scratch1: the RGBA32F levels between passes (the first needed
// from two passes on, the second from three).  atrous_check: what both entry points check before their own tables -- size,
// pass range, colorSigma, the format word, n_layers in 1..16, a layer table, every sigma finite and > 0 (NULL is refused).
int atrous_joint_out(mid_ctx *ctx, const mid_atrous_params *p, const float *layer_sigma, const void *in, const uint32_t *const *layers,
                     int n_layers, void *out, int out_fmt, void *scratch0, void *scratch1, hipStream_t s);
int atrous_check(const mid_atrous_params *p, const char *who, const float *layer_sigma, bool have_layers, int n_layers);
size_t atrous_scratch_frames(int n_passes);

// mid_atrous_joint_temporal without its checks (the caller has made them), per output frame one launch of the temporal pass and
// then atrous_joint_out for passes 1 .. N-1, all on `s`: atrous_temporal.hip; used by the frame pipeline
// (mid_sequence_atrous_joint_temporal), not exported.  scratch0 / scratch1: the levels, as above, shared by the call's outputs.
// atrous_temporal_check: what both entry points check before their own tables -- atrous_check, first_pass == 0, n_frames >= 1,
// k >= 0 and the pointer limit of one launch (nlm_layers_temporal_fits).
int atrous_temporal_out(mid_ctx *ctx, const mid_atrous_params *p, const float *layer_sigma, const void *const *frames,
                        const uint32_t *const *layers, int n_layers, int n_frames, int k, int first, int count, void *const *out,
                        int out_fmt, void *scratch0, void *scratch1, hipStream_t s);
int atrous_temporal_check(const mid_atrous_params *p, const char *who, const float *layer_sigma, bool have_layers, int n_layers,
                          int n_frames, int k);

// mid_atrous_moments / mid_atrous_variance without their checks (the caller has made them), one launch per output / per pass on
// `s`: atrous_variance.hip; used by the frame pipeline (mid_sequence_atrous_variance), not exported.  level / vlevel: the RGBA32F
// colour levels and the float variance levels between passes (the first pair needed from two passes on, the second from three);
// var_out == nullptr: the last pass stores no variance.  The checks: what the entry points check before their own tables.
int atrous_moments_out(mid_ctx *ctx, const mid_atrous_moments_params *p, const float *layer_sigma, const void *const *frames,
                       const uint32_t *const *layers, int n_layers, int n_frames, int k, int t, float *var_out, hipStream_t s);
int atrous_variance_out(mid_ctx *ctx, const mid_atrous_variance_params *p, const float *layer_sigma, const void *in, const float *var_in,
                        const uint32_t *const *layers, int n_layers, void *out, int out_fmt, float *var_out, void *const level[2],
                        float *const vlevel[2], hipStream_t s);
int atrous_moments_check(const mid_atrous_moments_params *p, const char *who, const float *layer_sigma, bool have_layers, int n_layers,
                         int n_frames, int k);
int atrous_variance_check(const mid_atrous_variance_params *p, const char *who, const float *layer_sigma, bool have_layers, int n_layers);

// mid_temporal_accumulate_clip without its checks (the caller has made them), one launch on `s`: temporal_accumulate.hip.
// clip_lo == clip_hi == nullptr: the unclipped kernel.
// temporal_accumulate_check: what the entry point checks before its tables -- the parameters, the format word, n_layers in
// 0..16 and, with layers, both tables and every sigma finite and > 0.
int temporal_accumulate_out(mid_ctx *ctx, const mid_temporal_accum_params *p, const float *layer_sigma, const void *cur,
                            const uint32_t *const *cur_layers, const uint32_t *const *prev_layers, int n_layers, const float *motion,
                            const mid_pixel *hist_color_in, const mid_pixel *hist_state_in, const float *var_spatial,
                            const mid_pixel *clip_lo, const mid_pixel *clip_hi, mid_pixel *color_out, mid_pixel *state_out, float *var_out,
                            hipStream_t s);
int temporal_accumulate_check(const mid_temporal_accum_params *p, const char *who, const float *layer_sigma, bool have_layers, int n_layers);

// mid_demodulate / mid_modulate without their checks (the caller has made them), one launch on `s`: albedo.hip; used by the frame
// pipeline (mid_sequence_atrous_recursive_albedo), not exported.  albedo_check: the size, the floor and the format word.
int demodulate_out(mid_ctx *ctx, const mid_albedo_params *p, const void *in, const void *albedo, mid_pixel *out, hipStream_t s);
int modulate_out(mid_ctx *ctx, const mid_albedo_params *p, const mid_pixel *in, const void *albedo, void *out, int out_fmt, hipStream_t s);
int albedo_check(const mid_albedo_params *p, const char *who);

// mid_firefly_clamp without its checks (the caller has made them), one launch on `s`: firefly.hip; used by the frame pipeline
// (mid_sequence_atrous_recursive_firefly), not exported.  firefly_check: the size, radius, rank, gain, floor and the format word.
int firefly_clamp_out(mid_ctx *ctx, const mid_firefly_params *p, const void *in, mid_pixel *out, hipStream_t s);
int firefly_check(const mid_firefly_params *p, const char *who);

// mid_color_bounds without its checks (the caller has made them), one launch on `s`: color_bounds.hip; used by the frame pipeline
// (mid_sequence_atrous_recursive_clip), not exported.  color_bounds_check: the size, radius, gamma and the format word.
int color_bounds_out(mid_ctx *ctx, const mid_color_bounds_params *p, const void *in, mid_pixel *lo, mid_pixel *hi, hipStream_t s);
int color_bounds_check(const mid_color_bounds_params *p, const char *who);

// mid_image_metrics without its pointer checks (the caller has made them), two launches on `s`: image_metrics.hip.
// image_metrics_check: the size, the two format words, peak, eps and the ssim flag.
int image_metrics_out(mid_ctx *ctx, const mid_image_metrics_params *p, const void *a, const void *b, void *work, float *map, hipStream_t s);
int image_metrics_check(const mid_image_metrics_params *p, const char *who);

// mid_guided_filter without its pointer checks (the caller has made them), two launches on `s`: guided.hip.  guide == nullptr or
// guide == in: the frame guides itself.  guided_check: the size, radius, eps and the format word; guided_work_bytes: what `work` holds.
int guided_out(mid_ctx *ctx, const mid_guided_params *p, const void *in, const void *guide, void *work, void *out, int out_fmt, hipStream_t s);
int guided_check(const mid_guided_params *p, const char *who);
size_t guided_work_bytes(const mid_guided_params *p);

// mid_median_filter without its pointer checks (the caller has made them), one launch on `s`: median.hip; used by the frame pipeline
// (mid_sequence_median), not exported.  median_check: the size, radius and format word, n_layers in 0..16, and with layers both tables
// and every sigma finite and > 0 (without: both tables NULL and no guide field).
int median_out(mid_ctx *ctx, const mid_median_params *p, const float *layer_sigma, const void *in, const uint32_t *const *layers, int n_layers,
               void *out, int out_fmt, hipStream_t s);
int median_check(const mid_median_params *p, const char *who, const float *layer_sigma, bool have_layers, int n_layers);

// ROCTx ranges (csrc/markers.cpp): no-ops unless the process already holds a ROCTx (rocprofv3 --marker-trace preloads one).
bool markers_active();
void range_push(const char *name);
void range_pop();
struct Range {
    bool on;
    explicit Range(const char *fmt, ...) __attribute__((format(printf, 2, 3)));
    ~Range();
    Range(const Range &) = delete;
    Range &operator=(const Range &) = delete;
};

// Raise the dynamic-LDS limit of `kern` once per context (kernels here use up to 160 KB).
inline int ensure_lds(mid_ctx *ctx, const void *kern, size_t bytes)
{
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (ctx->lds_configured.count(kern)) return MID_OK;
    MID_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    ctx->lds_configured.insert(kern);
    return MID_OK;
}

// ---- device side ------------------------------------------------------------------------
// Frame table passed by value to the batched kernels (kernarg space, scalar loads).
constexpr int kMaxFrames = 96;
struct FrameTable { const void *p[kMaxFrames]; };
struct OutTable   { void *p[kMaxFrames]; };

// UNORM texel decode, src/texture.cpp:16: the correctly rounded quotient c/255 for c = 0..255.  A product with
// 1/255 alone is off by one ulp for 126 of the 256 codes; one residual correction (r = c - 255 q exactly, q += r/255)
// lands on the IEEE quotient for all 256 -- checked exhaustively in exact arithmetic and by the bit-exact u8 tests --
// in 3 instructions instead of the ~12 plus two mode switches of a full fp32 division.
__device__ __forceinline__ float unorm8(float c)
{
    const float k = 1.0f / 255.0f;
    const float q = c * k;
    return fmaf(fmaf(-q, 255.0f, c), k, q);
}
__device__ __forceinline__ float4 decode_rgba8(uint32_t v)
{
    return make_float4(unorm8((float)(v & 0xffu)), unorm8((float)((v >> 8) & 0xffu)),
                       unorm8((float)((v >> 16) & 0xffu)), unorm8((float)(v >> 24)));
}

// u8 encode of the reference's read-back, src/main.cpp:97-103: (unsigned char)(255.0f * v), truncation, all four
// channels; clamped only where that C cast is undefined (v <= -1, v >= 256, NaN).
__device__ __forceinline__ uint32_t pack1(float x)
{
    const float v = 255.0f * x;                       // src/main.cpp:99
    if (!(v > -1.0f)) return 0u;                      // C cast undefined (and NaN): clamp
    if (v >= 256.0f) return 255u;
    return (uint32_t)(int)v;                          // truncation toward zero
}
__device__ __forceinline__ uint32_t pack_rgba8(float4 p)
{
    return pack1(p.x) | (pack1(p.y) << 8) | (pack1(p.z) << 16) | (pack1(p.w) << 24);
}

// RGBA16F texel: four IEEE binary16 values (R, G, B, A) in one 8-byte load.  The widening to fp32 is exact for every
// non-NaN half code -- subnormals, +-0, +-Inf -- so an RGBA16F frame without NaN texels filters to the bits of the RGBA32F frame
// it widens to (v_cvt_f32_f16; a NaN stays a NaN, quieted: a signalling NaN's payload bits are not kept).
__device__ __forceinline__ float half_lo(uint32_t v) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(v & 0xffffu)); }
__device__ __forceinline__ float half_hi(uint32_t v) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(v >> 16)); }
__device__ __forceinline__ float4 decode_rgba16f(uint2 v)
{
    return make_float4(half_lo(v.x), half_hi(v.x), half_lo(v.y), half_hi(v.y));
}
// fp32 -> binary16, round to nearest even (v_cvt_f16_f32 in the default rounding mode -- never the round-toward-zero
// packing instructions): overflow gives +-Inf, NaN stays NaN, results below the normal range are f16 subnormals.
__device__ __forceinline__ uint32_t pack_half2(float lo, float hi)
{
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)lo) | ((uint32_t)__builtin_bit_cast(uint16_t, (_Float16)hi) << 16);
}
__device__ __forceinline__ uint2 pack_rgba16f(float4 p) { return make_uint2(pack_half2(p.x, p.y), pack_half2(p.z, p.w)); }

// One pixel in the output format of the launch (a kernarg, so wave-uniform): float4, or the rounding of mid_pack_u8 /
// mid_pack_f16 of the float4 result (the frame pipeline's packed outputs).
__device__ __forceinline__ void store_out(void *out, size_t idx, int fmt, float4 o)
{
    if (fmt == MID_FMT_RGBA8) ((uint32_t *)out)[idx] = pack_rgba8(o);
    else if (fmt == MID_FMT_RGBA16F) ((uint2 *)out)[idx] = pack_rgba16f(o);
    else ((float4 *)out)[idx] = o;
}

// Bytes of one texel of a MID_FMT_* (host side: buffer sizes of the frame pipeline and the sharded exchange).
inline size_t fmt_bytes(int fmt) { return fmt == MID_FMT_RGBA8 ? 4 : fmt == MID_FMT_RGBA16F ? 8 : 16; }
// Output formats the fused NLM epilogue writes (NlmArgs::out_fmt): the input formats, RGBA8 = pack_rgba8, RGBA16F = pack_rgba16f.
inline bool fmt_known(int fmt) { return fmt == MID_FMT_RGBA32F || fmt == MID_FMT_RGBA8 || fmt == MID_FMT_RGBA16F; }
// Device pointers of RGBA16F images are read 8 bytes per texel: they must be 8-byte aligned (hipMalloc'd buffers are).
inline bool fmt_aligned(int fmt, const void *p) { return fmt != MID_FMT_RGBA16F || ((uintptr_t)p & 7u) == 0; }
// The two fields of mid_bilateral_params.format (MID_FMT_WITH_GUIDE): the frames' MID_FMT_* in bits 0..7, and in bits 8..15
// 0 (guide layers RGBA8) or 1 + MID_FMT_* of the guide layers.  fmt_guide: -1 for a code that names no format.
inline int fmt_frames(int format) { return format & 0xff; }
inline int fmt_guide(int format)
{
    const int c = (format >> 8) & 0xff;
    return c == 0 ? MID_FMT_RGBA8 : fmt_known(c - 1) ? c - 1 : -1;
}
// Guide layers are read one texel per load: RGBA16F ones must be 8-byte aligned, RGBA32F ones 16-byte aligned.
inline bool guide_aligned(int guide_fmt, const void *p)
{
    return ((uintptr_t)p & (guide_fmt == MID_FMT_RGBA16F ? 7u : guide_fmt == MID_FMT_RGBA32F ? 15u : 0u)) == 0;
}

// 2-D fetch with the zero-texel policy for out-of-image coordinates (texelFetch of the
// sampler2D shaders; SURVEY.md 8a: OOB = vec4(0)).
template <int FMT>
__device__ __forceinline__ float4 fetch_texture(const void *img, int w, int h, int x, int y)
{
    if ((unsigned)x >= (unsigned)w || (unsigned)y >= (unsigned)h) return make_float4(0.f, 0.f, 0.f, 0.f);
    const size_t idx = (size_t)y * w + x;
    if (FMT == MID_FMT_RGBA8) return decode_rgba8(((const uint32_t *)img)[idx]);
    if (FMT == MID_FMT_RGBA16F) return decode_rgba16f(((const uint2 *)img)[idx]);
    return ((const float4 *)img)[idx];
}

// Flat fetch of the samplerBuffer shader (bialteral_linear.comp:58): index y*w + x with x
// possibly outside the row, so it lands in the adjacent row; outside [0,N) = vec4(0).
template <int FMT>
__device__ __forceinline__ float4 fetch_linear(const void *img, int w, int h, int x, int y)
{
    const long idx = (long)y * w + x;
    if (idx < 0 || idx >= (long)w * h) return make_float4(0.f, 0.f, 0.f, 0.f);
    if (FMT == MID_FMT_RGBA8) return decode_rgba8(((const uint32_t *)img)[idx]);
    if (FMT == MID_FMT_RGBA16F) return decode_rgba16f(((const uint2 *)img)[idx]);
    return ((const float4 *)img)[idx];
}

// Cooperative fill of an LDS tile of tw x th texels whose top-left texel is image (x0,y0).
// Consecutive threads take consecutive texels of a tile row: 16 B/lane (RGBA16F 8 B, RGBA8 4 B) coalesced HBM reads.
template <int FMT, bool LINEAR>
__device__ __forceinline__ void fill_tile(float4 *lds, int tw, int th, const void *img, int w, int h,
                                          int x0, int y0, int tid, int nthreads, float rgb_scale = 1.0f, bool *opaque = nullptr)
{
    // `opaque` (optional): and-ed with "every texel THIS thread stored has alpha == 1.0f" (out-of-image texels are vec4(0): not opaque)
    // four texels per thread per trip: the four global loads are in flight together, so a tile costs
    // about n/(4*nthreads) memory latencies instead of n/nthreads
    const int n = tw * th;
    for (int t0 = tid; t0 < n; t0 += 4 * nthreads) {
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + j * nthreads;
            const int ty = t / tw, tx = t - ty * tw;
            v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < n) v[j] = LINEAR ? fetch_linear<FMT>(img, w, h, x0 + tx, y0 + ty)
                                     : fetch_texture<FMT>(img, w, h, x0 + tx, y0 + ty);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + j * nthreads;
            // rgb_scale is 1 except for the NLM strip kernels (exponent scale folded into the colours);
            // x * 1.0f is exact, and alpha is never scaled
            if (t < n) lds[t] = make_float4(v[j].x * rgb_scale, v[j].y * rgb_scale, v[j].z * rgb_scale, v[j].w);
            if (opaque && t < n) *opaque = *opaque && v[j].w == 1.0f;
        }
    }
}

// XCD-aware remap of a workgroup's tile index INSIDE its frame.  Workgroups are dealt round-robin over
// the 8 XCDs (XCD = linear id % 8).  Frames stay in launch order -- every XCD gets an equal share of every
// output frame, which matters because frames at the ends of a sequence have shorter temporal windows
// (an earlier whole-grid remap gave XCD 0 only 3-neighbour frames and XCD 3 only 5-neighbour ones: 18 %
// slower) -- and within a frame the tiles an XCD receives are made one contiguous run, so neighbouring
// tiles share halo texels in that XCD's L2.  Bijective for any tile count; speed only, never correctness.
__device__ __forceinline__ unsigned xcd_remap_in_frame(unsigned t, unsigned tiles, unsigned frame)
{
    const unsigned off = (frame * tiles) & 7u;          // XCD of this frame's tile 0
    const unsigned c = (t + off) & 7u;                  // XCD this workgroup runs on
    unsigned start = 0;                                 // tiles owned by XCDs before c
    for (unsigned cc = 0; cc < c; ++cc) {
        const unsigned first = (cc + 8u - off) & 7u;
        start += first < tiles ? (tiles - first + 7u) >> 3 : 0u;
    }
    const unsigned first_c = (c + 8u - off) & 7u;
    return start + ((t - first_c) >> 3);
}

// 2^x on the transcendental pipe.  On gfx950 a v_exp_f32 that is followed IMMEDIATELY by another vector instruction of the
// same wave costs about 7 cycles more than its own 8 (tools/microbench10/11.hip: 8 exps + 88 FMAs take 357 cycles per group per
// SIMD issued back to back, 302 with one wait state -- or any scalar instruction -- after each exp; the parts alone sum to 278).
// Issuing the instruction from here with its wait state attached keeps the pair together through scheduling.  Same
// instruction, same result bits as __builtin_amdgcn_exp2f.  Used by the bilateral kernels' single taps (measured +3.5 % on the
// tap-by-tap loop, profiles/r03_ab_exp_wait_state.txt); loops that issue their exps as a burst at raised priority -- the tiled
// bilateral kernel's row groups, the NLM offset loop -- use the builtin (there the wait states measured -2 % / -6 %).
__device__ __forceinline__ float exp2_hw(float x)
{
    float r;
    asm("v_exp_f32_e32 %0, %1\n\ts_nop 0" : "=v"(r) : "v"(x));
    return r;
}
// Whole-wave lane shifts through DPP (no LDS traffic): value of lane l-1 / l+1; lanes without
// a source read 0.
__device__ __forceinline__ float wave_shr1(float v)   // result[l] = v[l-1]
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_shl1(float v)   // result[l] = v[l+1]
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, false));
}

}  // namespace mid
