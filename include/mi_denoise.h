/*
 * mi_denoise.h -- C-ABI of libmi_denoise.so, the MI355X (gfx950) denoise hot path.
 *
 * The reference (Reefufui/image_denoising_filter) has no library/FFI surface: its "operator
 * interface" is the set of descriptor bindings + push-constant blocks each GLSL kernel is
 * dispatched with, and the ComputeApplication methods that drive them.  Each entry point
 * below names the reference interface it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every function returns 0 (MID_OK) or a MID_ERR_* code; mid_last_error() gives the
 *     thread-local message.  No exception crosses the ABI.  (Reference: VK_CHECK_RESULT =
 *     print+assert, src/vk_utils.h:55-63; std::runtime_error -> EXIT_FAILURE, src/main.cpp:1987.)
 *   - all image pointers are DEVICE pointers unless a name says host; the caller owns every
 *     buffer (reference: the application owns every VkBuffer/VkImage, src/main.cpp:1398-1437).
 *   - `stream` is a hipStream_t passed as void*; NULL = the context's own compute stream.
 *     Calls are asynchronous on that stream.  (The legacy default stream's handle is 0 too, so it cannot be named here:
 *     a caller whose buffers are produced on the default stream -- e.g. torch.cuda.current_stream().cuda_stream == 0 --
 *     passes a created stream that it orders after that work, or synchronises first.)
 *   - images are row-major, pixel index = width*y + x (shaders/bialteral.comp:81).
 *   - there is NO CPU fallback: without a usable HIP device mid_ctx_create fails.
 */
#ifndef MI_DENOISE_H
#define MI_DENOISE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MID_VERSION 100

enum {
    MID_OK = 0,
    MID_ERR_INVALID = 1,      /* bad argument / illegal mode combination (reference: assert, src/main.cpp:1315-1316) */
    MID_ERR_HIP = 2,          /* a HIP runtime call failed */
    MID_ERR_NO_DEVICE = 3,    /* no gfx950-capable device: the product path refuses to run */
    MID_ERR_UNSUPPORTED = 4,  /* parameter combination without a kernel */
    MID_ERR_IO = 5            /* file decode/encode failure (codec + CLI layer) */
};

/* struct Pixel {float r,g,b,a;}  -- src/main.cpp:39-41, the shaders' `struct Pixel{vec4 value;}` */
typedef struct mid_pixel { float r, g, b, a; } mid_pixel;

/* struct WeightInfo {vec4 weightColor; float normWeight;} at std430 stride 32 B --
 * shaders/nonlocal.comp:10-14, shaders/bialteral_layers.comp:8-12, shaders/normalize.comp:13-17;
 * host agrees: src/main.cpp:43-46 (struct NLM), :1399 (bufferSizeWeights). */
typedef struct mid_weightinfo {
    float weightColor[4];
    float normWeight;
    float _pad[3];
} mid_weightinfo;

/* Texel format of an input image: the reference creates RGBA32F textures for .exr and
 * RGBA8_UNORM for .png (src/texture.cpp:16, src/main.cpp:333-346).
 * MID_FMT_RGBA16F: four IEEE binary16 values in R, G, B, A order, 8 B per pixel -- the buffers renderers and HDR frame
 * sequences hand over (EXR HALF channels).  Device pointers to RGBA16F images must be 8-byte aligned (MID_ERR_INVALID
 * otherwise).  Kernels widen each texel exactly (subnormals, +-0, +-Inf), so for frames without NaN texels every filter gives
 * the bits of the same call with MID_FMT_RGBA32F on the widened frame.  A NaN texel stays a NaN but is quieted by the widening
 * (v_cvt_f32_f16), so a signalling NaN's bits may differ from a host widening that keeps them.  Accepted wherever a
 * params.format is read. */
enum { MID_FMT_RGBA32F = 0, MID_FMT_RGBA8 = 1, MID_FMT_RGBA16F = 2 };

/* Guide-layer format of the layer-guided BILATERAL calls.  mid_bilateral_params.format is one word with two fields:
 * format = MID_FMT_* of the frames in bits 0..7; bits 8..15 = 0 (guide layers RGBA8, as always) or 1 + MID_FMT_* of the guide layers.
 * A caller that passes 0, 1 or 2 gets what it always got.  The guide field is read by mid_bilateral_layers_accum,
 * mid_bilateral_layers, mid_bilateral_layers_pair_accum, mid_bilateral_temporal with a layer table, and mid_sequence_bilateral /
 * mid_sequence_bilateral_temporal with host_layers; all layers of one call share the one format.  Every other entry point that
 * reads a `format` -- the plain and linear bilateral, mid_bilateral_batch, mid_bilateral_pair_accum, the plain forms of
 * mid_bilateral_temporal and the two pipelines, everything that takes mid_nlm_params -- refuses a non-zero guide field with
 * MID_ERR_INVALID before anything is queued (layer-guided NLM takes RGBA8 guides only: its patch distances are exact integer
 * sums of byte values).  Also MID_ERR_INVALID: a guide code that names no format, bits above 15, an RGBA16F guide layer that is
 * not 8-byte aligned, an RGBA32F one that is not 16-byte aligned (device pointers; the pipelines' host layers need no alignment).
 * What a guide texel means is said in section a3. */
#define MID_FMT_WITH_GUIDE(fmt, guide_fmt) ((fmt) | (((guide_fmt) + 1) << 8))

/* Addressing of the bilateral input: bialteral.comp (sampler2D, 2-D texelFetch, out-of-image
 * texel = 0) vs bialteral_linear.comp (samplerBuffer, flat index c + j + i*width: columns wrap
 * into the adjacent row, index outside [0,N) = 0).  m_linear = !nonlinear, src/main.cpp:1311. */
enum { MID_LAYOUT_TEXTURE = 0, MID_LAYOUT_LINEAR = 1 };

/* Push-constant block of bialteral.comp / bialteral_linear.comp / bialteral_layers.comp
 * (shaders/bialteral.comp:13-20: {int width; int height; float spatialSigma; float colorSigma},
 * 16 B, pushed at src/main.cpp:801-808 and :873-877 with {2.0f, 0.2f}); the first 16 bytes are
 * that block byte for byte.  `radius` replaces `#define TEXEL_WINDOW 20` (shaders/bialteral.comp:5). */
typedef struct mid_bilateral_params {
    int32_t width;
    int32_t height;
    float   spatialSigma;
    float   colorSigma;
    int32_t radius;   /* window is (2*radius+1)^2; kernels exist for 1..24 */
    int32_t layout;   /* MID_LAYOUT_* (ignored by the layers kernels: always texture) */
    int32_t format;   /* MID_FMT_* of `in` (RGBA32F, RGBA8 or RGBA16F); guide layers are RGBA8 unless MID_FMT_WITH_GUIDE says otherwise */
} mid_bilateral_params;

/* Push-constant block of nonlocal.comp (shaders/nonlocal.comp:16-22: {int width; int height;
 * float filteringParameter}, 12 B, pushed at src/main.cpp:865-872 with 0.5f).  The ranges
 * replace `#define WINDOW 7` / `#define PATCH_WINDOW 3` (shaders/nonlocal.comp:5-6) and are
 * HALF-OPEN [lo,hi) like the shader's loops (:36-44): the reference is search [-7,7) patch
 * [-3,3); the 21x21 / 7x7 benchmark configuration is search [-10,11) patch [-3,4).
 * Limits: both ranges contain 0, search width <= 64, patch width <= 16.  Every search range and every patch of the forms
 * [-P,P) and [-P,P] up to 16 wide runs on the LDS-tiled kernel as long as its tile of (64 + S - 1) x (T + P - 1 + S - 1)
 * RGBA32F texels fits 160 KB (search width S, patch width P, T = 32 rows, 16 for patches 10 wide and up): search width
 * <= 52 at a 7x7 patch, <= 50 at 9x9, <= 55 at 1x1, <= 56 at 16x16; anything else (lopsided patches, wider windows) is
 * computed by a per-pixel kernel -- same results, the reference's S^2 * P^2 work. */
typedef struct mid_nlm_params {
    int32_t width;
    int32_t height;
    float   filteringParameter;
    int32_t search_lo, search_hi;
    int32_t patch_lo, patch_hi;
    int32_t format;   /* MID_FMT_* of target and neighbour images (RGBA32F, RGBA8 or RGBA16F) */
} mid_nlm_params;

/* Push-constant block of normalize.comp (shaders/normalize.comp:19-24), 8 B. */
typedef struct mid_normalize_params { int32_t width; int32_t height; } mid_normalize_params;

typedef struct mid_ctx mid_ctx;   /* opaque; bound to one HIP device */

/* ---- context / errors / memory -------------------------------------------------------
 * Replaces the Vulkan bootstrap (src/vk_utils.cpp:13-305) and buffer factories
 * (src/main.cpp:247-401): a context is one device + one compute stream. */
int         mid_ctx_create(int device, mid_ctx **out);
void        mid_ctx_destroy(mid_ctx *ctx);
/* Frees the device buffers and events the frame pipeline (mid_sequence_nlm*, mid_sequence_bilateral, mid_nlm_multiframe) keeps in the context
 * between calls -- at 1080p RGBA32F and k = 2 about 400 MB -- and the 32 MiB of page-locked bounce buffers; the next call
 * allocates again.  Without it the cache follows the calls: it grows to the largest frame size seen, and a call whose frames
 * are more than four times smaller than the cached buffers gives those back and keeps buffers of its own size. */
int         mid_ctx_release_cached(mid_ctx *ctx);
const char *mid_last_error(void);
int         mid_version(void);
int         mid_device_name(mid_ctx *ctx, char *buf, size_t buflen);
/* The context's four streams -- [0] compute (the default for stream = NULL), [1] the frame pipeline's second kernel stream,
 * [2] its upload and [3] its download stream -- are created together by mid_ctx_create; the two copy streams at the device's
 * highest stream priority (numerically lowest: `greatest`), so that they never share one of the runtime's hardware queues with
 * the kernel streams or with the caller's streams (csrc/capi.cpp has the measurements).  Stands where the reference takes its
 * single queue (vkGetDeviceQueue, src/main.cpp:1335). */
int         mid_ctx_stream_priorities(mid_ctx *ctx, int priority[4], int *least, int *greatest);

int mid_alloc(mid_ctx *ctx, size_t bytes, void **dptr);              /* CreateWriteOnlyBuffer & co */
int mid_free(mid_ctx *ctx, void *dptr);
int mid_alloc_host(mid_ctx *ctx, size_t bytes, void **hptr);         /* pinned staging (CreateStagingBuffer/CreateDynamicBuffer) */
int mid_free_host(mid_ctx *ctx, void *hptr);
/* Pin memory the caller already owns (a decoded frame in a std::vector, say) so that copies from/to it are truly
 * asynchronous (the pinning holds for every device of the process); undo with mid_host_unregister before the memory is
 * freed and after every copy that uses it has completed.  Measured on MI355X, 16 x 1080p RGBA32F through
 * mid_sequence_nlm: buffers from mid_alloc_host 12.8 ms, memory registered in place 25.1 ms (+6 ms to register), pageable
 * memory (bounced inside the library, see mid_memcpy_h2d) slower than either -- so decode into mid_alloc_host buffers when
 * throughput matters, and register in place when the frames already exist in ordinary memory. */
int mid_host_register(mid_ctx *ctx, void *hptr, size_t bytes);
int mid_host_unregister(mid_ctx *ctx, void *hptr);
/* Host <-> device copies.  Page-locked host memory (mid_alloc_host, mid_host_register, mid_image_load_pinned) is DMA'd in
 * place and the call is asynchronous on `stream`.  ANY OTHER host memory is accepted too, but it never reaches the HIP
 * runtime (whose pin-on-the-fly path for pageable copies of more than 1 MiB the library does not rely on): it is moved in
 * 8 MiB chunks through page-locked bounce buffers the context owns (32 MiB, allocated on first use), and the call returns
 * when src_host has been consumed (h2d; the last chunks may still be in flight on `stream`) or dst_host holds the data (d2h).
 * The same holds for every host frame handed to mid_sequence_nlm* / mid_nlm_multiframe.  Pageable copies cost a host memcpy
 * on top of the DMA (measured: see LABNOTES R5.1), so decode into pinned memory when throughput matters.
 * Threads: a context has ONE pair of bounce buffers per direction, guarded by a lock the copying thread holds from its first chunk
 * to its last, INCLUDING the waits for `stream` to reach each chunk.  Pageable copies of one direction on one context are therefore
 * serialised, also across independent streams, and two threads must not make them depend on each other: if thread A's copy sits on a
 * stream that waits (hipStreamWaitEvent) for work queued behind thread B's pageable copy of the same direction on the same context,
 * A holds the lock while its stream waits for B and B waits for the lock -- a deadlock.  Pinned copies take no lock; threads that
 * need independent pageable copies use one context each (contexts share nothing). */
int mid_memcpy_h2d(mid_ctx *ctx, void *dst, const void *src_host, size_t bytes, void *stream);  /* LoadImageDataToBuffer + copy-to-texture, src/main.cpp:1105-1142,990-1076 */
int mid_memcpy_d2h(mid_ctx *ctx, void *dst_host, const void *src, size_t bytes, void *stream);  /* vkCmdCopyBuffer to staging + GetImageFromGPU, src/main.cpp:835-840,91-123 */
int mid_memset(mid_ctx *ctx, void *dst, int value, size_t bytes, void *stream);                 /* the reference never clears its weight buffer; callers of *_accum must */
int mid_stream_sync(mid_ctx *ctx, void *stream);                     /* vkWaitForFences, src/main.cpp:1092 */

/* ---- recorded command sequences ---------------------------------------------------------
 * The reference works on RECORDED command buffers: every RecordCommandsOf* brackets its dispatches, barriers and copies with
 * vkBeginCommandBuffer / vkEndCommandBuffer (src/main.cpp:791/846, 855/886, 895/988, 996/1075) and RunCommandBuffer submits the
 * recording (vkQueueSubmit, :1078-1103); it records anew before each submission.  Here a sequence is recorded ONCE and submitted
 * as often as needed -- the HIP counterpart of a command buffer is a captured graph (csrc/recording.cpp):
 *   mid_record_begin(ctx, stream)          vkBeginCommandBuffer: `stream` (NULL = the context's compute stream) stops executing
 *                                          and records instead;
 *   ... kernel-level calls on that stream  mid_bilateral*, mid_nlm_accum, mid_nlm_temporal, mid_normalize, mid_pack_u8,
 *                                          mid_unpack_u8, mid_memset, mid_memcpy_* from / to PAGE-LOCKED memory: everything that only
 *                                          enqueues on the one stream.  Arguments are taken as they are at record time: the same
 *                                          buffers are read and written by every submission (like bound descriptors), their
 *                                          CONTENT is whatever it is when the submission runs;
 *   mid_record_end(ctx, stream, &rec)      vkEndCommandBuffer; the stream executes again;
 *   mid_recording_submit(rec, stream)      vkQueueSubmit: asynchronous on `stream` (any stream of the context's device), ordered
 *                                          like one launch; the same recording must not be in flight twice at the same time;
 *   mid_recording_destroy(rec)             after its last submission has completed.
 * One runtime call per submission instead of one per dispatch.  Measured on MI355X (profiles/r06_recording_replay.txt, bench.py
 * also.graph_replay_literal_nlm): the same bytes, and NOT faster than the calls issued one by one from compiled code -- about 4 us per
 * launch either way, and the reference's literal multi-frame sequence is bound by its chain of dependent kernels at every frame size.
 * A matter of program shape; for speed use the fused entry points (mid_nlm_temporal, mid_bilateral_batch, mid_bilateral_layers).
 * mid_record_begin and mid_record_end of one recording are called on the same thread.
 * Refused while a stream records (MID_ERR_INVALID, the recording stays valid): calls that wait on the host, drive several streams or
 * bounce pageable memory -- mid_stream_sync, mid_timer_tick/tock, mid_sequence_nlm* (mid_sequence_nlm_layers_temporal among them),
 * mid_sequence_bilateral, mid_nlm_multiframe, mid_nlm_temporal_sharded,
 * mid_comm_loopback, copies from / to pageable host memory.  Do not allocate or free (mid_alloc*, mid_free*, mid_host_register) on the
 * recording thread between begin and end: the runtime fails such calls and invalidates the recording (mid_record_end then reports
 * it).  The capture is thread-local: other threads keep using their own streams meanwhile.  A kernel's first ever launch may be
 * inside a recording (raising its LDS limit is not a stream operation). */
typedef struct mid_recording mid_recording;
int mid_record_begin(mid_ctx *ctx, void *stream);
int mid_record_end(mid_ctx *ctx, void *stream, mid_recording **out);
int mid_recording_submit(mid_recording *rec, void *stream);
int mid_recording_info(mid_recording *rec, int *n_nodes /* graph nodes */, int *n_kernels /* of them kernel launches */);
int mid_recording_destroy(mid_recording *rec);

/* ---- a1/a2: plain bilateral -----------------------------------------------------------
 * Replaces the dispatch of shaders/bialteral.comp / bialteral_linear.comp recorded by
 * RecordCommandsOfExecuteAndTransfer(normKernel=false), src/main.cpp:785-847: bindings
 * {0: vec4 out[N]; 1: image}. */
int mid_bilateral(mid_ctx *ctx, const mid_bilateral_params *p,
                  const void *in, mid_pixel *out, void *stream);
/* The same dispatch for n_frames independent frames of one size in ONE launch (grid = tiles x frames): what the
 * reference does by calling RunOnGPU once per file (src/main.cpp:1952-1985) in one launch instead of n (measured: the same
 * rate per frame -- at r = 8 a 1080p frame is 2040 workgroups on 1024 slots, four 40 KB tiles per CU, 1.99 rounds, so there is
 * little tail to save; tools/microbench19.hip).  in/out: host arrays of n_frames device pointers.
 * Results are bit-identical to n_frames calls of mid_bilateral (same tile code).
 * No aliasing: an `out` buffer must not be any `in` buffer of the same call (all frames are filtered concurrently) nor
 * appear twice; mid_bilateral likewise rejects in == out.  Violations return MID_ERR_INVALID. */
int mid_bilateral_batch(mid_ctx *ctx, const mid_bilateral_params *p, const void *const *in /* n_frames device ptrs */,
                        mid_pixel *const *out /* n_frames device ptrs */, int n_frames, void *stream);

/* ---- a3: layer-guided bilateral ---------------------------------------------------------
 * mid_bilateral_layers_accum = one dispatch of shaders/bialteral_layers.comp
 * (RecordCommandsOfExecuteNLM(nlm=false), src/main.cpp:849-887): W[p] += sums, bindings
 * {0: WeightInfo W[N]; 1: inputTex; 2: layerTex (always RGBA8, src/main.cpp:1396,1419-1420)}.
 * mid_bilateral_layers = the whole per-layer loop src/main.cpp:1610-1623 plus normalize
 * (:1649-1652) fused in one kernel: no WeightInfo traffic.
 * Half and float guide layers (p->format = MID_FMT_WITH_GUIDE(frames' format, MID_FMT_RGBA16F or MID_FMT_RGBA32F)): what a
 * renderer writes beside an HDR beauty pass -- normals in [-1, 1], depth in scene units, HDR albedo -- guides the filter as it
 * is.  A guide texel's r, g, b are read as IEEE values (half values are widened exactly, as for frames); the guide's alpha is
 * ignored; an out-of-image guide texel is vec4(0).  The weight is the formula of the RGBA8 guides,
 *   exp(-0.5 |G(p) - G(p+o)|^2_rgb / colorSigma^2),
 * with NO clamping to [0, 1].  Non-finite guide texels follow IEEE arithmetic: an Inf against a finite value gives weight 0;
 * Inf against Inf, or a NaN, poisons (NaN) the pixels whose windows hold it.  Precision: the kernels carry a guide value as the
 * fp32 product g * sqrt(0.5 log2 e) / colorSigma -- as they always did for RGBA8 -- so the relative precision of a weight falls
 * off as about 2^-24 |g| / colorSigma.  Up to |g| <= 16 colorSigma the results stay inside the bilateral tolerance of the
 * RGBA8 guides (1e-5 relative); scale depth-like layers (subtract an offset, divide by the scene's extent) or colorSigma so
 * that |g| / colorSigma stays moderate.  A float guide with rgb = the fp32 quotient c / 255 gives the bits of the RGBA8 guide c,
 * and a half guide the bits of the float guide it widens to.
 * The layer parameters keep their C type whatever the guide format: with RGBA16F / RGBA32F guides the caller casts its
 * pointers (8 / 16 bytes per texel) to const uint32_t *. */
int mid_bilateral_layers_accum(mid_ctx *ctx, const mid_bilateral_params *p, const void *in,
                               const uint32_t *layer_rgba8 /* or, cast, an RGBA16F / RGBA32F layer: MID_FMT_WITH_GUIDE */,
                               mid_weightinfo *W, void *stream);
int mid_bilateral_layers(mid_ctx *ctx, const mid_bilateral_params *p, const void *in,
                         const uint32_t *const *layers_rgba8 /* host array of device ptrs; cast RGBA16F / RGBA32F layers with MID_FMT_WITH_GUIDE */,
                         int n_layers, mid_pixel *out, void *stream);

/* ---- a4: non-local means ----------------------------------------------------------------
 * mid_nlm_accum = one dispatch of shaders/nonlocal.comp (RecordCommandsOfExecuteNLM(nlm=true),
 * src/main.cpp:849-887, loop :1577-1606): W[p] += (weightColor, 0.001 + sum of weights) for one
 * neighbour frame, target fixed; bindings {0: W; 1: u_targetImage; 2: u_neighbourImage}.
 * mid_nlm_temporal = the multi-frame mode (src/main.cpp:1539-1606) for an animation: for each
 * output frame t in [first, first+count) it accumulates over neighbour frames
 * max(0,t-k)..min(n_frames-1,t+k) in ascending order (target = frame t) and normalizes, all in
 * one launch (grid.z = output frame); k = 0 is independent single-frame NLM over a batch.
 * (Version note: the strip kernels now add most rows' squared differences straight onto the vertical running sums, one rounding fewer
 * per row -- the last bits of NLM outputs differ from earlier builds; they still do not depend on the launch shape.) */
int mid_nlm_accum(mid_ctx *ctx, const mid_nlm_params *p, const void *target,
                  const void *neighbour, mid_weightinfo *W, void *stream);
/* (mid_nlm_temporal: no aliasing -- an `out` buffer must not be a frame of the sequence nor appear twice: MID_ERR_INVALID, as for mid_bilateral_batch.) */
int mid_nlm_temporal(mid_ctx *ctx, const mid_nlm_params *p,
                     const void *const *frames /* host array of n_frames device ptrs */,
                     int n_frames, int k, int first, int count,
                     mid_pixel *const *out /* host array of `count` device ptrs */, void *stream);

/* ---- a4b: layer-guided non-local means ---------------------------------------------------
 * The layer-guided loop of src/main.cpp:1610-1623 with nonlocal.comp as its kernel instead of bialteral_layers.comp: the patch
 * distance is taken on an RGBA8 guide layer (albedo, normal, depth ...; texels c/255, out-of-image texels 0) and the colour from
 * the input image (RGBA32F, RGBA8 or RGBA16F per p->format; out-of-image texels 0).
 * mid_nlm_layers_accum = one dispatch for guide layer `layer_rgba8`: for each pixel p and search offset s,
 *   d = sum over the patch of |G(p+q) - G(p+s+q)|^2_rgb,  w = exp(-d/h^2),  W[p].weightColor += w * in(p+s),
 *   W[p].normWeight += w, plus 0.001 once per dispatch (nonlocal.comp:32-33, :55-62).
 * mid_nlm_layers = n_layers such dispatches into a zeroed W (layers in the given order) followed by mid_normalize, fused in one
 * kernel: no WeightInfo traffic, and the bits of that chain of calls.  With n_layers == 0 every pixel is the magenta sentinel,
 * as in mid_bilateral_layers.  With one layer equal to an RGBA8 input the result is mid_nlm_temporal(k = 0) of that input to
 * rounding (the guide's distances are summed as exact integers here).  A non-finite input texel (NaN, +-Inf) makes every output
 * whose search window contains it non-finite in the channels where the texel is, Inf * 0 being NaN as in IEEE arithmetic.
 * The windows and their limits are mid_nlm_accum's: the two tuned windows run on an LDS-tiled kernel, every other one on a
 * per-pixel kernel.  MID_ERR_INVALID for: the parameter checks of mid_nlm_accum; a NULL pointer; n_layers outside 0..16; an
 * RGBA16F input that is not 8-byte aligned; `out` equal to `in` or to a layer (mid_nlm_layers). */
int mid_nlm_layers_accum(mid_ctx *ctx, const mid_nlm_params *p, const void *in,
                         const uint32_t *layer_rgba8, mid_weightinfo *W, void *stream);
int mid_nlm_layers(mid_ctx *ctx, const mid_nlm_params *p, const void *in,
                   const uint32_t *const *layers_rgba8 /* host array of device ptrs */,
                   int n_layers, mid_pixel *out, void *stream);

/* ---- a4c: layer-guided non-local means over neighbouring frames --------------------------
 * mid_nlm_layers with the neighbouring frames of an animation as further sources of samples: the guide layers, which are free
 * of noise, say which pixels belong together; the frames t-k..t+k supply more samples of them.
 * mid_nlm_layers_pair_accum = one dispatch with a target guide Gt, a neighbour guide Gn and a neighbour colour image In (guides
 * RGBA8, texels c/255; In in p->format; out-of-image texels 0 everywhere): for each pixel p and search offset s,
 *   d = sum over the patch of |Gt(p+q) - Gn(p+s+q)|^2_rgb,  w = exp(-d/h^2),  W[p].weightColor += w * In(p+s),
 *   W[p].normWeight += w, plus 0.001 once per dispatch.
 * With target_layer_rgba8 == neighbour_layer_rgba8 it gives the bits of mid_nlm_layers_accum(p, neighbour_in, that layer, W).
 * mid_nlm_layers_temporal = outputs [first, first+count) of a sequence of n_frames frames with n_layers layers each.  Output t:
 * into a zeroed W, for each neighbour f = max(0,t-k) .. min(n_frames-1,t+k), ascending, and inside it each layer l = 0 ..
 * n_layers-1, ascending, one such dispatch with Gt = layer[t][l], Gn = layer[f][l], In = frame[f]; then mid_normalize and, for
 * out_format MID_FMT_RGBA8 / MID_FMT_RGBA16F, mid_pack_u8 / mid_pack_f16.  Fused in one kernel per output frame (no WeightInfo
 * traffic), with the bits of that chain of calls; with k == 0 the bits of mid_nlm_layers; with n_layers == 0 every pixel is the
 * magenta sentinel.  A non-finite texel of a frame makes every output of the frames t-k..t+k whose search window contains it
 * non-finite, as in mid_nlm_layers.  frames: host array of n_frames device pointers in p->format; layers_rgba8: host array of n_frames * n_layers
 * device pointers, frame-major (NULL only with n_layers == 0); out: host array of `count` device pointers in out_format.  Only
 * the frames and layers of [first-k, first+count+k) are read.
 * Windows as for mid_nlm_layers: the two tuned ones run on an LDS-tiled kernel, every other one on a per-pixel kernel.
 * A launch carries the pointers of one output's window by value, so MID_ERR_INVALID for
 *   min(2k+1, n_frames) * (n_layers + 1) > MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS
 * (k = 2 with 16 layers needs 85, k = 4 with 16 layers 153), and for: the parameter checks of mid_nlm_accum; a NULL pointer;
 * n_layers outside 0..16; k < 0, first < 0, count < 1, first + count > n_frames; an unknown out_format; an RGBA16F frame or output
 * that is not 8-byte aligned; an output that is also a frame or layer of the window, or appears twice. */
#define MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS 176
int mid_nlm_layers_pair_accum(mid_ctx *ctx, const mid_nlm_params *p, const uint32_t *target_layer_rgba8,
                              const uint32_t *neighbour_layer_rgba8, const void *neighbour_in, mid_weightinfo *W, void *stream);
int mid_nlm_layers_temporal(mid_ctx *ctx, const mid_nlm_params *p,
                            const void *const *frames /* host array of n_frames device ptrs */,
                            const uint32_t *const *layers_rgba8 /* host array of n_frames * n_layers device ptrs */,
                            int n_layers, int n_frames, int k, int first, int count,
                            void *const *out /* host array of `count` device ptrs */, int out_format, void *stream);

/* ---- a4d: the bilateral filter over neighbouring frames -----------------------------------
 * mid_bilateral / mid_bilateral_layers with the neighbouring frames of an animation as further sources of samples.  Texture
 * addressing only (out-of-image texel = vec4(0)); guides RGBA8, texels c/255 -- or, with MID_FMT_WITH_GUIDE in p->format, RGBA16F
 * / RGBA32F guides with the semantics of section a3 (IEEE values, alpha ignored, no clamping, non-finite texels by IEEE
 * arithmetic, |g| <= 16 colorSigma for the tolerance; the layer parameters keep their C type and the caller casts); frames in
 * the frames' field of p->format; radius, spatialSigma and colorSigma as in mid_bilateral.
 * One pair dispatch has a target guide Gt, a neighbour guide Gn and a neighbour colour image In: for each pixel p and tap
 * o = (i, j), |i|, |j| <= radius,
 *   w = exp(-0.5 |o|^2 / spatialSigma^2) * exp(-0.5 |Gt(p) - Gn(p+o)|^2_rgb / colorSigma^2)
 *   W[p].weightColor += w * In(p+o),   W[p].normWeight += w.
 * Only the centre comes from the target; everything under the taps comes from the neighbour (bialteral_layers.comp with
 * layerColor fetched from a second image).
 * mid_bilateral_pair_accum = the plain form: Gt = target, Gn = In = neighbour, both frames in p->format.
 * mid_bilateral_layers_pair_accum = the layered form: Gt = target_layer_rgba8, Gn = neighbour_layer_rgba8, In = neighbour_in.
 * With target guide == neighbour guide (the same buffer, or equal texels) a pair dispatch gives the bits of
 * mid_bilateral_layers_accum(p, neighbour_in, that layer, W).
 * mid_bilateral_temporal = outputs [first, first+count) of a sequence of n_frames frames.  Output t: into a zeroed W, for each
 * neighbour f = max(0,t-k) .. min(n_frames-1,t+k), ascending -- plain form (layers_rgba8 == NULL, n_layers must be 0): one
 * mid_bilateral_pair_accum(frame[t], frame[f]); layered form: for each layer l = 0 .. n_layers-1, ascending, one
 * mid_bilateral_layers_pair_accum(layer[t][l], layer[f][l], frame[f]) -- then mid_normalize and, for out_format MID_FMT_RGBA8 /
 * MID_FMT_RGBA16F, mid_pack_u8 / mid_pack_f16.  Fused in one kernel per output frame (accumulators in registers, no WeightInfo
 * traffic), with the bits of that chain of calls; with k == 0 the bits of mid_bilateral (plain) / mid_bilateral_layers
 * (layered); layered with n_layers == 0 (a non-NULL table) every pixel is the magenta sentinel, as in mid_bilateral_layers.
 * There is no temporal falloff weight: a neighbour frame weighs by range and space only, as in the temporal NLM modes.
 * frames: host array of n_frames device pointers in p->format; layers_rgba8: host array of n_frames * n_layers device pointers,
 * frame-major; out: host array of `count` device pointers in out_format.  Only the frames and layers of
 * [first-k, first+count+k) are read.  Radii 4, 8, 10 and 20 run on tuned LDS-tiled kernels, every other radius on a
 * run-time-radius tiled kernel, the layered form at radius > 17 (two tiles exceed LDS) on a per-pixel kernel.
 * A launch carries the pointers of one output's window by value, so MID_ERR_INVALID, before anything is queued, for
 *   min(2k+1, n_frames) * (n_layers + 1) > MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS
 * (the limit and the rule of mid_nlm_layers_temporal), and for: the parameter checks of mid_bilateral; MID_LAYOUT_LINEAR (the
 * linear variant exists to time a buffer against a texture and has no temporal form); a NULL pointer; n_layers outside 0..16,
 * or not 0 in the plain form; k < 0, first < 0, count < 1, first + count > n_frames; an unknown out_format; an RGBA16F frame or
 * output that is not 8-byte aligned; an output that is also a frame or layer of the window, or appears twice; a guide field in
 * the plain forms, an unknown guide code, an RGBA16F guide layer that is not 8-byte aligned, an RGBA32F one not 16-byte aligned. */
int mid_bilateral_pair_accum(mid_ctx *ctx, const mid_bilateral_params *p, const void *target, const void *neighbour,
                             mid_weightinfo *W, void *stream);
/* (both layers in the guide format of p->format: RGBA8, or cast RGBA16F / RGBA32F layers with MID_FMT_WITH_GUIDE) */
int mid_bilateral_layers_pair_accum(mid_ctx *ctx, const mid_bilateral_params *p, const uint32_t *target_layer_rgba8,
                                    const uint32_t *neighbour_layer_rgba8, const void *neighbour_in, mid_weightinfo *W, void *stream);
int mid_bilateral_temporal(mid_ctx *ctx, const mid_bilateral_params *p,
                           const void *const *frames /* host array of n_frames device ptrs */,
                           const uint32_t *const *layers_rgba8 /* host array of n_frames * n_layers device ptrs, or NULL; cast RGBA16F / RGBA32F layers with MID_FMT_WITH_GUIDE */,
                           int n_layers, int n_frames, int k, int first, int count,
                           void *const *out /* host array of `count` device ptrs */, int out_format, void *stream);

/* ---- a4e: the joint (cross) bilateral: one weight from all guide layers ---------------------
 * mid_bilateral_temporal's layered form runs one complete filter per layer with one colorSigma and adds them.  The joint filter
 * forms ONE weight per tap, the product of the spatial term and one range term per layer, each layer l with its own sigma_l:
 *   w(p, f, o) = exp(-0.5 |o|^2 / spatialSigma^2) * prod_l exp(-0.5 |G[t][l](p) - G[f][l](p+o)|^2_rgb / sigma_l^2)
 *   out_t(p)   = sum_{f, o} w * In_f(p+o)  /  sum_{f, o} w          (magenta (1,0,1,1) where the denominator is 0)
 * f = max(0,t-k) .. min(n_frames-1,t+k), o = (i, j) with |i|, |j| <= radius, l = 0 .. n_layers-1; out-of-image texels are
 * vec4(0) in frames and guides; only the centre G[t][l](p) comes from the target frame's layers.  One frame: n_frames = 1, k = 0.
 * There is no accumulate form: a product of weights cannot be chained through WeightInfo.
 * Everything else is mid_bilateral_temporal's layered form: frame-major tables of device pointers, the window rule ("only the
 * frames and layers of [first-k, first+count+k) are read"), out_format, the alias rules, the pointer limit
 * MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS, texture layout only, radius 1..24, the frames' format and -- through MID_FMT_WITH_GUIDE --
 * the guide format with the semantics of section a3 (IEEE values, alpha ignored, no clamping, non-finite texels by IEEE
 * arithmetic), RGBA16F guides 8-byte and RGBA32F guides 16-byte aligned.
 * layer_sigma: n_layers host floats, read during the call; NULL: every layer uses p->colorSigma.  Each entry must be > 0, as
 * colorSigma must (which is checked as well, also when it is not used).
 * Arithmetic: layer l is scaled by sc_l = (float)(sqrt(0.5 * log2 e) / (double)sigma_l); a guide value g enters as the fp32 product
 * g * sc_l, and the exponent of a tap is one chain of FMAs from the spatial term through layer 0's x, y, z, layer 1's, ...,
 * followed by one 2^x.  Per neighbour frame the taps are summed on their own and then added to the totals.
 * Precision: results are within 1e-5 * max(1, |ref|) of the formula in float64 while |g| <= 16 sigma_l for every layer l (as a3).
 * Bit identities:
 *   - n_layers == 1 with layer_sigma = {s}, or NULL and colorSigma = s: the bits of mid_bilateral_temporal's layered form with
 *     that layer and colorSigma = s, at every radius, k, frame, guide and output format;
 *   - appending all-zero layers (any sigmas) to a layer set leaves the bits, as long as both sets run tiled (below);
 *   - an RGBA16F guide gives the bits of the RGBA32F guide it widens to, an RGBA32F guide c/255 the bits of the RGBA8 guide c.
 * Classes: LDS-tiled while n_layers <= 4 and the colour tile (16 B per texel) plus n_layers guide tiles (12 B per texel) of
 * (64 + 2 radius) x (T + 2 radius) texels fit 160 KB -- T = 16 rows, 32 at radius 10, 8 at radius 20 -- which is every radius
 * <= 8 at n_layers <= 4, radius <= 9 at 3, radius <= 14 except 10 at 2; with one layer, the radii mid_bilateral_temporal's
 * layered form runs tiled (<= 17 and 20).  Radii 4, 8, 10 and 20 run on tuned kernels, the others on a run-time-radius one;
 * everything else -- n_layers > 4 included -- on a per-pixel kernel.
 * MID_ERR_INVALID before anything is queued, outputs untouched: n_layers outside 1..16 (an empty product would be a plain
 * Gaussian blur, so 0 is refused rather than given the magenta meaning); a NULL layer table; a sigma that is not > 0; and every
 * refusal of mid_bilateral_temporal's layered form. */
int mid_bilateral_joint(mid_ctx *ctx, const mid_bilateral_params *p, const float *layer_sigma /* n_layers host floats, or NULL */,
                        const void *const *frames /* host array of n_frames device ptrs */,
                        const uint32_t *const *layers /* host array of n_frames * n_layers device ptrs; cast RGBA16F / RGBA32F layers with MID_FMT_WITH_GUIDE */,
                        int n_layers, int n_frames, int k, int first, int count,
                        void *const *out /* host array of `count` device ptrs */, int out_format, void *stream);
/* mid_sequence_bilateral_temporal (section a8) with mid_bilateral_joint as the compute stage: host frames and host layers in,
 * host frames out, output t with the bits of mid_bilateral_joint for frame t.  Same ring, same layer ring (4 / 8 / 16 B per
 * texel), same direct-store rule, same refusals (a call inside a recording among them), same timings_ms and timeline export;
 * plus the refusals above, which leave host_out and timings_ms untouched. */
int mid_sequence_bilateral_joint(mid_ctx *ctx, const mid_bilateral_params *p, const float *layer_sigma,
                                 const void *const *host_frames, int n_frames, const void *const *host_layers, int n_layers,
                                 int k, int first, int count, void *const *host_out, int out_format, int overlap, float *timings_ms);

/* ---- a4f: joint layer-guided non-local means: one patch weight from all guide layers ---------
 * mid_nlm_layers_temporal runs one complete NLM pass per guide layer with one filteringParameter and adds them: a sample across
 * a depth edge is kept whenever the albedo patch happens to match.  The joint filter forms ONE weight per search offset from the
 * patch distances of all layers, each layer l with its own h_l.  Sequence of n_frames frames with n_layers RGBA8 layers each;
 * texels c/255; out-of-image texels are 0 in frames and guides:
 *   d_l(p,f,s) = sum_{q in patch} |G[t][l](p+q) - G[f][l](p+s+q)|^2_rgb
 *   w(p,f,s)   = exp( - sum_l d_l(p,f,s) / h_l^2 )
 *   out_t(p)   = sum_{f,s} w * In_f(p+s)  /  sum_f ( 0.001 + sum_s w )
 * f = max(0,t-k) .. min(n_frames-1,t+k), ascending; s over the search window; l = 0 .. n_layers-1; all four channels are
 * filtered; the 0.001 is added once per neighbour frame (nonlocal.comp:32-33), so one layer reproduces mid_nlm_layers_temporal.
 * One frame: n_frames = 1, k = 0.  There is no accumulate form, for the reason a4e gives: a product of weights cannot be chained
 * through WeightInfo.
 * Everything else is mid_nlm_layers_temporal's: frame-major tables of device pointers, the window rule ("only the frames and
 * layers of [first-k, first+count+k) are read"), out_format, the alignment and alias rules, the pointer limit
 * MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS, the window limits of the parameter checks of mid_nlm_accum -- a guide-format field in
 * p->format is refused there: layers are RGBA8 -- and non-finite texels by IEEE arithmetic.
 * layer_h: n_layers host floats, read during the call; NULL: every layer uses p->filteringParameter.  Each entry must be finite
 * and > 0, as filteringParameter must be > 0 (which is checked as well, also when it is not used), and the two factors of the
 * arithmetic below must be finite and > 0 in fp32: kd (h_0 between about 1e-21 and 1e16) and every r_l (h_0 / h_l between about
 * 4e-23 and 1.8e19).
 * Arithmetic: texels enter as their byte values, so a layer's squared differences and their patch sums are exact integers in
 * fp32.  The scale is applied relative to layer 0: the distance of an offset is D = D_0 + sum_{l>=1} r_l D_l with
 * r_l = (float)(h_0^2 / h_l^2) -- summed per texel before the box sums on the LDS-tiled kernels, per layer after them on the
 * per-pixel kernel -- and w = 2^(-D * kd), kd = (float)(log2 e / (255^2 h_0^2)), one multiplication and one exp2 per offset.
 * Precision: results are within 2e-5 * max(1, |ref|) of the formula in float64.
 * Bit identities:
 *   1. n_layers == 1 with layer_h = {h}, or NULL and filteringParameter = h: the bits of mid_nlm_layers_temporal with that layer
 *      and h, for every window class, k, frame format and output format, translucent frames included (the one-layer class keeps
 *      the layered kernel's tile shape and takes its opaque-tile vote per neighbour colour tile).
 *   2. appending all-zero layers (any h) to a layer set leaves the bits as long as both sets run in one class of the table
 *      below (2, 3 and 4 layers of a tuned window count as one: they share their tile shape and their arithmetic).  From one
 *      layer to two the tile shape changes, and with it the tiles that hold an out-of-image texel or a texel whose alpha is not 1
 *      and take the general form of the weight sums: there the two results may differ by the 5e-7 the opaque and the general
 *      form differ by (the last bit of normWeight), also on frames whose alpha is 1 everywhere -- at the pixels of tiles that
 *      reach over the image border.  From four layers to five the kernel changes (tiled to per pixel) and with it the order in
 *      which the offsets are added: only the precision bound holds across that step.
 *   3. out_format MID_FMT_RGBA8 / MID_FMT_RGBA16F gives mid_pack_u8 / mid_pack_f16 of the float result; output t of
 *      mid_sequence_nlm_joint has the bits of mid_nlm_joint for frame t.
 * Classes (every tiled class: eight waves per workgroup, 64 columns per wave, two waves per SIMD, no scratch):
 *   window               n_layers  rows per wave  tile rows  guide rings  packed target strips  LDS bytes
 *   21x21 / 7x7          1         8              64         float        0                     143136
 *   21x21 / 7x7          2         4              32         float        0                     108864
 *   21x21 / 7x7          3         4              32         packed       0                     128352
 *   21x21 / 7x7          4         4              32         packed       1                     147840
 *   14x14 / 6x6          1         8              64         float        0                     120120
 *   14x14 / 6x6          2         4              32         float        0                     86240
 *   14x14 / 6x6          3         4              32         packed       0                     101640
 *   14x14 / 6x6          4         4              32         packed       1                     117040
 * (21x21 / 7x7 = search [-10,11) patch [-3,4); 14x14 / 6x6 = search [-7,7) patch [-3,3)); every other window, n_layers > 4 and a
 * device whose LDS does not hold the tiles: one thread per pixel.
 * MID_ERR_INVALID before anything is queued, outputs untouched: n_layers outside 1..16 (0 is refused, as in the joint
 * bilateral); a NULL layer table; an h that is not finite and > 0, or outside the range above; and every refusal of mid_nlm_layers_temporal. */
int mid_nlm_joint(mid_ctx *ctx, const mid_nlm_params *p, const float *layer_h /* n_layers host floats, or NULL */,
                  const void *const *frames /* host array of n_frames device ptrs */,
                  const uint32_t *const *layers_rgba8 /* host array of n_frames * n_layers device ptrs */,
                  int n_layers, int n_frames, int k, int first, int count,
                  void *const *out /* host array of `count` device ptrs */, int out_format, void *stream);
/* mid_sequence_nlm_layers_temporal (section a8) with mid_nlm_joint as the compute stage: host frames and host RGBA8 layers in,
 * host frames out, output t with the bits of mid_nlm_joint for frame t.  Same ring, same layer ring (4 B per texel), same
 * direct-store rule, same refusals (a call inside a recording among them), same timings_ms and timeline export; plus the
 * refusals above, which leave host_out and timings_ms untouched. */
int mid_sequence_nlm_joint(mid_ctx *ctx, const mid_nlm_params *p, const float *layer_h,
                           const void *const *host_frames, int n_frames, const void *const *host_layers, int n_layers,
                           int k, int first, int count, void *const *host_out, int out_format, int overlap, float *timings_ms);

/* ---- a4g: the edge-avoiding a-trous filter guided by render layers -----------------------------
 * The bilateral family ends at radius 24 and costs (2 radius + 1)^2 taps.  The edge-avoiding a-trous wavelet filter (Dammertz et
 * al. 2010; the spatial stage of SVGF) reaches much further with the same guide layers: N passes of a 5x5 B3-spline kernel, pass
 * i sampling with holes at step s = 2^i.  Five passes reach +-62 pixels for 125 taps per pixel, eight reach +-510.
 * C_0 is the frame widened to fp32 (RGBA8 texels as c/255, as everywhere); G_l, l = 0 .. n_layers-1, are the frame's guide
 * layers; k1 = (1, 4, 6, 4, 1)/16 and K(o) = k1[i+2] k1[j+2] for o = (i, j), |i|, |j| <= 2.  Pass i, for q = p + s o:
 *   w(p,o)     = K(o) * prod_l exp(-0.5 |G_l(p) - G_l(q)|^2_rgb / sigma_l^2)
 *                     * [colorSigma > 0:  exp(-0.5 |C_i(p) - C_i(q)|^2_rgb / (colorSigma * 2^-i)^2)]
 *   C_{i+1}(p) = sum_o w C_i(q) / sum_o w          over the taps whose q lies inside the image
 * Taps outside the image are SKIPPED, not read as vec4(0) -- unlike the reference-derived filters, on purpose: at step 16 a zero
 * texel would darken a 32-pixel border.  The centre tap always counts, so the denominator is never 0 for finite inputs (there is
 * no magenta sentinel here).  All four colour channels are filtered; the colour term reads r, g, b.  Guide texels mean what
 * sections a3 / a4e say: IEEE values, alpha ignored, no clamping, non-finite texels by IEEE arithmetic (a NaN guide texel, or
 * Inf against Inf, poisons the pixels whose taps meet it; a skipped tap poisons nothing).
 * One frame per call; the form over neighbouring frames is section a4h.  p->first_pass is the ABSOLUTE index of the call's first pass (its step is
 * 2^first_pass), so a filter can be continued: passes [0, N) in one call are, bit for bit, N calls of one pass each with
 * first_pass = i through RGBA32F buffers.
 * Data path: the levels between passes are RGBA32F frames in `scratch` -- mid_atrous_scratch_bytes(p): 0 bytes for one pass
 * (NULL is accepted), one float frame for two passes, two for three and more; 16-byte aligned -- and the last pass stores
 * out_format, mid_pack_u8 / mid_pack_f16 of the float result.  p->format: the frame's MID_FMT_* and, through MID_FMT_WITH_GUIDE,
 * the guide format, as in a4e.  layer_sigma: n_layers host floats, read during the call; NULL is refused (there is no sigma to
 * fall back on: colorSigma belongs to the colour term, and 0 switches that off).
 * Arithmetic: layer l is scaled by sc_l = (float)(sqrt(0.5 log2 e) / (double)sigma_l) and a guide value g enters as the fp32
 * product g * sc_l; the colour differences are scaled by scc_i = (float)(sqrt(0.5 log2 e) / (colorSigma * 2^-i)).  The exponent
 * of a tap is one chain of FMAs that starts at 0: arg = fma(-d, d, arg) with d = G_l(p) sc_l - G_l(q) sc_l for layer 0's x, y,
 * z, then layer 1's, ..., then d = (C(p) - C(q)) scc_i for r, g, b; one 2^x follows and K(o) multiplies its result (K(o) is
 * exact in fp32).  The sums run over the taps in the order j = -2 .. 2 (rows), inside it i = -2 .. 2, each as
 * acc = fma(C(q), w, acc) and accw += w, and the pixel is acc / accw, an IEEE division per channel.  Every class computes
 * exactly this, so a pixel does not depend on the class that computed it.
 * Precision: within 1e-5 * max(1, |ref|) of the formula in float64, end to end over up to 8 passes, while |g| <= 16 sigma_l.
 * Bit identities:
 *   - the chain identity above;
 *   - an RGBA8 / RGBA16F frame gives the bits of the RGBA32F call on the widened frame, a half guide the bits of the float guide
 *     it widens to, a float guide c/255 (fp32 quotient) the bits of the RGBA8 guide c; RGBA8 / RGBA16F outputs are mid_pack_u8 /
 *     mid_pack_f16 of the float result;
 *   - appending all-zero layers (any sigmas) leaves the bits, and one live layer in any slot among zero layers gives the bits
 *     of that layer alone.
 * Classes (lanes run along x in all three; no scratch memory; eight waves per workgroup in the LDS classes):
 *   step     n_layers  kernel  tile     LDS tile   LDS bytes  workgroups per CU
 *   1        1         tiled   64 x 16  68 x 20    38080      4
 *   1        2         tiled   64 x 16  68 x 20    54400      3
 *   1        3         tiled   64 x 16  68 x 20    70720      2
 *   1        4         comb    64 x 8   68 x 12    52224      3
 *   2        1         tiled   64 x 16  72 x 24    48384      3
 *   2        2         tiled   64 x 16  72 x 24    69120      2
 *   2        3         comb    64 x 16  72 x 20    74880      2
 *   2        4         comb    64 x 8   72 x 12    55296      2
 *   4        1         comb    64 x 16  80 x 20    44800      3
 *   4        2         comb    64 x 16  80 x 20    64000      2
 *   4        3         comb    64 x 8   80 x 12    49920      3
 *   4        4         comb    64 x 8   80 x 12    61440      2
 *   8        1         comb    64 x 16  96 x 20    53760      3
 *   8        2         comb    64 x 16  96 x 20    76800      2
 *   8        3         comb    64 x 8   96 x 12    59904      2
 *   8        4         comb    64 x 8   96 x 12    73728      2
 *   16       1         comb    64 x 16  128 x 20   71680      2
 *   16       2         comb    64 x 8   128 x 12   61440      2
 *   16       3         comb    64 x 8   128 x 12   79872      2
 *   16       4         comb    64 x 8   128 x 12   98304      1
 *   32       1         comb    64 x 8   192 x 12   64512      2
 *   32       2         comb    64 x 8   192 x 12   92160      1
 *   32       3         comb    64 x 8   192 x 12   119808     1
 *   32       4         comb    64 x 8   192 x 12   147456     1
 *   1..32    5..16     global  64 x 4   -          0          -
 *   64, 128  1..16     global  64 x 4   -          0          -
 * tiled: a workgroup filters 64 x 16 pixels from LDS tiles of (64 + 4 step) x (16 + 4 step) texels -- the colour tile as float4,
 * three planes of floats per layer, already scaled, the guide format decoded when the tile is filled -- at steps 1 and 2 while two
 * such workgroups fit the 160 KB of a CU.  comb: the same tiles for rows of ONE residue class y = y0 (mod step), which form an
 * independent problem: the vertical halo is 4 rows at every step and only the horizontal halo (2 step columns on either side)
 * grows; 16 rows per workgroup while two workgroups fit a CU, else 8; every step up to 32 that is not tiled.  global: one pixel
 * per lane, the taps read from global memory.  The class follows from (step, n_layers) and the device's LDS size alone, never
 * from n_passes or first_pass.
 * MID_ERR_INVALID before anything is queued, outputs and scratch untouched: a NULL pointer (scratch only where bytes are needed);
 * n_layers outside 1..16; a sigma that is not finite and > 0; colorSigma < 0 or not finite; first_pass < 0, n_passes < 1 or
 * first_pass + n_passes > 8; an unknown frame, guide or output format; the alignment rules of a4e (scratch: 16 bytes); `out` or
 * `scratch` overlapping `in`, a layer or each other; width or height < 1, or 2^30 pixels and more. */
typedef struct mid_atrous_params {
    int32_t width, height;
    int32_t first_pass;   /* absolute index of the first pass, 0..7 */
    int32_t n_passes;     /* >= 1, first_pass + n_passes <= 8 */
    float   colorSigma;   /* 0: no colour term; otherwise > 0 and finite */
    int32_t format;       /* MID_FMT_* of the frame, guide format through MID_FMT_WITH_GUIDE as in a4e */
} mid_atrous_params;
size_t mid_atrous_scratch_bytes(const mid_atrous_params *p);
int mid_atrous_joint(mid_ctx *ctx, const mid_atrous_params *p, const float *layer_sigma /* n_layers host floats */, const void *in,
                     const uint32_t *const *layers /* host array of n_layers device ptrs; cast RGBA16F / RGBA32F layers with MID_FMT_WITH_GUIDE */,
                     int n_layers, void *out, int out_format, void *scratch, void *stream);
/* mid_sequence_bilateral_joint at k = 0 (section a8) with mid_atrous_joint as the compute stage: host frames and host layers in,
 * host frames out, output t with the bits of mid_atrous_joint for frame t.  Same ring, same layer ring (4 / 8 / 16 B per texel),
 * same direct-store rule, same refusals (a call inside a recording among them), same timings_ms and timeline export; plus the
 * refusals above, which leave host_out and timings_ms untouched.  The levels between passes live in the context's cache, one
 * set per kernel stream of the schedule, and are released with the rest (mid_ctx_release_cached). */
int mid_sequence_atrous_joint(mid_ctx *ctx, const mid_atrous_params *p, const float *layer_sigma,
                              const void *const *host_frames, int n_frames, const void *const *host_layers, int n_layers,
                              int first, int count, void *const *host_out, int out_format, int overlap, float *timings_ms);

/* ---- a4h: the a-trous filter over neighbouring frames -------------------------------------------
 * The temporal half of the filter of a4g, taken the way mid_bilateral_joint and mid_nlm_joint take temporal samples: no motion
 * vectors, the frames' own guide layers reject a neighbour's samples where the scene moved.  Pass 0 (step 1) of output frame t
 * takes its taps from every frame f of the window lo = max(0, t-k) .. hi = min(n_frames-1, t+k) (clipped at the sequence ends, as
 * in the other temporal forms); the centre always comes from frame t.  For q = p + o, o = (i, j), |i|, |j| <= 2:
 *   w(p,f,o)   = K(o) * prod_l exp(-0.5 |G[t][l](p) - G[f][l](q)|^2_rgb / sigma_l^2)
 *                     * [colorSigma > 0:  exp(-0.5 |C[t](p) - C[f](q)|^2_rgb / colorSigma^2)]
 *   C_1(p)     = sum_{f = lo..hi} sum_o w C[f](q) / sum_{f,o} w       over the taps whose q lies inside the image
 * Passes 1 .. n_passes-1 are a4g's, unchanged, on C_1 with frame t's layers: the temporal samples enter once and the later passes
 * filter the accumulated estimate (a temporal form of the later passes would need the levels of every neighbour).  Everything
 * else is a4g's: taps outside the image are skipped, all four channels are filtered, guide texels are IEEE values in the guide
 * format of MID_FMT_WITH_GUIDE, there is no magenta sentinel.
 * Arithmetic: a4g's chain with the centre from frame t and the tap from frame f -- arg starts at 0 and runs through layer 0's
 * x, y, z of d = G[t][l](p) sc_l - G[f][l](q) sc_l, then layer 1's, ..., then d = (C[t](p) - C[f](q)) scc_0 for r, g, b; one 2^x
 * follows, times the exact K(o).  ONE pair of accumulators runs across the whole window: frames in ascending order lo .. hi,
 * inside a frame j = -2 .. 2, then i = -2 .. 2, acc = fma(C[f](q), w, acc) and accw += w; one IEEE division per channel at the
 * end.  Every class computes exactly this per pixel, and with a window of one frame it is mid_atrous_joint's chain.
 * Precision: a4g's, within 1e-5 * max(1, |ref|) of the formula in float64 end to end.
 * Bit identities:
 *   - k = 0, or n_frames = 1 with any k, gives the bits of mid_atrous_joint for frame t;
 *   - neighbours whose every weight is exactly 0 leave the bits of k = 0;
 *   - N passes in one call are the temporal pass alone (n_passes = 1) into an RGBA32F buffer followed by mid_atrous_joint with
 *     first_pass = 1, n_passes = N - 1 on that buffer with frame t's layers;
 *   - the format and zero-layer identities of a4g.
 * frames / layers: frame-major tables as in mid_bilateral_joint (layers[f * n_layers + l]); the call produces outputs
 * [first, first + count) into out[0 .. count).  scratch: mid_atrous_scratch_bytes(p) bytes, 16-byte aligned, shared by all
 * outputs of the call, which run in stream order.  n_passes = 1 stores out_format directly.
 * Classes of the temporal pass (lanes run along x; no scratch memory; one neighbour's tiles are resident at a time, so the LDS
 * bytes are those of a4g's step-1 rows; the later passes have a4g's classes):
 *   layers 1       kernel tiled   pixels 64 x 16  LDS tile 68 x 20  bytes 38080  workgroups per CU 4 by LDS, 2 by registers
 *   layers 2       kernel tiled   pixels 64 x 16  LDS tile 68 x 20  bytes 54400  workgroups per CU 3 by LDS, 2 by registers
 *   layers 3       kernel tiled   pixels 64 x 16  LDS tile 68 x 20  bytes 70720  workgroups per CU 2
 *   layers 4       kernel tiled   pixels 64 x 8   LDS tile 68 x 12  bytes 52224  workgroups per CU 3
 *   layers 5..16   kernel global  pixels 64 x 4   no LDS
 * tiled: per neighbour the colour tile and the scaled guide planes are refilled (two barriers), the centres C[t](p) and
 * G[t][l](p) sc_l and the accumulators stay in registers.  global: one pixel per lane, every neighbour's taps from global memory.
 * The class follows from n_layers and the device's LDS size alone.
 * MID_ERR_INVALID before anything is queued, outputs and scratch untouched: every refusal of a4g; p->first_pass != 0 (the
 * temporal pass is pass 0; a filter is continued with mid_atrous_joint); n_frames < 1; k < 0;
 * min(2k+1, n_frames) * (n_layers + 1) > MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS; a bad output range; the NULL, alignment and alias
 * checks of the window [first - k, first + count - 1 + k] as in mid_bilateral_joint (an output that is a frame or layer of the
 * window, or given twice); scratch overlapping a frame or layer of the window or an output. */
int mid_atrous_joint_temporal(mid_ctx *ctx, const mid_atrous_params *p, const float *layer_sigma /* n_layers host floats */,
                              const void *const *frames /* host array of n_frames device ptrs */,
                              const uint32_t *const *layers /* host array of n_frames * n_layers device ptrs */,
                              int n_layers, int n_frames, int k, int first, int count,
                              void *const *out /* host array of `count` device ptrs */, int out_format, void *scratch, void *stream);
/* mid_sequence_atrous_joint with a window: mid_sequence_bilateral_joint's schedule at k (section a8) with
 * mid_atrous_joint_temporal as the compute stage -- each host frame and its layers are uploaded once, output t has the bits of
 * mid_atrous_joint_temporal for frame t.  Same ring, same layer ring (4 / 8 / 16 B per texel), same levels per kernel stream,
 * same direct-store rule, same refusals (a call inside a recording among them), same timings_ms and timeline export; plus the
 * refusals above, which leave host_out and timings_ms untouched. */
int mid_sequence_atrous_joint_temporal(mid_ctx *ctx, const mid_atrous_params *p, const float *layer_sigma,
                                       const void *const *host_frames, int n_frames, const void *const *host_layers, int n_layers,
                                       int k, int first, int count, void *const *host_out, int out_format, int overlap, float *timings_ms);

/* ---- a4i: the variance-guided a-trous filter ----------------------------------------------------
 * What gives SVGF its name: a per-pixel variance of the luminance steers the colour edge-stopping term of a4g's passes and is
 * filtered along with the colour.  a4g's only colour term is one global colorSigma halved every pass: too tight where a
 * path-traced frame is noisy, too loose where it has converged.  The term here is wide where the estimate is noisy and narrow
 * where it is not.  Two entry points: mid_atrous_moments estimates V_0, mid_atrous_variance runs the passes.
 * Luminance everywhere: l(C) = fma(0.0722f, b, fma(0.7152f, g, 0.2126f * r)) of the widened fp32 texel (RGBA8 texels c/255).
 *
 * (1) mid_atrous_moments.  For output frame t the window is f = max(0, t-k) .. min(n_frames-1, t+k), k >= 0, and in every frame
 * of it a 7x7 neighbourhood o = (i, j), |i|, |j| <= 3, is taken; taps outside the image are skipped.  With q = p + o:
 *   w(p,f,o) = prod_l exp(-0.5 |G[t][l](p) - G[f][l](q)|^2_rgb / sigma_l^2)                       (no spatial kernel)
 *   d        = l(C[f](q)) - l(C[t](p))       -- shifted by the centre's luminance, so that the subtraction below does not cancel
 *   W += w;  wd = w * d;  s1 += wd;  s2 = fma(wd, d, s2)     frames ascending, inside a frame j = -3 .. 3, then i = -3 .. 3
 *   m = s1 / W;  v = fma(-m, m, s2 / W);  V_0(p) = v < 0 ? 0 : v                                   (a NaN stays a NaN)
 * The layer exponent is a4g's FMA chain with the same sc_l, started at 0; w = 2^arg.  The centre tap has w = 1 and d = 0, so
 * W >= 1.  k = 0 is SVGF's spatial estimate; k > 0 the temporal one under this library's policy: no motion vectors, the layers
 * reject what moved.  var_out: one fp32 plane of width * height floats, 16-byte aligned.  frames / layers: frame-major tables as
 * in mid_atrous_joint_temporal (layers[f * n_layers + l]).  p->format: the frames' MID_FMT_* and, through MID_FMT_WITH_GUIDE,
 * the guide format.
 * Precision: |V - V_ref| <= 1e-5 * max(1, M2_ref), M2 = s2 / W in float64: both terms of v carry the rounding of a sum of that
 * size.  Bit identities: appended all-zero layers leave the bits; neighbour frames whose every weight is exactly 0 leave the
 * bits of k = 0; an RGBA8 / RGBA16F frame gives the bits of the float frame it widens to.
 * Classes (lanes run along x; no scratch memory; no register array indexed by a run-time value):
 *   layers 1       kernel tiled   pixels 64 x 16  LDS tile 70 x 22  bytes 24640  workgroups per CU 6 by LDS, 3 by registers
 *   layers 2       kernel tiled   pixels 64 x 16  LDS tile 70 x 22  bytes 43120  workgroups per CU 3
 *   layers 3       kernel tiled   pixels 64 x 16  LDS tile 70 x 22  bytes 61600  workgroups per CU 2
 *   layers 4       kernel tiled   pixels 64 x 16  LDS tile 70 x 22  bytes 80080  workgroups per CU 2
 *   layers 5..16   kernel global  pixels 64 x 4   no LDS
 * tiled: eight waves, two rows per wave; per neighbour frame the tile is refilled with ONE plane of luminances and 3 L planes of
 * scaled guide values (two barriers); the centres and the sums W, s1, s2 stay in registers.  global: one pixel per lane.
 * MID_ERR_INVALID before anything is queued, var_out untouched: a NULL pointer; n_layers outside 1..16; a sigma that is not
 * finite and > 0; an unknown frame or guide format; the alignment rules of a4e (var_out: 16 bytes); n_frames < 1, k < 0, t
 * outside [0, n_frames); var_out overlapping a frame or layer of the window;
 * min(2k+1, n_frames) * (n_layers + 1) > MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS; width or height < 1, or 2^30 pixels and more.
 *
 * (2) mid_atrous_variance.  Pass i at step s = 2^i over the colour level C_i and the variance plane V_i (V of the call's first
 * pass is var_in); K, k1, sc_l, the tap order and the skipped taps are a4g's.  For q = p + s o:
 *   vt(p)      = sum g(i) g(j) V_i(p + (i,j)) / sum g(i) g(j),  g = (1, 2, 1)/4, |i|, |j| <= 1 at step 1 whatever s, in-image
 *                taps only, j then i; num = fma(g g, V, num), den += g g, one IEEE division
 *   scv(p)     = (float)log2(e) / fma(sigmaLum, sqrtf(vt(p)), epsilon)         (IEEE sqrt and division, once per pixel)
 *   arg        = a4g's layer chain from 0, then  arg = fma(-|l(C_i(p)) - l(C_i(q))|, scv(p), arg)
 *   w          = K(o) * 2^arg,  0 for q outside the image;  order j = -2 .. 2, inside it i = -2 .. 2
 *   acc = fma(C_i(q), w, acc);  accw += w;  accv = fma(w * w, V_i(q), accv)
 *   C_{i+1}(p) = acc / accw (per channel);     V_{i+1}(p) = accv / (accw * accw)
 * that is, the luminance weight is SVGF's exp(-|dl| / (sigmaLum sqrt(vt) + epsilon)) and the variance of a weighted mean of
 * independent samples is propagated.  sigmaLum == 0 switches the luminance term off: vt is not read, the colour output has the
 * bits of mid_atrous_joint with colorSigma = 0, and the variance is still propagated.  Otherwise sigmaLum > 0 and finite (SVGF
 * uses 4) and epsilon > 0 and finite.
 * Why epsilon is a parameter and not SVGF's 1e-8: where vt = 0 the denominator IS epsilon.  Two texels of a level that differ
 * only by the rounding of earlier passes differ by about 1e-7 |l|; with a denominator below that resolution their weight is
 * exp(-10) or exp(0) by the toss of a coin, and so is the result -- in fp32 and in float64 alike, with different tosses.  epsilon
 * belongs well above the fp32 resolution of the luminances it meets: 1e-3 suits values of order 1.
 * Arguments: `in` the frame; var_in a const float plane; layers, layer_sigma, out, out_format as in a4g; var_out a float plane
 * for V of the last pass, or NULL: the last pass then stores no variance (a wave-uniform flag) and the colour bits are the same.
 * scratch: mid_atrous_variance_scratch_bytes(p) = (0, 1 or 2 for n_passes 1, 2, 3 and more) * (16 + 4) * width * height bytes,
 * 16-byte aligned, the RGBA32F colour levels first, then the float variance levels.  var_in / var_out: 16-byte aligned.
 * Chain identity: passes [0, N) in one call are, bit for bit, N one-pass calls with first_pass = i through RGBA32F buffers and
 * float planes; a launch knows its step and nothing of n_passes.
 * Precision: colour within 1e-5 * max(1, |ref|) and V within 1e-5 * max(1, max V_ref) of the formula in float64, end to end, on
 * inputs where the float64 formula itself is stable against fp32 rounding of its levels (see epsilon above).
 * Classes (lanes run along x; no scratch memory; eight waves per workgroup in the LDS class).  comb is a4g's row comb with one
 * plane more: float4 colour, one float of V and 3 L floats of scaled guides, 16 + 4 + 12 L bytes per texel; 16 rows per
 * workgroup while two workgroups fit a CU, else 8.  vt(p) is loaded by each lane from global memory, nine loads over three
 * rows: in a comb tile the rows y +- 1 belong to other residue classes.  There is no fixed-step tiled class.
 *   layers 1   step 1    kernel comb  pixels 64 x 16  LDS tile 68 x 20   bytes 43520   workgroups per CU 3
 *   layers 2   step 1    kernel comb  pixels 64 x 16  LDS tile 68 x 20   bytes 59840   workgroups per CU 2
 *   layers 3   step 1    kernel comb  pixels 64 x 16  LDS tile 68 x 20   bytes 76160   workgroups per CU 2
 *   layers 4   step 1    kernel comb  pixels 64 x 8   LDS tile 68 x 12   bytes 55488   workgroups per CU 2
 *   layers 1   step 2    kernel comb  pixels 64 x 16  LDS tile 72 x 20   bytes 46080   workgroups per CU 3
 *   layers 2   step 2    kernel comb  pixels 64 x 16  LDS tile 72 x 20   bytes 63360   workgroups per CU 2
 *   layers 3   step 2    kernel comb  pixels 64 x 16  LDS tile 72 x 20   bytes 80640   workgroups per CU 2
 *   layers 4   step 2    kernel comb  pixels 64 x 8   LDS tile 72 x 12   bytes 58752   workgroups per CU 2
 *   layers 1   step 4    kernel comb  pixels 64 x 16  LDS tile 80 x 20   bytes 51200   workgroups per CU 3
 *   layers 2   step 4    kernel comb  pixels 64 x 16  LDS tile 80 x 20   bytes 70400   workgroups per CU 2
 *   layers 3   step 4    kernel comb  pixels 64 x 8   LDS tile 80 x 12   bytes 53760   workgroups per CU 3
 *   layers 4   step 4    kernel comb  pixels 64 x 8   LDS tile 80 x 12   bytes 65280   workgroups per CU 2
 *   layers 1   step 8    kernel comb  pixels 64 x 16  LDS tile 96 x 20   bytes 61440   workgroups per CU 2
 *   layers 2   step 8    kernel comb  pixels 64 x 8   LDS tile 96 x 12   bytes 50688   workgroups per CU 3
 *   layers 3   step 8    kernel comb  pixels 64 x 8   LDS tile 96 x 12   bytes 64512   workgroups per CU 2
 *   layers 4   step 8    kernel comb  pixels 64 x 8   LDS tile 96 x 12   bytes 78336   workgroups per CU 2
 *   layers 1   step 16   kernel comb  pixels 64 x 16  LDS tile 128 x 20  bytes 81920   workgroups per CU 2
 *   layers 2   step 16   kernel comb  pixels 64 x 8   LDS tile 128 x 12  bytes 67584   workgroups per CU 2
 *   layers 3   step 16   kernel comb  pixels 64 x 8   LDS tile 128 x 12  bytes 86016   workgroups per CU 1
 *   layers 4   step 16   kernel comb  pixels 64 x 8   LDS tile 128 x 12  bytes 104448  workgroups per CU 1
 *   layers 1   step 32   kernel comb  pixels 64 x 8   LDS tile 192 x 12  bytes 73728   workgroups per CU 2
 *   layers 2   step 32   kernel comb  pixels 64 x 8   LDS tile 192 x 12  bytes 101376  workgroups per CU 1
 *   layers 3   step 32   kernel comb  pixels 64 x 8   LDS tile 192 x 12  bytes 129024  workgroups per CU 1
 *   layers 4   step 32   kernel comb  pixels 64 x 8   LDS tile 192 x 12  bytes 156672  workgroups per CU 1
 *   layers 5..16  step 1..32     kernel global  pixels 64 x 4  no LDS
 *   layers 1..16  step 64, 128   kernel global  pixels 64 x 4  no LDS
 * The class follows from (step, n_layers) and the device's LDS size alone; nothing is refused for LDS reasons: what does not
 * fit takes global taps.  Against a4g's table only (step 8, 2 layers) falls from 16 rows to 8 because of the extra plane.
 * MID_ERR_INVALID before anything is queued, out, var_out and scratch untouched: every refusal of a4g that applies (there is no
 * colorSigma); sigmaLum < 0 or not finite; with sigmaLum > 0, epsilon <= 0 or not finite; NULL var_in; var_in or var_out not
 * 16-byte aligned; `out`, var_out or `scratch` overlapping `in`, var_in, a layer or each other. */
typedef struct mid_atrous_moments_params {
    int32_t width, height;
    int32_t format;       /* MID_FMT_* of the frames, guide format through MID_FMT_WITH_GUIDE as in a4e */
} mid_atrous_moments_params;
int mid_atrous_moments(mid_ctx *ctx, const mid_atrous_moments_params *p, const float *layer_sigma /* n_layers host floats */,
                       const void *const *frames /* host array of n_frames device ptrs */,
                       const uint32_t *const *layers /* host array of n_frames * n_layers device ptrs */,
                       int n_layers, int n_frames, int k, int t, float *var_out, void *stream);
typedef struct mid_atrous_variance_params {
    int32_t width, height;
    int32_t first_pass;   /* absolute index of the first pass, 0..7 */
    int32_t n_passes;     /* >= 1, first_pass + n_passes <= 8 */
    float   sigmaLum;     /* 0: no luminance term; otherwise > 0 and finite */
    float   epsilon;      /* > 0 and finite where sigmaLum > 0 */
    int32_t format;       /* MID_FMT_* of the frame, guide format through MID_FMT_WITH_GUIDE as in a4e */
} mid_atrous_variance_params;
size_t mid_atrous_variance_scratch_bytes(const mid_atrous_variance_params *p);
int mid_atrous_variance(mid_ctx *ctx, const mid_atrous_variance_params *p, const float *layer_sigma /* n_layers host floats */,
                        const void *in, const float *var_in,
                        const uint32_t *const *layers /* host array of n_layers device ptrs; cast RGBA16F / RGBA32F layers with MID_FMT_WITH_GUIDE */,
                        int n_layers, void *out, int out_format, float *var_out, void *scratch, void *stream);
/* An animation through the frame pipeline (section a8) with the variance-guided filter as its compute stage:
 * mid_sequence_atrous_joint_temporal's schedule, where k is the window of the MOMENTS.  Per output frame t: mid_atrous_moments over
 * the window into a V_0 plane, then mid_atrous_variance (var_out = NULL) on frame t alone with frame t's layers; output t has the
 * bits of those two calls.  p->first_pass must be 0.  Each host frame and its layers are uploaded once.  The colour levels, the
 * variance levels and the V_0 plane live in the context's cache, one set per kernel stream, and are released with the rest
 * (mid_ctx_release_cached).  Same ring, same layer ring, same direct-store rule, same refusals (a call inside a recording among
 * them), same timings_ms and timeline export as the other stages; plus the refusals of both calls, which leave host_out and
 * timings_ms untouched. */
int mid_sequence_atrous_variance(mid_ctx *ctx, const mid_atrous_variance_params *p, const float *layer_sigma,
                                 const void *const *host_frames, int n_frames, const void *const *host_layers, int n_layers,
                                 int k, int first, int count, void *const *host_out, int out_format, int overlap, float *timings_ms);

/* ---- a4j: recursive temporal accumulation with motion vectors -----------------------------
 * SVGF's temporal stage: a history of the colour and of the luminance moments that lives from frame to frame, reprojected by
 * per-pixel motion vectors and blended with the new frame as lerp(history, frame, max(1 / N, alpha)) with a per-pixel history
 * length N.  Where a window of 2k+1 frames (a4h, a4i) gives 2k+1 samples per pixel for a pass over 2k+1 frames, the recursion
 * gives 1 / alpha samples for one frame's worth of traffic.  The policy of the other temporal forms is kept: the guide layers
 * weigh every history tap softly, there is no disocclusion threshold.  Motion vectors are an OPTIONAL input: without them the
 * reprojection is the identity and the layers alone reject what moved.
 * Planes.  hist_color_in / color_out: RGBA32F.  hist_state_in / state_out: one float4 per pixel, (m1, m2, N, 0) -- the first and
 * second moment of the luminance and the history length, one 16-byte load per reprojection tap.  motion: width * height float2,
 * 8-byte aligned, in pixels: pixel p of this frame was at p + motion(p) in the previous frame; NULL = zero motion.  var_spatial,
 * var_out: a4i's float planes (var_spatial is mid_atrous_moments at k = 0 of this frame, or NULL; var_out may be NULL).  cur is
 * widened as in a4i and l() is a4i's luminance; cur_layers are this frame's guide layers, prev_layers those of the frame the
 * history belongs to (both tables are required with n_layers > 0, also where there is no history).
 * Per pixel p = (x, y), C = cur(p) widened, l = l(C), Hc / Hs the history colour / state, Vs = var_spatial(p):
 *   1. previous position: ppx = (float)x + mx (one fp32 add), x0 = floorf(ppx), fx = ppx - x0 (exact); likewise y.
 *   2. taps are taken only if ppx > -1 && ppx < width && ppy > -1 && ppy < height, compared in fp32 BEFORE any float -> int
 *      conversion: false for NaN and +-Inf, and such a pixel has no history.  motion == NULL: pp = p exactly.
 *   3. the four taps q = (x0 + a, y0 + b) in the order b = 0, 1, inside it a = 0, 1; bw = (a ? fx : 1 - fx) * (b ? fy : 1 - fy).
 *      A tap outside the image or with bw == 0 is SKIPPED -- not read: integer motion reads one texel, nothing leaks in from
 *      beyond the frame.  For the others: arg = a4g's layer chain from 0 between cur_layers[l](p) and prev_layers[l](q), same
 *      sc_l;  w = bw * 2^arg;  S += w;  hc = fma(Hc(q), w, hc) (four channels);  h1 = fma(Hs(q).x, w, h1),
 *      h2 = fma(Hs(q).y, w, h2), hn = fma(Hs(q).z, w, hn).
 *   4. S > 0: hc /= S, h1 /= S, h2 /= S (IEEE divisions); otherwise all are 0 (this includes a call without history).
 *   5. N' = fminf(historyMax, hn + 1.0f): hn is the UNNORMALISED sum (sum bw <= 1 and every 2^arg <= 1), so a history that is
 *      only half believed counts half and N' falls to 1 continuously as S -> 0.
 *   6. a = fmaxf(1.0f / N', alpha);  color_out = fma(a, C - hc, hc) per channel.
 *   7. am = fmaxf(1.0f / N', alphaMoments);  m1' = fma(am, l - h1, h1);  m2' = fma(am, l * l - h2, h2);
 *      state_out = (m1', m2', N', 0).
 *   8. v = fma(-m1', m1', m2');  Vt = v < 0 ? 0 : v (a NaN stays).  With var_spatial: tt = fminf(1, (N' - 1) / (historyFull - 1)),
 *      var_out = fma(tt, Vt - Vs, Vs) -- SVGF's "spatial estimate while the history is short", made continuous; else var_out = Vt.
 * Out of scope: SVGF's 3 x 3 search when the bilinear taps fail, mesh ids, and a temporal falloff of the weights.
 * The tap geometry (steps 1 - 3 up to bw and the skip rule) is one host / device function, csrc/reproject_taps.hpp, which
 * tools/reproject_taps_sanitize.cpp sweeps on the CPU under sanitizers.
 * Precision: colour, m1, m2 within 1e-5 * max(1, |ref|), N' within 1e-5 * max(1, N'), the variance within 1e-5 * max(1, m2_ref)
 * of the formula in float64 with steps 1 - 2 taken in fp32 (both terms of v carry the rounding of a value of that size).  Bit
 * identities: no history gives the widened cur, the state (l, l * l, 1, 0) and var_out == var_spatial; motion == NULL is an
 * all-zero motion plane; a u8 / f16 frame gives the bits of the float frame it widens to; appended all-zero layers leave the bits.
 * Class: one kernel, one pixel per lane, 64 x 4 pixels per workgroup of four waves, no LDS (the tap addresses depend on the
 * data; motion is locally coherent, so neighbouring lanes' taps share cache lines), no scratch memory, no register array indexed
 * by a run-time value; the layer loop is wave-uniform; 2 n_layers + 8 pointers by value.
 * MID_ERR_INVALID before anything is queued, the outputs untouched: NULL cur, color_out or state_out; exactly one of the two
 * history inputs NULL; n_layers outside 0..16; with layers a NULL table, a NULL entry, or a sigma that is not finite and > 0;
 * alpha or alphaMoments outside (0, 1] or not finite; historyMax < 1 or not finite; historyFull <= 1 or not finite; an unknown
 * frame or guide format; the alignment rules of a4e (motion: 8 bytes; histories, states and variance planes: 16 bytes); any
 * output overlapping any input or another output (color_out may not be hist_color_in: the gather reads neighbours); width or
 * height < 1, or 2^30 pixels and more. */
typedef struct mid_temporal_accum_params {
    int32_t width, height;
    float   alpha;          /* floor of the colour blend factor, (0, 1]; SVGF 0.2 */
    float   alphaMoments;   /* floor of the moments' blend factor, (0, 1]; SVGF 0.2 */
    float   historyMax;     /* cap of the history length N, >= 1, finite; default 32 */
    float   historyFull;    /* N from which the temporal variance is used alone, > 1, finite; SVGF 4 */
    int32_t format;         /* MID_FMT_* of `cur`, guide format through MID_FMT_WITH_GUIDE as in a4e */
} mid_temporal_accum_params;
int mid_temporal_accumulate(mid_ctx *ctx, const mid_temporal_accum_params *p, const float *layer_sigma /* n_layers host floats */,
                            const void *cur, const uint32_t *const *cur_layers, const uint32_t *const *prev_layers, int n_layers /* 0..16 */,
                            const float *motion /* width*height float2, or NULL = zero motion */,
                            const mid_pixel *hist_color_in, const mid_pixel *hist_state_in /* both NULL: no history */,
                            const float *var_spatial /* float plane or NULL */,
                            mid_pixel *color_out, mid_pixel *state_out, float *var_out /* or NULL */, void *stream);
/* An animation through the frame pipeline (section a8) with the recursion as its compute stage.  For t from s = max(0, first -
 * warmup) on, in order: (1) Vs = mid_atrous_moments at k = 0 on frame t with its layers; (2) mid_temporal_accumulate with cur = t,
 * the layers of t and of t-1, host_motion[t], the history frame t-1 left and Vs -- frame s has no history; (3) mid_atrous_variance
 * (vp, first_pass 0) on the accumulated colour and var_out with frame t's layers.  feedback 0: the colour history of frame t+1 is
 * the accumulated colour.  feedback 1 (SVGF's choice): it is the level after pass 0 -- pass 0 is run on its own into the next
 * history buffer and passes 1.. continue from it with first_pass = 1, which is a4i's chain identity, so the bits stay those of the
 * public calls.  Frames s .. first-1 are warm-up: computed, neither stored nor downloaded; host_out has `count` entries.  Output t
 * has, bit for bit, the result of that chain of public calls started at frame s -- so a call with first > 0 (a frame block of a
 * sharded run) equals the whole run bit for bit only when warmup reaches frame 0.
 * host_motion: n_frames planes of width * height float2 (as in mid_temporal_accumulate), or NULL: zero motion; a plane rides in
 * its frame's upload interval.  ap and vp must agree on width, height and format.  The launches of consecutive frames run IN
 * ORDER on one kernel stream (the other stages alternate between two); uploads and downloads overlap them as elsewhere.  The two
 * histories (ping-pong), Vs, var_out and the levels live in the context's cache and go with mid_ctx_release_cached.
 * MID_ERR_INVALID before anything is queued, host_out and timings_ms untouched: the refusals of the three calls and of the other
 * sequence entry points; vp->first_pass != 0; feedback outside {0, 1}; warmup < 0; a NULL frame, layer or motion plane among the
 * frames max(0, s-1) .. min(n_frames-1, first+count); an output that is one of those. */
int mid_sequence_atrous_recursive(mid_ctx *ctx, const mid_temporal_accum_params *ap, const mid_atrous_variance_params *vp,
                                  const float *layer_sigma, const void *const *host_frames, int n_frames,
                                  const void *const *host_layers, int n_layers /* 1..16 */,
                                  const void *const *host_motion /* n_frames float2 planes, or NULL */, int feedback /* 0 | 1 */,
                                  int warmup /* >= 0 */, int first, int count, void *const *host_out, int out_format, int overlap,
                                  float *timings_ms);

/* ---- a4k: albedo demodulation ---------------------------------------------------------------
 * SVGF filters ILLUMINATION, not colour: the noisy radiance is divided by the surface albedo before it is accumulated and
 * filtered, and the albedo is multiplied back at the end.  A texture then neither stops the filter (as it does when the albedo is
 * a guide layer) nor is blurred away (as it is when the albedo is left out).  Two streaming passes:
 *   mid_demodulate  I = C / max(A, floor)     `in` a frame in the frame format of p->format, `out` RGBA32F
 *   mid_modulate    O = I * max(A, floor)     `in` RGBA32F (any other frame format in p->format is refused), `out` in out_format
 * p->format is a MID_FMT_WITH_GUIDE word: the frame format RGBA8, RGBA16F or RGBA32F, and the format of the albedo plane in the
 * guide field.  The albedo is read exactly as a guide texel is (a3 / a4e): IEEE values, alpha ignored, no clamping, RGBA8 texels
 * the correctly rounded c / 255.  C is widened as a4i widens a frame.
 * Per pixel and per channel c in {R, G, B}:  d_c = fmaxf(A_c, floor)  -- a NaN or negative albedo therefore gives floor --
 *   demodulate: I_c = C_c / d_c, one IEEE division;      modulate: O_c = I_c * d_c, one multiplication;
 * alpha passes through unchanged in both.  mid_modulate writes out_format with the packing rules of mid_pack_u8 / mid_pack_f16
 * (a6); its `out` may be page-locked host memory addressed from the device, which is how the frame pipeline stores its final
 * output.  Everything else is IEEE arithmetic, nothing is clamped: a NaN or Inf colour stays one; an albedo of +Inf demodulates
 * to 0 (of a finite colour) and modulates 0 * Inf to NaN, so an infinite albedo does NOT round-trip; an albedo below floor
 * round-trips (both passes use floor) but the illumination is C / floor, not C / A.
 * floor must be finite and > 0; every higher layer defaults to 1e-3, the usual choice of SVGF implementations.  It is a parameter
 * for the reason a4i gives for epsilon: what counts as "no albedo" depends on the renderer's units.
 * Precision: the bits of the formulas in IEEE binary32 (the build keeps -ffp-contract=off and uses no fast-math flag) -- those of
 * numpy float32.  modulate(demodulate(C)) is within 2^-22 |C| of C for normal-range values: two roundings.
 * Class: pointwise (a5 / a6): one pixel per lane, a 16 / 8 / 4-byte load of the frame and one of the albedo, grid-stride (at most
 * 8 workgroups of 256 lanes per CU), index arithmetic in size_t, the formats run-time wave-uniform values, no LDS, no scratch.
 * MID_ERR_INVALID before anything is queued, `out` untouched: a NULL pointer; floor not finite or <= 0; an unknown frame, guide or
 * output format; the alignment rules of a4e, each plane to its texel size (4 / 8 / 16 bytes); width or height < 1, or 2^30 pixels
 * and more; `out` overlapping `albedo`; `out` overlapping `in` -- except exactly in place with equal texel size (RGBA32F to
 * RGBA32F), which is allowed because the pass is pointwise. */
typedef struct mid_albedo_params {
    int32_t width, height;
    float   floor;        /* lower bound of the divisor, finite and > 0; default 1e-3 */
    int32_t format;       /* MID_FMT_WITH_GUIDE(frame format, albedo format); mid_modulate: the frame format must be RGBA32F */
} mid_albedo_params;
int mid_demodulate(mid_ctx *ctx, const mid_albedo_params *p, const void *in, const void *albedo, mid_pixel *out, void *stream);
int mid_modulate(mid_ctx *ctx, const mid_albedo_params *p, const mid_pixel *in, const void *albedo, void *out, int out_format,
                 void *stream);
/* mid_sequence_atrous_recursive with an albedo plane per frame.  host_albedo == NULL: it IS that call (albedo_floor is not read),
 * and that entry point is this one with NULL.  Otherwise host_albedo holds n_frames host planes in the guide format of ap->format
 * (they obey the layers' format) and, per frame t: (0) mid_demodulate of frame t with host_albedo[t] into an RGBA32F plane;
 * (1) - (3) of mid_sequence_atrous_recursive on that plane (frame format RGBA32F), the passes' final level written as RGBA32F;
 * (4) mid_modulate of that level with host_albedo[t] into host_out in out_format -- the kernel-stored output of the pipeline
 * where the other stages' last pass stores it.  The histories and both feedback forms stay in illumination space.  Output t has,
 * bit for bit, the result of that chain of public calls.  An albedo plane is one more side slot of its frame, after the layers
 * and the motion plane, uploaded in the frame's upload interval.  The block of the context's cache grows by two RGBA32F planes
 * (32 B per pixel) to 164 B per pixel.
 * MID_ERR_INVALID before anything is queued, host_out and timings_ms untouched: the refusals of mid_sequence_atrous_recursive;
 * albedo_floor not finite or <= 0; a NULL albedo plane among the frames max(0, s-1) .. min(n_frames-1, first+count); an output
 * that is one of those planes. */
int mid_sequence_atrous_recursive_albedo(mid_ctx *ctx, const mid_temporal_accum_params *ap, const mid_atrous_variance_params *vp,
                                         const float *layer_sigma, const void *const *host_frames, int n_frames,
                                         const void *const *host_layers, int n_layers /* 1..16 */,
                                         const void *const *host_motion /* n_frames float2 planes, or NULL */,
                                         const void *const *host_albedo /* n_frames planes in the guide format, or NULL */,
                                         float albedo_floor, int feedback /* 0 | 1 */, int warmup /* >= 0 */, int first, int count,
                                         void *const *host_out, int out_format, int overlap, float *timings_ms);

/* ---- a4l: firefly clamp and NaN repair --------------------------------------------------------
 * Every stage of the recursive chain is IEEE arithmetic in which a NaN stays a NaN (a4i, a4j, a4k).  Fed by a path tracer that is
 * the wrong behaviour for the chain as a whole: one NaN or Inf texel enters the histories, is spread +-62 pixels by five passes
 * and, with feedback 1, never leaves; a finite outlier of 10^3 - 10^4 x its surroundings opens the luminance term of a4i where it
 * sits and is smeared into a blob that the history keeps for about 1 / alpha frames.  mid_firefly_clamp is the outlier clamp that
 * production SVGF puts in front of the temporal stage: one pass that limits the luminance of every pixel by that of its
 * neighbourhood and repairs non-finite pixels from it.
 * Per pixel p, with C the texel widened as a4i widens a frame and l() a4i's luminance, literally
 * fma(0.0722f, b, fma(0.7152f, g, 0.2126f * r)):
 *   neighbours  q = p + (i, j), |i|, |j| <= radius, (i, j) != (0, 0), q inside the image.  A neighbour is VALID iff l(C(q)) is
 *               finite (NaN and +-Inf fail); n is the number of valid neighbours.
 *   n == 0      (a 1 x 1 frame, or a surrounding that is all non-finite): out = C in all four channels.
 *   limit       m = the min(rank, n)-th largest valid neighbour luminance, as a multiset (equal values count separately);
 *               T = fmaxf(gain * m, floor): one multiplication and one fmaxf; T >= 0.
 *   centre      lc = l(C(p)).   lc finite and lc <= T: out = C, bit for bit.
 *               lc finite and lc > T: s = T / lc (one IEEE division), out_c = C_c * s for c in {R, G, B} (one multiplication each).
 *               lc not finite (which is the case exactly when a colour channel is non-finite): out_R = out_G = out_B = T -- the
 *               pixel is repaired to a grey of the limit luminance.
 *   alpha       passes through unchanged in every case.  A non-finite ALPHA is not repaired.
 * One pass, no iteration: every limit is taken from the INPUT's luminances, so the result depends on no evaluation order, and the
 * selection is exact (max and min only).  Precision: the bits of the formulas in IEEE binary32 (-ffp-contract=off, no fast-math)
 * -- those of a numpy float32 evaluation; NaN payloads and signs are left open, as in a4k.
 * Identity: a frame that is constant apart from one texel whose RGB is 4096 x its surroundings comes back, with rank 1, gain 1,
 * floor 0, as the constant frame bit for bit (s is exactly 2^-12).  Two such texels side by side survive rank 1 -- each is the
 * other's maximum -- and are removed by rank 2; a 2 x 2 block of them needs rank 4.
 * floor is a luminance that is always let through, in the units of `in`: in the frame pipeline the clamp runs AFTER
 * demodulation, so there it is in illumination units.
 * Class: tiled (csrc/firefly.hip): a workgroup of four waves covers 64 x 16 pixels from an LDS tile of
 * (64 + 2 radius) x (16 + 2 radius) luminances; index arithmetic in size_t.
 * MID_ERR_INVALID before anything is queued, `out` untouched: a NULL pointer; radius outside {1, 2}; rank outside 1..4; gain not
 * finite or <= 0; floor not finite or < 0; an unknown frame format, or guide bits set in format; `in` not aligned to its texel
 * size, `out` not to 16 bytes; width or height < 1, or 2^30 pixels and more; `out` overlapping `in` in any way -- the pass is a
 * stencil, so exactly in place is refused too, unlike a4k. */
typedef struct mid_firefly_params {
    int32_t width, height;
    int32_t radius;   /* 1 | 2: 3x3 or 5x5 neighbourhood, centre excluded */
    int32_t rank;     /* 1..4: the k-th largest neighbour luminance is the limit */
    float   gain;     /* finite, > 0; default 1 */
    float   floor;    /* finite, >= 0; a luminance always let through; default 0 */
    int32_t format;   /* MID_FMT_* of `in`; the guide field must be 0 */
} mid_firefly_params;
int mid_firefly_clamp(mid_ctx *ctx, const mid_firefly_params *p, const void *in, mid_pixel *out /* RGBA32F */, void *stream);
/* mid_sequence_atrous_recursive_albedo with the clamp in front of the chain.  fp == NULL: it IS that call, and that entry point is
 * this one with NULL.  Otherwise, per frame t: (0) mid_demodulate, if there is an albedo; (0') mid_firefly_clamp into one more
 * RGBA32F plane of the cache block -- it reads the illumination plane as RGBA32F, or the frame itself in the frames' format;
 * (1) - (3) on that plane with frame format RGBA32F; (4) mid_modulate, if there is an albedo.  The clamp runs AFTER demodulation:
 * fp->floor is in illumination units.  Output t has, bit for bit, the result of that chain of public calls.  The cache block grows
 * by 16 B per pixel: 148 B per pixel without albedo, 180 with.  No new host plane, side slot or upload; everything runs on the one
 * in-order kernel stream.
 * MID_ERR_INVALID before anything is queued, host_out and timings_ms untouched: the refusals of
 * mid_sequence_atrous_recursive_albedo; those of mid_firefly_clamp's parameters; fp->width / fp->height other than ap's; fp->format
 * other than the frames' format with no guide bits (both values are named). */
int mid_sequence_atrous_recursive_firefly(mid_ctx *ctx, const mid_temporal_accum_params *ap, const mid_atrous_variance_params *vp,
                                          const float *layer_sigma, const void *const *host_frames, int n_frames,
                                          const void *const *host_layers, int n_layers /* 1..16 */,
                                          const void *const *host_motion /* n_frames float2 planes, or NULL */,
                                          const void *const *host_albedo /* n_frames planes in the guide format, or NULL */,
                                          float albedo_floor, const mid_firefly_params *fp /* NULL: no clamp */,
                                          int feedback /* 0 | 1 */, int warmup /* >= 0 */, int first, int count,
                                          void *const *host_out, int out_format, int overlap, float *timings_ms);

/* ---- a4m: history clipping -------------------------------------------------------------------
 * mid_temporal_accumulate rejects history only through the guide layers; there is deliberately no disocclusion threshold (a4j).
 * When the lighting changes and the geometry does not -- a light switching, a moving shadow, a reflection, an emissive texture --
 * every layer says "same surface", the history is fully believed and the output carries a ghost of the old lighting that decays
 * as (1 - alpha)^j.  The firefly clamp (a4l) bounds the current frame by its neighbourhood; history clipping bounds the HISTORY by
 * the current frame: neighbourhood variance clipping of the reprojected history (Salvi 2016), the "history clamping" or "anti-lag"
 * of SVGF's production descendants.  Two pieces: mid_color_bounds computes a colour box per pixel from the current frame, and
 * mid_temporal_accumulate_clip clips the normalised history to it before the blend.
 *
 * mid_color_bounds.  Per pixel p, with C the texel widened as a4i widens a frame:
 *   window    q = p + (i, j), |i|, |j| <= radius, the centre INCLUDED, q inside the image.  q is VALID iff R, G and B of C(q) are all
 *             finite (fabsf(c) < INFINITY); n is the number of valid q.
 *   n == 0    lo.rgb = -INFINITY, hi.rgb = +INFINITY: nothing will be clipped.
 *   else      per channel c over the valid q:  mu = (sum v) / n, rounded to fp32;  var = (sum (v - mu)^2) / n -- the TWO-PASS form:
 *             the one-pass E[v^2] - mu^2 loses everything on flat HDR regions;  sigma = sqrtf(var);
 *             lo_c = fmaf(-gamma, sigma, mu);  hi_c = fmaf(gamma, sigma, mu).
 *   alpha     lo.w = hi.w = (float)n.  Alpha is never clipped.
 * The order of the sums inside the window is the kernel's own: the sum of the mean is taken in binary64 and the quotient rounded
 * once to fp32, so a window of one repeated value v has mu == v, var == 0 and lo == hi == v bit for bit, whatever v is; the
 * deviations, their squares (one fma each) and their sum are fp32.  Scaling the frame by a power of two scales lo and hi by it,
 * bit for bit, while nothing leaves the normal range.  A window whose deviations overflow when squared (|v - mu| >= 2^64) has
 * sigma = +Inf: the box is everything, or NaN -- which clips nothing either -- for gamma == 0.
 * Precision: lo and hi within 1e-5 * max(1, |mu| + gamma sigma) of the formula in float64 with mu rounded to fp32; .w exact.
 * Class: tiled (csrc/color_bounds.hip): the firefly clamp's geometry (csrc/firefly_tile.hpp), a workgroup of four
 * waves covers 64 x 16 pixels from an LDS tile of (64 + 2 radius) x (16 + 2 radius) x 3 floats; index arithmetic in size_t.
 * MID_ERR_INVALID before anything is queued, `lo` and `hi` untouched: a NULL pointer; radius outside {1, 2}; gamma not finite or
 * < 0; an unknown frame format, or guide bits set in format; `in` not aligned to its texel size, `lo` or `hi` not to 16 bytes;
 * width or height < 1, or 2^30 pixels and more; `lo` or `hi` overlapping `in`, or each other. */
typedef struct mid_color_bounds_params {
    int32_t width, height;
    int32_t radius;   /* 1 | 2: 3x3 or 5x5 window, centre INCLUDED */
    float   gamma;    /* finite, >= 0: half-width of the box in standard deviations; default 1 */
    int32_t format;   /* MID_FMT_* of `in`; guide bits must be 0 */
} mid_color_bounds_params;
int mid_color_bounds(mid_ctx *ctx, const mid_color_bounds_params *p, const void *in, mid_pixel *lo /* RGBA32F */,
                     mid_pixel *hi /* RGBA32F */, void *stream);
/* mid_temporal_accumulate with a clip box.  clip_lo == clip_hi == NULL: it IS mid_temporal_accumulate, and that entry point is this
 * one with NULL.  Otherwise both are width * height RGBA32F planes (mid_color_bounds of `cur`, usually) and, after step 4 of a4j
 * where S > 0 (with S == 0 nothing changes), per channel c in {R, G, B}, literally:
 *   hc'_c = hc_c < lo_c ? lo_c : (hc_c > hi_c ? hi_c : hc_c)      -- a NaN hc stays NaN; a NaN bound clips nothing
 *   d   = l(hc') - l(hc)                                           -- a4i's luminance on (x, y, z), both fma chains
 *   h1' = h1 + d
 *   h2' = fmaf(d, fmaf(2.0f, h1, d), h2)                           -- the mean moves by d, the variance h2 - h1^2 stays
 * hc.w and hn (and so N') are unchanged; steps 5 - 8 read hc', h1' and h2'.  Where nothing is clipped d is exactly 0 and the bits
 * are those of the unclipped call.  lo > hi is not refused: the formula is taken literally (hc < lo gives lo).  The `.w` of the
 * planes is not read.  Precision and class as a4j: a compile-time variant of the same kernel, two more 16-byte loads per pixel.
 * MID_ERR_INVALID, the outputs untouched: the refusals of mid_temporal_accumulate; exactly one of the two planes NULL; a plane
 * not 16-byte aligned; any output overlapping a clip plane. */
int mid_temporal_accumulate_clip(mid_ctx *ctx, const mid_temporal_accum_params *p, const float *layer_sigma /* n_layers host floats */,
                                 const void *cur, const uint32_t *const *cur_layers, const uint32_t *const *prev_layers,
                                 int n_layers /* 0..16 */, const float *motion /* width*height float2, or NULL = zero motion */,
                                 const mid_pixel *hist_color_in, const mid_pixel *hist_state_in /* both NULL: no history */,
                                 const float *var_spatial /* float plane or NULL */,
                                 const mid_pixel *clip_lo, const mid_pixel *clip_hi /* both NULL: no clip */,
                                 mid_pixel *color_out, mid_pixel *state_out, float *var_out /* or NULL */, void *stream);
/* mid_sequence_atrous_recursive_firefly with the history clipped.  cp == NULL: it IS that call, and that entry point is this one
 * with NULL.  Otherwise, per frame t: after (0) the demodulation and (0') the firefly clamp, mid_color_bounds (cp's radius and
 * gamma) runs on THE PLANE THE ACCUMULATION READS -- the frame itself in the frames' format, or the illumination / clamped plane as
 * RGBA32F -- into two more RGBA32F planes of the cache block (32 B per pixel more), and step (2) is mid_temporal_accumulate_clip
 * with them.  The box is computed for frame s too, whose accumulation has no history and clips nothing: the schedule is the same
 * for every frame.  Output t has, bit for bit, the result of that chain of public calls.  No new host plane, side slot or upload;
 * everything runs on the one in-order kernel stream.  A frame block of a sharded run needs nothing new: the box comes from the
 * frame itself.
 * MID_ERR_INVALID before anything is queued, host_out and timings_ms untouched: the refusals of
 * mid_sequence_atrous_recursive_firefly; those of mid_color_bounds's parameters; cp->width / cp->height other than ap's; cp->format
 * other than the frames' format with no guide bits (both values are named). */
int mid_sequence_atrous_recursive_clip(mid_ctx *ctx, const mid_temporal_accum_params *ap, const mid_atrous_variance_params *vp,
                                       const float *layer_sigma, const void *const *host_frames, int n_frames,
                                       const void *const *host_layers, int n_layers /* 1..16 */,
                                       const void *const *host_motion /* n_frames float2 planes, or NULL */,
                                       const void *const *host_albedo /* n_frames planes in the guide format, or NULL */,
                                       float albedo_floor, const mid_firefly_params *fp /* NULL: no clamp */,
                                       const mid_color_bounds_params *cp /* NULL: no history clip */,
                                       int feedback /* 0 | 1 */, int warmup /* >= 0 */, int first, int count,
                                       void *const *host_out, int out_format, int overlap, float *timings_ms);

/* ---- a4n: full-reference image quality metrics ------------------------------------------------
 * What tells one setting of the chain above from another: the distance of a test image `a` from a reference image `b` (a
 * converged render, usually) as MSE, PSNR, MAE, the largest difference, relMSE and SSIM.  The sums are taken on the GPU by a
 * reduction whose bits depend on the inputs and the parameters alone; the definitions of the derived values are one host function.
 * a and b have p->width x p->height texels, each in its own format (MID_FMT_RGBA8 | RGBA16F | RGBA32F, no guide bits); alpha is
 * ignored; a == b is allowed.  Texels are widened as a4i widens a frame and then converted to binary64, which is exact.
 * A pixel is VALID iff R, G and B of both a(p) and b(p) are finite.  Everything below runs over valid pixels only, in binary64.
 *
 * Pointwise sums, with d_c = a_c - b_c (one binary64 subtraction): the numbers of valid and of not valid pixels; per channel
 * sum d_c^2, sum |d_c| and sum d_c^2 / (b_c^2 + eps) (one multiplication, one addition, one division per term); max |d_c| over
 * pixels and channels.
 *
 * SSIM (Wang, Bovik, Sheikh, Simoncelli 2004), with p->ssim == 1, on a4i's luminance l() taken in fp32 exactly as a4i takes it and
 * then widened to binary64 (la, lb):
 *   window    q = p + (i, j), |i|, |j| <= 5, q inside the image and VALID;   w(q) = g_|i| * g_|j|,  g_k = exp(-k^2 / 4.5)
 *             (a Gaussian of sigma 1.5), the six binary64 constants MID_METRICS_G0 .. MID_METRICS_G5 below
 *   W = sum w.  Taps that are missing are skipped and the weights renormalised, as every filter here treats the border.
 *   mu_a = (sum w la) / W;  S_aa = (sum w la^2) / W - mu_a^2;  likewise mu_b, S_bb;  S_ab = (sum w la lb) / W - mu_a mu_b.  No clamping.
 *   C1 = (0.01 peak)^2,  C2 = (0.03 peak)^2
 *   ssim(p) = ((2 mu_a mu_b + C1) (2 S_ab + C2)) / ((mu_a^2 + mu_b^2 + C1) (S_aa + S_bb + C2))      for a VALID centre p
 * The order of the sums is the kernel's own: per row of the window the eleven taps left to right, then the eleven rows top to
 * bottom, each moment by fma.  With a == b every expression of the numerator equals its partner of the denominator bit for bit, so
 * ssim(p) is exactly 1.0.  Scaling a, b and peak by 2^k and eps by 4^k leaves relMSE's sums and every ssim(p) unchanged, bit for
 * bit, while nothing leaves the normal range.  A VALID pixel whose fp32 luminance overflows takes part as +-Inf: the ssim of the
 * windows that hold it is NaN, and so is the sum.
 * map: NULL, or a width x height float plane that receives ssim(p) rounded to fp32 and a quiet NaN where p is not VALID.  With
 * p->ssim == 0 map must be NULL and the SSIM sum is 0.
 *
 * Result and workspace.  work: a caller-owned device buffer of mid_image_metrics_workspace(width, height) bytes, 16-byte aligned.
 * After the call its first MID_METRICS_N doubles are the sums, at the MID_METRICS_* indices below (slots 13 .. 15 are 0); the rest
 * is scratch.  Nothing is kept in the context: two calls on two streams with two workspaces cannot meet.
 * Determinism: the frame is cut into the firefly clamp's 64 x 16 tiles (csrc/firefly_tile.hpp) and min(tiles, 4096) workgroups are
 * launched -- a number that depends on the size alone, not on the device; workgroup g takes the tiles g, g + G, ... in that order,
 * a lane adds its four pixels of every tile top to bottom, the lanes of a wave are added by a butterfly, the four waves in index
 * order, and the workgroup stores one row of MID_METRICS_N partials to `work`; a second launch of one workgroup adds the rows in
 * index order, sixty-four interleaved chains joined by a fixed tree.  No atomics.  p->ssim == 0 runs the same reduction without the
 * windows: its pointwise sums have the bits of p->ssim == 1.
 * Class (csrc/image_metrics.hip): tiled, a workgroup of four waves per 64 x 16 tile, lanes along x, a lane owning
 * four pixels of one column; with ssim two LDS tiles of (64 + 10) x (16 + 10) fp32 luminances (15392 bytes), NaN in the first
 * where the pixel is outside the image or not VALID -- a marker that gives the tap weight 0 by a select; the horizontal eleven-tap
 * sums of w, w la, w lb, w la^2, w lb^2, w la lb of a lane's fourteen rows stay in registers and feed the vertical sums of its four
 * pixels.  Index arithmetic in size_t; the formats are run-time, wave-uniform values.
 * MID_ERR_INVALID before anything is queued, `work` and `map` untouched: a NULL ctx, p, a, b or work; width or height < 1, or
 * 2^30 pixels and more; an unknown format, or guide bits set; a or b not aligned to its texel, work not to 16 bytes, map not to
 * 4; peak or eps not finite or <= 0; ssim outside {0, 1}; map given with ssim == 0; work or map overlapping an input or each other. */
#define MID_METRICS_N 16
enum {
    MID_METRICS_N_VALID = 0, MID_METRICS_N_INVALID = 1,
    MID_METRICS_SQ_R = 2, MID_METRICS_SQ_G = 3, MID_METRICS_SQ_B = 4,           /* sum d_c^2 */
    MID_METRICS_ABS_R = 5, MID_METRICS_ABS_G = 6, MID_METRICS_ABS_B = 7,        /* sum |d_c| */
    MID_METRICS_MAX_ABS = 8,                                                    /* max |d_c| */
    MID_METRICS_REL_R = 9, MID_METRICS_REL_G = 10, MID_METRICS_REL_B = 11,      /* sum d_c^2 / (b_c^2 + eps) */
    MID_METRICS_SSIM = 12                                                       /* sum ssim(p); 13 .. 15 are 0 */
};
/* g_k = exp(-k^2 / 4.5), k = 0 .. 5, to the nearest binary64 */
#define MID_METRICS_G0 1.0
#define MID_METRICS_G1 0.80073740291680806
#define MID_METRICS_G2 0.41111229050718745
#define MID_METRICS_G3 0.1353352832366127
#define MID_METRICS_G4 0.028565500784550377
#define MID_METRICS_G5 0.0038659201394728076
typedef struct mid_image_metrics_params {
    int32_t width, height;
    int32_t format_a, format_b;   /* MID_FMT_* of `a` and of `b`; guide bits must be 0 */
    float   peak;                 /* finite, > 0: the data range (1 for unit-range frames, 255 for integer levels); default 1 */
    float   eps;                  /* finite, > 0: relMSE's regulariser, in squared units of the data; default 1e-2 */
    int32_t ssim;                 /* 0 | 1 */
} mid_image_metrics_params;
typedef struct mid_image_metrics_result {
    double n_valid, n_invalid;
    double mse;                   /* (sum over c of sum d_c^2) / (3 n_valid) */
    double mse_r, mse_g, mse_b;   /* (sum d_c^2) / n_valid */
    double mae;                   /* (sum over c of sum |d_c|) / (3 n_valid) */
    double max_abs;               /* max |d_c|; 0 where nothing is valid */
    double psnr;                  /* 10 log10(peak^2 / mse); +Inf at mse == 0 */
    double relmse;                /* (sum over c of sum d_c^2 / (b_c^2 + eps)) / (3 n_valid) */
    double ssim;                  /* (sum ssim(p)) / n_valid; NaN with p->ssim == 0: it was not computed */
} mid_image_metrics_result;
size_t mid_image_metrics_workspace(int width, int height);   /* 0 for a size mid_image_metrics refuses */
int mid_image_metrics(mid_ctx *ctx, const mid_image_metrics_params *p, const void *a, const void *b, void *work,
                      float *map /* width * height floats, or NULL */, void *stream);
/* The derived values of MID_METRICS_N sums copied to the host: a pure host function, the one statement of the definitions in the
 * struct above.  Every ratio is NaN at n_valid == 0.  Reads width / height of p not at all: peak and ssim only.
 * MID_ERR_INVALID for a NULL pointer, or peak not finite or <= 0. */
int mid_image_metrics_derive(const double *sums_host, const mid_image_metrics_params *p, mid_image_metrics_result *out);

/* ---- a4o: the guided filter --------------------------------------------------------------------
 * Every filter above is a weighted average: the guide layers decide the weights and nothing else.  The guided filter (He, Sun,
 * Tang 2010, with a colour guide; Bauszat et al. 2011 use it on path-traced frames) fits, inside every window, the frame as an
 * AFFINE function of the guide's colour, p ~ a^T I + b, and evaluates the averaged fit at the pixel's own guide texel: the output
 * is locally a linear transform of the guide, whose edges and texture are reproduced, not merely respected.  Everything is made of
 * box means, so the cost does not depend on the radius.
 * p(q), I(q): the RGB of `in` and of `guide`, widened as a4i widens a frame; the guide's alpha is ignored.  guide == NULL, or guide
 * == in as pointers: I = p and the guide format is the frame's (with guide == in the format word must say so).
 * A texel q is VALID iff all six values are finite.  w(k): the window |i|, |j| <= radius around k, cut at the image.  n_k: the
 * number of VALID texels of w(k).
 * Stage 1, per window centre k inside the image with n_k > 0, every mean over the VALID q of w(k), divided by n_k:
 *   mu = mean I (3);  nu = mean p (3);  Sigma = mean(I I^T) - mu mu^T (3 x 3, symmetric);
 *   C = mean(I p^T) - mu nu^T (3 x 3: row = guide channel j, column = output channel c);
 *   a_k = (Sigma + eps U)^-1 C (U the identity);   b_k = nu - a_k^T mu.             A window with n_k = 0 has no model.
 * Stage 2, per pixel i: abar, bbar = the means of a_k, b_k over the k of w(i) that have a model, m_i their number.
 *   i VALID and m_i > 0:   out_c = fmaf(abar_0c, I_i0, fmaf(abar_1c, I_i1, fmaf(abar_2c, I_i2, bbar_c)))     -- fp32, this order
 *   otherwise:             out.rgb = p_i unchanged: a NaN stays a NaN (the firefly clamp, a4l, is the repair)
 *   out.a = in.a in every case.  `out` is stored in out_format by the rule of mid_atrous_joint's outputs (float4, or mid_pack_u8 /
 *   mid_pack_f16 of it).
 * Arithmetic (csrc/guided.hip).  The window sums are taken in binary64 -- the product of two fp32 values is exact
 * there -- of I - s_I and p - s_p, s the texel of the workgroup's first output pixel (a channel of it that is not finite: 0):
 * covariances do not change under a shift, and a flat HDR region or a depth-like guide no longer cancels in mean(I I^T) - mu mu^T.
 * The solve is the adjugate of the symmetric positive definite Sigma + eps U in binary64; a, b are rounded once to fp32 into `work`
 * (with b back in the unshifted units); the stage-2 sums are binary64 and abar, bbar are rounded once to fp32; then the chain above.
 * Error: with T_ic = sum_j mean_k|a_k,jc| |I_ij| + mean_k|b_k,c|, the five roundings named and the three fmas are at most 7 units
 * of 2^-24 T, and the bound is |out - exact| <= 8 * 2^-24 * T_ic, PROVIDED the binary64 sums stay below the eighth unit.  With D
 * the largest deviation of a guide channel from s_I inside the workgroup's 256 x (32 + 2 radius) footprint: a column's running sum
 * takes at most 96 roundings of 2^-53 * 34 D^2 (2^-41.3 D^2), the 33 columns of a window bring 2^-36.3 D^2 of that, and the two
 * prefix slots add 10 roundings each of 2^-53 * 256 * 33 D^2 (2^-35.6 D^2 together): 2^-34.9 D^2 on a window sum, 2^-34.9 D^2 / n_k
 * on a mean, and through (Sigma + eps U)^-1 at most 2^-34.9 D^2 / (n_k eps) relative on a.  That stays below 2^-24 when
 *     D^2 / eps <= 2^10 * n_min,      n_min the smallest non-zero n_k of the frame ((radius + 1)^2 where every texel is VALID).
 * (A unit-range guide at radius 2 and eps = 1e-3 has D^2 / eps <= 1000 against 9216; a depth guide of +-30 units around s at
 * eps = 1 has 900.)  The bound is a worst case over every rounding going one way.
 * work: caller-provided device scratch of mid_guided_workspace bytes = 52 bytes per pixel (thirteen fp32 planes: a_jc at plane
 * 3 j + c, b_c at 9 + c, the model flag at 12) and no constant, 16-byte aligned; the stage-1 models cross it as fp32; its contents
 * after the call are unspecified.  Nothing is kept in the context: two calls on two streams with two workspaces cannot meet.
 * Class: two launches; a workgroup of four waves holds 256 columns, lanes along x, and walks a segment of 32 output rows; the
 * vertical sums of a column stay in its lane's registers (row entering added, row leaving subtracted) and RESTART with every
 * segment; per output row the column sums cross LDS once as prefix sums along x and a window is the difference of two slots
 * (csrc/guided_box.hpp).  Index arithmetic in size_t; min(tiles, 8192) workgroups; no atomics, so the bits depend on the inputs
 * and the parameters alone.
 * MID_ERR_INVALID before anything is queued, `out` and `work` untouched: a NULL p, in, work, out or bytes; radius outside 1..16;
 * eps not finite or <= 0; an unknown frame, guide or output format, or bits above 15; in, guide or out not aligned to its texel
 * size, work not to 16 bytes; width or height < 1, or 2^30 pixels and more; out or work overlapping in, guide or each other in any
 * way (the pass is a stencil: exactly in place is refused too); guide == in with a guide format that is not the frame's. */
typedef struct mid_guided_params {
    int32_t width, height;
    int32_t radius;   /* 1..16: (2 radius + 1)^2 windows, clipped at the image */
    float   eps;      /* finite, > 0: the regulariser, in squared guide units */
    int32_t format;   /* MID_FMT_* of `in`; MID_FMT_WITH_GUIDE(fmt, guide_fmt) names the guide's format (guide field 0: RGBA8) */
} mid_guided_params;
int mid_guided_workspace(const mid_guided_params *p, size_t *bytes);
int mid_guided_filter(mid_ctx *ctx, const mid_guided_params *p, const void *in, const void *guide /* NULL: `in` guides itself */,
                      void *work, void *out, int out_format, void *stream);
/* The frame pipeline (section 8d) with the guided filter as its compute stage, at k = 0 as mid_sequence_atrous_joint: outputs
 * [first, first + count) of the sequence, output t with the bits of mid_guided_filter on frame t (and host_guides[t]) in
 * out_format.  host_frames: n_frames HOST pointers in the frame format of p->format; host_guides: n_frames HOST pointers, one
 * plane per frame in the guide format of p->format, uploaded with its frame -- or NULL: every frame guides itself.  The workspace
 * comes from the context's cache, one per kernel stream (mid_ctx_release_cached frees it).  Outputs are stored by the kernel or
 * downloaded by the rule of mid_sequence_bilateral; overlap and timings_ms as for mid_sequence_nlm.  Launch range "guided t".
 * MID_ERR_INVALID, before anything is queued, for: what mid_guided_filter refuses in p; a NULL frame, guide or output of the
 * range; bad first or count; an unknown out_format; an output that is also an input frame or guide of the range (or appears
 * twice); a call while the context's stream records. */
int mid_sequence_guided(mid_ctx *ctx, const mid_guided_params *p, const void *const *host_frames, int n_frames,
                        const void *const *host_guides /* one plane per frame, or NULL */, int first, int count,
                        void *const *host_out, int out_format, int overlap, float *timings_ms);

/* ---- a4p: the median and the layer-weighted median ------------------------------------------------
 * Every filter above is a weighted mean or a local linear fit: one texel of value 50 inside a 5 x 5 window moves it by 2 however
 * the weights fall.  The median is a SELECTION -- the output is one of the inputs -- and ignores outliers of either sign: dark
 * dropouts, salt-and-pepper noise, dead texels, a NaN.  Its guide-aware form is the weighted median under the per-tap layer weights
 * of the joint filters: the render layers decide which taps belong to the pixel's surface, the median is robust within that set.
 * C(q) is the widened texel of `in` (widened as a4i widens a frame), p the output pixel, the taps q the window |i|, |j| <= radius
 * around p, cut at the image.
 * Weight of a tap.  n_layers == 0, the plain median: w(q) = 1.  Otherwise w(q) = 2^arg, arg the FMA chain of a4g without its colour
 * term and without K(o): it starts at 0, arg = fma(-d, d, arg) with d = G_l(p) sc_l - G_l(q) sc_l for layer 0's x, y, z, then layer
 * 1's, ...; sc_l as in a4e, a guide value entering as the fp32 product g * sc_l.  There is no spatial term.  A weight that is not
 * finite (a NaN or Inf guide texel at p or q) is 0, and so is a weight below the fp32 normal range (arg < -126, in fp32 as computed).
 * The guide's alpha is ignored.  The centre is a tap like any other; its weight is
 * 1 when its guide texels are finite.
 * Per channel c of r, g, b:  V_c = the taps with C_c(q) finite and w(q) > 0;  W_c = sum_{V_c} w;
 *   S_c(v) = sum_{q in V_c, C_c(q) <= v} w(q);       out_c = min { C_c(q) : q in V_c, 2 S_c(C_c(q)) >= W_c }
 * -- the lower weighted median, the usual median when the weights are 1 and the count is odd.  V_c empty: out_c = C_c(p) unchanged.
 * out.a = in.a.  So a NaN centre with valid neighbours is repaired, a NaN neighbour takes no part, and a frame with nothing valid
 * comes back as it went in.  `out` is stored in out_format by a4g's output rule.  Where +0 and -0 both qualify either may come back.
 * Arithmetic.  The sums are fp32.  A tap's place in a sum is its place in the window (rows top to bottom, a row left to right); a
 * tap that takes no part adds an exact 0: the order depends on the inputs and the parameters alone -- no atomics, the same bits on
 * every call, stream and kernel class.  When every weight of a window is exactly 0 or 1 every sum is an integer <= 49, exact in
 * fp32, and the output is determined exactly: the plain form, and a weighted window whose guide differences are either 0 or so large
 * that 2^arg underflows to 0, are bit for bit the answer of integer arithmetic.
 * Precision otherwise.  Let L' be the number of layers whose differences are not all 0 in the window and A the largest |arg| among
 * the taps with w > 2^-24 W (A < 30 always: 2^-24 W <= 49 * 2^-24).  A term d^2 carries the subtraction's rounding, 2^-23 relative;
 * each of the 3 L' FMAs rounds once, at most 2^-24 of the partial sum, which never exceeds |arg|: the chain is within
 * (3 L' + 2) * 2^-24 * A of its float64 value on the scaled guide values, which is (3 L' + 2) * 2^-24 * A * ln 2 relative on w.
 * v_exp_f32 is good to one unit, 2^-23 relative, and up to 49 fp32 additions of non-negative terms add 49 * 2^-24 relative on a sum:
 *     |S_fp32 / S_float64 - 1| <= ((3 L' + 2) * A * ln 2 + 51) * 2^-24   <=   delta = 2^-16    while (3 L' + 2) * A <= 295.
 * (One layer: every A; three layers: A <= 26.8; sixteen live layers: A <= 5.9.)  Under it the output is a valid tap
 * value v whose float64 sums satisfy S_<(v) <= (1/2 + delta) W and S_<=(v) >= (1/2 - delta) W, and where the float64 margin
 * min(S_<=(v*) - W/2, W/2 - S_<(v*)) / W of the exact answer v* exceeds delta the output is v* bit for bit.
 * Bit identities: an RGBA8 / RGBA16F frame or guide gives the bits of the widened call (a4g's wording); n_layers == 0 gives the bits
 * of any number of all-zero layers with any sigmas; one live layer among zero layers gives the bits of that layer alone; in * 2^k
 * gives out * 2^k while nothing overflows or goes subnormal; the plain median of a frame flipped or transposed is the flipped or
 * transposed output; every kernel class gives the same bits.
 * Classes (csrc/median.hip; lanes along x, no scratch memory, no atomics; tiles dealt to at most 4 workgroups per CU):
 *   n_layers  radius  kernel            tile     LDS tile  LDS bytes (n_layers 0 .. 4)
 *   0 .. 4    1       tiled             64 x 16  66 x 18   14260, 28516, 42772, 57028, 71284
 *   0 .. 4    2       tiled             64 x 16  68 x 20   16324, 32644, 48964, 65284, 81604
 *   0 .. 4    3       tiled             64 x 16  70 x 22   18484, 36964, 55444, 73924, 92404
 *   0         1 .. 3  plain selection   a tile of the tiled class whose every texel is inside the image with finite r, g, b (a vote
 *                                       of the workgroup): the taps go through a min / max / median-of-three selection network, the
 *                                       9-input median network at radius 1, forgetful selection over 25 and 49 inputs at radius 2, 3
 *   5 .. 16   1 .. 3  global            64 x 4   -         0
 * tiled: the colour as three float planes (NaN outside the image, so "outside" and "not valid" are one case) and three scaled planes
 * per layer, decoded from the guide format at the fill (csrc/median_tile.hpp); the weights of a pixel are computed once, and per
 * channel the window's values and weights sit in registers while every candidate's rank is counted.  global: one pixel per lane,
 * the taps read from global memory.
 * MID_ERR_INVALID before anything is queued, `out` untouched: a NULL p, in or out; radius outside 1..3; n_layers outside 0..16; a
 * layer table or sigma table that is NULL with n_layers > 0 or non-NULL with n_layers == 0; a NULL layer; a sigma that is not finite
 * and > 0; a non-zero guide field with n_layers == 0; an unknown frame, guide or output format, or bits above 15; in, a layer or out
 * not aligned to its texel size; out overlapping in or a layer in any way (the filter is a stencil); width or height < 1, or 2^30
 * pixels and more. */
typedef struct mid_median_params {
    int32_t width, height;
    int32_t radius;   /* 1..3: (2 radius + 1)^2 = 9, 25, 49 taps, cut at the image */
    int32_t format;   /* MID_FMT_* of `in`; guide format through MID_FMT_WITH_GUIDE as in a4e */
} mid_median_params;
int mid_median_filter(mid_ctx *ctx, const mid_median_params *p, const float *layer_sigma /* n_layers host floats, NULL iff n_layers == 0 */,
                      const void *in, const uint32_t *const *layers /* n_layers device ptrs, NULL iff n_layers == 0 */, int n_layers,
                      void *out, int out_format, void *stream);
/* mid_sequence_atrous_joint (section a4g) with mid_median_filter as the compute stage, k = 0 and no levels: host frames and host
 * layers in, host frames out, output t with the bits of mid_median_filter on frame t.  host_layers == NULL with n_layers == 0 is
 * the plain form (nothing is uploaded beside the frames).  Launch range "median t".  The refusals above and those of
 * mid_sequence_atrous_joint, which leave host_out and timings_ms untouched. */
int mid_sequence_median(mid_ctx *ctx, const mid_median_params *p, const float *layer_sigma, const void *const *host_frames, int n_frames,
                        const void *const *host_layers, int n_layers, int first, int count, void *const *host_out, int out_format,
                        int overlap, float *timings_ms);

/* ---- a5: normalize ----------------------------------------------------------------------
 * One dispatch of shaders/normalize.comp (RecordCommandsOfExecuteAndTransfer(normKernel=true)):
 * out = weightColor / normWeight, or (1,0,1,1) where normWeight == 0; bindings {0: out; 1: W}. */
int mid_normalize(mid_ctx *ctx, const mid_normalize_params *p,
                  const mid_weightinfo *W, mid_pixel *out, void *stream);

/* ---- a6: u8 <-> float -------------------------------------------------------------------
 * unpack flavour 0 = UNORM texel decode c/255 (src/texture.cpp:16, src/main.cpp:341);
 *        flavour 1 = CPU decode (float)c * (1.0f/255.0f) (src/main.cpp:1804-1807).
 * pack = (unsigned char)(255.0f*v), truncation (GetImageFromGPU, src/main.cpp:97-103), clamped
 * to [0,255] only where that cast is undefined in C.  n_values counts channels, not pixels.
 * The u8 buffer must be 4-byte aligned and the float buffer 16-byte aligned (hipMalloc'd buffers are). */
int mid_unpack_u8(mid_ctx *ctx, const uint8_t *in, size_t n_values, int flavour, float *out, void *stream);
int mid_pack_u8(mid_ctx *ctx, const float *in, size_t n_values, uint8_t *out, void *stream);
/* RGBA16F <-> float: unpack widens each binary16 value exactly; pack rounds to nearest even (overflow -> +-Inf, NaN stays
 * NaN, f16 subnormals kept) -- the bits of numpy.float16(x).  n_values counts channels.  The half buffer must be 8-byte and the
 * float buffer 16-byte aligned; in-place is refused (MID_ERR_INVALID); n_values = 0 is a no-op. */
int mid_unpack_f16(mid_ctx *ctx, const uint16_t *in, size_t n_values, float *out, void *stream);
int mid_pack_f16(mid_ctx *ctx, const float *in, size_t n_values, uint16_t *out, void *stream);

/* ---- a8: frame pipeline -----------------------------------------------------------------
 * Replaces RecordCommandsOfOverlappingNLM + the ping-pong loop (src/main.cpp:889-989,
 * :1539-1573): host frames in, host frames out.  Frame t+k+1 is uploaded (hipMemcpyAsync from
 * pinned slots on an upload stream) while frame t is filtered on the compute stream and frame
 * t-1 is downloaded on a third stream; a device ring keeps 2k+4 frames and four
 * output slots in flight, so each stage may run up to three frames away from its neighbours, and
 * consecutive frames are filtered on two alternating kernel streams (one launch's tail overlaps the next one's head).
 * host_frames/host_out are arrays of n_frames HOST pointers (RGBA32F, RGBA8 or RGBA16F per p->format;
 * output RGBA32F here, RGBA8 / RGBA16F from the _u8 / _f16 variants).  Synchronous: returns when every output is on the host.
 * The device ring, the output slots and the events are kept in the context between calls (grown when a call needs more
 * or larger ones; mid_ctx_release_cached / mid_ctx_destroy free them), so only a context's first call -- or the first
 * at a larger frame size -- allocates.  Calls on one context are serialised (they share its four streams).
 * timings_ms (optional, 3 floats): wall time of the WHOLE call, set-up included; sum of kernel time; sum of copy time.
 * The same machinery runs the bilateral over a whole animation: mid_sequence_bilateral below (window k = 0, each frame's guide
 * layers uploaded with it, RGBA32F / RGBA8 / RGBA16F outputs chosen by an argument). */
int mid_sequence_nlm(mid_ctx *ctx, const mid_nlm_params *p, const void *const *host_frames,
                     int n_frames, int k, mid_pixel *const *host_out, int overlap, float *timings_ms);
/* Same, for the output frames [first, first+count) only (host_out has `count` entries): the unit of
 * frame-block sharding -- a device filters its block and uploads the k halo frames on either side. */
int mid_sequence_nlm_range(mid_ctx *ctx, const mid_nlm_params *p, const void *const *host_frames,
                           int n_frames, int k, int first, int count, mid_pixel *const *host_out,
                           int overlap, float *timings_ms);
/* Same, with the reference's u8 read-back conversion (GetImageFromGPU, src/main.cpp:97-103: truncating
 * (unsigned char)(255.0f*v), see mid_pack_u8) done on the device before the download: host_out receives RGBA8
 * frames, a quarter of the PCIe bytes -- the LDR (PNG in, PNG out) path of the reference. */
int mid_sequence_nlm_range_u8(mid_ctx *ctx, const mid_nlm_params *p, const void *const *host_frames,
                              int n_frames, int k, int first, int count, uint8_t *const *host_out,
                              int overlap, float *timings_ms);
/* Same, with RGBA16F outputs: the kernel's epilogue rounds each normalized pixel to binary16 (nearest even; the bits of
 * numpy.float16 of mid_sequence_nlm_range's output) and host_out receives 8 B per pixel -- half the PCIe bytes of RGBA32F.
 * Input frames may be in any of the three formats.  An output that lies inside ONE page-locked allocation or registration of
 * this device (mid_alloc_host, mid_host_register, mid_image_load_pinned; checked per output with hipMemGetAddressRange) is
 * stored by the kernel itself, with no download stage; any other output is downloaded from device slots. */
int mid_sequence_nlm_range_f16(mid_ctx *ctx, const mid_nlm_params *p, const void *const *host_frames,
                               int n_frames, int k, int first, int count, uint16_t *const *host_out,
                               int overlap, float *timings_ms);

/* The same pipeline with the bilateral as its compute stage (window k = 0: output i reads frame i only), for a whole animation.
 * Output i has the bits of mid_bilateral(p, frame i) -- host_layers == NULL, either layout -- or of mid_bilateral_layers(p, frame
 * i, its n_layers layers) -- host_layers != NULL, texture layout -- followed by mid_pack_u8 / mid_pack_f16 when out_format is
 * MID_FMT_RGBA8 / MID_FMT_RGBA16F (the kernel's epilogue packs).  With host_layers set and n_layers == 0 every output pixel is the
 * magenta sentinel, as in mid_bilateral_layers.  host_frames: n_frames HOST pointers in p->format; host_layers: n_frames *
 * n_layers HOST pointers, frame-major (frame i's layers are uploaded with frame i), RGBA8 -- or RGBA16F / RGBA32F layers when
 * p->format = MID_FMT_WITH_GUIDE(frames' format, layers' format): the layer ring then holds 8 / 16 bytes per texel, host layers
 * need no alignment, pageable ones go through the bounce buffers like frames; host_out: n_frames HOST pointers.
 * A packed output (RGBA8 or RGBA16F) is stored by the kernel itself when every output lies inside ONE page-locked allocation or
 * registration of this device; otherwise the outputs are downloaded from device slots (through the bounce buffers where an
 * output is not inside one mapping).  Frames are independent: a frame block is a sub-array, so there is no _range variant.
 * overlap and timings_ms as for mid_sequence_nlm.  MID_ERR_INVALID, before anything is queued, for: a NULL frame, layer or output;
 * n_layers outside 0..16; layers with MID_LAYOUT_LINEAR; an unknown out_format; an output that is also an input frame or layer
 * (or appears twice); the parameter checks of mid_bilateral; a guide field in p->format without host_layers, or an unknown guide
 * code; a call while the context's stream records. */
int mid_sequence_bilateral(mid_ctx *ctx, const mid_bilateral_params *p, const void *const *host_frames, int n_frames,
                           const void *const *host_layers, int n_layers, void *const *host_out, int out_format,
                           int overlap, float *timings_ms);

/* The same pipeline with layer-guided NLM as its compute stage (one frame's window; mid_sequence_nlm_layers_temporal adds the
 * neighbouring frames), for a whole animation: output i has the bits of
 * mid_nlm_layers(p, frame i, its n_layers layers) followed by mid_pack_u8 / mid_pack_f16 when out_format is MID_FMT_RGBA8 /
 * MID_FMT_RGBA16F (the kernel's epilogue packs).  host_frames: n_frames HOST pointers in p->format; host_layers: n_frames *
 * n_layers RGBA8 HOST pointers, frame-major (frame i's layers are uploaded with frame i; NULL only with n_layers == 0, which gives
 * magenta outputs); host_out: n_frames HOST pointers.  Outputs are stored by the kernel or downloaded by the rule of
 * mid_sequence_bilateral; frames are independent, so a frame block is a sub-array.  overlap and timings_ms as for
 * mid_sequence_nlm.  MID_ERR_INVALID, before anything is queued, for: a NULL frame, layer or output; n_layers outside 0..16; an
 * unknown out_format; an output that is also an input frame or layer (or appears twice); the parameter checks of mid_nlm_accum;
 * a call while the context's stream records. */
int mid_sequence_nlm_layers(mid_ctx *ctx, const mid_nlm_params *p, const void *const *host_frames, int n_frames,
                            const void *const *host_layers, int n_layers, void *const *host_out, int out_format,
                            int overlap, float *timings_ms);

/* The same pipeline with layer-guided NLM over neighbouring frames as its compute stage: outputs [first, first+count) of the
 * sequence, output t with the bits of mid_nlm_layers_temporal(p, frames, layers, k) for frame t in out_format.  The temporal
 * window is mid_sequence_nlm_range's (ring of 2k+4 frames; only the frames of [first-k, first+count+k) are read and uploaded,
 * so a frame block plus k halo frames on either side is the unit of sharding) and the layer ring is mid_sequence_nlm_layers':
 * frame f's layers are uploaded with frame f and live as long as its ring slot, across the 2k+1 outputs that read them.
 * host_frames: n_frames HOST pointers in p->format; host_layers: n_frames * n_layers RGBA8 HOST pointers, frame-major (NULL only
 * with n_layers == 0, which gives magenta outputs); host_out: `count` HOST pointers.  Outputs are stored by the kernel or
 * downloaded by the rule of mid_sequence_bilateral.  overlap and timings_ms as for mid_sequence_nlm.  MID_ERR_INVALID, before
 * anything is queued, for: a NULL frame, layer or output of the range; n_layers outside 0..16; bad k, first or count (k >= 0,
 * 2k+2 <= 96, first >= 0, count >= 1, first + count <= n_frames); the pointer limit of mid_nlm_layers_temporal; an unknown
 * out_format; an output that is also an input frame or layer of the range (or appears twice); the parameter checks of
 * mid_nlm_accum; a call while the context's stream records. */
int mid_sequence_nlm_layers_temporal(mid_ctx *ctx, const mid_nlm_params *p, const void *const *host_frames, int n_frames,
                                     const void *const *host_layers, int n_layers, int k, int first, int count,
                                     void *const *host_out, int out_format, int overlap, float *timings_ms);

/* The same pipeline with the bilateral over neighbouring frames as its compute stage: outputs [first, first+count) of the
 * sequence, output t with the bits of mid_bilateral_temporal(p, frames, layers, k) for frame t in out_format.  host_layers ==
 * NULL selects the plain form (n_layers must be 0); host layers are RGBA8, or RGBA16F / RGBA32F with MID_FMT_WITH_GUIDE in p->format,
 * as in mid_sequence_bilateral (a guide field in the plain form is MID_ERR_INVALID).  Schedule, layer ring and output rule are mid_sequence_nlm_layers_temporal's:
 * ring of 2k+4 frames, frame f's layers uploaded with frame f and alive as long as its slot, only the frames of
 * [first-k, first+count+k) read, packed outputs stored by the kernel only when every one lies inside ONE page-locked allocation
 * or registration.  MID_ERR_INVALID, before anything is queued, for: a NULL frame, layer or output of the range; n_layers
 * outside 0..16 (not 0 in the plain form); bad k, first or count (k >= 0, 2k+2 <= 96, first >= 0, count >= 1, first + count <=
 * n_frames); the pointer limit and the parameter checks of mid_bilateral_temporal (MID_LAYOUT_LINEAR among them); an unknown
 * out_format; an output that is also an input frame or layer of the range (or appears twice); a call while the context's
 * stream records. */
int mid_sequence_bilateral_temporal(mid_ctx *ctx, const mid_bilateral_params *p, const void *const *host_frames, int n_frames,
                                    const void *const *host_layers, int n_layers, int k, int first, int count,
                                    void *const *host_out, int out_format, int overlap, float *timings_ms);

/* Debug export: the DEVICE timeline of this context's last mid_sequence_nlm*, mid_sequence_bilateral[_temporal], mid_sequence_nlm_layers or
 * mid_sequence_nlm_layers_temporal call, from the events the call recorded on
 * its streams (no profiler: the call ran at its own pace).  All times in ms from the start of the call's first upload.
 * upload_ms[2*i], [2*i+1]: start / end of the upload of frame first_upload_frame + i; output_ms[4*j .. 4*j+3]: kernel
 * start, kernel end, download start, download end of output frame first_output_frame + j (output j runs on kernel stream
 * j & 1; an output stored by the kernel reports an empty download interval at its kernel's end; the upload interval of a
 * layer-guided mid_sequence_bilateral frame spans the frame and its layers).  cap = rows either array can hold.  Valid until the next pipeline call or mid_ctx_release_cached on the context.
 * The events are read once, by the first call after a pipeline call; until the next pipeline call completes every call returns those
 * same numbers, whatever else ran on the context in between (a refused pipeline call does not replace them).
 * Stands where the reference prints its per-submit timestamps (src/main.cpp:1095-1101). */
int mid_pipe_last_timeline(mid_ctx *ctx, int cap, float *upload_ms /* cap x 2 */, int *n_uploads, int *first_upload_frame,
                           float *output_ms /* cap x 4 */, int *n_outputs, int *first_output_frame);

/* The reference's literal multi-frame mode (src/main.cpp:1539-1606): ONE target, its neighbour frames
 * streamed from the host.  W = sum over frames of one nonlocal.comp dispatch each (target fixed), then
 * normalize.  overlap != 0 replaces RecordCommandsOfOverlappingNLM (:889-989): frame i+1 is uploaded on
 * the upload stream into the other of two device slots while frame i is being accumulated.
 * host_frames: n_frames HOST pointers (format p->format, any of the three); host_out: w*h RGBA32F on the host.
 * timings_ms (optional, 3 floats): wall, kernel sum, copy sum. */
int mid_nlm_multiframe(mid_ctx *ctx, const mid_nlm_params *p, const void *host_target,
                       const void *const *host_frames, int n_frames, mid_pixel *host_out,
                       int overlap, float *timings_ms);

/* ---- 8e: an animation sharded over GPUs (frame blocks + RCCL halo) ----------------------------
 * New capability with the reference's multi-frame semantics (the reference is single-device: deviceId{0},
 * src/main.cpp:1321; its neighbour-frame loop is src/main.cpp:1577-1606).  One rank per GPU owns a contiguous block of
 * an n-frame sequence, resident in its HBM; temporal NLM over t-k..t+k needs the k frames on either side of the block,
 * which are exchanged GPU to GPU in ONE step (ncclSend/ncclRecv in one group, point to point over xGMI) -- no other
 * collective.  Interior outputs are launched while the halo is in flight, boundary outputs after it.
 * RCCL is loaded at run time on the first mid_comm_* call (no link-time dependency; MID_ERR_UNSUPPORTED if absent).
 *
 * mid_shard_block: the partition -- rank r owns frames [start, start+count), the first n % world ranks one extra.
 * mid_shard_halo_plan / mid_shard_launch_plan: the exchange and the launches of one rank as pure data (host only, no
 *   GPU): receives/sends as (peer rank, global frame id) in issue order; launch rows {interior, w_lo, w_hi, first,
 *   count, out_offset}: frames w_lo..w_hi form the table handed to mid_nlm_temporal, outputs are table entries
 *   [first, first+count), stored at block-relative out_offset.  `cap` = capacity of the caller's arrays.
 * mid_comm_unique_id + mid_comm_create: one process per GPU (rank 0 makes the id and hands it to the others out of
 *   band -- a file, MPI, torch.distributed); mid_comm_create_all: one process, one context per device.
 *   RCCL is looked up as librccl.so.1 / librccl.so / /opt/rocm/lib/librccl.so.1; the environment variable
 *   MID_RCCL_LIBRARY (read once, on the first mid_comm_* call) names the library to load instead.
 * mid_nlm_temporal_sharded: `block` = this rank's `count` device frames in order, `out` = `count` device outputs.
 *   Asynchronous on `stream`.  COLLECTIVE: every rank of the communicator must call it, with the same n_frames, k and
 *   frame size -- also a rank that owns no frame.  Blocks may be RGBA32F, RGBA8 or RGBA16F (p->format; halo frames travel
 *   at that size, so RGBA16F halves the wire bytes of RGBA32F); outputs are RGBA32F.  Everything that can fail locally (arguments, the stream rule below,
 *   receive-buffer allocation) is checked before the first RCCL call, so a rank that returns an error there has not
 *   entered the exchange; its peers then wait for it, and the caller must mid_comm_abort (or destroy) the communicator
 *   on EVERY rank -- there is no other way out of a half-entered collective.
 *   Stream rule: the receive buffers are reused from call to call, ordered only through the stream the calls are issued
 *   on.  A call on a different stream than the previous one returns MID_ERR_INVALID unless the previous call's work has
 *   finished (e.g. after mid_stream_sync on the earlier stream).
 *   Results are the bits of one mid_nlm_temporal over the whole sequence by construction (same kernels, same tile
 *   shape, same frame tables: tests/test_shard_native_plan.py).  Executed so far: with RCCL itself for world = 1; with 2-4
 *   ranks sharing one device against a test-only stand-in for the transport (tests/standin_rccl), bit-identical in 12
 *   partitions.  RCCL between two devices has not run yet: bench.py gates it with `bit_identical_to_single_launch_per_rank`.
 * mid_comm_reserve: allocates the 2k receive buffers for frames of up to max_frame_bytes up front, so that no sharded
 *   call allocates (optional; otherwise they are allocated on first use and retired, not freed, when the frame size grows).
 * mid_comm_abort: ncclCommAbort -- tears the rank's connections down without waiting for outstanding operations; the
 *   handle then only accepts mid_comm_destroy.
 * mid_comm_loopback: a send+receive addressed to this very rank (the exchange's call pattern without the wire), asynchronous on
 *   `stream`; mid_comm_last_loopback: (waits for it) t[0] start / t[1] end of that group on the exchange stream, in ms from the
 *   moment `stream` reached the call.  Its events are its own: the last sharded call's timeline is not disturbed.
 * mid_comm_last_exchange: bytes received/sent by the last sharded call and (waits for it) the exchange's duration.
 * mid_comm_last_timeline: (waits for the call) its device timeline in ms from the call's first event on the caller's stream:
 *   t[0] exchange start, t[1] exchange end (both 0 when nothing was exchanged), t[2] end of the interior launches, t[3] end of
 *   the last launch.  The share of the exchange hidden behind interior compute is (min(t[1], t[2]) - t[0]) / (t[1] - t[0]).
 * mid_comm_last_issue_order: what the call put on its streams, in host issue order -- 'X' exchange group (exchange stream), 'I'
 *   interior launch (caller's stream), then per edge of the block 'W' the wait for the exchange and 'B' the boundary launch, on
 *   that edge's boundary stream of the communicator ("X I.. W B W B"), so that boundary workgroups fill the interior launch's
 *   tail; the caller's stream joins both before the call's work is complete on it; every 'I' precedes the first 'W' by construction.
 * mid_comm_stream_priority: the exchange stream's priority and the device's range (numerically lower = higher); the stream
 *   is created with the highest, so RCCL's send/receive kernels are dispatched ahead of queued interior workgroups.
 * mid_comm_boundary_priority: the two boundary streams' priority -- the device's LOWEST (`least`).  Streams and hardware queues:
 *   the HIP runtime gives each of its three priority levels a pool of four hardware queues and a queue runs its packets in order,
 *   so two busy streams that share a queue serialise.  The library's streams are placed so that this cannot happen among them,
 *   whatever the application creates: highest level = upload, download, exchange (3 of 4 queues); lowest level = the two boundary
 *   streams (2 of 4); default level = the context's two kernel streams, beside the caller's own streams. */
typedef struct mid_comm mid_comm;
#define MID_COMM_ID_BYTES 128
int mid_shard_block(int n_frames, int world, int rank, int *start, int *count);
int mid_shard_halo_plan(int n_frames, int world, int k, int rank, int cap,
                        int *recv_peer, int *recv_frame, int *n_recv, int *send_peer, int *send_frame, int *n_send);
int mid_shard_launch_plan(int n_frames, int world, int k, int rank, int cap, int *rows /* cap x 6 ints */, int *n_rows);
int mid_comm_unique_id(uint8_t id[MID_COMM_ID_BYTES]);
int mid_comm_create(mid_ctx *ctx, const uint8_t id[MID_COMM_ID_BYTES], int rank, int world, mid_comm **out);
int mid_comm_create_all(mid_ctx *const *ctxs, int world, mid_comm **out /* world entries */);
int mid_comm_destroy(mid_comm *comm);
int mid_comm_abort(mid_comm *comm);
int mid_comm_reserve(mid_comm *comm, size_t max_frame_bytes, int k);
int mid_comm_rank(mid_comm *comm, int *rank, int *world);
int mid_comm_loopback(mid_comm *comm, const void *src, void *dst, size_t bytes, void *stream);
int mid_comm_last_loopback(mid_comm *comm, float t_ms[2]);
int mid_nlm_temporal_sharded(mid_comm *comm, const mid_nlm_params *p, const void *const *block /* count device frames */,
                             int n_frames, int k, mid_pixel *const *out /* count device frames */, void *stream);
int mid_comm_last_exchange(mid_comm *comm, size_t *bytes_recv, size_t *bytes_sent, float *exchange_ms);
int mid_comm_last_timeline(mid_comm *comm, float t_ms[4]);
int mid_comm_last_issue_order(mid_comm *comm, char *buf, size_t buflen);
int mid_comm_stream_priority(mid_comm *comm, int *priority, int *least, int *greatest);
int mid_comm_boundary_priority(mid_comm *comm, int priority[2]);
/* What RCCL itself reports for the communicator: ncclCommCount, ncclCommUserRank, ncclGetVersion (-1 where unavailable). */
int mid_comm_rccl_info(mid_comm *comm, int *nranks, int *user_rank, int *version);

/* ---- 8f-2: image files ------------------------------------------------------------------
 * mid_image_load = LoadImages (src/main.cpp:145-229): ".exr" -> RGBA32F (tinyexr LoadEXR: missing
 * alpha = 1), anything else is decoded as PNG -> RGBA8 (lodepng::decode).  `data` is host memory
 * owned by the library until mid_image_free.  mid_image_save = SaveEXR(rgba,w,h,4,0) (:1699) for
 * MID_FMT_RGBA32F, lodepng::encode (:1717) for MID_FMT_RGBA8; MID_FMT_RGBA16F writes channels A,B,G,R as HALF with
 * the FLOAT writer's compression.  Host-only: no GPU needed. */
typedef struct mid_image {
    int32_t width, height;
    int32_t format;   /* MID_FMT_* */
    void   *data;
} mid_image;
int  mid_image_load(const char *path, mid_image *out);
void mid_image_free(mid_image *img);
/* The same decode, but the pixels are written DIRECTLY into pinned (page-locked) host memory of `ctx`'s device, so the
 * frame can be handed to mid_sequence_nlm* / mid_memcpy_h2d as a true asynchronous DMA source without another copy --
 * the reference likewise decodes and memcpy's straight into its mapped staging buffer (LoadImageDataToBuffer,
 * src/main.cpp:1105-1142).  Release with mid_image_free_pinned (never mid_image_free). */
int  mid_image_load_pinned(mid_ctx *ctx, const char *path, mid_image *out);
int  mid_image_free_pinned(mid_ctx *ctx, mid_image *img);
/* An .exr as MID_FMT_RGBA16F: HALF channels are copied bit for bit, FLOAT and UINT channels are rounded to nearest even on
 * the host (overflow -> +-Inf, NaN stays NaN, subnormals kept; UINT through float first), a missing alpha is 1.0 (0x3C00).
 * PNG files are refused (MID_ERR_INVALID).  ctx == NULL: host memory, released by mid_image_free; otherwise pinned memory of
 * ctx's device, released by mid_image_free_pinned.  mid_image_load itself still returns RGBA32F for an .exr. */
int  mid_image_load_f16(mid_ctx *ctx, const char *path, mid_image *out);
int  mid_image_save(const char *path, const void *data, int32_t width, int32_t height, int32_t format);
/* The codecs work on the independent blocks of a file in parallel (EXR chunks; PNG: filter rows and 1 MiB deflate segments on
 * encode -- the inflate of a PNG is one serial stream): by default on up to min(16, hardware threads) host threads per call.
 * mid_image_threads(n) sets that number FOR IMAGE CALLS MADE BY THE CALLING THREAD (n = 0: the default again, n < 0: query only)
 * and returns the previous setting.  A host that loads or saves many files at once -- one per thread -- sets 1 on those threads:
 * mi_denoise --animation decodes and encodes its frames that way (64 x 1080p PNG: the serial inflate of one file no longer
 * serialises the sequence).  File bytes do not depend on the thread count.  The reference does its image I/O on one thread
 * (lodepng / tinyexr calls, src/main.cpp:155,196,1699,1717). */
int  mid_image_threads(int n);

/* ---- measurement helper -----------------------------------------------------------------
 * Timestamps around a region on a stream (reference: vkCmdWriteTimestamp pool,
 * src/main.cpp:747-755,793-796,812-814).  tick/tock record hipEvents on `stream`;
 * mid_timer_ms waits for the tock and returns elapsed milliseconds. */
typedef struct mid_timer mid_timer;
int mid_timer_create(mid_ctx *ctx, mid_timer **out);
int mid_timer_destroy(mid_timer *t);
int mid_timer_tick(mid_timer *t, void *stream);
int mid_timer_tock(mid_timer *t, void *stream);
int mid_timer_ms(mid_timer *t, float *ms);

/* Named host ranges for a trace (ROCTx; `rocprofv3 --marker-trace`): the counterpart, for a profiler's timeline, of the
 * timestamp pairs the reference writes around every submit (src/main.cpp:793-796,812-814,842-844).  The frame pipeline
 * emits "upload f" / "nlm t" / "download t" inside one range per call; callers bracket their own stages with these two.
 * Bound to whatever ROCTx the process has ALREADY loaded (rocprofv3 preloads one); nothing is loaded otherwise and the
 * calls do nothing.  Return 1 when a ROCTx is present, 0 when not. */
int mid_range_push(const char *name);
int mid_range_pop(void);

#ifdef __cplusplus
}
#endif
#endif /* MI_DENOISE_H */
