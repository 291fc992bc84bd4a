// pipeline.cpp -- the frame pipeline: host frames in, denoised host frames out.
//
// Replaces the reference's single-queue ping-pong (RecordCommandsOfOverlappingNLM,
// src/main.cpp:889-989, loop :1539-1573: one command buffer holding "dispatch on texture A"
// followed, without a barrier, by "copy staging -> texture B", descriptor sets swapped by
// parity, and a fence wait after every submit).  Here the stages run concurrently on their own HIP streams:
//
//   upload   : hipMemcpyAsync host frame f -> device ring slot f % RING; a stage with guide layers uploads frame f's layers into
//              the layer ring's slot f % RING in the same upload interval
//   compute  : one launch per output frame t over the ring slots t-k..t+k and the layers uploaded with them (k = 0: slot t alone).
//              The schedule knows a stage only by its description (struct Stage: sizes, layers, output rule, marker name) and by
//              one callable that queues a batch's outputs; each entry point supplies that callable around its own filter --
//              temporal NLM (mid_sequence_nlm*), the bilateral plain or layer-guided (mid_sequence_bilateral, k = 0), layer-guided
//              NLM (mid_sequence_nlm_layers, k = 0; mid_sequence_nlm_layers_temporal; mid_sequence_nlm_joint), the bilateral and the joint bilateral over
//              neighbouring frames (mid_sequence_bilateral_temporal, mid_sequence_bilateral_joint) -- after check_sequence, the one
//              statement of the argument checks they share
//   download : hipMemcpyAsync device out slot t % 4 -> host   (RGBA32F and RGBA16F outputs, and RGBA8 outputs in pageable memory)
//              RGBA8 outputs in page-locked memory have NO download stage: the kernel's epilogue stores the packed pixels
//              straight into the caller's buffer (4 B per pixel = 17-19 GB/s at the kernel's frame rate, a third of the link);
//              nor have RGBA16F outputs that lie inside one page-locked allocation each (8 B per pixel); the bilateral's RGBA8 and
//              RGBA16F outputs are stored by the kernel only under that stronger rule, for both formats
//
// joined only by events: compute(t) waits for upload(t+k); upload(f) waits for the last
// compute that still reads the slot it overwrites; download(t) waits for compute(t);
// compute(t) waits for download(t-4) before reusing an output slot (no slots and no such wait for direct RGBA8 outputs).  One output frame per launch
// (B = 1 below; coarser batches were measured and lose overlap); the ring holds 2k+4 frames and
// there are four output slots, so uploads run up to three frames ahead of the kernel and
// downloads up to three behind: the stages are decoupled and the slowest one (measured: the
// 33 MB/frame download, 0.70 ms) sets the frame rate.  This is the ONE schedule the library ships
// (a gated chunk-launch alternative was measured in round 2 and removed: LABNOTES.md).  Host frames
// allocated with mid_alloc_host (pinned) are DMA'd directly; pageable memory still works, but it is
// moved through the context's page-locked bounce buffers (csrc/hostcopy.cpp: a host memcpy per 8 MiB
// chunk, never the runtime's pin-on-the-fly path) and the host's memcpy rate -- not the link -- sets
// the pace (uploads on the calling thread, pageable outputs on a helper thread of the call).
//
// Frame selection differs from the reference on purpose: frames are taken
// in the order given, window t-k..t+k clipped at the sequence ends; the reference's "every
// file of the directory in directory order, target twice, last frame never filtered" is not
// reproduced.
#include "common.hpp"
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <thread>
#include <vector>

using namespace mid;

namespace {


// `n` device buffers of at least `bytes` each from the context's cache.  Every pipeline call ends with all four streams
// synchronised, so whatever the cache holds is idle when the next call (serialised by pipe.mu) resizes it.
// Shrink rule: buffers MORE than four times larger than this call needs are given back and reallocated at the size needed (a caller
// that moves from 1080p RGBA32F frames to thumbnails does not keep 400 MB of HBM for them), while alternating between RGBA32F
// and RGBA8 sequences of one frame size -- exactly a factor of four -- keeps the larger set and allocates nothing.
int reserve(mid_pipe_set &s, size_t n, size_t bytes)
{
    if (bytes > s.bytes || (s.bytes > 4 * bytes && !s.p.empty())) {
        for (void *q : s.p) (void)hipFree(q);
        s.p.clear();
        s.bytes = bytes;
    }
    while (s.p.size() < n) { void *q = nullptr; MID_HIP(hipMalloc(&q, s.bytes)); s.p.push_back(q); }
    return MID_OK;
}

int reserve_events(mid_pipe_cache &c, size_t n)
{
    while (c.ev.size() < n) { hipEvent_t e = nullptr; MID_HIP(hipEventCreate(&e)); c.ev.push_back(e); }
    return MID_OK;
}


// A pipeline call that returns early (an error half way) must still leave the context's streams idle: the cached buffers its
// queued work reads and writes belong to the next call the moment this one returns.
struct DrainOnExit {
    mid_ctx *ctx;
    ~DrainOnExit()
    {
        (void)hipStreamSynchronize(ctx->upload);
        (void)hipStreamSynchronize(ctx->compute);
        (void)hipStreamSynchronize(ctx->compute2);
        (void)hipStreamSynchronize(ctx->download);
    }
};

}  // namespace

void mid::pipe_cache_release(mid_ctx *ctx)
{
    mid_pipe_cache &c = ctx->pipe;
    for (mid_pipe_set *s : {&c.ring, &c.out, &c.layers, &c.atrous, &c.target, &c.slots, &c.weights, &c.result}) {
        for (void *q : s->p) (void)hipFree(q);
        s->p.clear();
        s->bytes = 0;
    }
    for (hipEvent_t e : c.ev) (void)hipEventDestroy(e);
    c.ev.clear();
    c.last = mid_pipe_last{};
}

// One compute stage, as the schedule sees it: whose call it is, what is uploaded beside each frame, which rule admits kernel-stored
// outputs, the name of the launch range -- nothing about the filter.  The filter is the `launch` callable given to run_pipeline
// beside the stage: each entry point supplies a lambda around its own *_out function.
struct Stage {
    const char *who;                          // the entry point, for ranges and messages
    int width, height, format;                // the input frames
    size_t layer_bytes;                       // one guide layer (RGBA8, or what a bilateral format word names)
    const void *const *host_layers;           // n_layers host layers per frame, frame-major; NULL: nothing is uploaded beside the frames
    int n_layers;
    bool proven;                              // outputs are kernel-stored only inside ONE page-locked mapping (every stage but temporal NLM)
    const char *marker;                       // the launch range, "nlm %d": profiles and the marker tests read these names
    size_t level_bytes = 0;                   // a stage that keeps levels between its passes (a-trous): bytes of one, and how many
    int n_levels = 0;                         // per kernel stream -- reserved in the context's cache (pipe.atrous) for both streams
    // A recursive stage (mid_sequence_atrous_recursive): output t needs what output t-1 left on the device.
    bool in_order = false;                    // every launch on ONE kernel stream, in output order (no alternation between two)
    const void *const *host_motion = nullptr; // one float2 plane per frame, uploaded in the frame's upload interval into one more slot
                                              // beside its layers: the launch finds it at lt[j * n_side + n_layers], n_side the side slots per frame
    int skip = 0;                             // leading outputs that are computed into a device slot and neither stored nor downloaded
                                              // (warm-up); host_out[0 .. skip) is not read
    const void *const *host_albedo = nullptr; // one plane per frame in the layers' format (layer_bytes), uploaded in the frame's upload interval
                                              // into one more side slot, after the layers and the motion plane
};

// Outputs [first, first+count) of an n-frame host sequence; frames outside that range are only
// uploaded as far as the temporal window needs them (the halo of a frame block).  The caller has checked every argument.
// launch(tbl, n_win, lt, k, t0, bn, out, out_fmt, stream) queues the outputs of one batch: tbl holds the n_win device frames of
// the batch's window (ring slots lo..need), lt their device layers, frame-major (lt[j * n_layers + l]: layer l of tbl[j]), the
// outputs are window frames t0 .. t0+bn-1 and go to out[0..bn) in out_fmt.  A k = 0 stage reads its one slot from the same tables.
template <typename Launch>
static int run_pipeline(mid_ctx *ctx, const Stage &st, const Launch &launch, const void *const *host_frames,
                        int n, int k, int first, int count, void *const *host_out, int out_fmt,
                        int overlap, float *timings_ms)
{
    const int f_lo = first - k < 0 ? 0 : first - k;                                  // first frame ever uploaded
    const int f_hi = first + count - 1 + k > n - 1 ? n - 1 : first + count - 1 + k;  // last one
    const size_t npix = (size_t)st.width * st.height;
    const size_t in_bytes = npix * fmt_bytes(st.format), layer_bytes = st.layer_bytes;
    const int n_layers = st.host_layers ? st.n_layers : 0;
    const int n_side = n_layers + (st.host_motion ? 1 : 0) + (st.host_albedo ? 1 : 0);   // slots beside a frame: its layers, its motion plane, its albedo plane
    const size_t motion_bytes = npix * 2 * sizeof(float);
    const size_t side_bytes = st.host_motion && motion_bytes > layer_bytes ? motion_bytes : layer_bytes;
    const int skip = st.skip;
    const size_t dl_bytes = npix * fmt_bytes(out_fmt);            // one output frame, as it is written and downloaded
    const int n_up = f_hi - f_lo + 1;
    // Outputs could be filtered in batches of B frames per launch.  Measured on MI355X (16 x 1080p, 21x21/7x7):
    // B=1 2084 Mpixel/s, B=2 1341, B=4 1472, B=8 1403 -- coarser batches bunch the copies and lose overlap
    // while the kernel time barely changes, so one frame per launch it is (the indexing below stays general in B).  Re-measured in
    // round 6 for RGBA8 frames with direct output stores (no download stage to bunch): B = 1 / 2 / 4 4096-4109 / 4106-4121 / 4107-4132
    // Mpixel/s, k = 2 898-904 / 907 / 906 -- the same (profiles/r06_pipe_batch_u8_ab.txt).
    constexpr int B = 1;
    const int nb = (count + B - 1) / B;
    constexpr int DEPTH = 4;                                  // batches in flight per stage
    const int ring = n_up < 2 * k + DEPTH * B ? n_up : 2 * k + DEPTH * B;

    // The clock starts HERE: timings_ms[0] is what the caller waits for, set-up included.  The device ring, the output slots
    // and the events live in the context and are only allocated when a call needs more or larger ones than any call before
    // it (the first call of a context, a larger frame size, a wider window): in a steady stream of sequences nothing is.
    const auto wall0 = std::chrono::steady_clock::now();
    Range call_range("mid_%s frames=%d k=%d outputs=[%d,%d)%s", st.who, n, k, first, first + count,
                          out_fmt == MID_FMT_RGBA8 ? " u8" : out_fmt == MID_FMT_RGBA16F ? " f16" : "");
    std::lock_guard<std::mutex> pipe_lock(ctx->pipe.mu);
    DrainOnExit drain{ctx};
    // Where do the outputs go?  RGBA8 outputs in page-locked memory are written by the kernel itself (`direct`): a pinned buffer is
    // mapped into the device's address space, the packed pixel is 4 B, and at the kernel's frame rate that is 17-19 GB/s of posted
    // writes -- a third of the link -- so the download stage, its output slots and the wait for a free slot disappear.  Measured
    // on 64 x 1080p (profiles/r06_pipeline_u8_timeline.txt, LABNOTES R6.1): staged through hipMemcpyAsync the runtime's copies
    // went from 0.19 to 0.67 ms per frame part way into a call and the four output slots then gated every launch (3230-3590
    // Mpixel/s, 5-10 % spread); direct 4040-4080, spread 1-3 %.  RGBA32F outputs (16 B per pixel: more than the link carries at the
    // kernel's rate) and pageable outputs keep the staged download.
    // RGBA16F outputs (8 B per pixel, about 31 GB/s of posted writes at the kernel's frame rate) are stored directly too, but only
    // when every output is PROVEN to lie inside one page-locked allocation or registration mapped for this device
    // (host_range_in_one_mapping): a range whose two ends are pinned but which spans two registrations would fault the GPU.
    // Measured on 64 x 1080p (profiles/r07_half_rates.txt): the staged download ran at a fraction of the link part way into the call.
    // The bilateral and layer-guided NLM take the proven rule for BOTH packed formats: their outputs are stored by the kernel only
    // when every one lies inside one page-locked allocation or registration; otherwise they are downloaded, and an output that is
    // not inside one mapping goes through the bounce buffers (`bounced`) even where both of its ends are page-locked.
    const bool proven = st.proven;
    bool out_pinned = true;
    std::vector<char> bounced(count, 0);
    if (proven) {
        for (int i = skip; i < count; ++i) { bounced[i] = !host_range_in_one_mapping(host_out[i], dl_bytes); out_pinned = out_pinned && !bounced[i]; }
    } else {
        for (int i = skip; i < count; ++i) out_pinned = out_pinned && host_is_pinned(host_out[i], dl_bytes);
    }
    bool direct = out_fmt == MID_FMT_RGBA8 && out_pinned;
    if (proven) {                                 // (and aligned for the kernel's 4 B / 8 B stores)
        direct = out_fmt != MID_FMT_RGBA32F && out_pinned;
        for (int i = skip; direct && i < count; ++i) direct = ((uintptr_t)host_out[i] & (fmt_bytes(out_fmt) - 1)) == 0;
    }
    else if (out_fmt == MID_FMT_RGBA16F) {
        direct = true;
        for (int i = skip; direct && i < count; ++i) direct = host_range_in_one_mapping(host_out[i], dl_bytes);
    }
    for (int i = skip; direct && i < count; ++i) {
        void *dp = nullptr;
        if (hipHostGetDevicePointer(&dp, host_out[i], 0) != hipSuccess || !dp) { (void)hipGetLastError(); direct = false; }
    }
    mid_pipe_set &dring = ctx->pipe.ring, &dout = ctx->pipe.out, &dlayers = ctx->pipe.layers;
    if (int rc = reserve(dring, ring, in_bytes)) return rc;
    if (n_side) { if (int rc = reserve(dlayers, (size_t)ring * n_side, side_bytes)) return rc; }
    if (!direct || skip) { if (int rc = reserve(dout, DEPTH * B, dl_bytes)) return rc; }
    // (one set per kernel stream in use: an in-order stage launches on ctx->compute alone)
    if (st.n_levels) { if (int rc = reserve(ctx->pipe.atrous, (size_t)(overlap && !st.in_order ? 2 : 1) * st.n_levels, st.level_bytes)) return rc; }
    if (int rc = reserve_events(ctx->pipe, 2 * (size_t)n_up + 4 * (size_t)nb)) return rc;
    ctx->pipe.last = mid_pipe_last{};
    struct Events { hipEvent_t *ev; } up0{ctx->pipe.ev.data()}, up1{up0.ev + n_up}, c0{up1.ev + n_up}, c1{c0.ev + nb}, d0{c1.ev + nb}, d1{d0.ev + nb};
    auto slot = [&](int f) { return dring.p[(f - f_lo) % ring]; };
    auto layer_slot = [&](int f, int l) { return dlayers.p[((f - f_lo) % ring) * n_side + l]; };   // frame f's layer l (l >= n_layers: its motion plane, its albedo plane)

    int next_upload = f_lo;
    auto upload = [&](int f) -> int {
        Range r("upload %d", f);
        if (f - f_lo >= ring) {   // the slot still holds frame f-ring, read by outputs (f-ring)-k .. (f-ring)+k
            int last_reader = f - ring + k;
            if (last_reader > first + count - 1) last_reader = first + count - 1;
            if (last_reader >= first) {
                // Batches alternate between the two kernel streams, so the readers of this slot sit on BOTH:
                // batch lb and every earlier same-parity batch are ordered before c1[lb] by stream order, the
                // other-parity readers (lb-1, lb-3, ...) before c1[lb-1].  Waiting on both makes the overwrite
                // safe by construction, not by the kernels happening to finish in launch order.
                const int lb = (last_reader - first) / B;
                MID_HIP(hipStreamWaitEvent(ctx->upload, c1.ev[lb], 0));
                if (lb >= 1) MID_HIP(hipStreamWaitEvent(ctx->upload, c1.ev[lb - 1], 0));
            }
        }
        MID_HIP(hipEventRecord(up0.ev[f - f_lo], ctx->upload));
        if (int rc = copy_h2d(ctx, slot(f), host_frames[f], in_bytes, ctx->upload)) return rc;
        for (int l = 0; l < n_layers; ++l)      // (its guide layers ride in the same upload interval: they share the slot's lifetime)
            if (int rc = copy_h2d(ctx, layer_slot(f, l), st.host_layers[(size_t)f * n_layers + l], layer_bytes, ctx->upload)) return rc;
        if (st.host_motion) { if (int rc = copy_h2d(ctx, layer_slot(f, n_layers), st.host_motion[f], motion_bytes, ctx->upload)) return rc; }
        if (st.host_albedo) { if (int rc = copy_h2d(ctx, layer_slot(f, n_side - 1), st.host_albedo[f], layer_bytes, ctx->upload)) return rc; }
        MID_HIP(hipEventRecord(up1.ev[f - f_lo], ctx->upload));
        return MID_OK;
    };
    // Pinned outputs: download(bi) is queued right behind compute(bi) and the host runs on.  Pageable outputs: copy_d2h returns
    // only when the frame is in the caller's buffer (a host memcpy per chunk out of the bounce buffers), so those downloads run on
    // a helper thread of this call: the calling thread keeps bouncing uploads in and queueing launches while the helper copies
    // finished frames out -- the two memcpy streams overlap (16 x 1080p RGBA32F with pageable frames on both sides: 42.9 ms with
    // both on one thread).  The helper takes batch bi once compute(bi) has been queued; compute(bi) is queued only when the helper
    // has recorded d1[bi-DEPTH] (the output slot is free) -- the event order of the pinned case, kept by two counters.
    auto download = [&](int bi) -> int {
        const int b0 = first + bi * B, bn = (first + count - b0) < B ? (first + count - b0) : B;
        Range r("download %d", b0);
        MID_HIP(hipStreamWaitEvent(ctx->download, c1.ev[bi], 0));
        MID_HIP(hipEventRecord(d0.ev[bi], ctx->download));
        for (int i = 0; i < bn && bi >= skip; ++i)      // (a warm-up output stays in its slot: the events alone are recorded)
            if (int rc = copy_d2h(ctx, host_out[b0 - first + i], dout.p[(bi % DEPTH) * B + i], dl_bytes, ctx->download,
                                  bounced[b0 - first + i] != 0)) return rc;
        MID_HIP(hipEventRecord(d1.ev[bi], ctx->download));
        return MID_OK;
    };
    struct Helper {
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        int issued = -1;                 // highest batch whose launch has been queued          (caller -> helper)
        int done = -1;                   // highest batch whose download has finished, d1 recorded (helper -> caller)
        bool stop = false;
        int rc = MID_OK;
        char err[512] = "";
        ~Helper()
        {
            if (!th.joinable()) return;
            { std::lock_guard<std::mutex> l(mu); stop = true; }
            cv.notify_all();
            th.join();                   // before DrainOnExit and before anything the download lambda refers to goes away
        }
    } helper;
    bool threaded = !out_pinned && overlap;
    if (threaded) try {
        helper.th = std::thread([&] {
            (void)hipSetDevice(ctx->device);
            for (int bi = 0; bi < nb; ++bi) {
                {
                    std::unique_lock<std::mutex> l(helper.mu);
                    helper.cv.wait(l, [&] { return helper.stop || helper.issued >= bi; });
                    if (helper.issued < bi) return;          // stopped before this batch was launched
                }
                const int rc = download(bi);
                {
                    std::lock_guard<std::mutex> l(helper.mu);
                    if (rc) { helper.rc = rc; snprintf(helper.err, sizeof helper.err, "%s", mid_last_error()); helper.stop = true; }
                    else helper.done = bi;
                }
                helper.cv.notify_all();
                if (rc) return;
            }
        });
    } catch (...) {
        threaded = false;            // no thread to be had (EAGAIN under a thread limit): the downloads run on the calling thread
    }
    // the helper's error, if any, becomes this thread's error
    auto helper_failed = [&]() -> int {
        std::lock_guard<std::mutex> l(helper.mu);
        return helper.rc ? set_error(helper.rc, "%s", helper.err) : MID_OK;
    };

    for (int bi = 0; bi < nb; ++bi) {
        const int b0 = first + bi * B, bn = (first + count - b0) < B ? (first + count - b0) : B;
        const int need = b0 + bn - 1 + k < n - 1 ? b0 + bn - 1 + k : n - 1;
        const int ahead = overlap ? (need + (DEPTH - 1) * B < f_hi ? need + (DEPTH - 1) * B : f_hi) : need;
        // frames up to the batch's last window must be resident; with overlap the next batches' frames are
        // started now as well: they only wait for kernels already enqueued and ride beside this one
        while (next_upload <= need) { if (int rc = upload(next_upload++)) return rc; }
        // Consecutive batches go to alternating kernel streams: every dependency between them is an explicit
        // event (inputs, ring-slot reuse, output-slot reuse), so the tail of one launch -- 1156 workgroups on 512
        // slots leave the last round a quarter full -- overlaps the head of the next instead of idling the CUs.
        // (measured: one kernel stream 2385, two 2575, three 1892, four 1652 Mpixel/s; giving the second stream a
        // lower or higher priority than the first: 2410-2430; splitting every download over two copy streams: 1860)
        hipStream_t cs = overlap && (bi & 1) && !st.in_order ? ctx->compute2 : ctx->compute;
        MID_HIP(hipStreamWaitEvent(cs, up1.ev[need - f_lo], 0));
        // Output slot bi % DEPTH was written by batch bi-DEPTH and is read only by download(bi-DEPTH), which
        // itself waited for c1[bi-DEPTH]: d1[bi-DEPTH] therefore orders both the writer and the only reader of
        // the slot before this batch, whichever kernel stream they ran on.
        if (bi >= DEPTH && !direct) {
            if (threaded) {              // d1[bi-DEPTH] must have been RECORDED before a stream can be told to wait for it
                std::unique_lock<std::mutex> l(helper.mu);
                helper.cv.wait(l, [&] { return helper.stop || helper.done >= bi - DEPTH; });
                if (helper.rc) { l.unlock(); return helper_failed(); }
            }
            MID_HIP(hipStreamWaitEvent(cs, d1.ev[bi - DEPTH], 0));
        }

        const int lo = b0 - k < 0 ? 0 : b0 - k;
        const void *tbl[kMaxFrames];
        for (int f = lo; f <= need; ++f) tbl[f - lo] = slot(f);
        mid_pixel *o[kMaxFrames];
        for (int i = 0; i < bn; ++i) {
            if (direct && bi >= skip) MID_HIP(hipHostGetDevicePointer((void **)&o[i], host_out[b0 - first + i], 0));
            else o[i] = (mid_pixel *)dout.p[(bi % DEPTH) * B + i];
        }
        // the window's layers, frame-major like tbl: output b0 + i reads ring slots b0+i-k .. b0+i+k and the layers uploaded with them
        static_assert(B == 1, "one output per launch: its window is what nlm_layers_temporal_fits admitted");
        static_assert(kMaxLayers <= MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS, "the k = 0 stages pass up to kMaxLayers layers unchecked by that rule");
        const uint32_t *lt[MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS];
        MID_REQUIRE((need - lo + 1) * n_side <= MID_NLM_LAYERS_TEMPORAL_MAX_POINTERS, "%s: the window's layers exceed one launch", st.who);
        for (int f = lo; f <= need; ++f)
            for (int l = 0; l < n_side; ++l) lt[(f - lo) * n_side + l] = (const uint32_t *)layer_slot(f, l);
        {
            Range launch_range(st.marker, b0);
            MID_HIP(hipEventRecord(c0.ev[bi], cs));
            if (int rc = launch(tbl, need - lo + 1, lt, k, b0 - lo, bn, (void *const *)o, out_fmt, cs)) return rc;
            MID_HIP(hipEventRecord(c1.ev[bi], cs));
        }

        while (next_upload <= ahead) { if (int rc = upload(next_upload++)) return rc; }

        if (direct) {
            // nothing to download: the launch wrote the caller's buffer (or, in a warm-up, a slot nobody reads)
        } else if (threaded) {
            { std::lock_guard<std::mutex> l(helper.mu); helper.issued = bi; }
            helper.cv.notify_all();
        } else if (int rc = download(bi)) return rc;

        if (!overlap) {   // the reference's behaviour: a fence wait after every submit (src/main.cpp:1092)
            MID_HIP(hipStreamSynchronize(ctx->upload));
            MID_HIP(hipStreamSynchronize(ctx->compute));
            MID_HIP(hipStreamSynchronize(ctx->download));
        }
    }
    if (threaded) {
        {
            std::unique_lock<std::mutex> l(helper.mu);
            helper.cv.wait(l, [&] { return helper.stop || helper.done >= nb - 1; });
        }
        helper.th.join();
        if (int rc = helper_failed()) return rc;
    }
    {
        Range r("drain");
        MID_HIP(hipStreamSynchronize(ctx->upload));
        MID_HIP(hipStreamSynchronize(ctx->compute));
        MID_HIP(hipStreamSynchronize(ctx->compute2));
        MID_HIP(hipStreamSynchronize(ctx->download));
    }
    const auto wall1 = std::chrono::steady_clock::now();
    ctx->pipe.last = {n_up, nb, f_lo, first, B, direct};

    if (timings_ms) {
        float kern = 0.f, copy = 0.f, ms = 0.f;
        for (int bi = 0; bi < nb; ++bi) {
            MID_HIP(hipEventElapsedTime(&ms, c0.ev[bi], c1.ev[bi])); kern += ms;
            if (!direct) { MID_HIP(hipEventElapsedTime(&ms, d0.ev[bi], d1.ev[bi])); copy += ms; }
        }
        for (int i = 0; i < n_up; ++i) { MID_HIP(hipEventElapsedTime(&ms, up0.ev[i], up1.ev[i])); copy += ms; }
        timings_ms[0] = std::chrono::duration<float, std::milli>(wall1 - wall0).count();
        timings_ms[1] = kern;
        timings_ms[2] = copy;
    }
    return MID_OK;
}

// How one entry point words and bounds the shared checks: its name in the messages, the word it has for its frame count ("n",
// "n_frames"), whether it takes (k, first, count) -- the k = 0 entry points word a bad frame count their own way -- and whether an
// output may be one of the call's inputs.
struct SeqRules {
    const char *who, *n_word;
    bool windowed, refuse_alias;
};

// The argument checks every sequence entry point shares, made before anything is queued: the tables, the frame count and the
// output range [first, first + count) with its window k, every frame and layer of the uploaded range [first - k, first + count - 1
// + k] and every output non-NULL, a known output format, and (refuse_alias) no output among exactly those frames and layers nor given
// twice -- an output that is also an input would be overwritten by a direct store while uploads that run ahead (or the kernel of
// another stream) still read it.  The k = 0 entry points are the case (k, first, count) = (0, 0, n).  n_layers is read only with a
// layer table and has been checked by the caller (0..16).
static int check_sequence(const SeqRules &r, const void *const *host_frames, int n, const void *const *host_layers, int n_layers,
                          int k, int first, int count, void *const *host_out, int out_fmt)
{
    const char *who = r.who;
    MID_REQUIRE(host_frames && host_out, "%s: NULL argument", who);
    if (!r.windowed) MID_REQUIRE(n >= 1, "%s: n_frames %d < 1", who, n);
    MID_REQUIRE(n >= 1 && k >= 0 && 2 * (long)k + 2 <= kMaxFrames, "%s: bad %s=%d k=%d", who, r.n_word, n, k);
    MID_REQUIRE(first >= 0 && count >= 1 && (long)first + count <= n, "%s: bad range first=%d count=%d %s=%d", who, first, count, r.n_word, n);
    MID_REQUIRE(fmt_known(out_fmt), "%s: unknown output format %d", who, out_fmt);
    if (!host_layers) n_layers = 0;
    const int f_lo = first - k < 0 ? 0 : first - k;
    const int f_hi = first + count - 1 + k > n - 1 ? n - 1 : first + count - 1 + k;
    for (int f = f_lo; f <= f_hi; ++f) {
        MID_REQUIRE(host_frames[f], "%s: frame %d is NULL", who, f);
        for (int l = 0; l < n_layers; ++l) MID_REQUIRE(host_layers[(size_t)f * n_layers + l], "%s: layer %d of frame %d is NULL", who, l, f);
    }
    for (int i = 0; i < count; ++i) MID_REQUIRE(host_out[i], "%s: output %d is NULL", who, i);
    if (!r.refuse_alias) return MID_OK;
    std::vector<const void *> inputs;
    try {
        inputs.reserve((size_t)(f_hi - f_lo + 1) * (n_layers + 1));
    } catch (...) {
        return set_error(MID_ERR_INVALID, "%s: no host memory for the alias check", who);
    }
    for (int f = f_lo; f <= f_hi; ++f) {
        inputs.push_back(host_frames[f]);
        for (int l = 0; l < n_layers; ++l) inputs.push_back(host_layers[(size_t)f * n_layers + l]);
    }
    return check_no_alias(who, "an input frame or layer of this call", inputs.data(), (int)inputs.size(), (const void *const *)host_out, count);
}

// Temporal NLM of output t over the frames t-k..t+k.  Its outputs may be frames of the sequence: every host frame is read once,
// by its upload, before the first output that could overwrite it is launched -- so this stage alone makes no alias check.
static int sequence_impl(mid_ctx *ctx, const mid_nlm_params *p, const void *const *host_frames,
                         int n, int k, int first, int count, void *const *host_out, int out_fmt,
                         int overlap, float *timings_ms)
{
    Bind b(ctx, nullptr);
    if (b.rc) return b.rc;
    if (int rc = refuse_if_recording(ctx->compute, "mid_sequence_nlm (four streams, host-side waits)")) return rc;
    MID_REQUIRE(p, "sequence_nlm: NULL argument");
    if (int rc = check_sequence({"sequence_nlm", "n", true, false}, host_frames, n, nullptr, 0, k, first, count, host_out, out_fmt)) return rc;
    MID_REQUIRE(p->width > 0 && p->height > 0, "sequence_nlm: bad size");
    MID_REQUIRE(fmt_known(p->format), "sequence_nlm: unknown format %d", p->format);
    const Stage st{"sequence_nlm", p->width, p->height, p->format, 0, nullptr, 0, false, "nlm %d"};
    // RGBA8 outputs: GetImageFromGPU's u8 conversion (src/main.cpp:97-103) in the kernel's epilogue -- a quarter of the
    // bytes to write and to download; RGBA16F outputs: round to nearest even there -- half of them
    auto launch = [&](const void *const *tbl, int n_win, const uint32_t *const *, int k, int t0, int bn, void *const *out, int out_fmt, hipStream_t s) {
        return nlm_temporal_out(ctx, p, tbl, n_win, k, t0, bn, out, out_fmt, s, 1);
    };
    return run_pipeline(ctx, st, launch, host_frames, n, k, first, count, host_out, out_fmt, overlap, timings_ms);
}

// Frames are independent (k = 0), so a frame block is a sub-array: no _range variant.  A non-NULL layer table with n_layers == 0
// is the layered form with zero layers (magenta output), as in mid_bilateral_layers.
extern "C" int mid_sequence_bilateral(mid_ctx *ctx, const mid_bilateral_params *p, const void *const *host_frames, int n_frames,
                                      const void *const *host_layers, int n_layers, void *const *host_out, int out_format,
                                      int overlap, float *timings_ms)
{
    Bind b(ctx, nullptr);
    if (b.rc) return b.rc;
    if (int rc = refuse_if_recording(ctx->compute, "mid_sequence_bilateral (four streams, host-side waits)")) return rc;
    MID_REQUIRE(p, "sequence_bilateral: NULL argument");
    if (int rc = bilateral_check_params(p, "sequence_bilateral", host_layers != nullptr)) return rc;
    MID_REQUIRE(n_layers >= 0 && n_layers <= kMaxLayers, "sequence_bilateral: n_layers %d outside 0..16", n_layers);
    MID_REQUIRE(!host_layers || p->layout == MID_LAYOUT_TEXTURE, "sequence_bilateral: layers exist for the texture layout only");
    if (int rc = check_sequence({"sequence_bilateral", "n_frames", false, true}, host_frames, n_frames, host_layers, n_layers, 0, 0, n_frames, host_out, out_format)) return rc;
    const size_t npix = (size_t)p->width * p->height;
    const Stage st{"sequence_bilateral", p->width, p->height, fmt_frames(p->format), npix * fmt_bytes(fmt_guide(p->format)), host_layers, n_layers, true, "bilateral %d"};
    auto launch = [&](const void *const *tbl, int, const uint32_t *const *lt, int, int t0, int bn, void *const *out, int out_fmt, hipStream_t s) {
        for (int i = 0; i < bn; ++i)              // (k = 0: output t0 + i reads slot t0 + i and its layers only)
            if (int rc = bilateral_out(ctx, p, tbl[t0 + i], host_layers ? lt + (size_t)(t0 + i) * n_layers : nullptr, n_layers, out[i], out_fmt, s)) return rc;
        return (int)MID_OK;
    };
    return run_pipeline(ctx, st, launch, host_frames, n_frames, 0, 0, n_frames, host_out, out_format, overlap, timings_ms);
}

// Layer-guided NLM of every frame: mid_sequence_bilateral's schedule with nlm_layers_out as the compute stage.  n_layers == 0 is
// "no layers", with or without a table.
extern "C" int mid_sequence_nlm_layers(mid_ctx *ctx, const mid_nlm_params *p, const void *const *host_frames, int n_frames,
                                       const void *const *host_layers, int n_layers, void *const *host_out, int out_format,
                                       int overlap, float *timings_ms)
{
    Bind b(ctx, nullptr);
    if (b.rc) return b.rc;
    if (int rc = refuse_if_recording(ctx->compute, "mid_sequence_nlm_layers (four streams, host-side waits)")) return rc;
    MID_REQUIRE(p, "sequence_nlm_layers: NULL argument");
    if (int rc = nlm_check_params(p)) return rc;
    MID_REQUIRE(n_layers >= 0 && n_layers <= kMaxLayers, "sequence_nlm_layers: n_layers %d outside 0..16", n_layers);
    MID_REQUIRE(host_layers || n_layers == 0, "sequence_nlm_layers: host_layers is NULL");
    if (int rc = check_sequence({"sequence_nlm_layers", "n_frames", false, true}, host_frames, n_frames, host_layers, n_layers, 0, 0, n_frames, host_out, out_format)) return rc;
    const Stage st{"sequence_nlm_layers", p->width, p->height, p->format, (size_t)p->width * p->height * 4, n_layers ? host_layers : nullptr, n_layers, true, "nlm_layers %d"};
    auto launch = [&](const void *const *tbl, int, const uint32_t *const *lt, int, int t0, int bn, void *const *out, int out_fmt, hipStream_t s) {
        for (int i = 0; i < bn; ++i)              // (k = 0, as in mid_sequence_bilateral)
            if (int rc = nlm_layers_out(ctx, p, tbl[t0 + i], lt + (size_t)(t0 + i) * n_layers, n_layers, out[i], out_fmt, s)) return rc;
        return (int)MID_OK;
    };
    return run_pipeline(ctx, st, launch, host_frames, n_frames, 0, 0, n_frames, host_out, out_format, overlap, timings_ms);
}

// Layer-guided NLM over neighbouring frames: sequence_impl's temporal window (ring of 2k+4 frames, outputs [first, first+count),
// halo frames uploaded only as far as the windows need them) with mid_sequence_nlm_layers' layer ring.
extern "C" int mid_sequence_nlm_layers_temporal(mid_ctx *ctx, const mid_nlm_params *p, const void *const *host_frames, int n_frames,
                                                const void *const *host_layers, int n_layers, int k, int first, int count,
                                                void *const *host_out, int out_format, int overlap, float *timings_ms)
{
    Bind b(ctx, nullptr);
    if (b.rc) return b.rc;
    if (int rc = refuse_if_recording(ctx->compute, "mid_sequence_nlm_layers_temporal (four streams, host-side waits)")) return rc;
    MID_REQUIRE(p, "sequence_nlm_layers_temporal: NULL argument");
    if (int rc = nlm_check_params(p)) return rc;
    MID_REQUIRE(n_layers >= 0 && n_layers <= kMaxLayers, "sequence_nlm_layers_temporal: n_layers %d outside 0..16", n_layers);
    MID_REQUIRE(host_layers || n_layers == 0, "sequence_nlm_layers_temporal: host_layers is NULL");
    if (int rc = check_sequence({"sequence_nlm_layers_temporal", "n_frames", true, true}, host_frames, n_frames, host_layers, n_layers, k, first, count, host_out, out_format)) return rc;
    if (int rc = nlm_layers_temporal_fits("sequence_nlm_layers_temporal", n_layers, n_frames, k)) return rc;
    const Stage st{"sequence_nlm_layers_temporal", p->width, p->height, p->format, (size_t)p->width * p->height * 4, n_layers ? host_layers : nullptr, n_layers, true, "nlm_layers %d"};
    auto launch = [&](const void *const *tbl, int n_win, const uint32_t *const *lt, int k, int t0, int bn, void *const *out, int out_fmt, hipStream_t s) {
        return nlm_layers_temporal_out(ctx, p, tbl, lt, n_layers, n_win, k, t0, bn, out, out_fmt, s);
    };
    return run_pipeline(ctx, st, launch, host_frames, n_frames, k, first, count, host_out, out_format, overlap, timings_ms);
}

// Joint layer-guided NLM over neighbouring frames: mid_sequence_nlm_layers_temporal's schedule and layer ring (4 B per texel) with
// nlm_joint_out as the compute stage and its checks (layer_h: n_layers floats, or NULL for filteringParameter in every layer).
extern "C" int mid_sequence_nlm_joint(mid_ctx *ctx, const mid_nlm_params *p, const float *layer_h, const void *const *host_frames,
                                      int n_frames, const void *const *host_layers, int n_layers, int k, int first, int count,
                                      void *const *host_out, int out_format, int overlap, float *timings_ms)
{
    Bind b(ctx, nullptr);
    if (b.rc) return b.rc;
    if (int rc = refuse_if_recording(ctx->compute, "mid_sequence_nlm_joint (four streams, host-side waits)")) return rc;
    MID_REQUIRE(p, "sequence_nlm_joint: NULL argument");
    if (int rc = nlm_joint_check(p, "sequence_nlm_joint", layer_h, host_layers != nullptr, n_layers, n_frames, k)) return rc;
    if (int rc = check_sequence({"sequence_nlm_joint", "n_frames", true, true}, host_frames, n_frames, host_layers, n_layers, k, first, count, host_out, out_format)) return rc;
    const Stage st{"sequence_nlm_joint", p->width, p->height, p->format, (size_t)p->width * p->height * 4, host_layers, n_layers, true, "nlm_joint %d"};
    auto launch = [&](const void *const *tbl, int n_win, const uint32_t *const *lt, int k, int t0, int bn, void *const *out, int out_fmt, hipStream_t s) {
        return nlm_joint_out(ctx, p, layer_h, tbl, lt, n_layers, n_win, k, t0, bn, out, out_fmt, s);
    };
    return run_pipeline(ctx, st, launch, host_frames, n_frames, k, first, count, host_out, out_format, overlap, timings_ms);
}

// The bilateral over neighbouring frames: mid_sequence_nlm_layers_temporal's schedule and layer ring; host_layers == NULL is the
// plain form, a table with n_layers == 0 the layered form with zero layers.
// joint: mid_sequence_bilateral_joint, the same call with bilateral_joint_out as the compute stage and its checks (layer_sigma:
// n_layers floats or NULL for colorSigma in every layer).
static int sequence_bilateral_temporal(mid_ctx *ctx, const char *who, bool joint, const mid_bilateral_params *p, const float *layer_sigma,
                                       const void *const *host_frames, int n_frames, const void *const *host_layers, int n_layers, int k,
                                       int first, int count, void *const *host_out, int out_format, int overlap, float *timings_ms)
{
    Bind b(ctx, nullptr);
    if (b.rc) return b.rc;
    if (int rc = refuse_if_recording(ctx->compute, joint ? "mid_sequence_bilateral_joint (four streams, host-side waits)" : "mid_sequence_bilateral_temporal (four streams, host-side waits)")) return rc;
    MID_REQUIRE(p, "%s: NULL argument", who);
    if (int rc = joint ? bilateral_joint_check(p, who, layer_sigma, host_layers != nullptr, n_layers, n_frames, k)
                       : bilateral_temporal_check(p, who, host_layers != nullptr, n_layers, n_frames, k)) return rc;
    if (int rc = check_sequence({who, "n_frames", true, true}, host_frames, n_frames, host_layers, n_layers, k, first, count, host_out, out_format)) return rc;
    const size_t npix = (size_t)p->width * p->height;
    const Stage st{who, p->width, p->height, fmt_frames(p->format), npix * fmt_bytes(fmt_guide(p->format)), host_layers, n_layers, true, "bilateral %d"};
    auto launch = [&](const void *const *tbl, int n_win, const uint32_t *const *lt, int k, int t0, int bn, void *const *out, int out_fmt, hipStream_t s) {
        if (joint) return bilateral_joint_out(ctx, p, layer_sigma, tbl, lt, n_layers, n_win, k, t0, bn, out, out_fmt, s);
        return bilateral_temporal_out(ctx, p, tbl, host_layers ? lt : nullptr, n_layers, n_win, k, t0, bn, out, out_fmt, s);
    };
    return run_pipeline(ctx, st, launch, host_frames, n_frames, k, first, count, host_out, out_format, overlap, timings_ms);
}

extern "C" int mid_sequence_bilateral_temporal(mid_ctx *ctx, const mid_bilateral_params *p, const void *const *host_frames, int n_frames,
                                               const void *const *host_layers, int n_layers, int k, int first, int count,
                                               void *const *host_out, int out_format, int overlap, float *timings_ms)
{
    return sequence_bilateral_temporal(ctx, "sequence_bilateral_temporal", false, p, nullptr, host_frames, n_frames, host_layers, n_layers, k,
                                       first, count, host_out, out_format, overlap, timings_ms);
}

extern "C" int mid_sequence_bilateral_joint(mid_ctx *ctx, const mid_bilateral_params *p, const float *layer_sigma,
                                            const void *const *host_frames, int n_frames, const void *const *host_layers, int n_layers,
                                            int k, int first, int count, void *const *host_out, int out_format, int overlap, float *timings_ms)
{
    return sequence_bilateral_temporal(ctx, "sequence_bilateral_joint", true, p, layer_sigma, host_frames, n_frames, host_layers, n_layers, k,
                                       first, count, host_out, out_format, overlap, timings_ms);
}

// The a-trous filter of every frame: mid_sequence_bilateral_joint's schedule at k = 0 (frames are independent, outputs [first,
// first + count) of the sequence) with atrous_joint_out as the compute stage.  The levels between the passes come from the
// context's cache: one set of up to two RGBA32F frames per kernel stream, so that consecutive outputs, which alternate between
// the two streams, never share a level.
extern "C" int mid_sequence_atrous_joint(mid_ctx *ctx, const mid_atrous_params *p, const float *layer_sigma,
                                         const void *const *host_frames, int n_frames, const void *const *host_layers, int n_layers,
                                         int first, int count, void *const *host_out, int out_format, int overlap, float *timings_ms)
{
    Bind b(ctx, nullptr);
    if (b.rc) return b.rc;
    const char *who = "sequence_atrous_joint";
    if (int rc = refuse_if_recording(ctx->compute, "mid_sequence_atrous_joint (four streams, host-side waits)")) return rc;
    if (int rc = atrous_check(p, who, layer_sigma, host_layers != nullptr, n_layers)) return rc;
    if (int rc = check_sequence({who, "n_frames", true, true}, host_frames, n_frames, host_layers, n_layers, 0, first, count, host_out, out_format)) return rc;
    const size_t npix = (size_t)p->width * p->height;
    const int n_levels = (int)atrous_scratch_frames(p->n_passes);
    Stage st{who, p->width, p->height, fmt_frames(p->format), npix * fmt_bytes(fmt_guide(p->format)), host_layers, n_layers, true, "atrous %d"};
    st.level_bytes = npix * 16; st.n_levels = n_levels;
    auto launch = [&](const void *const *tbl, int, const uint32_t *const *lt, int, int t0, int bn, void *const *out, int out_fmt, hipStream_t s) {
        void *const *lv = ctx->pipe.atrous.p.data() + (s == ctx->compute2 ? n_levels : 0);
        for (int i = 0; i < bn; ++i)              // (k = 0: output t0 + i reads slot t0 + i and its layers only)
            if (int rc = atrous_joint_out(ctx, p, layer_sigma, tbl[t0 + i], lt + (size_t)(t0 + i) * n_layers, n_layers, out[i], out_fmt,
                                          n_levels >= 1 ? lv[0] : nullptr, n_levels >= 2 ? lv[1] : nullptr, s)) return rc;
        return (int)MID_OK;
    };
    return run_pipeline(ctx, st, launch, host_frames, n_frames, 0, first, count, host_out, out_format, overlap, timings_ms);
}

// The guided filter of every frame (section a4o): mid_sequence_atrous_joint's schedule at k = 0 with guided_out as the compute
// stage.  A frame's guide plane travels as the stage's single layer (none when the frames guide themselves); the workspace comes
// from the context's cache as the a-trous levels do, one per kernel stream.
extern "C" int mid_sequence_guided(mid_ctx *ctx, const mid_guided_params *p, const void *const *host_frames, int n_frames,
                                   const void *const *host_guides, int first, int count, void *const *host_out, int out_format,
                                   int overlap, float *timings_ms)
{
    Bind b(ctx, nullptr);
    if (b.rc) return b.rc;
    const char *who = "sequence_guided";
    if (int rc = refuse_if_recording(ctx->compute, "mid_sequence_guided (four streams, host-side waits)")) return rc;
    if (int rc = guided_check(p, who)) return rc;
    const int n_layers = host_guides ? 1 : 0;
    if (int rc = check_sequence({who, "n_frames", true, true}, host_frames, n_frames, host_guides, n_layers, 0, first, count, host_out, out_format)) return rc;
    const size_t npix = (size_t)p->width * p->height;
    Stage st{who, p->width, p->height, fmt_frames(p->format), npix * fmt_bytes(fmt_guide(p->format)), host_guides, n_layers, true, "guided %d"};
    st.level_bytes = guided_work_bytes(p); st.n_levels = 1;
    auto launch = [&](const void *const *tbl, int, const uint32_t *const *lt, int, int t0, int bn, void *const *out, int out_fmt, hipStream_t s) {
        void *work = ctx->pipe.atrous.p[s == ctx->compute2 ? 1 : 0];
        for (int i = 0; i < bn; ++i)              // (k = 0: output t0 + i reads slot t0 + i and its guide only)
            if (int rc = guided_out(ctx, p, tbl[t0 + i], n_layers ? (const void *)lt[t0 + i] : nullptr, work, out[i], out_fmt, s)) return rc;
        return (int)MID_OK;
    };
    return run_pipeline(ctx, st, launch, host_frames, n_frames, 0, first, count, host_out, out_format, overlap, timings_ms);
}

// The median of every frame (section a4p): mid_sequence_atrous_joint's schedule at k = 0 with median_out as the compute stage and no
// levels.  host_layers == NULL (with n_layers == 0) is the plain form: nothing is uploaded beside the frames.
extern "C" int mid_sequence_median(mid_ctx *ctx, const mid_median_params *p, const float *layer_sigma, const void *const *host_frames,
                                   int n_frames, const void *const *host_layers, int n_layers, int first, int count, void *const *host_out,
                                   int out_format, int overlap, float *timings_ms)
{
    Bind b(ctx, nullptr);
    if (b.rc) return b.rc;
    const char *who = "sequence_median";
    if (int rc = refuse_if_recording(ctx->compute, "mid_sequence_median (four streams, host-side waits)")) return rc;
    if (int rc = median_check(p, who, layer_sigma, host_layers != nullptr, n_layers)) return rc;
    if (int rc = check_sequence({who, "n_frames", true, true}, host_frames, n_frames, host_layers, n_layers, 0, first, count, host_out, out_format)) return rc;
    const size_t npix = (size_t)p->width * p->height;
    const Stage st{who, p->width, p->height, fmt_frames(p->format), npix * fmt_bytes(fmt_guide(p->format)), host_layers, n_layers, true, "median %d"};
    auto launch = [&](const void *const *tbl, int, const uint32_t *const *lt, int, int t0, int bn, void *const *out, int out_fmt, hipStream_t s) {
        for (int i = 0; i < bn; ++i)              // (k = 0: output t0 + i reads slot t0 + i and its layers only)
            if (int rc = median_out(ctx, p, layer_sigma, tbl[t0 + i], n_layers ? lt + (size_t)(t0 + i) * n_layers : nullptr, n_layers, out[i], out_fmt, s))
                return rc;
        return (int)MID_OK;
    };
    return run_pipeline(ctx, st, launch, host_frames, n_frames, 0, first, count, host_out, out_format, overlap, timings_ms);
}

// The a-trous filter over neighbouring frames: mid_sequence_atrous_joint with a window -- mid_sequence_bilateral_joint's schedule
// and layer ring at k, the launch callable of sequence_bilateral_temporal's window tables, the levels of the call above.
extern "C" int mid_sequence_atrous_joint_temporal(mid_ctx *ctx, const mid_atrous_params *p, const float *layer_sigma,
                                                  const void *const *host_frames, int n_frames, const void *const *host_layers, int n_layers,
                                                  int k, int first, int count, void *const *host_out, int out_format, int overlap,
                                                  float *timings_ms)
{
    Bind b(ctx, nullptr);
    if (b.rc) return b.rc;
    const char *who = "sequence_atrous_joint_temporal";
    if (int rc = refuse_if_recording(ctx->compute, "mid_sequence_atrous_joint_temporal (four streams, host-side waits)")) return rc;
    if (int rc = atrous_temporal_check(p, who, layer_sigma, host_layers != nullptr, n_layers, n_frames, k)) return rc;
    if (int rc = check_sequence({who, "n_frames", true, true}, host_frames, n_frames, host_layers, n_layers, k, first, count, host_out, out_format)) return rc;
    const size_t npix = (size_t)p->width * p->height;
    const int n_levels = (int)atrous_scratch_frames(p->n_passes);
    Stage st{who, p->width, p->height, fmt_frames(p->format), npix * fmt_bytes(fmt_guide(p->format)), host_layers, n_layers, true, "atrous %d"};
    st.level_bytes = npix * 16; st.n_levels = n_levels;
    auto launch = [&](const void *const *tbl, int n_win, const uint32_t *const *lt, int k, int t0, int bn, void *const *out, int out_fmt, hipStream_t s) {
        void *const *lv = ctx->pipe.atrous.p.data() + (s == ctx->compute2 ? n_levels : 0);
        return atrous_temporal_out(ctx, p, layer_sigma, tbl, lt, n_layers, n_win, k, t0, bn, out, out_fmt,
                                   n_levels >= 1 ? lv[0] : nullptr, n_levels >= 2 ? lv[1] : nullptr, s);
    };
    return run_pipeline(ctx, st, launch, host_frames, n_frames, k, first, count, host_out, out_format, overlap, timings_ms);
}

// The variance-guided a-trous filter of an animation: mid_sequence_atrous_joint_temporal's schedule and layer ring at k, where k is
// the window of the MOMENTS.  Per output: the moments over the window into a V_0 plane, then the passes on frame t alone with frame
// t's layers.  Everything between the kernels lives in ONE block of the context's cache per kernel stream -- the colour levels,
// the variance levels (mid_atrous_variance's scratch layout) and, behind them, the V_0 plane.
extern "C" int mid_sequence_atrous_variance(mid_ctx *ctx, const mid_atrous_variance_params *p, const float *layer_sigma,
                                            const void *const *host_frames, int n_frames, const void *const *host_layers, int n_layers,
                                            int k, int first, int count, void *const *host_out, int out_format, int overlap,
                                            float *timings_ms)
{
    Bind b(ctx, nullptr);
    if (b.rc) return b.rc;
    const char *who = "sequence_atrous_variance";
    if (int rc = refuse_if_recording(ctx->compute, "mid_sequence_atrous_variance (four streams, host-side waits)")) return rc;
    if (int rc = atrous_variance_check(p, who, layer_sigma, host_layers != nullptr, n_layers)) return rc;
    MID_REQUIRE(p->first_pass == 0, "%s: first_pass %d: the moments estimate the variance of the unfiltered frame (continue a filter with mid_atrous_variance)", who, p->first_pass);
    const mid_atrous_moments_params mp{p->width, p->height, p->format};
    if (int rc = atrous_moments_check(&mp, who, layer_sigma, host_layers != nullptr, n_layers, n_frames, k)) return rc;
    if (int rc = check_sequence({who, "n_frames", true, true}, host_frames, n_frames, host_layers, n_layers, k, first, count, host_out, out_format)) return rc;
    const size_t npix = (size_t)p->width * p->height;
    const size_t sets = atrous_scratch_frames(p->n_passes);
    const size_t v0_at = (sets * npix * (16 + 4) + 15) & ~(size_t)15;
    Stage st{who, p->width, p->height, fmt_frames(p->format), npix * fmt_bytes(fmt_guide(p->format)), host_layers, n_layers, true, "atrous variance %d"};
    st.level_bytes = v0_at + npix * 4; st.n_levels = 1;
    auto launch = [&](const void *const *tbl, int n_win, const uint32_t *const *lt, int k, int t0, int bn, void *const *out, int out_fmt, hipStream_t s) {
        char *blk = (char *)ctx->pipe.atrous.p[s == ctx->compute2 ? 1 : 0];
        void *level[2] = {sets >= 1 ? blk : nullptr, sets >= 2 ? blk + npix * 16 : nullptr};
        char *vb = blk + sets * npix * 16;
        float *vlevel[2] = {sets >= 1 ? (float *)vb : nullptr, sets >= 2 ? (float *)(vb + npix * 4) : nullptr};
        float *v0 = (float *)(blk + v0_at);
        for (int i = 0; i < bn; ++i) {
            const int t = t0 + i;
            if (int rc = atrous_moments_out(ctx, &mp, layer_sigma, tbl, lt, n_layers, n_win, k, t, v0, s)) return rc;
            if (int rc = atrous_variance_out(ctx, p, layer_sigma, tbl[t], v0, lt + (size_t)t * n_layers, n_layers, out[i], out_fmt, nullptr,
                                             level, vlevel, s)) return rc;
        }
        return (int)MID_OK;
    };
    return run_pipeline(ctx, st, launch, host_frames, n_frames, k, first, count, host_out, out_format, overlap, timings_ms);
}

// Recursive temporal accumulation of an animation (section a4j): per frame t from s = max(0, first - warmup) on, IN ORDER on one
// kernel stream, mid_atrous_moments at k = 0 -> Vs, mid_temporal_accumulate with the history frame t-1 left (none for frame s), then
// mid_atrous_variance on the accumulated colour and variance.  feedback 0: the next colour history is the accumulated colour;
// feedback 1: the level after pass 0, which is then run on its own into the history buffer and continued with first_pass = 1
// (a4i's chain identity keeps the bits of the public calls).  Frames s .. first-1 are warm-up: computed, not stored.  The window
// of the schedule is k = 1 -- frame t-1's layers must be resident -- and ONE block of the context's cache holds the two
// histories (colour and state each), the accumulated colour, Vs, the blended variance, the variance after pass 0, and the levels:
// 132 B per pixel.
// With an albedo plane per frame (section a4k) the chain runs on ILLUMINATION: frame t is demodulated into an RGBA32F plane of the
// block, the three steps read that plane as an RGBA32F frame, the passes' final level goes as RGBA32F into one more plane, and
// mid_modulate with frame t's albedo stores the output.  The histories hold illumination.  The block then has 164 B per pixel.
// With firefly parameters (section a4l) mid_firefly_clamp runs in front of the three steps, after the demodulation: it reads the
// illumination plane, or the frame itself, into one more RGBA32F plane of the block (16 B per pixel more), which the three steps
// read as an RGBA32F frame.
// With colour-bounds parameters (section a4m) mid_color_bounds runs on the plane the accumulation reads -- the frame itself, or the
// illumination / clamped plane -- into two more RGBA32F planes at the block's end (32 B per pixel more), and the accumulation is
// mid_temporal_accumulate_clip with them.  The box of frame s is computed too (its accumulation has no history and clips nothing).
// The block: 132 B per pixel, + 32 with albedo, + 16 with firefly parameters, + 32 with the clip: at most 212.
extern "C" int mid_sequence_atrous_recursive_clip(mid_ctx *ctx, const mid_temporal_accum_params *ap, const mid_atrous_variance_params *vp,
                                                  const float *layer_sigma, const void *const *host_frames, int n_frames,
                                                  const void *const *host_layers, int n_layers, const void *const *host_motion,
                                                  const void *const *host_albedo, float albedo_floor, const mid_firefly_params *ff,
                                                  const mid_color_bounds_params *cb, int feedback, int warmup, int first, int count,
                                                  void *const *host_out, int out_format, int overlap, float *timings_ms)
{
    Bind b(ctx, nullptr);
    if (b.rc) return b.rc;
    const char *who = cb ? "sequence_atrous_recursive_clip" : ff ? "sequence_atrous_recursive_firefly" : host_albedo ? "sequence_atrous_recursive_albedo" : "sequence_atrous_recursive";
    if (int rc = refuse_if_recording(ctx->compute, cb ? "mid_sequence_atrous_recursive_clip (four streams, host-side waits)"
                                                   : ff ? "mid_sequence_atrous_recursive_firefly (four streams, host-side waits)"
                                                   : host_albedo ? "mid_sequence_atrous_recursive_albedo (four streams, host-side waits)"
                                                                 : "mid_sequence_atrous_recursive (four streams, host-side waits)")) return rc;
    if (int rc = temporal_accumulate_check(ap, who, layer_sigma, host_layers != nullptr, n_layers)) return rc;
    if (int rc = atrous_variance_check(vp, who, layer_sigma, host_layers != nullptr, n_layers)) return rc;
    MID_REQUIRE(vp->first_pass == 0, "%s: first_pass %d: the passes start on the accumulated colour (continue a filter with mid_atrous_variance)", who, vp->first_pass);
    MID_REQUIRE(ap->width == vp->width && ap->height == vp->height && ap->format == vp->format,
                "%s: the two parameter blocks disagree on size or format (%dx%d 0x%x against %dx%d 0x%x)", who, ap->width, ap->height, ap->format,
                vp->width, vp->height, vp->format);
    MID_REQUIRE(feedback == 0 || feedback == 1, "%s: feedback %d is neither 0 (the accumulated colour) nor 1 (the level after pass 0)", who, feedback);
    MID_REQUIRE(warmup >= 0, "%s: warmup %d < 0", who, warmup);
    const mid_albedo_params dp{ap->width, ap->height, albedo_floor, ap->format};     // demodulate: the frames' format, the albedo in the guide format
    if (host_albedo) { if (int rc = albedo_check(&dp, who)) return rc; }
    mid_firefly_params fq{};                                // the clamp reads the illumination plane (RGBA32F) or the frame itself
    if (ff) {
        if (int rc = firefly_check(ff, who)) return rc;
        MID_REQUIRE(ff->width == ap->width && ff->height == ap->height, "%s: the firefly parameters are for %dx%d, the frames are %dx%d", who, ff->width,
                    ff->height, ap->width, ap->height);
        MID_REQUIRE(ff->format == fmt_frames(ap->format), "%s: the firefly format 0x%x is not the frames' format %d without guide bits", who, ff->format,
                    fmt_frames(ap->format));
        fq = *ff;
        if (host_albedo) fq.format = MID_FMT_RGBA32F;
    }
    mid_color_bounds_params cq{};                           // the box reads the plane the accumulation reads: RGBA32F with albedo or firefly
    if (cb) {
        if (int rc = color_bounds_check(cb, who)) return rc;
        MID_REQUIRE(cb->width == ap->width && cb->height == ap->height, "%s: the colour-bounds parameters are for %dx%d, the frames are %dx%d", who,
                    cb->width, cb->height, ap->width, ap->height);
        MID_REQUIRE(cb->format == fmt_frames(ap->format), "%s: the colour-bounds format 0x%x is not the frames' format %d without guide bits", who,
                    cb->format, fmt_frames(ap->format));
        cq = *cb;
        if (host_albedo || ff) cq.format = MID_FMT_RGBA32F;
    }
    const mid_atrous_moments_params mp{ap->width, ap->height, ap->format};
    if (int rc = atrous_moments_check(&mp, who, layer_sigma, host_layers != nullptr, n_layers, 1, 0)) return rc;
    if (int rc = check_sequence({who, "n_frames", true, true}, host_frames, n_frames, host_layers, n_layers, 0, first, count, host_out, out_format)) return rc;
    const int s0 = first - warmup < 0 ? 0 : first - warmup, skip = first - s0;
    {   // the warm-up frames, frame s0 - 1 (the schedule's window uploads it) and frame first + count, their layers, motion and albedo planes
        const int lo = s0 - 1 < 0 ? 0 : s0 - 1, hi = first + count > n_frames - 1 ? n_frames - 1 : first + count;
        std::vector<const void *> inputs;
        for (int f = lo; f <= hi; ++f) {
            MID_REQUIRE(host_frames[f], "%s: frame %d is NULL", who, f);
            inputs.push_back(host_frames[f]);
            for (int l = 0; l < n_layers; ++l) {
                MID_REQUIRE(host_layers[(size_t)f * n_layers + l], "%s: layer %d of frame %d is NULL", who, l, f);
                inputs.push_back(host_layers[(size_t)f * n_layers + l]);
            }
            if (host_motion) {
                MID_REQUIRE(host_motion[f], "%s: the motion plane of frame %d is NULL", who, f);
                inputs.push_back(host_motion[f]);
            }
            if (host_albedo) {
                MID_REQUIRE(host_albedo[f], "%s: the albedo plane of frame %d is NULL", who, f);
                inputs.push_back(host_albedo[f]);
            }
        }
        if (int rc = check_no_alias(who, host_albedo ? "an input frame, layer, motion or albedo plane of this call" : "an input frame, layer or motion plane of this call",
                                    inputs.data(), (int)inputs.size(), (const void *const *)host_out, count)) return rc;
    }
    const size_t npix = (size_t)ap->width * ap->height;
    const int gfmt = fmt_guide(ap->format);
    const size_t plane = (npix * sizeof(float) + 15) & ~(size_t)15;       // one float plane, the next one 16-byte aligned
    mid_atrous_variance_params fp = *vp;                    // the passes read RGBA32F levels, whatever the frames are
    fp.format = MID_FMT_WITH_GUIDE(MID_FMT_RGBA32F, gfmt);
    // with albedo the moments and the accumulation read the demodulated plane: an RGBA32F frame
    mid_temporal_accum_params aq = *ap;
    mid_atrous_moments_params mq = mp;
    const mid_albedo_params mo{ap->width, ap->height, albedo_floor, fp.format};       // modulate: RGBA32F in
    if (host_albedo || ff) aq.format = mq.format = fp.format;
    Stage st{who, ap->width, ap->height, fmt_frames(ap->format), npix * fmt_bytes(gfmt), host_layers, n_layers, true, "atrous recursive %d"};
    st.level_bytes = npix * 16 * 7 + 5 * plane + (host_albedo ? npix * 32 : 0) + (ff ? npix * 16 : 0) + (cb ? npix * 32 : 0); st.n_levels = 1;
    st.in_order = true; st.host_motion = host_motion; st.skip = skip; st.host_albedo = host_albedo;
    const int n_side = n_layers + (host_motion ? 1 : 0) + (host_albedo ? 1 : 0);
    int step = 0;                                           // frames accumulated so far: the launches come in output order
    auto launch = [&](const void *const *tbl, int, const uint32_t *const *lt, int, int t0, int bn, void *const *out, int out_fmt, hipStream_t s) {
        char *blk = (char *)ctx->pipe.atrous.p[0];
        mid_pixel *hc[2] = {(mid_pixel *)blk, (mid_pixel *)(blk + npix * 16)}, *hs[2] = {(mid_pixel *)(blk + npix * 32), (mid_pixel *)(blk + npix * 48)};
        mid_pixel *acc = (mid_pixel *)(blk + npix * 64);
        void *level[2] = {blk + npix * 80, blk + npix * 96};
        char *fb = blk + npix * 112;
        float *vs = (float *)fb, *vt = (float *)(fb + plane), *v1 = (float *)(fb + 2 * plane);
        float *vlevel[2] = {(float *)(fb + 3 * plane), (float *)(fb + 4 * plane)};
        mid_pixel *illum = (mid_pixel *)(fb + 5 * plane), *fin = illum + npix;        // (with albedo only: the block ends before them otherwise)
        mid_pixel *clamped = host_albedo ? fin + npix : illum;                        // (with firefly parameters only: one plane after those)
        mid_pixel *box_lo = ff ? clamped + npix : clamped, *box_hi = box_lo + npix;   // (with the clip only: the block's last two planes)
        for (int i = 0; i < bn; ++i, ++step) {
            const int t = t0 + i, cur = step & 1, prev = cur ^ 1;
            const uint32_t *const *ly = lt + (size_t)t * n_side;
            const uint32_t *const *pl = step ? lt + (size_t)(t - 1) * n_side : ly;
            const float *mv = host_motion ? (const float *)ly[n_layers] : nullptr;
            const void *alb = host_albedo ? (const void *)ly[n_side - 1] : nullptr;
            const void *frame = tbl[t];
            if (alb) {
                if (int rc = demodulate_out(ctx, &dp, tbl[t], alb, illum, s)) return rc;
                frame = illum;
            }
            if (ff) {
                if (int rc = firefly_clamp_out(ctx, &fq, frame, clamped, s)) return rc;
                frame = clamped;
            }
            // the passes' last level: the output itself, or with albedo the plane that mid_modulate reads
            void *last = alb ? (void *)fin : out[i];
            const int last_fmt = alb ? (int)MID_FMT_RGBA32F : out_fmt;
            if (int rc = atrous_moments_out(ctx, &mq, layer_sigma, &frame, ly, n_layers, 1, 0, 0, vs, s)) return rc;
            mid_pixel *col = feedback ? acc : hc[cur];
            if (cb) { if (int rc = color_bounds_out(ctx, &cq, frame, box_lo, box_hi, s)) return rc; }
            if (int rc = temporal_accumulate_out(ctx, &aq, layer_sigma, frame, ly, pl, n_layers, mv, step ? hc[prev] : nullptr, step ? hs[prev] : nullptr,
                                                 vs, cb ? box_lo : nullptr, cb ? box_hi : nullptr, col, hs[cur], vt, s)) return rc;
            if (!feedback) {
                if (int rc = atrous_variance_out(ctx, &fp, layer_sigma, col, vt, ly, n_layers, last, last_fmt, nullptr, level, vlevel, s)) return rc;
            } else {
                mid_atrous_variance_params p0 = fp, p1 = fp;
                p0.n_passes = 1;
                p1.first_pass = 1; p1.n_passes = fp.n_passes - 1;
                if (int rc = atrous_variance_out(ctx, &p0, layer_sigma, col, vt, ly, n_layers, hc[cur], MID_FMT_RGBA32F, v1, level, vlevel, s)) return rc;
                if (p1.n_passes >= 1) {
                    if (int rc = atrous_variance_out(ctx, &p1, layer_sigma, hc[cur], v1, ly, n_layers, last, last_fmt, nullptr, level, vlevel, s)) return rc;
                } else if (int rc = atrous_variance_out(ctx, &p0, layer_sigma, col, vt, ly, n_layers, last, last_fmt, nullptr, level, vlevel, s)) return rc;
            }
            if (alb) { if (int rc = modulate_out(ctx, &mo, fin, alb, out[i], out_fmt, s)) return rc; }
        }
        return (int)MID_OK;
    };
    std::vector<void *> outs((size_t)skip + count, nullptr);
    for (int i = 0; i < count; ++i) outs[(size_t)skip + i] = host_out[i];
    return run_pipeline(ctx, st, launch, host_frames, n_frames, 1, s0, skip + count, outs.data(), out_format, overlap, timings_ms);
}

extern "C" int mid_sequence_atrous_recursive_firefly(mid_ctx *ctx, const mid_temporal_accum_params *ap, const mid_atrous_variance_params *vp,
                                                     const float *layer_sigma, const void *const *host_frames, int n_frames,
                                                     const void *const *host_layers, int n_layers, const void *const *host_motion,
                                                     const void *const *host_albedo, float albedo_floor, const mid_firefly_params *ff, int feedback,
                                                     int warmup, int first, int count, void *const *host_out, int out_format, int overlap,
                                                     float *timings_ms)
{
    return mid_sequence_atrous_recursive_clip(ctx, ap, vp, layer_sigma, host_frames, n_frames, host_layers, n_layers, host_motion, host_albedo, albedo_floor,
                                              ff, nullptr, feedback, warmup, first, count, host_out, out_format, overlap, timings_ms);
}

extern "C" int mid_sequence_atrous_recursive_albedo(mid_ctx *ctx, const mid_temporal_accum_params *ap, const mid_atrous_variance_params *vp,
                                                    const float *layer_sigma, const void *const *host_frames, int n_frames,
                                                    const void *const *host_layers, int n_layers, const void *const *host_motion,
                                                    const void *const *host_albedo, float albedo_floor, int feedback, int warmup, int first,
                                                    int count, void *const *host_out, int out_format, int overlap, float *timings_ms)
{
    return mid_sequence_atrous_recursive_firefly(ctx, ap, vp, layer_sigma, host_frames, n_frames, host_layers, n_layers, host_motion, host_albedo, albedo_floor,
                                                 nullptr, feedback, warmup, first, count, host_out, out_format, overlap, timings_ms);
}

extern "C" int mid_sequence_atrous_recursive(mid_ctx *ctx, const mid_temporal_accum_params *ap, const mid_atrous_variance_params *vp,
                                             const float *layer_sigma, const void *const *host_frames, int n_frames,
                                             const void *const *host_layers, int n_layers, const void *const *host_motion, int feedback,
                                             int warmup, int first, int count, void *const *host_out, int out_format, int overlap,
                                             float *timings_ms)
{
    return mid_sequence_atrous_recursive_albedo(ctx, ap, vp, layer_sigma, host_frames, n_frames, host_layers, n_layers, host_motion, nullptr, 0.f, feedback,
                                                warmup, first, count, host_out, out_format, overlap, timings_ms);
}

// Device timeline of the context's last mid_sequence_nlm*, mid_sequence_bilateral or mid_sequence_nlm_layers[_temporal] call, read back from the events the call left in the context's
// cache (valid until the next pipeline call on this context; no profiler involved, so the call ran at its own pace).
extern "C" int mid_pipe_last_timeline(mid_ctx *ctx, int cap, float *upload_ms, int *n_uploads, int *first_upload_frame,
                                      float *output_ms, int *n_outputs, int *first_output_frame)
{
    Bind b(ctx, nullptr);
    if (b.rc) return b.rc;
    MID_REQUIRE(upload_ms && n_uploads && first_upload_frame && output_ms && n_outputs && first_output_frame && cap >= 0,
                "pipe_last_timeline: bad argument");
    std::lock_guard<std::mutex> pipe_lock(ctx->pipe.mu);
    mid_pipe_last &L = ctx->pipe.last;
    MID_REQUIRE(L.n_up > 0, "pipe_last_timeline: no mid_sequence_nlm* or mid_sequence_bilateral call has completed on this context");
    MID_REQUIRE(cap >= L.n_up && cap >= L.nb, "pipe_last_timeline: cap=%d, need %d uploads and %d outputs", cap, L.n_up, L.nb);
    MID_REQUIRE(ctx->pipe.ev.size() >= 2 * (size_t)L.n_up + 4 * (size_t)L.nb, "pipe_last_timeline: the event cache was released");
    // The events are read back once per call of the pipeline.  hipEventElapsedTime of the same two events is not the same float
    // every time it is asked (the runtime may convert the timestamps anew, a nanosecond apart, after work on other streams), and
    // "the timeline of the last call" must not change while no pipeline call has run: a refused call leaves it alone.
    if (L.up_ms.empty()) {
        std::vector<float> up(2 * (size_t)L.n_up), out(4 * (size_t)L.nb);
        hipEvent_t *up0 = ctx->pipe.ev.data(), *up1 = up0 + L.n_up, *c0 = up1 + L.n_up, *c1 = c0 + L.nb, *d0 = c1 + L.nb, *d1 = d0 + L.nb;
        for (int i = 0; i < L.n_up; ++i) {
            MID_HIP(hipEventElapsedTime(&up[2 * i], up0[0], up0[i]));
            MID_HIP(hipEventElapsedTime(&up[2 * i + 1], up0[0], up1[i]));
        }
        for (int i = 0; i < L.nb; ++i) {
            MID_HIP(hipEventElapsedTime(&out[4 * i], up0[0], c0[i]));
            MID_HIP(hipEventElapsedTime(&out[4 * i + 1], up0[0], c1[i]));
            // direct (kernel-stored) outputs have no download stage: reported as an empty interval at the end of the launch
            MID_HIP(hipEventElapsedTime(&out[4 * i + 2], up0[0], L.direct ? c1[i] : d0[i]));
            MID_HIP(hipEventElapsedTime(&out[4 * i + 3], up0[0], L.direct ? c1[i] : d1[i]));
        }
        L.up_ms.swap(up); L.out_ms.swap(out);
    }
    memcpy(upload_ms, L.up_ms.data(), L.up_ms.size() * sizeof(float));
    memcpy(output_ms, L.out_ms.data(), L.out_ms.size() * sizeof(float));
    *n_uploads = L.n_up; *first_upload_frame = L.f_lo; *n_outputs = L.nb; *first_output_frame = L.first;
    return MID_OK;
}

extern "C" int mid_sequence_nlm_range(mid_ctx *ctx, const mid_nlm_params *p, const void *const *host_frames,
                                      int n, int k, int first, int count, mid_pixel *const *host_out,
                                      int overlap, float *timings_ms)
{
    return sequence_impl(ctx, p, host_frames, n, k, first, count, (void *const *)host_out, MID_FMT_RGBA32F, overlap, timings_ms);
}

extern "C" int mid_sequence_nlm_range_u8(mid_ctx *ctx, const mid_nlm_params *p, const void *const *host_frames,
                                         int n, int k, int first, int count, uint8_t *const *host_out,
                                         int overlap, float *timings_ms)
{
    return sequence_impl(ctx, p, host_frames, n, k, first, count, (void *const *)host_out, MID_FMT_RGBA8, overlap, timings_ms);
}

extern "C" int mid_sequence_nlm_range_f16(mid_ctx *ctx, const mid_nlm_params *p, const void *const *host_frames,
                                          int n, int k, int first, int count, uint16_t *const *host_out,
                                          int overlap, float *timings_ms)
{
    return sequence_impl(ctx, p, host_frames, n, k, first, count, (void *const *)host_out, MID_FMT_RGBA16F, overlap, timings_ms);
}

extern "C" int mid_sequence_nlm(mid_ctx *ctx, const mid_nlm_params *p, const void *const *host_frames,
                                int n, int k, mid_pixel *const *host_out, int overlap, float *timings_ms)
{
    return mid_sequence_nlm_range(ctx, p, host_frames, n, k, 0, n, host_out, overlap, timings_ms);
}

// The reference's own multi-frame mode: target fixed, neighbours streamed (see mi_denoise.h).
extern "C" int mid_nlm_multiframe(mid_ctx *ctx, const mid_nlm_params *p, const void *host_target,
                                  const void *const *host_frames, int n, mid_pixel *host_out,
                                  int overlap, float *timings_ms)
{
    Bind b(ctx, nullptr);
    if (b.rc) return b.rc;
    if (int rc = refuse_if_recording(ctx->compute, "mid_nlm_multiframe (three streams, host-side waits)")) return rc;
    MID_REQUIRE(p && host_target && host_frames && host_out, "nlm_multiframe: NULL argument");
    MID_REQUIRE(n >= 1 && p->width > 0 && p->height > 0, "nlm_multiframe: bad n=%d or size", n);
    MID_REQUIRE(fmt_known(p->format), "nlm_multiframe: unknown format %d", p->format);
    for (int i = 0; i < n; ++i) MID_REQUIRE(host_frames[i], "nlm_multiframe: frame %d is NULL", i);
    const size_t npix = (size_t)p->width * p->height;
    const size_t in_bytes = npix * fmt_bytes(p->format), out_bytes = npix * 16;

    // (clock and cached buffers as in sequence_impl: timings_ms[0] covers the whole call)
    const auto wall0 = std::chrono::steady_clock::now();
    Range call_range("mid_nlm_multiframe frames=%d overlap=%d", n, overlap);
    std::lock_guard<std::mutex> pipe_lock(ctx->pipe.mu);
    DrainOnExit drain{ctx};
    mid_pipe_set &dtarget = ctx->pipe.target, &dslot = ctx->pipe.slots, &dW = ctx->pipe.weights, &dout = ctx->pipe.result;
    if (int rc = reserve(dtarget, 1, in_bytes)) return rc;
    constexpr int SLOTS = 3;                                   // neighbour frames in flight: uploads run two dispatches ahead
    if (int rc = reserve(dslot, n < SLOTS ? n : SLOTS, in_bytes)) return rc;
    if (int rc = reserve(dW, 1, npix * sizeof(mid_weightinfo))) return rc;
    if (int rc = reserve(dout, 1, out_bytes)) return rc;
    if (int rc = reserve_events(ctx->pipe, 4 * (size_t)n + 4)) return rc;
    ctx->pipe.last = mid_pipe_last{};                         // the cached events are about to be re-recorded in another layout
    struct Events { hipEvent_t *ev; } up0{ctx->pipe.ev.data()}, up1{up0.ev + n}, c0{up1.ev + n}, c1{c0.ev + n}, misc{c1.ev + n};

    // target + cleared weight buffer (the reference relies on a fresh allocation being zero)
    MID_HIP(hipEventRecord(misc.ev[0], ctx->upload));
    if (int rc = copy_h2d(ctx, dtarget.p[0], host_target, in_bytes, ctx->upload)) return rc;
    MID_HIP(hipEventRecord(misc.ev[1], ctx->upload));
    MID_HIP(hipMemsetAsync(dW.p[0], 0, npix * sizeof(mid_weightinfo), ctx->compute));
    MID_HIP(hipStreamWaitEvent(ctx->compute, misc.ev[1], 0));

    auto upload = [&](int f) -> int {
        Range r("upload %d", f);
        if (f >= SLOTS) MID_HIP(hipStreamWaitEvent(ctx->upload, c1.ev[f - SLOTS], 0));   // slot still read by dispatch f-SLOTS
        MID_HIP(hipEventRecord(up0.ev[f], ctx->upload));
        if (int rc = copy_h2d(ctx, dslot.p[f % SLOTS], host_frames[f], in_bytes, ctx->upload)) return rc;
        MID_HIP(hipEventRecord(up1.ev[f], ctx->upload));
        return MID_OK;
    };
    int next_upload = 0;
    for (int f = 0; f < n; ++f) {
        while (next_upload <= f) { if (int rc = upload(next_upload++)) return rc; }
        {
            Range r("nlm %d", f);
            MID_HIP(hipStreamWaitEvent(ctx->compute, up1.ev[f], 0));
            MID_HIP(hipEventRecord(c0.ev[f], ctx->compute));
            if (int rc = mid_nlm_accum(ctx, p, dtarget.p[0], dslot.p[f % SLOTS], (mid_weightinfo *)dW.p[0], ctx->compute)) return rc;
            MID_HIP(hipEventRecord(c1.ev[f], ctx->compute));
        }
        // overlap: frames f+1, f+2 ride beside dispatch f (their slots were last read by dispatches already enqueued).  They are
        // started AFTER dispatch f has been queued, as in sequence_impl: a pageable frame blocks the calling thread inside
        // copy_h2d until its chunks have gone through the bounce buffers, and the device must not sit idle meanwhile.
        const int ahead = overlap ? (f + SLOTS - 1 < n - 1 ? f + SLOTS - 1 : n - 1) : f;
        while (next_upload <= ahead) { if (int rc = upload(next_upload++)) return rc; }
        if (!overlap) {   // fence after every submit, src/main.cpp:1092
            MID_HIP(hipStreamSynchronize(ctx->compute));
            MID_HIP(hipStreamSynchronize(ctx->upload));
        }
    }
    mid_normalize_params np{p->width, p->height};
    if (int rc = mid_normalize(ctx, &np, (const mid_weightinfo *)dW.p[0], (mid_pixel *)dout.p[0], ctx->compute)) return rc;
    MID_HIP(hipEventRecord(misc.ev[2], ctx->compute));
    if (int rc = copy_d2h(ctx, host_out, dout.p[0], out_bytes, ctx->compute)) return rc;
    MID_HIP(hipEventRecord(misc.ev[3], ctx->compute));
    MID_HIP(hipStreamSynchronize(ctx->upload));
    MID_HIP(hipStreamSynchronize(ctx->compute));
    const auto wall1 = std::chrono::steady_clock::now();
    if (timings_ms) {
        float kern = 0.f, copy = 0.f, ms = 0.f;
        for (int f = 0; f < n; ++f) {
            MID_HIP(hipEventElapsedTime(&ms, c0.ev[f], c1.ev[f])); kern += ms;
            MID_HIP(hipEventElapsedTime(&ms, up0.ev[f], up1.ev[f])); copy += ms;
        }
        MID_HIP(hipEventElapsedTime(&ms, misc.ev[0], misc.ev[1])); copy += ms;
        MID_HIP(hipEventElapsedTime(&ms, misc.ev[2], misc.ev[3])); copy += ms;
        MID_HIP(hipEventElapsedTime(&ms, c1.ev[n - 1], misc.ev[2])); kern += ms;   // normalize
        timings_ms[0] = std::chrono::duration<float, std::milli>(wall1 - wall0).count();
        timings_ms[1] = kern;
        timings_ms[2] = copy;
    }
    return MID_OK;
}
