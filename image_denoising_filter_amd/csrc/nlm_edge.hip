// nlm_edge.hip -- the ragged right-edge tile column of a LONG launch of the tuned NLM windows, packed four tiles a workgroup.
//
// A wave of the strip kernel yields 64 - (PW - 1) columns, and 1920 = 33 x 58 + 6: a 1080p frame is 34 tile columns of which the last holds 6
// of the image's columns.  Its workgroups -- 34 of a frame's 1156, 2.9 % of a launch -- walk all 441 offsets for a tenth of a tile's outputs,
// in the general form (their tiles hold out-of-image texels and never vote opaque).  Here such a column is covered by the PACKED shape of the
// same kernel (nlm_strip.hpp, TAG = kNlmEdgeTag; same bits): a workgroup per four tile rows, cdiv(tiles_y, 4) x frames workgroups instead of
// tiles_y x frames, while the main launch covers one tile column less.  The packed launch runs BESIDE the main one, on a stream of the
// context's at the device's lowest priority that is forked from and joined to the caller's stream with events -- the sharded call's
// arrangement for its boundary launches (sharded.cpp) -- so that its workgroups go where no workgroup of the main launch waits instead
// of queueing behind the main launch's last round.
//
// Packed: k = 0 launches of the two tuned windows that nlm_small.hip has not taken (more than kNlmSmallRounds rounds of workgroups), when the
// last tile column's columns fit a group of 16 lanes (nlm_edge_packs: valid + PW - 1 <= 12 -- 6 columns at the 7x7 patch, 1920- and 1280-wide
// frames; 7 at 6x6) and the frame has another tile column.  Left whole, one launch as before: a caller's stream that is being captured (a
// recording keeps its one-stream shape, recording.cpp), launches of the frame pipeline (corunning: its two kernel streams fill each other's
// tails already), and a context whose edge stream cannot be had.
//
// Compiled with nlm.hip's flags (Makefile).
#include "nlm_strip.hpp"

namespace mid {

template <int SLO, int SHI, int PLO, int PHI, int FMT, bool FUSED>
static int launch_edge(mid_ctx *ctx, NlmArgs &a, hipStream_t s)
{
    constexpr int PW = PHI - PLO, VW = 64 - (PW - 1), TILE_H = 32, SW = SHI - SLO;
    constexpr size_t lds_bytes = (size_t)kNlmEdgePitch * nlm_edge_tile_rows(TILE_H, PW, SW) * sizeof(float4);
    static_assert(lds_bytes <= 80 * 1024, "two workgroups a CU");
    auto kern = nlm_strip_kernel<SLO, SHI, PLO, PHI, 8, 4, FMT, FUSED, false, false, kNlmEdgeTag>;
    if ((int)lds_bytes > ctx->lds_max)
        return set_error(MID_ERR_UNSUPPORTED, "nlm edge tile needs %zu B of LDS, device offers %d", lds_bytes, ctx->lds_max);
    if (int rc = ensure_lds(ctx, (const void *)kern, lds_bytes)) return rc;
    a.tiles_x = (int)cdiv(a.w, VW);          // the kernel works on tile column tiles_x - 1
    a.tiles_y = (int)cdiv(a.h, TILE_H);
    a.wg_first = 0;
    const unsigned n = cdiv((unsigned)a.tiles_y, (unsigned)kNlmEdgeGroups) * (unsigned)(FUSED ? a.count : 1);
    hipLaunchKernelGGL(kern, dim3(n), dim3(4 * 64), lds_bytes, s, a);
    MID_HIP(hipGetLastError());
    return MID_OK;
}

template <int SLO, int SHI, int PLO, int PHI>
static int edge_window(mid_ctx *ctx, NlmArgs &a, hipStream_t s, int fmt, bool fused)
{
    if (fmt == MID_FMT_RGBA8) return fused ? launch_edge<SLO, SHI, PLO, PHI, MID_FMT_RGBA8, true>(ctx, a, s)
                                           : launch_edge<SLO, SHI, PLO, PHI, MID_FMT_RGBA8, false>(ctx, a, s);
    if (fmt == MID_FMT_RGBA16F) return fused ? launch_edge<SLO, SHI, PLO, PHI, MID_FMT_RGBA16F, true>(ctx, a, s)
                                             : launch_edge<SLO, SHI, PLO, PHI, MID_FMT_RGBA16F, false>(ctx, a, s);
    return fused ? launch_edge<SLO, SHI, PLO, PHI, MID_FMT_RGBA32F, true>(ctx, a, s)
                 : launch_edge<SLO, SHI, PLO, PHI, MID_FMT_RGBA32F, false>(ctx, a, s);
}

// The context's edge stream and its two events, created on first use (ctx->edge.mu held); false: they cannot be had.
static bool edge_stream_ready(mid_ctx *ctx)
{
    mid_edge &e = ctx->edge;
    if (e.failed) return false;
    if (e.s) return true;
    int least = 0, greatest = 0;
    bool ok = hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess;          // numerically lower = higher priority
    ok = ok && hipStreamCreateWithPriority(&e.s, hipStreamNonBlocking, least) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&e.fork, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&e.join, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (e.s) (void)hipStreamDestroy(e.s);
        for (hipEvent_t *ev : {&e.fork, &e.join}) { if (*ev) (void)hipEventDestroy(*ev); *ev = nullptr; }
        e.s = nullptr;
        e.failed = true;
    }
    return ok;
}

int nlm_dispatch_edge(mid_ctx *ctx, const mid_nlm_params *p, NlmArgs &a, hipStream_t s, int fmt, bool fused, nlm_main_launch main_launch)
{
    const bool bench = p->search_lo == -10 && p->search_hi == 11 && p->patch_lo == -3 && p->patch_hi == 4;
    const bool ref = p->search_lo == -7 && p->search_hi == 7 && p->patch_lo == -3 && p->patch_hi == 3;
    const int pw = p->patch_hi - p->patch_lo;
    const bool packs = (bench || ref) && a.k == 0 && !a.corunning &&
                       nlm_edge_packs(nlm_edge_valid(a.w, pw), pw, (int)cdiv((unsigned)a.w, (unsigned)(64 - (pw - 1)))) && !stream_is_recording(s);
    if (!packs) return main_launch(ctx, a, s, 0);
    std::lock_guard<std::mutex> lock(ctx->edge.mu);
    if (!edge_stream_ready(ctx)) return main_launch(ctx, a, s, 0);
    mid_edge &e = ctx->edge;
    // fork: the edge launch reads what the caller's stream has produced so far ...
    MID_HIP(hipEventRecord(e.fork, s));
    MID_HIP(hipStreamWaitEvent(e.s, e.fork, 0));
    int rc = main_launch(ctx, a, s, 1);
    if (rc == MID_OK) rc = bench ? edge_window<-10, 11, -3, 4>(ctx, a, e.s, fmt, fused) : edge_window<-7, 7, -3, 3>(ctx, a, e.s, fmt, fused);
    // ... join: and the caller's stream goes on behind it (also after a failed launch: whatever was queued on the edge stream is waited for)
    if (hipEventRecord(e.join, e.s) != hipSuccess || hipStreamWaitEvent(s, e.join, 0) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(e.s);        // (a broken device: a host-side join)
    }
    return rc;
}

}  // namespace mid
