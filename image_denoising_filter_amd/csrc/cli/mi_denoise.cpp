// mi_denoise -- drop-in command-line driver (replaces the reference's `vulkan_denoice`,
// src/main.cpp:1935-1994) on top of libmi_denoise.so.
//
//   mi_denoise [image] [options]
//
// With no options it behaves like the reference: the positional argument is the target image
// (default Animations/CornellBox/Animation01_LDR_0000.png, src/main.cpp:1945); six GPU modes and two
// CPU runs execute in the reference's order (src/main.cpp:1952-1985), print the same banners and
// timing lines (:1924-1933) and write output{-linear|-nonlinear}{-nlm|-bialteral}[-multiframe]
// [-overlap][-layers].{png|exr} and output-cpu.{png|exr} into the current directory (:1677-1686,
// :1870-1901).  Unlike the reference it does not need to be started from the repo root (kernels are
// linked in, not loaded from shaders/*.spv).  The parameters the reference hard-codes (windows
// shaders/*.comp:5-6, sigmas/h src/main.cpp:806,870,875,1833-1835, CPU window :1819, device :1321)
// are options whose defaults are those values.
//
// There is no CPU fallback for the GPU modes: if the device is missing they fail and the exit code
// is EXIT_FAILURE.  The two "Running on CPU" modes are the reference's own RunOnCPU feature
// (src/main.cpp:1732-1921), implemented here as part of the driver.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <condition_variable>
#include <iostream>
#include <mutex>
#include <stdexcept>
#include <string>
#include <atomic>
#include <system_error>
#include <thread>
#include <vector>

#include "../../../include/mi_denoise.h"

namespace fs = std::filesystem;

// console colours of the timing lines, src/main.cpp:21-23
#define FOREGROUND_COLOR "\033[38;2;0;0;0m"
#define BACKGROUND_COLOR "\033[48;2;0;255;0m"
#define CLEAR_COLOR      "\033[0m"

struct Pixel { float r, g, b, a; };   // src/main.cpp:39-41

struct Options {
    std::string image = "Animations/CornellBox/Animation01_LDR_0000.png";   // src/main.cpp:1945
    std::string outdir = ".";
    int device = 0;                 // deviceId{0}, src/main.cpp:1321
    int radius = 20;                // TEXEL_WINDOW, shaders/bialteral.comp:5
    float sigma_s = 2.0f, sigma_c = 0.2f;      // src/main.cpp:806,875
    std::vector<float> sigma_layers;           // the joint modes: one range sigma per layer in discovery order (empty: sigma_c for all)
    float nlm_h = 0.5f;             // src/main.cpp:870
    std::vector<float> h_layers;    // the joint NLM modes: one h per layer in discovery order (empty: nlm_h for all)
    int passes = 5;                 // the a-trous modes: passes of the 5x5 kernel, pass i at step 2^i (1..8)
    float atrous_sigma_color = 0.f; // the a-trous modes: sigma of the colour term at pass 0, halved every pass (0: off)
    float atrous_sigma_lum = 4.f;   // atrous-variance: sigma of the luminance term in standard deviations of the pixel (SVGF's 4; 0: off)
    float atrous_epsilon = 1e-3f;   // atrous-variance: what is added to sigma_lum * sqrt(variance) (> 0)
    float alpha = 0.2f, alpha_moments = 0.2f, history_max = 32.f;   // atrous-recursive: mid_temporal_accum_params (historyFull stays SVGF's 4)
    int feedback = 1, warmup = 16;  // atrous-recursive: the next colour history (0: accumulated colour, 1: level after pass 0); warm-up frames of a block
    std::string motion_layer;       // atrous-recursive: substring of the .exr render element that holds the motion (R, G in pixels); empty: zero motion
    float motion_sx = 1.f, motion_sy = 1.f;   // --motion-scale
    std::string albedo_layer;       // atrous-recursive: substring of the render element that holds the albedo; empty: the filter runs on colour
    float albedo_floor = 1e-3f;     // --albedo-floor: lower bound of the divisor (mid_albedo_params.floor)
    bool albedo_floor_given = false;
    int firefly_rank = 0, firefly_radius = 1;       // atrous-recursive: --firefly-rank 1..4 switches the clamp on (mid_firefly_params); 0: off
    float firefly_gain = 1.f, firefly_floor = 0.f;
    const char *firefly_other = nullptr;            // the first of --firefly-radius / --firefly-gain / --firefly-floor given
    bool history_clip = false, history_clip_radius_given = false;   // atrous-recursive: --history-clip GAMMA switches the clip on (mid_color_bounds_params)
    float history_clip_gamma = 1.f;
    int history_clip_radius = 1;
    int search_lo = -7, search_hi = 7, patch_lo = -3, patch_hi = 3;   // shaders/nonlocal.comp:5-6, half-open
    int temporal_k = -1;            // <0: the reference's frame list; >=0: window t-k..t+k of the sorted sequence
    int cpu_radius = 10;            // windowSize, src/main.cpp:1819
    float cpu_sigma_s = 10.0f, cpu_sigma_c = 0.2f;   // src/main.cpp:1833-1835
    bool cpu_blue_bug = true;       // pow(texColor.b - texColor.b, 2), src/main.cpp:1850
    std::vector<int> cpu_threads = {1, 8};     // src/main.cpp:1979,1984
    bool run_gpu = true, run_cpu = true;
    std::string modes = "all";      // comma list of: bilateral,layers,linear,nlm,multiframe,overlap (all of them: "all"), nlm-layers, joint, nlm-joint, atrous, atrous-variance
    bool animation = false;         // new capability: temporal NLM of EVERY frame of the sequence
    std::string animation_filter = "nlm";   // animation mode: nlm | bilateral | linear | layers (the bilateral of every frame) | nlm-layers | nlm-layers-temporal | bilateral-temporal | layers-temporal | joint | joint-temporal | nlm-joint | nlm-joint-temporal | atrous | atrous-temporal | atrous-variance
    int gpus = 1;                   // animation mode: frame blocks over this many devices
    bool share_device = false;      // animation mode: every block on --device (rehearsal of --gpus N on fewer devices)
    bool halo_rccl = false;         // animation mode: blocks resident in HBM, halo frames GPU to GPU over RCCL (mid_nlm_temporal_sharded)
    bool pageable_host = false;     // reference modes: keep decoded images and results in ordinary memory (the C-ABI bounces them)
    long pinned_mb = 16384;         // animation mode: at most this much page-locked host memory (inputs + outputs); the rest is pageable
    int io_threads = 0;             // animation mode: files decoded / encoded at a time (0 = min(16, hardware threads))
    bool half = false;              // GPU modes and animation, .exr inputs: frames as RGBA16F (mid_image_load_f16), HALF EXR outputs
    int guided_radius = 8;          // the guided filter (--modes guided, --animation-filter guided): mid_guided_params.radius, 1..16
    float guided_eps = 1e-2f;       // and its regulariser, in squared guide units
    std::string guide_layer;        // substring of the render element that is the guide; empty: every frame guides itself
    const char *guided_other = nullptr;        // the first of --guided-radius / --guided-eps / --guide-layer given
    int median_radius = 1;          // the median (--modes median, --animation-filter median): mid_median_params.radius, 1..3
    bool median_plain = false;      // --median-plain: no layers are loaded, the plain median
    const char *median_other = nullptr;        // the first of --median-radius / --median-plain given
    bool compare = false;           // --compare TEST REFERENCE: the sub-mode that measures and filters nothing (mid_image_metrics)
    std::string compare_test, compare_ref;
    float peak = 1.f, relmse_eps = 1e-2f;      // --peak, --relmse-eps (mid_image_metrics_params)
    bool compare_ssim = true;       // --no-ssim clears it
    const char *compare_other = nullptr;       // the first of --peak / --relmse-eps / --no-ssim given
};

#define MID_CHECK(call)                                                                          \
    do {                                                                                         \
        if ((call) != 0) throw std::runtime_error(std::string(#call) + ": " + mid_last_error()); \
    } while (0)

// --animation-filter, parsed once: the mid_sequence_* family a value runs, what that family reads, and the words of the value.
enum SeqFamily { SEQ_NLM, SEQ_BILATERAL, SEQ_NLM_LAYERS, SEQ_NLM_LAYERS_TEMPORAL, SEQ_BILATERAL_TEMPORAL, SEQ_BILATERAL_JOINT, SEQ_NLM_JOINT, SEQ_ATROUS, SEQ_ATROUS_TEMPORAL, SEQ_ATROUS_VARIANCE, SEQ_ATROUS_RECURSIVE, SEQ_GUIDED, SEQ_MEDIAN };
struct AnimationFilter {
    const char *name;
    SeqFamily family;
    bool layers;            // every frame is guided by its own RenderElements layers
    bool temporal;          // the frames t-k..t+k (--temporal-k); false: k = 0
    bool linear;            // MID_LAYOUT_LINEAR
    const char *infix;      // output-animation-<infix><frame file name>
    const char *words;      // of the summary line, before r= / the layers / k=
    const char *banner;     // "Running on GPU (animation, <banner>)"
    bool bilateral() const { return family == SEQ_BILATERAL || family == SEQ_BILATERAL_TEMPORAL || family == SEQ_BILATERAL_JOINT; }
    bool windowed() const { return family != SEQ_BILATERAL && family != SEQ_NLM_LAYERS && family != SEQ_ATROUS && family != SEQ_GUIDED && family != SEQ_MEDIAN; }     // blocks with k halo frames on either side
};
static const AnimationFilter kAnimationFilters[] = {
    {"nlm", SEQ_NLM, false, true, false, "", "", "temporal nonlocal"},
    {"bilateral", SEQ_BILATERAL, false, false, false, "nonlinear-bialteral-", "bilateral bilateral", "nonlinear bialteral"},
    {"linear", SEQ_BILATERAL, false, false, true, "linear-bialteral-", "linear bilateral", "linear bialteral"},
    {"layers", SEQ_BILATERAL, true, false, false, "nonlinear-bialteral-layers-", "layers bilateral", "nonlinear bialteral + layers"},
    {"nlm-layers", SEQ_NLM_LAYERS, true, false, false, "nonlinear-nlm-layers-", "nonlocal", "nonlocal + layers"},
    {"nlm-layers-temporal", SEQ_NLM_LAYERS_TEMPORAL, true, true, false, "nonlinear-nlm-layers-multiframe-", "nonlocal", "nonlocal + layers, multiframe"},
    {"bilateral-temporal", SEQ_BILATERAL_TEMPORAL, false, true, false, "nonlinear-bialteral-multiframe-", "bilateral", "nonlinear bialteral, multiframe"},
    {"layers-temporal", SEQ_BILATERAL_TEMPORAL, true, true, false, "nonlinear-bialteral-layers-multiframe-", "bilateral", "nonlinear bialteral + layers, multiframe"},
    {"joint", SEQ_BILATERAL_JOINT, true, false, false, "nonlinear-bialteral-joint-", "joint bilateral", "joint bialteral"},
    {"joint-temporal", SEQ_BILATERAL_JOINT, true, true, false, "nonlinear-bialteral-joint-multiframe-", "joint bilateral", "joint bialteral, multiframe"},
    {"nlm-joint", SEQ_NLM_JOINT, true, false, false, "nonlinear-nlm-joint-", "joint nonlocal", "joint nonlocal"},
    {"nlm-joint-temporal", SEQ_NLM_JOINT, true, true, false, "nonlinear-nlm-joint-multiframe-", "joint nonlocal", "joint nonlocal, multiframe"},
    {"atrous", SEQ_ATROUS, true, false, false, "nonlinear-atrous-", "a-trous", "a-trous + layers"},
    {"atrous-temporal", SEQ_ATROUS_TEMPORAL, true, true, false, "nonlinear-atrous-multiframe-", "a-trous", "a-trous + layers, multiframe"},
    {"atrous-variance", SEQ_ATROUS_VARIANCE, true, true, false, "nonlinear-atrous-variance-", "variance-guided a-trous", "a-trous + layers, variance-guided"},
    {"atrous-recursive", SEQ_ATROUS_RECURSIVE, true, false, false, "nonlinear-atrous-recursive-", "recursive a-trous", "a-trous + layers, recursive accumulation"},
    // (layers: the one render element --guide-layer names, if it is given; RunAnimation decides)
    {"guided", SEQ_GUIDED, false, false, false, "nonlinear-guided-", "guided filter", "guided filter"},
    // (layers: unless --median-plain; RunAnimation decides)
    {"median", SEQ_MEDIAN, true, false, false, "nonlinear-median-", "median", "median"},
};
static const AnimationFilter *animation_filter(const std::string &name)
{
    for (const AnimationFilter &f : kAnimationFilters) if (name == f.name) return &f;
    return nullptr;
}

// ---- RunOnCPU, src/main.cpp:1732-1921 -----------------------------------------------------------------
// The reference's CPU bilateral: window `radius`, double-precision pow/sqrt/exp stored to float, float
// accumulators, rows [radius, h-radius] and columns [radius, w-radius] INCLUSIVE (the last row/column
// read one past the image; here flat indices >= N read a zero pixel), range distance over r,g only when
// blue_bug (the reference's typo), alpha forced to 1, untouched border = Pixel{}.
static void cpu_bilateral_refpath(const std::vector<Pixel> &in, int w, int h, int radius, float spatialSigma,
                                  float colorSigma, bool blue_bug, int numThreads, std::vector<Pixel> &out)
{
    const long n = (long)w * h;
    out.assign((size_t)n, Pixel{0.f, 0.f, 0.f, 0.f});
    auto fetch = [&](long idx) -> Pixel { return (idx >= 0 && idx < n) ? in[(size_t)idx] : Pixel{0.f, 0.f, 0.f, 0.f}; };
    for (int y = radius; y <= h - radius && y < h; ++y) {
#pragma omp parallel for default(shared) num_threads(numThreads)
        for (int x = radius; x <= w - radius; ++x) {
            if (x >= w) continue;
            const Pixel texColor = in[(size_t)y * w + x];
            float normWeight = 0.0f, wr = 0.f, wg = 0.f, wb = 0.f;
            for (int i = -radius; i <= radius; ++i)
                for (int j = -radius; j <= radius; ++j) {
                    const float spatialDistance = (float)std::sqrt((double)(float)std::pow((double)i, 2.0) + std::pow((double)j, 2.0));
                    const float spatialWeight = (float)std::exp(-0.5 * std::pow((double)(spatialDistance / spatialSigma), 2.0));
                    const Pixel cur = fetch((long)w * (i + y) + j + x);
                    const double db = blue_bug ? std::pow((double)(texColor.b - texColor.b), 2.0) : std::pow((double)(texColor.b - cur.b), 2.0);
                    const float colorDistance = (float)std::sqrt(std::pow((double)(texColor.r - cur.r), 2.0) + std::pow((double)(texColor.g - cur.g), 2.0) + db);
                    const float colorWeight = (float)std::exp(-0.5 * std::pow((double)(colorDistance / colorSigma), 2.0));
                    const float resultWeight = spatialWeight * colorWeight;
                    wr += cur.r * resultWeight; wg += cur.g * resultWeight; wb += cur.b * resultWeight;
                    normWeight += resultWeight;
                }
            out[(size_t)y * w + x] = Pixel{wr / normWeight, wg / normWeight, wb / normWeight, 1.0f};
        }
    }
}

// A named ROCTx range (mid_range_push/pop): shows up in `rocprofv3 --marker-trace`, does nothing otherwise.  The reference
// brackets the same stages with timestamp queries (src/main.cpp:793-796,812-814,842-844).
struct TraceRange {
    explicit TraceRange(const std::string &name) { (void)mid_range_push(name.c_str()); }
    ~TraceRange() { (void)mid_range_pop(); }
    TraceRange(const TraceRange &) = delete;
    TraceRange &operator=(const TraceRange &) = delete;
};

// Frame / layer discovery, src/main.cpp:1343-1378, for any frame of a sequence: its siblings of its extension and ITS OWN layers
// (the files one directory down whose path holds its id).  Differences from the reference, all documented in DESIGN.md: entries are
// sorted by name (the reference uses directory order, which is unspecified), and the 4-character frame id comes from the file name's
// stem (the reference's find(".") breaks on "./x").  The one statement of the rule: DenoiseApplication::discover_for and --compare's
// pairing both call it.
static std::string frame_id_of(const fs::path &f)
{
    const std::string stem = f.stem().string();
    return stem.size() >= 4 ? stem.substr(stem.size() - 4) : stem;
}

static void discover_files(const std::string &image, std::vector<std::string> &frames, std::vector<std::string> &layers, bool want_frames,
                           bool want_layers)
{
    const fs::path target(image);
    fs::path parent = target.parent_path();
    if (parent.empty()) parent = ".";
    const std::string imageID = frame_id_of(target);
    std::vector<fs::path> entries;
    for (auto &p : fs::directory_iterator(parent)) entries.push_back(p.path());
    std::sort(entries.begin(), entries.end());
    for (auto &e : entries) {
        if (fs::is_directory(e)) {
            if (!want_layers) continue;
            std::vector<fs::path> inner;
            for (auto &pp : fs::directory_iterator(e)) inner.push_back(pp.path());
            std::sort(inner.begin(), inner.end());
            for (auto &l : inner)
                if (!fs::is_directory(l) && l.string().find(imageID) != std::string::npos) layers.push_back(l.string());
        } else if (e.extension() == target.extension() && want_frames) {
            frames.push_back(e.string());
        }
    }
}

class DenoiseApplication {
    Options opt;
    double m_execMs = 0, m_transferMs = 0;

    static bool is_hdr(const std::string &p) { return fs::path(p).extension() == ".exr"; }   // src/main.cpp:1380

    // A decoded image.  With a context it lives in page-locked memory (mid_image_load_pinned), the HIP counterpart of the
    // host-visible staging buffer the reference memcpy's its decoded pixels into (LoadImageDataToBuffer,
    // src/main.cpp:1105-1142), so every copy the GPU modes issue is a plain asynchronous DMA.  Without one (RunOnCPU), or
    // when page-locked memory runs out, it is ordinary memory, which the C-ABI moves through its own pinned bounce buffers.
    struct HostImage {
        int w = 0, h = 0, format = 0;
        mid_ctx *pin_ctx = nullptr;          // non-NULL: `img.data` is pinned and freed through this context
        mid_image img{};
        HostImage() = default;
        HostImage(const HostImage &) = delete;
        HostImage &operator=(const HostImage &) = delete;
        HostImage(HostImage &&o) noexcept : w(o.w), h(o.h), format(o.format), pin_ctx(o.pin_ctx), img(o.img) { o.img.data = nullptr; }
        HostImage &operator=(HostImage &&o) noexcept
        {
            if (this != &o) { release(); w = o.w; h = o.h; format = o.format; pin_ctx = o.pin_ctx; img = o.img; o.img.data = nullptr; }
            return *this;
        }
        void release()
        {
            if (!img.data) return;
            if (pin_ctx) (void)mid_image_free_pinned(pin_ctx, &img); else mid_image_free(&img);
            img.data = nullptr;
        }
        ~HostImage() { release(); }
        size_t size() const { return (size_t)w * h * (format == MID_FMT_RGBA32F ? 16 : format == MID_FMT_RGBA16F ? 8 : 4); }
        const uint8_t *data() const { return (const uint8_t *)img.data; }
    };

    // half: an .exr as RGBA16F (--half): HALF channels bit for bit, FLOAT ones rounded to nearest even
    static HostImage load(const std::string &path, bool force_png, mid_ctx *ctx = nullptr, bool half = false)
    {
        // The reference decodes layers as PNG (src/main.cpp:1396 passes a_isHDR=false).  The bilateral modes also take .exr layers
        // (RGBA32F, or RGBA16F with --half: MID_FMT_WITH_GUIDE); layer-guided NLM keeps the rule, force_png
        if (force_png && is_hdr(path))
            throw std::runtime_error("layer " + path + " is not a PNG: layer-guided NLM takes RGBA8 guide layers only (its patch distances "
                                     "are exact integer sums of byte values); .exr layers guide the bilateral modes");
        HostImage h;
        if (half) {
            if (ctx && mid_image_load_f16(ctx, path.c_str(), &h.img) == MID_OK) h.pin_ctx = ctx;
            else if (mid_image_load_f16(nullptr, path.c_str(), &h.img)) throw std::runtime_error(mid_last_error());
        } else if (ctx && mid_image_load_pinned(ctx, path.c_str(), &h.img) == MID_OK) h.pin_ctx = ctx;
        else if (mid_image_load(path.c_str(), &h.img))
            throw std::runtime_error(mid_last_error());        // lodepng error -> runtime_error, src/main.cpp:202
        h.w = h.img.width; h.h = h.img.height; h.format = h.img.format;
        return h;
    }

    // All guide layers of a run share one format, decided by the first file: .png = RGBA8, .exr = RGBA32F, or RGBA16F with --half.
    // Refuses the run, naming the first file that differs, before anything is decoded.
    int layer_format(const std::vector<std::string> &names) const
    {
        auto fmt_of = [&](const std::string &f) { return !is_hdr(f) ? MID_FMT_RGBA8 : opt.half ? MID_FMT_RGBA16F : MID_FMT_RGBA32F; };
        for (const std::string &f : names)
            if (fmt_of(f) != fmt_of(names[0]))
                throw std::runtime_error("layer " + f + " is " + (is_hdr(f) ? "an .exr" : "a .png") + " but " + names[0] + " is " +
                                         (is_hdr(names[0]) ? "an .exr" : "a .png") + ": all guide layers of a run must have one format");
        return names.empty() ? MID_FMT_RGBA8 : fmt_of(names[0]);
    }

    // The joint modes' range sigmas, one per layer file in discovery (sorted) order: --sigma-layers, or --sigma-c for all of them.
    // Prints the banner's `layer <file> sigma <value>` lines.
    // nlm: the joint NLM modes' h per layer instead -- --h-layers, or --nlm-h for all of them; `layer <file> h <value>` lines.
    std::vector<float> layer_sigmas(const std::vector<std::string> &names, bool nlm = false) const
    {
        const std::vector<float> &given = nlm ? opt.h_layers : opt.sigma_layers;
        const std::string option = nlm ? "--h-layers" : "--sigma-layers", word = nlm ? "h" : "sigma";
        if (!given.empty() && given.size() != names.size())
            throw std::runtime_error(option + " gives " + std::to_string(given.size()) + " " + (nlm ? "value" : "sigma") + "(s), but " +
                                     std::to_string(names.size()) + " layer file(s) were found: one " + word + " per layer, in sorted order");
        std::vector<float> s(names.size(), nlm ? opt.nlm_h : opt.sigma_c);
        if (!given.empty()) s = given;
        for (size_t l = 0; l < names.size(); ++l) std::cout << "\tlayer " << names[l] << " " << word << " " << s[l] << "\n";
        return s;
    }

    std::string out_path(const std::string &name) const { return (fs::path(opt.outdir) / name).string(); }

    // Files of a sequence are decoded / encoded CONCURRENTLY, one file per worker thread: the reference does its image I/O on one
    // thread (lodepng / tinyexr calls, src/main.cpp:155,196,1699,1717), and a PNG's inflate is one serial stream, so files taken
    // one after the other leave all but one core idle for most of the time.  fn(i) runs for i in [first, n) on `files_at_a_time()`
    // threads; each of them lets its codec calls use the host threads that are left (mid_image_threads: all of them with
    // --io-threads 1, one with a file per host thread).  The first exception ends the loop and is rethrown here.
    int host_threads() const { return (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency())); }
    int files_at_a_time(int n) const { return std::max(1, std::min(opt.io_threads > 0 ? opt.io_threads : host_threads(), n)); }
    template <class Fn> void for_each_file(int first, int n, Fn fn) const
    {
        if (n <= first) return;
        const int nt = files_at_a_time(n - first), codec_threads = std::max(1, host_threads() / nt);
        std::atomic<int> next{first};
        std::vector<std::string> err(nt);
        auto worker = [&](int t) {
            const int before = mid_image_threads(codec_threads);
            try { for (int i = next++; i < n; i = next++) fn(i); }
            catch (const std::exception &e) { err[t] = e.what(); next = n; }
            (void)mid_image_threads(before);
        };
        std::vector<std::thread> th;
        try { for (int t = 1; t < nt; ++t) th.emplace_back(worker, t); }
        catch (const std::system_error &) {}              // no more threads to be had: the ones that started (and this one) do the work
        worker(0);                                         // the calling thread is worker 0
        for (auto &t : th) t.join();
        for (auto &e : err) if (!e.empty()) throw std::runtime_error(e);
    }

public:
    explicit DenoiseApplication(const Options &o) : opt(o) {}
    double GetTransferMs() const { return m_transferMs; }
    double GetExecMs() const { return m_execMs; }

    // Frame / layer discovery: discover_files above, for the target image ...
    void discover(std::vector<std::string> &frames, std::vector<std::string> &layers, bool want_frames, bool want_layers) const
    {
        discover_files(opt.image, frames, layers, want_frames, want_layers);
    }
    // ... and for any frame of the sequence: its siblings and ITS OWN layers.
    void discover_for(const std::string &image, std::vector<std::string> &frames, std::vector<std::string> &layers, bool want_frames,
                      bool want_layers) const
    {
        discover_files(image, frames, layers, want_frames, want_layers);
    }

    // RunOnGPU, src/main.cpp:1307-1730
    // joint (with useLayers): the joint bilateral (mid_bilateral_joint) or, with nlmFilter, joint layer-guided NLM (mid_nlm_joint): one weight from
    // all layers instead of the sum of one filter per layer
    // atrous (with useLayers and joint): 1 = the edge-avoiding a-trous filter (mid_atrous_joint) with the joint mode's layers and sigmas,
    // 2 = its variance-guided form (mid_atrous_moments of the image alone, then mid_atrous_variance)
    void RunOnGPU(bool nlmFilter, bool nonlinear, bool multiframe, bool execAndCopyOverlap, bool useLayers, bool joint = false, int atrous = 0)
    {
        const bool linear = !nonlinear;                                              // :1311
        TraceRange mode_range(std::string("RunOnGPU ") + (linear ? "linear" : "nonlinear") + (nlmFilter ? " nlm" : " bialteral") +
                              (multiframe ? " multiframe" : "") + (execAndCopyOverlap ? " overlap" : "") + (useLayers ? " layers" : ""));
        if (!(nlmFilter || !multiframe)) throw std::runtime_error("multiframe works only with nlm");        // assert :1315
        if (!(multiframe || !execAndCopyOverlap)) throw std::runtime_error("overlap needs multiframe");     // assert :1316
        if (linear && (nlmFilter || useLayers)) throw std::runtime_error("nlm/layers exist for the texture path only");
        m_execMs = m_transferMs = 0;
        std::cout << "\tinit hip for device " << opt.device << "\n";
        mid_ctx *ctx = nullptr;
        MID_CHECK(mid_ctx_create(opt.device, &ctx));
        struct CtxGuard { mid_ctx *c; ~CtxGuard() { mid_ctx_destroy(c); } } guard{ctx};

        std::cout << "\tloading image data\n";
        std::vector<std::string> frameNames, layerNames;
        discover(frameNames, layerNames, multiframe, useLayers);
        const bool hdr = is_hdr(opt.image);
        const bool half = hdr && opt.half;                               // --half: RGBA16F frames in, HALF EXR out
        mid_ctx *pin = opt.pageable_host ? nullptr : ctx;              // where decoded images live
        if (opt.pageable_host) std::cout << "\thost buffers: pageable (bounced inside the library)\n";
        HostImage target = [&] { TraceRange r("decode target"); return load(opt.image, false, pin, half); }();
        const int w = target.w, h = target.h;
        const size_t npix = (size_t)w * h, out_bytes = npix * sizeof(Pixel);
        const int fmt = target.format;
        auto check_dims = [&](const HostImage &im, const std::string &name) {
            if (im.w != w || im.h != h || im.format != fmt) throw std::runtime_error(name + ": size/format differs from the target image");
        };

        // the read-back target: page-locked like the reference's staging buffer (GetImageFromGPU maps it, src/main.cpp:91-96);
        // ordinary memory if that allocation fails
        struct Result {
            mid_ctx *c; void *pinned = nullptr; std::vector<Pixel> fallback;
            Result(mid_ctx *ctx, size_t n, bool want_pinned) : c(ctx)
            {
                if (!want_pinned || mid_alloc_host(c, n * sizeof(Pixel), &pinned)) { pinned = nullptr; fallback.resize(n); }
            }
            ~Result() { if (pinned) (void)mid_free_host(c, pinned); }
            Pixel *data() { return pinned ? (Pixel *)pinned : fallback.data(); }
        } result(ctx, npix, !opt.pageable_host);
        mid_timer *tm = nullptr;
        MID_CHECK(mid_timer_create(ctx, &tm));
        struct TimerGuard { mid_timer *t; ~TimerGuard() { mid_timer_destroy(t); } } tguard{tm};
        auto timed = [&](double &acc, auto &&fn) {
            MID_CHECK(mid_timer_tick(tm, nullptr));
            fn();
            MID_CHECK(mid_timer_tock(tm, nullptr));
            float ms = 0;
            MID_CHECK(mid_timer_ms(tm, &ms));
            acc += ms;
        };

        std::cout << "\tperforming computations\n";
        if (nlmFilter && multiframe) {
            // frame list: the reference loads the target first and then every sibling with the same
            // extension (the target again among them), src/main.cpp:1390-1393; in overlap mode it uploads 10
            // frames and dispatches over the first 9 (:1341,1539-1573).  --temporal-k switches to the explicit
            // window t-k..t+k of the sorted sequence instead.
            std::vector<std::string> list;
            if (opt.temporal_k >= 0) {
                auto it = std::find_if(frameNames.begin(), frameNames.end(), [&](const std::string &f) { return fs::equivalent(f, opt.image); });
                const int t = it == frameNames.end() ? 0 : (int)(it - frameNames.begin());
                for (int f = std::max(0, t - opt.temporal_k); f <= std::min((int)frameNames.size() - 1, t + opt.temporal_k); ++f) list.push_back(frameNames[f]);
                if (list.empty()) list.push_back(opt.image);
            } else {
                list.push_back(opt.image);
                list.insert(list.end(), frameNames.begin(), frameNames.end());
                if (execAndCopyOverlap && list.size() > 9) list.resize(9);
            }
            std::vector<HostImage> frames(list.size());
            for_each_file(0, (int)list.size(), [&](int i) {
                frames[i] = load(list[i], false, pin, half);
                check_dims(frames[i], list[i]);
            });
            std::vector<const void *> ptrs;
            for (auto &f : frames) ptrs.push_back(f.data());
            mid_nlm_params p{w, h, opt.nlm_h, opt.search_lo, opt.search_hi, opt.patch_lo, opt.patch_hi, fmt};
            float t[3] = {0, 0, 0};
            MID_CHECK(mid_nlm_multiframe(ctx, &p, target.data(), ptrs.data(), (int)ptrs.size(), (mid_pixel *)result.data(),
                                         execAndCopyOverlap ? 1 : 0, t));
            m_execMs = t[1]; m_transferMs = t[2];
        } else {
            void *dIn = nullptr, *dOut = nullptr;
            MID_CHECK(mid_alloc(ctx, target.size(), &dIn));
            MID_CHECK(mid_alloc(ctx, out_bytes, &dOut));
            { TraceRange r("upload target"); timed(m_transferMs, [&] { MID_CHECK(mid_memcpy_h2d(ctx, dIn, target.data(), target.size(), nullptr)); }); }
            TraceRange dispatch_range("dispatch");
            if (nlmFilter && !useLayers) {                                                      // single-frame NLM, :1577-1606 with one frame
                mid_nlm_params p{w, h, opt.nlm_h, opt.search_lo, opt.search_hi, opt.patch_lo, opt.patch_hi, fmt};
                const void *fr[1] = {dIn};
                mid_pixel *ou[1] = {(mid_pixel *)dOut};
                timed(m_execMs, [&] { MID_CHECK(mid_nlm_temporal(ctx, &p, fr, 1, 0, 0, 1, ou, nullptr)); });
            } else if (useLayers) {                                                             // :1608-1623 + normalize
                std::vector<void *> dLayers;
                std::vector<HostImage> layerImgs(layerNames.size());
                if (nlmFilter) for (const std::string &ln : layerNames) if (is_hdr(ln)) (void)load(ln, true);       // refuses, saying why
                const int lfmt = layer_format(layerNames);
                std::vector<float> jointSigma;
                if (joint) {
                    if (layerNames.empty() || layerNames.size() > 16)
                        throw std::runtime_error(opt.image + ": " + std::to_string(layerNames.size()) + " layer file(s) found, --modes " +
                                                 (atrous == 2 ? "atrous-variance" : atrous ? "atrous" : nlmFilter ? "nlm-joint" : "joint") + " needs 1..16");
                    jointSigma = layer_sigmas(layerNames, nlmFilter);
                }
                for_each_file(0, (int)layerNames.size(), [&](int i) {
                    layerImgs[i] = load(layerNames[i], nlmFilter, pin, lfmt == MID_FMT_RGBA16F);
                    if (layerImgs[i].format != lfmt) throw std::runtime_error(layerNames[i] + ": the decoded layer is not in the run's guide format");
                });
                for (size_t li = 0; li < layerNames.size(); ++li) {
                    const std::string &ln = layerNames[li];
                    std::cout << "\t\tfeeding layer to texture\n";
                    HostImage &l = layerImgs[li];
                    if (l.w != w || l.h != h) throw std::runtime_error(ln + ": layer size differs from the target image");
                    void *d = nullptr;
                    MID_CHECK(mid_alloc(ctx, l.size(), &d));
                    dLayers.push_back(d);
                    timed(m_transferMs, [&] { MID_CHECK(mid_memcpy_h2d(ctx, d, l.data(), l.size(), nullptr)); });
                    MID_CHECK(mid_stream_sync(ctx, nullptr));             // (the decoded layers are released with `layerImgs`)
                }
                if (nlmFilter && joint) {                                                       // one weight from all layers (mid_nlm_joint)
                    mid_nlm_params p{w, h, opt.nlm_h, opt.search_lo, opt.search_hi, opt.patch_lo, opt.patch_hi, fmt};
                    const void *fr[1] = {dIn};
                    void *ou[1] = {dOut};
                    timed(m_execMs, [&] {
                        MID_CHECK(mid_nlm_joint(ctx, &p, jointSigma.data(), fr, (const uint32_t *const *)dLayers.data(), (int)dLayers.size(), 1, 0, 0, 1,
                                                ou, MID_FMT_RGBA32F, nullptr));
                    });
                } else if (nlmFilter) {                                                         // the same loop with nonlocal.comp
                    mid_nlm_params p{w, h, opt.nlm_h, opt.search_lo, opt.search_hi, opt.patch_lo, opt.patch_hi, fmt};
                    timed(m_execMs, [&] {
                        MID_CHECK(mid_nlm_layers(ctx, &p, dIn, (const uint32_t *const *)dLayers.data(), (int)dLayers.size(), (mid_pixel *)dOut, nullptr));
                    });
                } else if (atrous == 2) {                                                       // the variance of the luminance, then the passes it guides
                    const int fw = lfmt == MID_FMT_RGBA8 ? fmt : MID_FMT_WITH_GUIDE(fmt, lfmt);
                    const mid_atrous_moments_params mp{w, h, fw};
                    const mid_atrous_variance_params p{w, h, 0, opt.passes, opt.atrous_sigma_lum, opt.atrous_epsilon, fw};
                    void *levels = nullptr, *variance = nullptr;
                    MID_CHECK(mid_alloc(ctx, npix * sizeof(float), &variance));
                    if (mid_atrous_variance_scratch_bytes(&p)) MID_CHECK(mid_alloc(ctx, mid_atrous_variance_scratch_bytes(&p), &levels));
                    const void *fr[1] = {dIn};
                    timed(m_execMs, [&] {
                        MID_CHECK(mid_atrous_moments(ctx, &mp, jointSigma.data(), fr, (const uint32_t *const *)dLayers.data(), (int)dLayers.size(), 1, 0, 0,
                                                     (float *)variance, nullptr));
                        MID_CHECK(mid_atrous_variance(ctx, &p, jointSigma.data(), dIn, (const float *)variance, (const uint32_t *const *)dLayers.data(),
                                                      (int)dLayers.size(), dOut, MID_FMT_RGBA32F, nullptr, levels, nullptr));
                    });
                    MID_CHECK(mid_stream_sync(ctx, nullptr));
                    if (levels) mid_free(ctx, levels);
                    mid_free(ctx, variance);
                } else if (atrous) {                                                            // N passes of the 5x5 kernel with holes (mid_atrous_joint)
                    mid_atrous_params p{w, h, 0, opt.passes, opt.atrous_sigma_color, lfmt == MID_FMT_RGBA8 ? fmt : MID_FMT_WITH_GUIDE(fmt, lfmt)};
                    void *levels = nullptr;
                    if (mid_atrous_scratch_bytes(&p)) MID_CHECK(mid_alloc(ctx, mid_atrous_scratch_bytes(&p), &levels));
                    timed(m_execMs, [&] {
                        MID_CHECK(mid_atrous_joint(ctx, &p, jointSigma.data(), dIn, (const uint32_t *const *)dLayers.data(), (int)dLayers.size(), dOut,
                                                   MID_FMT_RGBA32F, levels, nullptr));
                    });
                    MID_CHECK(mid_stream_sync(ctx, nullptr));
                    if (levels) mid_free(ctx, levels);
                } else if (joint) {
                    mid_bilateral_params p{w, h, opt.sigma_s, opt.sigma_c, opt.radius, MID_LAYOUT_TEXTURE,
                                           lfmt == MID_FMT_RGBA8 ? fmt : MID_FMT_WITH_GUIDE(fmt, lfmt)};
                    const void *fr[1] = {dIn};
                    void *ou[1] = {dOut};
                    timed(m_execMs, [&] {
                        MID_CHECK(mid_bilateral_joint(ctx, &p, jointSigma.data(), fr, (const uint32_t *const *)dLayers.data(), (int)dLayers.size(), 1, 0, 0, 1,
                                                      ou, MID_FMT_RGBA32F, nullptr));
                    });
                } else {
                    mid_bilateral_params p{w, h, opt.sigma_s, opt.sigma_c, opt.radius, MID_LAYOUT_TEXTURE,
                                           lfmt == MID_FMT_RGBA8 ? fmt : MID_FMT_WITH_GUIDE(fmt, lfmt)};
                    timed(m_execMs, [&] {
                        MID_CHECK(mid_bilateral_layers(ctx, &p, dIn, (const uint32_t *const *)dLayers.data(), (int)dLayers.size(), (mid_pixel *)dOut, nullptr));
                    });
                }
                for (void *d : dLayers) mid_free(ctx, d);
            } else {                                                                            // plain bialteral, :1654-1659
                mid_bilateral_params p{w, h, opt.sigma_s, opt.sigma_c, opt.radius, linear ? MID_LAYOUT_LINEAR : MID_LAYOUT_TEXTURE, fmt};
                timed(m_execMs, [&] { MID_CHECK(mid_bilateral(ctx, &p, dIn, (mid_pixel *)dOut, nullptr)); });
            }
            std::cout << "\tgetting image back\n";
            (void)mid_range_pop();                                                              // "dispatch" ends, "download" begins
            (void)mid_range_push("download");
            timed(m_transferMs, [&] { MID_CHECK(mid_memcpy_d2h(ctx, result.data(), dOut, out_bytes, nullptr)); });
            MID_CHECK(mid_stream_sync(ctx, nullptr));
            mid_free(ctx, dIn); mid_free(ctx, dOut);
        }

        std::string outputFileName{"output"};                                                   // :1677-1686
        outputFileName += linear ? "-linear" : "-nonlinear";
        outputFileName += nlmFilter ? "-nlm" : "-bialteral";
        outputFileName += multiframe ? "-multiframe" : "";
        outputFileName += execAndCopyOverlap ? "-overlap" : "";
        outputFileName += joint ? "-joint" : useLayers ? "-layers" : "";
        if (atrous) outputFileName = atrous == 2 ? "output-nonlinear-atrous-variance" : "output-nonlinear-atrous";
        if (half) {   // --half: the fp32 result rounded to RGBA16F on the device (mid_pack_f16), written as HALF EXR
            std::vector<uint16_t> px(npix * 4);
            void *dF = nullptr, *dH = nullptr;
            MID_CHECK(mid_alloc(ctx, out_bytes, &dF));
            MID_CHECK(mid_alloc(ctx, npix * 8, &dH));
            MID_CHECK(mid_memcpy_h2d(ctx, dF, result.data(), out_bytes, nullptr));
            MID_CHECK(mid_pack_f16(ctx, (const float *)dF, npix * 4, (uint16_t *)dH, nullptr));
            MID_CHECK(mid_memcpy_d2h(ctx, px.data(), dH, npix * 8, nullptr));
            MID_CHECK(mid_stream_sync(ctx, nullptr));
            mid_free(ctx, dF); mid_free(ctx, dH);
            TraceRange r("encode + write " + outputFileName);
            MID_CHECK(mid_image_save(out_path(outputFileName + ".exr").c_str(), px.data(), w, h, MID_FMT_RGBA16F));
        } else { TraceRange r("encode + write " + outputFileName); save(outputFileName, result.data(), w, h, hdr); }
        std::cout << "\tcleaning up\n";
    }

    // --modes guided: the guided filter of the target (mid_guided_filter, section a4o), guided by the one render element --guide-layer
    // names (.png as RGBA8, .exr as RGBA32F or, with --half, RGBA16F) or, without the option, by the target itself: no layer is loaded then.
    // Output output-nonlinear-guided.{png,exr}; with --half on an .exr target the kernel stores RGBA16F and the file is a HALF EXR.
    void RunGuided()
    {
        TraceRange mode_range("RunGuided");
        m_execMs = m_transferMs = 0;
        std::cout << "\tinit hip for device " << opt.device << "\n";
        mid_ctx *ctx = nullptr;
        MID_CHECK(mid_ctx_create(opt.device, &ctx));
        struct CtxGuard { mid_ctx *c; ~CtxGuard() { mid_ctx_destroy(c); } } guard{ctx};
        std::string guideName;
        if (!opt.guide_layer.empty()) {
            std::vector<std::string> none, layerNames, hits;
            discover(none, layerNames, false, true);
            for (const std::string &f : layerNames) if (fs::path(f).filename().string().find(opt.guide_layer) != std::string::npos) hits.push_back(f);
            if (hits.size() != 1)
                throw std::runtime_error(opt.image + ": --guide-layer " + opt.guide_layer + " matches " + std::to_string(hits.size()) +
                                         " layer file(s) of this frame, it must match exactly one");
            guideName = hits[0];
        }
        std::cout << "\tguided guide " << (guideName.empty() ? std::string("self") : guideName) << " radius " << opt.guided_radius << " eps " << opt.guided_eps << "\n";
        std::cout << "\tloading image data\n";
        const bool hdr = is_hdr(opt.image), half = hdr && opt.half;
        mid_ctx *pin = opt.pageable_host ? nullptr : ctx;
        HostImage target = load(opt.image, false, pin, half);
        const int w = target.w, h = target.h, fmt = target.format;
        const size_t npix = (size_t)w * h;
        HostImage guide;
        int gfmt = fmt;
        if (!guideName.empty()) {
            guide = load(guideName, false, pin, is_hdr(guideName) && opt.half);
            if (guide.w != w || guide.h != h) throw std::runtime_error(guideName + ": layer size differs from the target image");
            gfmt = guide.format;
        }
        const int out_fmt = half ? MID_FMT_RGBA16F : MID_FMT_RGBA32F;
        const size_t out_bytes = npix * (half ? 8 : 16);
        const mid_guided_params p{w, h, opt.guided_radius, opt.guided_eps, MID_FMT_WITH_GUIDE(fmt, gfmt)};
        size_t work_bytes = 0;
        MID_CHECK(mid_guided_workspace(&p, &work_bytes));
        std::vector<unsigned char> result(out_bytes);
        mid_timer *tm = nullptr;
        MID_CHECK(mid_timer_create(ctx, &tm));
        struct TimerGuard { mid_timer *t; ~TimerGuard() { mid_timer_destroy(t); } } tguard{tm};
        auto timed = [&](double &acc, auto &&fn) {
            MID_CHECK(mid_timer_tick(tm, nullptr));
            fn();
            MID_CHECK(mid_timer_tock(tm, nullptr));
            float ms = 0;
            MID_CHECK(mid_timer_ms(tm, &ms));
            acc += ms;
        };
        std::cout << "\tperforming computations\n";
        void *dIn = nullptr, *dGuide = nullptr, *dWork = nullptr, *dOut = nullptr;
        MID_CHECK(mid_alloc(ctx, target.size(), &dIn));
        if (!guideName.empty()) MID_CHECK(mid_alloc(ctx, guide.size(), &dGuide));
        MID_CHECK(mid_alloc(ctx, work_bytes, &dWork));
        MID_CHECK(mid_alloc(ctx, out_bytes, &dOut));
        timed(m_transferMs, [&] {
            MID_CHECK(mid_memcpy_h2d(ctx, dIn, target.data(), target.size(), nullptr));
            if (dGuide) MID_CHECK(mid_memcpy_h2d(ctx, dGuide, guide.data(), guide.size(), nullptr));
        });
        timed(m_execMs, [&] { MID_CHECK(mid_guided_filter(ctx, &p, dIn, dGuide, dWork, dOut, out_fmt, nullptr)); });
        std::cout << "\tgetting image back\n";
        timed(m_transferMs, [&] { MID_CHECK(mid_memcpy_d2h(ctx, result.data(), dOut, out_bytes, nullptr)); });
        MID_CHECK(mid_stream_sync(ctx, nullptr));
        mid_free(ctx, dIn); if (dGuide) mid_free(ctx, dGuide); mid_free(ctx, dWork); mid_free(ctx, dOut);
        const std::string outputFileName = "output-nonlinear-guided";
        if (half) MID_CHECK(mid_image_save(out_path(outputFileName + ".exr").c_str(), result.data(), w, h, MID_FMT_RGBA16F));
        else save(outputFileName, (const Pixel *)result.data(), w, h, hdr);
        std::cout << "\tcleaning up\n";
    }

    // --modes median: the median of the target (mid_median_filter, section a4p) -- weighted by the frame's RenderElements layers, loaded
    // and given their sigmas as for --modes atrous (--sigma-layers, else --sigma-c; .png or .exr, one format per run), or with
    // --median-plain the plain median, for which no layer is loaded.  Output output-nonlinear-median.{png,exr}; with --half on an .exr
    // target the kernel stores RGBA16F and the file is a HALF EXR.
    void RunMedian()
    {
        TraceRange mode_range("RunMedian");
        m_execMs = m_transferMs = 0;
        std::cout << "\tinit hip for device " << opt.device << "\n";
        mid_ctx *ctx = nullptr;
        MID_CHECK(mid_ctx_create(opt.device, &ctx));
        struct CtxGuard { mid_ctx *c; ~CtxGuard() { mid_ctx_destroy(c); } } guard{ctx};
        std::vector<std::string> none, layerNames;
        if (!opt.median_plain) {
            discover(none, layerNames, false, true);
            if (layerNames.empty() || layerNames.size() > 16)
                throw std::runtime_error(opt.image + ": " + std::to_string(layerNames.size()) + " layer file(s) found, --modes median needs 1..16 (or --median-plain)");
        }
        const int L = (int)layerNames.size(), lfmt = layer_format(layerNames);
        std::cout << "\tmedian radius " << opt.median_radius << " layers " << L << "\n";
        const std::vector<float> sigma = layer_sigmas(layerNames);
        std::cout << "\tloading image data\n";
        const bool hdr = is_hdr(opt.image), half = hdr && opt.half;
        mid_ctx *pin = opt.pageable_host ? nullptr : ctx;
        HostImage target = load(opt.image, false, pin, half);
        const int w = target.w, h = target.h, fmt = target.format;
        const size_t npix = (size_t)w * h;
        std::vector<HostImage> layerImgs(L);
        for_each_file(0, L, [&](int i) {
            layerImgs[i] = load(layerNames[i], false, pin, lfmt == MID_FMT_RGBA16F);
            if (layerImgs[i].w != w || layerImgs[i].h != h) throw std::runtime_error(layerNames[i] + ": layer size differs from the target image");
            if (layerImgs[i].format != lfmt) throw std::runtime_error(layerNames[i] + ": the decoded layer is not in the run's guide format");
        });
        // an LDR target comes back as RGBA8 (the kernel packs as mid_pack_u8 does), an .exr as RGBA32F, or RGBA16F with --half
        const int out_fmt = hdr ? (half ? MID_FMT_RGBA16F : MID_FMT_RGBA32F) : MID_FMT_RGBA8;
        const size_t out_bytes = npix * (out_fmt == MID_FMT_RGBA32F ? 16 : out_fmt == MID_FMT_RGBA16F ? 8 : 4);
        const mid_median_params p{w, h, opt.median_radius, L && lfmt != MID_FMT_RGBA8 ? MID_FMT_WITH_GUIDE(fmt, lfmt) : fmt};
        std::vector<unsigned char> result(out_bytes);
        mid_timer *tm = nullptr;
        MID_CHECK(mid_timer_create(ctx, &tm));
        struct TimerGuard { mid_timer *t; ~TimerGuard() { mid_timer_destroy(t); } } tguard{tm};
        auto timed = [&](double &acc, auto &&fn) {
            MID_CHECK(mid_timer_tick(tm, nullptr));
            fn();
            MID_CHECK(mid_timer_tock(tm, nullptr));
            float ms = 0;
            MID_CHECK(mid_timer_ms(tm, &ms));
            acc += ms;
        };
        std::cout << "\tperforming computations\n";
        struct Dev { mid_ctx *c; std::vector<void *> p; ~Dev() { for (auto q : p) if (q) (void)mid_free(c, q); } } dev{ctx, {}};
        auto dalloc = [&](size_t bytes) { void *d = nullptr; MID_CHECK(mid_alloc(ctx, bytes, &d)); dev.p.push_back(d); return d; };
        void *dIn = dalloc(target.size()), *dOut = dalloc(out_bytes);
        std::vector<const uint32_t *> dLayers;
        for (int i = 0; i < L; ++i) dLayers.push_back((const uint32_t *)dalloc(layerImgs[i].size()));
        timed(m_transferMs, [&] {
            MID_CHECK(mid_memcpy_h2d(ctx, dIn, target.data(), target.size(), nullptr));
            for (int i = 0; i < L; ++i) MID_CHECK(mid_memcpy_h2d(ctx, (void *)dLayers[i], layerImgs[i].data(), layerImgs[i].size(), nullptr));
        });
        timed(m_execMs, [&] { MID_CHECK(mid_median_filter(ctx, &p, L ? sigma.data() : nullptr, dIn, L ? dLayers.data() : nullptr, L, dOut, out_fmt, nullptr)); });
        std::cout << "\tgetting image back\n";
        timed(m_transferMs, [&] { MID_CHECK(mid_memcpy_d2h(ctx, result.data(), dOut, out_bytes, nullptr)); });
        MID_CHECK(mid_stream_sync(ctx, nullptr));
        const std::string name = std::string("output-nonlinear-median") + (hdr ? ".exr" : ".png");
        MID_CHECK(mid_image_save(out_path(name).c_str(), result.data(), w, h, out_fmt));
        std::cout << "\tcleaning up\n";
    }

    // Animation mode (BASELINE config 5; not in the reference, which filters one target per run): every
    // sibling frame of the target is denoised with temporal NLM over frames t-k..t+k.  Frames are split
    // into contiguous blocks, one per device; each device streams its block plus k halo frames on either
    // side through the 3-stream pipeline (mid_sequence_nlm_range): all frames sit in host memory, so by default
    // the halo is simply uploaded twice and needs no device-to-device exchange.  With --halo rccl every block is
    // uploaded once, stays resident in its GPU's HBM, and the halo frames travel GPU to GPU over RCCL/xGMI
    // (mid_nlm_temporal_sharded, csrc/sharded.cpp).  Outputs: output-animation-<frame file name>.
    // --animation-filter bilateral | linear | layers runs the bilateral of every frame instead (mid_sequence_bilateral: the same
    // pipeline with window k = 0, so blocks have no halo); `layers` guides each frame with its OWN RenderElements layers, found
    // by the discover rule with that frame's id and uploaded beside it.  Outputs: output-animation-<mode name>-<frame file name>,
    // the single-frame modes' names (nonlinear-bialteral, linear-bialteral, nonlinear-bialteral-layers).
    // --animation-filter nlm-layers is layer-guided NLM of every frame on its own (mid_sequence_nlm_layers); nlm-layers-temporal adds
    // the frames t-k..t+k and their layers (mid_sequence_nlm_layers_temporal: blocks with k halo frames, like nlm, from the host only).
    // --animation-filter bilateral-temporal | layers-temporal is the bilateral over the frames t-k..t+k, plain or guided by each
    // frame's layers (mid_sequence_bilateral_temporal: blocks with k halo frames and their layers, from the host only).
    void RunAnimation()
    {
        std::vector<std::string> frameNames, layerNames;
        discover(frameNames, layerNames, true, false);
        if (frameNames.empty()) throw std::runtime_error("no frames next to " + opt.image);
        // (joint | joint-temporal: the joint bilateral of every frame, alone (k = 0) or over the frames t-k..t+k -- mid_sequence_bilateral_joint,
        // the schedule of layers-temporal)
        const AnimationFilter &af = *animation_filter(opt.animation_filter);        // (main has refused unknown names)
        const int n = (int)frameNames.size(), k = !af.temporal ? 0 : opt.temporal_k < 0 ? 2 : opt.temporal_k;
        const bool guided = af.family == SEQ_GUIDED;
        const bool median = af.family == SEQ_MEDIAN;
        const bool use_layers = (af.layers && !(median && opt.median_plain)) || (guided && !opt.guide_layer.empty()), nlm_guides = af.family == SEQ_NLM_LAYERS || af.family == SEQ_NLM_LAYERS_TEMPORAL || af.family == SEQ_NLM_JOINT;
        if (!af.windowed() && opt.halo_rccl)
            throw std::runtime_error("--halo rccl is not available with --animation-filter " + opt.animation_filter +
                                     ": its frames read no other frame, there is no halo to exchange");
        if (af.family != SEQ_NLM && opt.halo_rccl)
            throw std::runtime_error("--halo rccl is not available with --animation-filter " + opt.animation_filter + ": the halo would have to "
                                     "carry every halo frame's layers as well, and that exchange is not built (use --halo host)");
        const bool recursive = af.family == SEQ_ATROUS_RECURSIVE;
        if (!recursive && !opt.motion_layer.empty())
            throw std::runtime_error("--motion-layer applies to --animation-filter atrous-recursive only");
        // every frame's own layers, all of them checked before anything is decoded: 1..16 per frame, the same count for all
        std::vector<std::vector<std::string>> frameLayers(use_layers ? n : 0);
        std::vector<std::string> motionNames;           // atrous-recursive with --motion-layer: the one render element of each frame that holds its motion
        std::vector<std::string> albedoNames;           // atrous-recursive with --albedo-layer: the one render element of each frame that holds its albedo
        int L = 0;
        for (int i = 0; i < (int)frameLayers.size(); ++i) {
            std::vector<std::string> none;
            discover_for(frameNames[i], none, frameLayers[i], false, true);
            if (!opt.motion_layer.empty()) {            // taken out of the guide layers
                std::vector<std::string> hits, rest;
                for (const std::string &f : frameLayers[i]) (fs::path(f).filename().string().find(opt.motion_layer) != std::string::npos ? hits : rest).push_back(f);
                if (hits.size() != 1)
                    throw std::runtime_error(frameNames[i] + ": --motion-layer " + opt.motion_layer + " matches " + std::to_string(hits.size()) +
                                             " layer file(s) of this frame, it must match exactly one");
                if (!is_hdr(hits[0]))
                    throw std::runtime_error("motion layer " + hits[0] + " is a .png: motion vectors are read from an .exr render element (R, G in pixels)");
                motionNames.push_back(hits[0]);
                frameLayers[i] = rest;
            }
            if (!opt.albedo_layer.empty()) {            // taken out of the guide layers too; a .png is as good as an .exr
                std::vector<std::string> hits, rest;
                for (const std::string &f : frameLayers[i]) (fs::path(f).filename().string().find(opt.albedo_layer) != std::string::npos ? hits : rest).push_back(f);
                if (hits.size() != 1)
                    throw std::runtime_error(frameNames[i] + ": --albedo-layer " + opt.albedo_layer + " matches " + std::to_string(hits.size()) +
                                             " layer file(s) of this frame, it must match exactly one");
                albedoNames.push_back(hits[0]);
                frameLayers[i] = rest;
            }
            if (guided) {                                // the one render element that guides; every other one is left alone
                std::vector<std::string> hits;
                for (const std::string &f : frameLayers[i]) if (fs::path(f).filename().string().find(opt.guide_layer) != std::string::npos) hits.push_back(f);
                if (hits.size() != 1)
                    throw std::runtime_error(frameNames[i] + ": --guide-layer " + opt.guide_layer + " matches " + std::to_string(hits.size()) +
                                             " layer file(s) of this frame, it must match exactly one");
                frameLayers[i] = hits;
            }
            const int li = (int)frameLayers[i].size();
            if (li < 1 || li > 16)
                throw std::runtime_error(frameNames[i] + ": " + std::to_string(li) + " layer file(s) found, --animation-filter " + opt.animation_filter + " needs 1..16 per frame");
            if (i > 0 && li != L)
                throw std::runtime_error(frameNames[i] + ": " + std::to_string(li) + " layer file(s), but " + frameNames[0] + " has " +
                                         std::to_string(L) + ": every frame needs the same layers");
            L = li;
        }
        // the layers' format, one for the run: .exr layers (RGBA32F, RGBA16F with --half) guide the bilateral filters only
        std::vector<std::string> allLayers;
        for (auto &fl : frameLayers) allLayers.insert(allLayers.end(), fl.begin(), fl.end());
        allLayers.insert(allLayers.end(), albedoNames.begin(), albedoNames.end());      // (the albedo planes obey the layers' one-format rule)
        if (nlm_guides) for (const std::string &ln : allLayers) if (is_hdr(ln)) (void)load(ln, true);   // refuses, saying why
        const int lfmt = layer_format(allLayers);
        const std::vector<float> jointSigma = median && !use_layers ? std::vector<float>() : median || af.family == SEQ_BILATERAL_JOINT || af.family == SEQ_ATROUS || af.family == SEQ_ATROUS_TEMPORAL || af.family == SEQ_ATROUS_VARIANCE || recursive ? layer_sigmas(frameLayers[0])            // (every frame has frame 0's layers)
                                              : af.family == SEQ_NLM_JOINT ? layer_sigmas(frameLayers[0], true) : std::vector<float>();
        std::cout << "\tloading " << n << " frames\n";
        // Frames are decoded STRAIGHT INTO pinned host memory (mid_image_load_pinned) and the results land in pinned
        // buffers too, so every copy of the pipeline is a true asynchronous DMA -- the reference memcpy's its decoded
        // pixels into mapped staging memory the same way (LoadImageDataToBuffer, src/main.cpp:1105-1142).  Measured,
        // 16 x 1080p RGBA32F through the pipeline: pinned 12.8 ms, pageable vectors 20.2 ms, vectors registered in
        // place 25.1 ms.  Page-locking is per process, so the one context used for loading serves every device.
        mid_ctx *io = nullptr;
        MID_CHECK(mid_ctx_create(opt.device, &io));
        // Page-locked memory is a bounded resource: at most --pinned-mb of it (default 16 GiB, inputs and outputs
        // together) is requested, and a frame whose pinned allocation fails -- or that would exceed the budget -- is
        // decoded into ordinary pageable memory instead (the pipeline accepts both; HIP then stages that copy and its
        // overlap is lost, nothing else changes).  A long or high-resolution sequence degrades, it does not abort.
        struct Pinned {                                   // owns the frames and outputs (pinned or pageable); released before `io`
            mid_ctx *c;
            std::vector<mid_image> frames;
            std::vector<char> frame_pinned;
            std::vector<void *> outs;
            std::vector<char> out_pinned;
            ~Pinned()
            {
                for (size_t i = 0; i < frames.size(); ++i) {
                    if (frame_pinned[i]) (void)mid_image_free_pinned(c, &frames[i]);
                    else mid_image_free(&frames[i]);
                }
                for (size_t i = 0; i < outs.size(); ++i) {
                    if (out_pinned[i]) (void)mid_free_host(c, outs[i]);
                    else free(outs[i]);
                }
                mid_ctx_destroy(c);
            }
        } pin{io, {}, {}, {}, {}};
        const size_t pinned_budget = (size_t)std::max(0l, opt.pinned_mb) << 20;
        size_t pinned_bytes = 0, frame_bytes_guess = 0;
        int n_pageable = 0;
        const auto tl0 = std::chrono::steady_clock::now();
        // Frame 0 is decoded first (its size fixes how many frames fit the page-locked budget: inputs and outputs share it frame
        // by frame, input i is pinned only if output i can be as well); the others are decoded concurrently (for_each_file).
        pin.frames.assign(n, mid_image{});
        pin.frame_pinned.assign(n, 0);
        // --half: .exr frames as RGBA16F (mid_image_load_f16), filtered as such, written back as HALF EXR from the kernel's epilogue
        const bool half = opt.half && is_hdr(frameNames[0]);
        if (half && opt.halo_rccl) throw std::runtime_error("--half is not available with --halo rccl (its outputs are RGBA32F)");
        auto decode = [&](int i, bool pinned) {            // throws on a bad file; falls back to pageable memory when no pinned memory is left
            mid_image img{};
            if (half) {
                if (pinned && mid_image_load_f16(io, frameNames[i].c_str(), &img)) pinned = false;
                if (!pinned && mid_image_load_f16(nullptr, frameNames[i].c_str(), &img)) throw std::runtime_error(mid_last_error());
                pin.frames[i] = img;
                pin.frame_pinned[i] = pinned ? 1 : 0;
                return;
            }
            if (pinned && mid_image_load_pinned(io, frameNames[i].c_str(), &img)) pinned = false;
            if (!pinned && mid_image_load(frameNames[i].c_str(), &img)) throw std::runtime_error(mid_last_error());
            pin.frames[i] = img;
            pin.frame_pinned[i] = pinned ? 1 : 0;
        };
        decode(0, pinned_budget > 0);                       // (the first frame's size is not known yet: any non-zero budget admits it)
        frame_bytes_guess = (size_t)pin.frames[0].width * pin.frames[0].height *
                            (pin.frames[0].format == MID_FMT_RGBA32F ? 16 : pin.frames[0].format == MID_FMT_RGBA16F ? 8 : 4);
        const size_t layer_bytes = (size_t)pin.frames[0].width * pin.frames[0].height *
                                   (lfmt == MID_FMT_RGBA32F ? 16 : lfmt == MID_FMT_RGBA16F ? 8 : 4);    // (its real size; checked against the frame below)
        // frames whose input AND output -- and their layers -- fit the budget
        const size_t n_side_planes = (size_t)L + (albedoNames.empty() ? 0 : 1);      // page-locked beside a frame: its layers and its albedo plane
        const size_t n_pin = pinned_budget / (2 * frame_bytes_guess + n_side_planes * layer_bytes);
        const int io_threads = files_at_a_time(n);
        for_each_file(1, n, [&](int i) {
            decode(i, (size_t)i < n_pin);
            const mid_image &a = pin.frames[i], &b = pin.frames[0];
            if (a.width != b.width || a.height != b.height || a.format != b.format)
                throw std::runtime_error(frameNames[i] + ": size/format differs from the first frame");
        });
        // --animation-filter layers / nlm-layers: PNG layers decoded as RGBA8 like the single-frame mode (.exr layers of the bilateral
        // filters as RGBA32F / RGBA16F), page-locked with their frame
        std::vector<HostImage> layerImgs((size_t)n * L);             // (released before `pin` and its context)
        for_each_file(0, (int)layerImgs.size(), [&](int j) {
            const int i = j / L;
            layerImgs[j] = load(frameLayers[i][j % L], nlm_guides, (size_t)i < n_pin ? io : nullptr, lfmt == MID_FMT_RGBA16F);
            const HostImage &l = layerImgs[j];
            if (l.w != pin.frames[0].width || l.h != pin.frames[0].height || l.format != lfmt)
                throw std::runtime_error(frameNames[i] + ": layer " + frameLayers[i][j % L] + " is not " +
                                         (lfmt == MID_FMT_RGBA8 ? "an RGBA8" : lfmt == MID_FMT_RGBA16F ? "an RGBA16F" : "an RGBA32F") + " image of the frame's size");
        });
        // the motion planes: R and G of the render element, times --motion-scale, one float2 per pixel
        std::vector<std::vector<float>> motionPlanes(motionNames.size());
        for_each_file(0, (int)motionNames.size(), [&](int i) {
            const HostImage m = load(motionNames[i], false);
            if (m.w != pin.frames[0].width || m.h != pin.frames[0].height || m.format != MID_FMT_RGBA32F)
                throw std::runtime_error("motion layer " + motionNames[i] + " is not an RGBA32F image of the frame's size");
            const float *px = (const float *)m.data();
            motionPlanes[i].resize((size_t)m.w * m.h * 2);
            for (size_t q = 0; q < (size_t)m.w * m.h; ++q) {
                motionPlanes[i][2 * q] = px[4 * q] * opt.motion_sx;
                motionPlanes[i][2 * q + 1] = px[4 * q + 1] * opt.motion_sy;
            }
        });
        // the albedo planes: decoded like the layers, in their format, page-locked with their frame
        std::vector<HostImage> albedoImgs(albedoNames.size());             // (released before `pin` and its context)
        for_each_file(0, (int)albedoImgs.size(), [&](int i) {
            albedoImgs[i] = load(albedoNames[i], false, (size_t)i < n_pin ? io : nullptr, lfmt == MID_FMT_RGBA16F);
            const HostImage &a = albedoImgs[i];
            if (a.w != pin.frames[0].width || a.h != pin.frames[0].height || a.format != lfmt)
                throw std::runtime_error("albedo layer " + albedoNames[i] + " is not " +
                                         (lfmt == MID_FMT_RGBA8 ? "an RGBA8" : lfmt == MID_FMT_RGBA16F ? "an RGBA16F" : "an RGBA32F") + " image of the frame's size");
        });
        std::vector<const void *> albedo_ptrs(albedoImgs.size());
        for (size_t i = 0; i < albedoImgs.size(); ++i) albedo_ptrs[i] = albedoImgs[i].data();
        if (!albedoNames.empty()) std::cout << "\talbedo " << albedoNames[0] << " floor " << opt.albedo_floor << "\n";
        if (opt.firefly_rank)
            std::cout << "\tfirefly radius " << opt.firefly_radius << " rank " << opt.firefly_rank << " gain " << opt.firefly_gain << " floor " << opt.firefly_floor << "\n";
        if (guided)
            std::cout << "\tguided guide " << (use_layers ? frameLayers[0][0] : std::string("self")) << " radius " << opt.guided_radius << " eps " << opt.guided_eps << "\n";
        if (median) std::cout << "\tmedian radius " << opt.median_radius << " layers " << L << "\n";
        if (opt.history_clip) std::cout << "\thistory-clip radius " << opt.history_clip_radius << " gamma " << opt.history_clip_gamma << "\n";
        std::vector<const void *> motion_ptrs(motionPlanes.size());
        for (size_t i = 0; i < motionPlanes.size(); ++i) motion_ptrs[i] = motionPlanes[i].data();
        if (!motionNames.empty()) std::cout << "\tmotion " << motionNames[0] << " scale " << opt.motion_sx << " " << opt.motion_sy << "\n";
        std::vector<const void *> layer_ptrs(layerImgs.size());
        for (size_t j = 0; j < layerImgs.size(); ++j) layer_ptrs[j] = layerImgs[j].data();
        for (int i = 0; i < n; ++i) { if (pin.frame_pinned[i]) pinned_bytes += 2 * frame_bytes_guess + n_side_planes * layer_bytes; else ++n_pageable; }
        const double load_sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - tl0).count();
        const int w = pin.frames[0].width, h = pin.frames[0].height, fmt = pin.frames[0].format;
        // LDR frames come back as RGBA8: the read-back conversion of GetImageFromGPU (:97-103) runs on the device
        // (mid_sequence_nlm_range_u8), a quarter of the download
        const bool hdr = fmt == MID_FMT_RGBA32F;           // (--half: fmt is RGBA16F, `half` set, `hdr` false)
        const size_t out_bytes = (size_t)w * h * (hdr ? 16 : half ? 8 : 4), in_bytes = out_bytes;
        std::vector<const void *> in(n);
        for (int i = 0; i < n; ++i) {
            in[i] = pin.frames[i].data;
            void *o = nullptr;
            bool pinned = pin.frame_pinned[i] != 0;
            if (pinned && mid_alloc_host(io, out_bytes, &o)) { pinned = false; o = nullptr; }
            if (!pinned) {
                o = malloc(out_bytes);
                if (!o) throw std::runtime_error("out of host memory for the output frames");
                if (pin.frame_pinned[i]) ++n_pageable;
            }
            pin.outs.push_back(o);
            pin.out_pinned.push_back(pinned ? 1 : 0);
        }
        if (n_pageable)
            std::cout << "	" << n_pageable << " frame(s) beyond the page-locked budget (--pinned-mb " << opt.pinned_mb
                      << ") use pageable host memory: their copies are staged by HIP and do not overlap\n";
        const int G = std::max(1, std::min(opt.gpus, n));
        // One context per device, created -- and its code object, streams and allocator warmed by filtering two tiny
        // frames -- BEFORE the clock starts: the timed region below is the frame pipeline itself (uploads, kernels,
        // downloads), like the reference's timestamps bracket its submits and not vkCreateDevice.
        std::vector<mid_ctx *> ctxs(G, nullptr);
        struct CtxGuard { std::vector<mid_ctx *> &v; ~CtxGuard() { for (auto c : v) if (c) mid_ctx_destroy(c); } } guard{ctxs};
        const mid_nlm_params p{w, h, opt.nlm_h, opt.search_lo, opt.search_hi, opt.patch_lo, opt.patch_hi, fmt};
        const mid_bilateral_params bp{w, h, opt.sigma_s, opt.sigma_c, opt.radius, af.linear ? MID_LAYOUT_LINEAR : MID_LAYOUT_TEXTURE,
                                      use_layers && lfmt != MID_FMT_RGBA8 ? MID_FMT_WITH_GUIDE(fmt, lfmt) : fmt};
        const int out_fmt = hdr ? MID_FMT_RGBA32F : half ? MID_FMT_RGBA16F : MID_FMT_RGBA8;
        // One stage call of this run's filter: outputs [start, start + count) of the nf frames (L layers each, frame-major) into outs[0..count).
        // The k = 0 families take the block as a sub-array of frames, layers and outputs; the others the whole sequence, of which they
        // upload the block plus kk halo frames on either side, and their layers, from the host.
        auto run_stage = [&](mid_ctx *c, const mid_nlm_params &np, const mid_bilateral_params &bpp, const void *const *frames, int nf,
                             const void *const *layers, const void *const *motion, const void *const *albedo, int kk, int start, int count, void *const *outs,
                             float *t) {
            const void *const *lp = use_layers ? layers : nullptr;
            switch (af.family) {
            case SEQ_BILATERAL:
                MID_CHECK(mid_sequence_bilateral(c, &bpp, frames + start, count, lp ? lp + (size_t)start * L : nullptr, L, outs, out_fmt, 1, t)); break;
            case SEQ_NLM_LAYERS:
                MID_CHECK(mid_sequence_nlm_layers(c, &np, frames + start, count, lp + (size_t)start * L, L, outs, out_fmt, 1, t)); break;
            case SEQ_NLM_LAYERS_TEMPORAL:
                MID_CHECK(mid_sequence_nlm_layers_temporal(c, &np, frames, nf, lp, L, kk, start, count, outs, out_fmt, 1, t)); break;
            case SEQ_BILATERAL_JOINT:      // one weight from all layers
                MID_CHECK(mid_sequence_bilateral_joint(c, &bpp, jointSigma.data(), frames, nf, lp, L, kk, start, count, outs, out_fmt, 1, t)); break;
            case SEQ_ATROUS: {             // N passes of the 5x5 kernel with holes, every frame alone (a block is a range of the sequence)
                const mid_atrous_params ap{bpp.width, bpp.height, 0, opt.passes, opt.atrous_sigma_color, bpp.format};
                MID_CHECK(mid_sequence_atrous_joint(c, &ap, jointSigma.data(), frames, nf, lp, L, start, count, outs, out_fmt, 1, t)); break;
            }
            case SEQ_ATROUS_TEMPORAL: {    // pass 0 over the frames t-k..t+k, the later passes on frame t's estimate
                const mid_atrous_params ap{bpp.width, bpp.height, 0, opt.passes, opt.atrous_sigma_color, bpp.format};
                MID_CHECK(mid_sequence_atrous_joint_temporal(c, &ap, jointSigma.data(), frames, nf, lp, L, kk, start, count, outs, out_fmt, 1, t)); break;
            }
            case SEQ_ATROUS_VARIANCE: {    // the moments over the frames t-k..t+k, then the variance-guided passes on frame t
                const mid_atrous_variance_params vp{bpp.width, bpp.height, 0, opt.passes, opt.atrous_sigma_lum, opt.atrous_epsilon, bpp.format};
                MID_CHECK(mid_sequence_atrous_variance(c, &vp, jointSigma.data(), frames, nf, lp, L, kk, start, count, outs, out_fmt, 1, t)); break;
            }
            case SEQ_ATROUS_RECURSIVE: {   // per frame, in order: the spatial moments, the accumulation into the history, the variance-guided passes
                const mid_temporal_accum_params ap{bpp.width, bpp.height, opt.alpha, opt.alpha_moments, opt.history_max, 4.f, bpp.format};
                const mid_atrous_variance_params vp{bpp.width, bpp.height, 0, opt.passes, opt.atrous_sigma_lum, opt.atrous_epsilon, bpp.format};
                // (albedo: the chain runs on illumination -- demodulated first, modulated into the output; NULL is the plain call.
                // firefly: the clamp in front of the chain, after the demodulation; NULL is the call without it.
                // history clip: the reprojected history clipped to the colour box of the plane the accumulation reads; NULL likewise)
                const mid_firefly_params fp{bpp.width, bpp.height, opt.firefly_radius, opt.firefly_rank, opt.firefly_gain, opt.firefly_floor, bpp.format & 0xff};
                const mid_color_bounds_params cp{bpp.width, bpp.height, opt.history_clip_radius, opt.history_clip_gamma, bpp.format & 0xff};
                MID_CHECK(mid_sequence_atrous_recursive_clip(c, &ap, &vp, jointSigma.data(), frames, nf, lp, L, motion, albedo, opt.albedo_floor,
                                                             opt.firefly_rank ? &fp : nullptr, opt.history_clip ? &cp : nullptr, opt.feedback, opt.warmup,
                                                             start, count, outs, out_fmt, 1, t)); break;
            }
            case SEQ_GUIDED: {             // the local linear fit to the guide plane (or to the frame itself), every frame alone
                const mid_guided_params gp{bpp.width, bpp.height, opt.guided_radius, opt.guided_eps, bpp.format};
                MID_CHECK(mid_sequence_guided(c, &gp, frames, nf, lp, start, count, outs, out_fmt, 1, t)); break;
            }
            case SEQ_MEDIAN: {             // the median of every frame alone, plain or weighted by the frame's layers
                const mid_median_params mp{bpp.width, bpp.height, opt.median_radius, bpp.format};
                MID_CHECK(mid_sequence_median(c, &mp, lp ? jointSigma.data() : nullptr, frames, nf, lp, lp ? L : 0, start, count, outs, out_fmt, 1, t)); break;
            }
            case SEQ_NLM_JOINT:            // one patch weight from all layers (jointSigma: the h of each layer)
                MID_CHECK(mid_sequence_nlm_joint(c, &np, jointSigma.data(), frames, nf, lp, L, kk, start, count, outs, out_fmt, 1, t)); break;
            case SEQ_BILATERAL_TEMPORAL:   // plain or with the layers
                MID_CHECK(mid_sequence_bilateral_temporal(c, &bpp, frames, nf, lp, L, kk, start, count, outs, out_fmt, 1, t)); break;
            case SEQ_NLM:     // (one entry per output format; the casts only name the element type the library stores: every pointer of outs is a void *)
                if (hdr) MID_CHECK(mid_sequence_nlm_range(c, &np, frames, nf, kk, start, count, (mid_pixel *const *)outs, 1, t));
                else if (half) MID_CHECK(mid_sequence_nlm_range_f16(c, &np, frames, nf, kk, start, count, (uint16_t *const *)outs, 1, t));
                else MID_CHECK(mid_sequence_nlm_range_u8(c, &np, frames, nf, kk, start, count, (uint8_t *const *)outs, 1, t));
            }
        };
        const auto tw0 = std::chrono::steady_clock::now();
        for (int g = 0; g < G; ++g) {
            MID_CHECK(mid_ctx_create(opt.share_device ? opt.device : opt.device + g, &ctxs[g]));
            // (a) the kernel's code object and the pipeline's streams: two tiny frames through the same entry point
            const int ww = 64, wh = 32;
            mid_nlm_params wp = p;
            wp.width = ww; wp.height = wh;
            mid_bilateral_params wbp = bp;
            wbp.width = ww; wbp.height = wh;
            std::vector<unsigned char> a((size_t)ww * wh * 16, 0), o((size_t)ww * wh * 16), lz((size_t)ww * wh * 16, 0);   // (lz: a layer of any guide format)
            const void *wi[2] = {a.data(), a.data()};
            const void *wl[32];
            for (int l = 0; l < 2 * L; ++l) wl[l] = lz.data();
            void *wo[1] = {o.data()};
            const void *wa[2] = {lz.data(), lz.data()};            // (an albedo plane of zeros: the floor divides)
            run_stage(ctxs[g], wp, wbp, wi, 2, wl, nullptr, albedo_ptrs.empty() ? nullptr : wa, k > 0 ? 1 : 0, 0, 1, wo, nullptr);
            // (b) the pinned-memory DMA path in both directions at the real frame size (its first use in a process
            // costs several ms): frame 0 up into a scratch buffer, and back down into the first result buffer
            void *scratch = nullptr;
            MID_CHECK(mid_alloc(ctxs[g], std::max(in_bytes, out_bytes), &scratch));
            int rc = mid_memcpy_h2d(ctxs[g], scratch, in[0], in_bytes, nullptr);
            if (!rc) rc = mid_memcpy_d2h(ctxs[g], pin.outs[0], scratch, out_bytes, nullptr);
            if (!rc) rc = mid_stream_sync(ctxs[g], nullptr);
            (void)mid_free(ctxs[g], scratch);
            if (rc) throw std::runtime_error(mid_last_error());
        }
        const double warm_sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - tw0).count();
        std::vector<std::string> errors(G);
        std::vector<float> kern(G, 0.f), copy(G, 0.f);
        std::vector<std::thread> workers;
        // --halo rccl: one communicator rank per device (one process, ncclCommInitAll); created before the clock starts,
        // like the contexts
        std::vector<mid_comm *> comms(G, nullptr);
        struct CommGuard { std::vector<mid_comm *> &v; ~CommGuard() { for (auto c : v) if (c) (void)mid_comm_destroy(c); } } cguard{comms};
        if (opt.halo_rccl) MID_CHECK(mid_comm_create_all(ctxs.data(), G, comms.data()));
        // all ranks report whether their local set-up succeeded; arrive() returns true only if every one of them did
        struct Rendezvous {
            std::mutex m; std::condition_variable cv; int arrived = 0; const int n; bool ok = true;
            explicit Rendezvous(int n_) : n(n_) {}
            bool arrive(bool mine)
            {
                std::unique_lock<std::mutex> l(m);
                ok = ok && mine;
                if (++arrived == n) cv.notify_all();
                else cv.wait(l, [&] { return arrived == n; });
                return ok;
            }
        } rendezvous(G);
        const auto t0 = std::chrono::steady_clock::now();
        for (int g = 0; g < G; ++g)
            workers.emplace_back([&, g] {
                try {
                    int start = 0, count = 0; MID_CHECK(mid_shard_block(n, G, g, &start, &count));     // this device's frames (cannot fail: g < G)
                    if (opt.halo_rccl) {
                        // GPU-resident variant: the block is uploaded once and stays in HBM; the k frames on either side come
                        // from the neighbouring devices over xGMI (ncclSend/ncclRecv, one group) while the interior frames are
                        // being filtered; no frame is uploaded twice.  Every rank calls in, also one that owns no frame.
                        // mid_nlm_temporal_sharded is collective, so the ranks first finish everything that can fail locally
                        // (buffers, uploads, timers, the halo receive buffers) and AGREE that all of them did; if one did not,
                        // no rank enters the exchange.  A failure after that point aborts every communicator, so that ranks
                        // already waiting for the failed one return with an error instead of hanging.
                        mid_ctx *ctx = ctxs[g];
                        struct Dev { mid_ctx *c; std::vector<void *> p; ~Dev() { for (auto q : p) if (q) (void)mid_free(c, q); } } din{ctx, {}}, dout{ctx, {}};
                        struct TG { mid_timer *a = nullptr, *b = nullptr; ~TG() { (void)mid_timer_destroy(a); (void)mid_timer_destroy(b); } } tg;
                        bool ready = false;
                        try {
                            MID_CHECK(mid_timer_create(ctx, &tg.a));
                            MID_CHECK(mid_timer_create(ctx, &tg.b));
                            MID_CHECK(mid_timer_tick(tg.b, nullptr));
                            for (int i = 0; i < count; ++i) {
                                void *d = nullptr;
                                MID_CHECK(mid_alloc(ctx, in_bytes, &d)); din.p.push_back(d);
                                MID_CHECK(mid_memcpy_h2d(ctx, d, in[start + i], in_bytes, nullptr));
                                MID_CHECK(mid_alloc(ctx, (size_t)w * h * 16, &d)); dout.p.push_back(d);
                            }
                            if (!hdr && count) { void *u8 = nullptr; MID_CHECK(mid_alloc(ctx, out_bytes, &u8)); din.p.push_back(u8); }
                            MID_CHECK(mid_comm_reserve(comms[g], in_bytes, k));
                            MID_CHECK(mid_timer_tock(tg.b, nullptr));
                            MID_CHECK(mid_stream_sync(ctx, nullptr));
                            ready = true;
                        } catch (const std::exception &e) { errors[g] = e.what(); }
                        if (!rendezvous.arrive(ready)) return;          // (the rank that failed has recorded why)
                        try {
                            mid_timer *tk = tg.a, *tc = tg.b;
                            MID_CHECK(mid_timer_tick(tk, nullptr));
                            MID_CHECK(mid_nlm_temporal_sharded(comms[g], &p, din.p.data(), n, k, (mid_pixel *const *)dout.p.data(), nullptr));
                            MID_CHECK(mid_timer_tock(tk, nullptr));
                            void *u8 = (!hdr && count) ? din.p.back() : nullptr;
                            for (int i = 0; i < count; ++i) {
                                if (hdr) MID_CHECK(mid_memcpy_d2h(ctx, pin.outs[start + i], dout.p[i], out_bytes, nullptr));
                                else {   // GetImageFromGPU's u8 conversion (:97-103) on the device, then a quarter of the bytes come back
                                    MID_CHECK(mid_pack_u8(ctx, (const float *)dout.p[i], (size_t)w * h * 4, (uint8_t *)u8, nullptr));
                                    MID_CHECK(mid_memcpy_d2h(ctx, pin.outs[start + i], u8, out_bytes, nullptr));
                                }
                            }
                            MID_CHECK(mid_stream_sync(ctx, nullptr));
                            float ms = 0.f;
                            MID_CHECK(mid_timer_ms(tk, &ms)); kern[g] = ms;
                            MID_CHECK(mid_timer_ms(tc, &ms)); copy[g] = ms;
                        } catch (const std::exception &e) {
                            errors[g] = e.what();
                            for (auto c : comms) if (c) (void)mid_comm_abort(c);
                        }
                        return;
                    }
                    if (count == 0) return;
                    mid_ctx *ctx = ctxs[g];
                    float t[3] = {0, 0, 0};
                    run_stage(ctx, p, bp, in.data(), n, layer_ptrs.data(), motion_ptrs.empty() ? nullptr : motion_ptrs.data(),
                              albedo_ptrs.empty() ? nullptr : albedo_ptrs.data(), k, start, count, pin.outs.data() + start, t);
                    kern[g] = t[1]; copy[g] = t[2];
                } catch (const std::exception &e) { errors[g] = e.what(); }
            });
        for (auto &t : workers) t.join();
        for (auto &e : errors) if (!e.empty()) throw std::runtime_error(e);
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        m_execMs = *std::max_element(kern.begin(), kern.end());
        m_transferMs = *std::max_element(copy.begin(), copy.end());
        std::cout << "\tdecoded " << n << " frames into pinned memory in " << load_sec << " sec (" << io_threads << " file(s) at a time); device set-up + warm-up " << warm_sec << " sec\n";
        std::string words = af.words;
        if (af.bilateral()) words += " r=" + std::to_string(opt.radius);
        if (use_layers && af.family != SEQ_BILATERAL) words += " + " + std::to_string(L) + " layers";
        if (af.family == SEQ_ATROUS || af.family == SEQ_ATROUS_TEMPORAL || af.family == SEQ_ATROUS_VARIANCE || recursive) words += ", " + std::to_string(opt.passes) + " passes";
        if (recursive) words += ", feedback=" + std::to_string(opt.feedback) + ", warmup=" + std::to_string(opt.warmup);
        else if (af.windowed()) words += (words.empty() ? "k=" : ", k=") + std::to_string(k);
        std::cout << "\t" << n << " frames, " << words
                  << ", " << G << " device(s): " << sec << " sec, "
                  << (double)n * w * h / 1e6 / sec << " Mpixel/s end to end (host frames in -> host frames out)\n";
        // SaveEXR :1699 / lodepng::encode :1717, straight from the pinned results -- one file per worker thread, like the decode
        const std::string mode_name = af.infix;
        const auto te0 = std::chrono::steady_clock::now();
        for_each_file(0, n, [&](int i) {
            const std::string name = "output-animation-" + mode_name + fs::path(frameNames[i]).stem().string() + (hdr || half ? ".exr" : ".png");
            if (mid_image_save(out_path(name).c_str(), pin.outs[i], w, h, hdr ? MID_FMT_RGBA32F : half ? MID_FMT_RGBA16F : MID_FMT_RGBA8))
                throw std::runtime_error(mid_last_error());
        });
        if (!hdr && !half) for (int i = 0; i < n; ++i) std::cout << "\t\tencoding png\n";
        std::cout << "\tencoded " << n << " frames in " << std::chrono::duration<double>(std::chrono::steady_clock::now() - te0).count()
                  << " sec (" << io_threads << " file(s) at a time)\n";
    }

    void save(std::string name, const Pixel *px, int w, int h, bool hdr) const
    {
        if (hdr) {
            name += ".exr";
            MID_CHECK(mid_image_save(out_path(name).c_str(), px, w, h, MID_FMT_RGBA32F));     // SaveEXR :1699
        } else {
            name += ".png";
            std::cout << "\t\tencoding png\n";
            std::vector<unsigned char> resultData((size_t)w * h * 4);
            const long npx = (long)w * h;
#pragma omp parallel for default(shared) schedule(static)
            for (long i = 0; i < npx; ++i) {                                                          // GetImageFromGPU :97-103
                const float v[4] = {255.0f * px[i].r, 255.0f * px[i].g, 255.0f * px[i].b, 255.0f * px[i].a};
                for (int c = 0; c < 4; ++c)      // truncation; clamped only where the C cast is undefined
                    resultData[i * 4 + c] = !(v[c] > -1.0f) ? 0 : v[c] >= 256.0f ? 255 : (unsigned char)v[c];
            }
            MID_CHECK(mid_image_save(out_path(name).c_str(), resultData.data(), w, h, MID_FMT_RGBA8));  // lodepng::encode :1717
        }
    }

    // RunOnCPU, src/main.cpp:1732-1921
    void RunOnCPU(const std::string &fileName, int numThreads)
    {
        HostImage img = load(fileName, false);
        const int w = img.w, h = img.h;
        std::vector<Pixel> inputPixels((size_t)w * h);
        if (img.format == MID_FMT_RGBA32F) {
            std::cout << "\tloading hdr\n";
            memcpy((void *)inputPixels.data(), img.data(), img.size());
        } else {
            for (size_t i = 0; i < (size_t)w * h; ++i) {                                              // :1804-1807
                inputPixels[i].r = (float)img.data()[4 * i + 0] * (1.0f / 255.0f);
                inputPixels[i].g = (float)img.data()[4 * i + 1] * (1.0f / 255.0f);
                inputPixels[i].b = (float)img.data()[4 * i + 2] * (1.0f / 255.0f);
                inputPixels[i].a = (float)img.data()[4 * i + 3] * (1.0f / 255.0f);
            }
        }
        std::cout << "\tdoing computations\n";
        std::vector<Pixel> outputPixels;
        cpu_bilateral_refpath(inputPixels, w, h, opt.cpu_radius, opt.cpu_sigma_s, opt.cpu_sigma_c, opt.cpu_blue_bug, numThreads, outputPixels);
        std::cout << "\tsaving image\n";
        save("output-cpu", outputPixels.data(), w, h, img.format == MID_FMT_RGBA32F);
    }
};

// ---- --compare TEST REFERENCE: full-reference metrics (mid_image_metrics, section a4n) ------------------------------------------
// A sub-mode that runs no filter and writes no image: both files are decoded (.png as RGBA8, .exr as RGBA32F or, with --half, as
// RGBA16F; the two may differ in type), uploaded and compared on one stream, pair by pair, and one line per pair is printed whose
// numbers read back bit for bit (%.17g).  With --animation TEST's siblings of its extension are paired with REFERENCE's by the
// 4-character frame id of discover_files's rule, and a last line gives the means of the per-frame values.
static std::string metrics_number(double v)
{
    char buf[64];
    if (std::isnan(v)) return "nan";                            // (printf would print the sign of a NaN)
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

static std::string metrics_fields(const mid_image_metrics_result &r)
{
    return "n " + metrics_number(r.n_valid) + " invalid " + metrics_number(r.n_invalid) + " mse " + metrics_number(r.mse) + " psnr " +
           metrics_number(r.psnr) + " mae " + metrics_number(r.mae) + " max " + metrics_number(r.max_abs) + " relmse " + metrics_number(r.relmse) +
           " ssim " + metrics_number(r.ssim);
}

// the siblings of `image` with its extension, sorted by name: discover_files's frames, no layers
static std::vector<std::string> compare_siblings(const std::string &image)
{
    std::vector<std::string> frames, none;
    discover_files(image, frames, none, true, false);
    return frames;
}

static void run_compare(const Options &opt)
{
    std::vector<std::pair<std::string, std::string>> pairs;
    if (!opt.animation) pairs.emplace_back(opt.compare_test, opt.compare_ref);
    else {
        const std::vector<std::string> tests = compare_siblings(opt.compare_test), refs = compare_siblings(opt.compare_ref);
        for (size_t i = 0; i < tests.size(); ++i) {
            const std::string id = frame_id_of(tests[i]);
            for (size_t k = 0; k < i; ++k)
                if (frame_id_of(tests[k]) == id)
                    throw std::runtime_error("--compare: test frames " + tests[k] + " and " + tests[i] + " share the frame id " + id + " and so the partner");
            std::vector<std::string> found;
            for (const std::string &r : refs) if (frame_id_of(r) == id) found.push_back(r);
            if (found.empty()) throw std::runtime_error("--compare: test frame " + tests[i] + " has no partner with the frame id " + id + " beside " + opt.compare_ref);
            if (found.size() > 1) throw std::runtime_error("--compare: test frame " + tests[i] + " has two partners, " + found[0] + " and " + found[1]);
            pairs.emplace_back(tests[i], found[0]);
        }
        if (pairs.empty()) throw std::runtime_error("--compare: no frames beside " + opt.compare_test);
    }

    mid_ctx *ctx = nullptr;
    MID_CHECK(mid_ctx_create(opt.device, &ctx));
    struct CtxGuard { mid_ctx *c; ~CtxGuard() { mid_ctx_destroy(c); } } guard{ctx};
    struct Dev {                                                // one device buffer, grown on demand, freed with the run
        mid_ctx *c; void *p = nullptr; size_t n = 0;
        ~Dev() { if (p) (void)mid_free(c, p); }
        void *need(size_t bytes)
        {
            if (bytes > n) { if (p) { MID_CHECK(mid_free(c, p)); p = nullptr; n = 0; } MID_CHECK(mid_alloc(c, bytes, &p)); n = bytes; }
            return p;
        }
    } da{ctx}, db{ctx}, dwork{ctx};
    struct Img { mid_image img{}; ~Img() { if (img.data) mid_image_free(&img); } };
    auto load = [&](const std::string &path, Img &im) {
        const bool hdr = fs::path(path).extension() == ".exr";
        if (hdr && opt.half ? mid_image_load_f16(nullptr, path.c_str(), &im.img) : mid_image_load(path.c_str(), &im.img)) throw std::runtime_error(mid_last_error());
    };
    auto bytes_of = [](const mid_image &i) { return (size_t)i.width * i.height * (i.format == MID_FMT_RGBA32F ? 16 : i.format == MID_FMT_RGBA16F ? 8 : 4); };

    double mean[11] = {0};
    for (const auto &pr : pairs) {
        Img a, b;
        {                                                       // the two files of a pair decode side by side: the run is decode-bound
            std::string err_b;
            std::thread tb([&] { try { load(pr.second, b); } catch (const std::exception &e) { err_b = e.what(); if (err_b.empty()) err_b = pr.second; } });
            try { load(pr.first, a); } catch (...) { tb.join(); throw; }
            tb.join();
            if (!err_b.empty()) throw std::runtime_error(err_b);
        }
        if (a.img.width != b.img.width || a.img.height != b.img.height)
            throw std::runtime_error("--compare: " + pr.first + " is " + std::to_string(a.img.width) + "x" + std::to_string(a.img.height) + " but " + pr.second +
                                     " is " + std::to_string(b.img.width) + "x" + std::to_string(b.img.height));
        mid_image_metrics_params p{a.img.width, a.img.height, a.img.format, b.img.format, opt.peak, opt.relmse_eps, opt.compare_ssim ? 1 : 0};
        const size_t nw = mid_image_metrics_workspace(p.width, p.height);
        if (!nw) throw std::runtime_error("--compare: " + pr.first + ": a frame of " + std::to_string(p.width) + "x" + std::to_string(p.height) + " is too large");
        void *pa = da.need(bytes_of(a.img)), *pb = db.need(bytes_of(b.img)), *pw = dwork.need(nw);
        MID_CHECK(mid_memcpy_h2d(ctx, pa, a.img.data, bytes_of(a.img), nullptr));
        MID_CHECK(mid_memcpy_h2d(ctx, pb, b.img.data, bytes_of(b.img), nullptr));
        MID_CHECK(mid_image_metrics(ctx, &p, pa, pb, pw, nullptr, nullptr));
        double sums[MID_METRICS_N];
        MID_CHECK(mid_memcpy_d2h(ctx, sums, pw, sizeof sums, nullptr));
        MID_CHECK(mid_stream_sync(ctx, nullptr));
        mid_image_metrics_result r;
        MID_CHECK(mid_image_metrics_derive(sums, &p, &r));
        std::cout << "metrics " << pr.first << " vs " << pr.second << " " << metrics_fields(r) << "\n";
        const double vals[11] = {r.n_valid, r.n_invalid, r.mse, r.mse_r, r.mse_g, r.mse_b, r.mae, r.max_abs, r.psnr, r.relmse, r.ssim};
        for (int i = 0; i < 11; ++i) mean[i] += vals[i];
    }
    if (opt.animation) {
        const double n = (double)pairs.size();
        mid_image_metrics_result m{mean[0] / n, mean[1] / n, mean[2] / n, mean[3] / n, mean[4] / n, mean[5] / n, mean[6] / n, mean[7] / n, mean[8] / n, mean[9] / n, mean[10] / n};
        std::cout << "metrics mean over " << pairs.size() << " frames " << metrics_fields(m) << "\n";
    }
}

static void usage()
{
    std::cout <<
        "usage: mi_denoise [image] [options]\n"
        "  image                     target .png or .exr (default Animations/CornellBox/Animation01_LDR_0000.png)\n"
        "  --outdir DIR              where output-*.{png,exr} go (default .)\n"
        "  --device N                HIP device (default 0)\n"
        "  --modes LIST              comma list of bilateral,layers,linear,nlm,multiframe,overlap (default all, reference order),\n"
        "                            and nlm-layers (not part of all): NLM with its weights taken from the image's RenderElements\n"
        "                            layers (--nlm-h / --search / --patch apply), output output-nonlinear-nlm-layers.{png,exr};\n"
        "                            and joint (not part of all): the joint (cross) bilateral, ONE weight per tap from all of the\n"
        "                            image's layers -- the product of the spatial term and one range term per layer, each layer\n"
        "                            with its own sigma (--sigma-layers, else --sigma-c for all; --radius / --sigma-s apply),\n"
        "                            output output-nonlinear-bialteral-joint.{png,exr};\n"
        "                            and nlm-joint (not part of all): joint layer-guided NLM, ONE weight per search offset from the\n"
        "                            patch distances of all of the image's layers, each layer with its own h (--h-layers, else\n"
        "                            --nlm-h for all; --search / --patch apply; .png layers only, as nlm-layers),\n"
        "                            output output-nonlinear-nlm-joint.{png,exr};\n"
        "                            and atrous (not part of all): the edge-avoiding a-trous filter, --passes passes of a 5x5 B3-spline\n"
        "                            kernel, pass i sampling with holes at step 2^i (five passes reach +-62 pixels), every tap weighed\n"
        "                            by all of the image's layers at once as in joint (--sigma-layers, else --sigma-c for all; the\n"
        "                            layer rules of joint, .png or .exr) and, with --atrous-sigma-color, by the colour itself,\n"
        "                            output output-nonlinear-atrous.{png,exr};\n"
        "                            and atrous-variance (not part of all): the same passes guided by the per-pixel variance of the\n"
        "                            luminance -- estimated from a 7x7 neighbourhood weighed by the layers, it sets the width of a\n"
        "                            luminance term per pixel (wide where the image is noisy, narrow where it has converged) and is\n"
        "                            filtered along with the colour (--passes, --sigma-layers, --atrous-sigma-lum, --atrous-epsilon;\n"
        "                            the layer rules of atrous), output output-nonlinear-atrous-variance.{png,exr};\n"
        "                            and median (not part of all): the median of the (2 R + 1)^2 window per channel, weighted by the frame's\n"
        "                            layers or plain (--median-radius, --median-plain), output output-nonlinear-median.{png,exr}; texels\n"
        "                            that are not finite take no part, so a NaN pixel is repaired from its neighbours\n"
        "                            and guided (not part of all): the guided filter -- inside every (2 R + 1)^2 window the image is fitted\n"
        "                            as an affine function of the guide's colour and the averaged fit is evaluated at the pixel's own guide\n"
        "                            texel, so the guide's edges and texture are reproduced and the cost does not depend on R\n"
        "                            (--guided-radius, --guided-eps, --guide-layer), output output-nonlinear-guided.{png,exr}.\n"
        "                            Layer files: .png (RGBA8) -- or, for the bilateral modes only (layers and joint here, layers,\n"
        "                            layers-temporal, joint and joint-temporal under --animation-filter), .exr: normals, depth, HDR albedo as rendered, read as\n"
        "                            RGBA32F, or as RGBA16F with --half; all layers of a run must have one format; nlm-layers and\n"
        "                            nlm-layers-temporal take .png layers only (their patch distances are integer sums of bytes)\n"
        "  --gpu-only | --cpu-only   run only the GPU modes / only the CPU runs\n"
        "  --radius R                bilateral window radius (default 20 = TEXEL_WINDOW)\n"
        "  --sigma-s S --sigma-c C   bilateral sigmas (default 2.0 0.2)\n"
        "  --sigma-layers A,B,...    the joint modes: one range sigma per layer, in the sorted order the layer files are found in (the\n"
        "                            run prints one `layer <file> sigma <value>` line each); a count other than the layer count\n"
        "                            is refused.  Default: --sigma-c for every layer.  Scale it to the layer's units: normals ~0.3,\n"
        "                            depth in scene units, HDR albedo ~0.5\n"
        "  --nlm-h H                 NLM filtering parameter (default 0.5)\n"
        "  --h-layers A,B,...        the joint NLM modes: one h per layer, in the sorted order the layer files are found in (the run\n"
        "                            prints one `layer <file> h <value>` line each); a count other than the layer count is refused.\n"
        "                            Default: --nlm-h for every layer\n"
        "  --passes N                the a-trous modes: passes of the 5x5 kernel, 1..8 (default 5; pass i has step 2^i)\n"
        "  --atrous-sigma-color X    the a-trous modes: sigma of the colour term at pass 0, halved with every pass (default 0: no\n"
        "                            colour term, the layers alone stop the filter at edges)\n"
        "  --atrous-sigma-lum X      atrous-variance: the luminance term lets through differences of about X standard deviations of\n"
        "                            the pixel's luminance (default 4; 0: no luminance term)\n"
        "  --atrous-epsilon X        atrous-variance: added to X * sqrt(variance), so that a converged pixel (variance 0) still averages\n"
        "                            texels that differ by rounding alone (default 1e-3, for luminances of order 1; > 0)\n"
        "  --median-radius R         median (--modes median, --animation-filter median): window radius, 1..3 (default 1): 9, 25 or 49 taps\n"
        "  --median-plain            median: load no layers, the plain median; otherwise the frame's RenderElements layers weigh the taps as\n"
        "                            for atrous (--sigma-layers, else --sigma-c).  The run prints `median radius <r> layers <n>`\n"
        "  --guided-radius R         guided (--modes guided, --animation-filter guided): window radius, 1..16 (default 8)\n"
        "  --guided-eps X            guided: the regulariser, finite and > 0, in squared units of the guide (default 0.01): windows whose\n"
        "                            guide varies by much less than sqrt(X) are averaged, windows that vary by more carry the guide's edge\n"
        "  --guide-layer SUBSTR      guided: the render element whose file name contains SUBSTR is the guide (.png read as RGBA8, .exr as\n"
        "                            RGBA32F, or RGBA16F with --half); no match or several are refused.  Without it the image guides\n"
        "                            itself and no layers are loaded.  The run prints `guided guide <file|self> radius <r> eps <x>`\n"
        "  --search LO,HI --patch LO,HI   half-open NLM ranges (default -7,7 and -3,3; 21x21/7x7 is -10,11 and -3,4)\n"
        "  --alpha X                 atrous-recursive: floor of the colour blend factor, (0, 1] (default 0.2)\n"
        "  --alpha-moments X         atrous-recursive: floor of the moments' blend factor, (0, 1] (default 0.2)\n"
        "  --history-max N           atrous-recursive: cap of the per-pixel history length (default 32)\n"
        "  --feedback 0|1            atrous-recursive: the next colour history is the accumulated colour (0) or the level after pass 0 (1, default)\n"
        "  --warmup N                atrous-recursive: frames accumulated before a block's first output and not written (default 16)\n"
        "  --motion-layer SUBSTR     atrous-recursive: the .exr render element of every frame whose file name contains SUBSTR holds the\n"
        "                            motion in its R and G channels, in pixels (pixel p was at p + motion(p) in the previous frame); it is\n"
        "                            taken out of the guide layers.  Without it motion is zero.  A .png, no match or several are refused\n"
        "  --motion-scale SX,SY      atrous-recursive: factors on the motion's R and G (default 1,1)\n"
        "  --albedo-layer SUBSTR     atrous-recursive: the render element of every frame (.png or .exr, in the guide layers' format) whose\n"
        "                            file name contains SUBSTR holds the surface albedo; it is taken out of the guide layers.  The filter\n"
        "                            then runs on illumination: every frame is divided by max(albedo, floor) before it is accumulated and\n"
        "                            filtered, and the albedo is multiplied back into the output, so a texture neither stops the filter\n"
        "                            nor is blurred.  Without it the filter runs on colour.  No match or several are refused\n"
        "  --albedo-floor X          atrous-recursive with --albedo-layer: lower bound of the divisor, finite and > 0 (default 0.001)\n"
        "  --firefly-rank K          atrous-recursive: 1..4 switches the firefly clamp on, in front of the accumulation and after the\n"
        "                            demodulation: a pixel brighter than G times the K-th largest finite luminance of its neighbourhood\n"
        "                            is scaled down to that limit, a pixel with a NaN or Inf channel becomes a grey of the limit, so\n"
        "                            neither a firefly nor a NaN enters the history.  K = 2 also removes fireflies that come in pairs\n"
        "  --firefly-radius R        with --firefly-rank: 1 | 2, a 3x3 or 5x5 neighbourhood (default 1)\n"
        "  --firefly-gain G          with --firefly-rank: factor on the limit, finite and > 0 (default 1)\n"
        "  --firefly-floor X         with --firefly-rank: a luminance that is always let through, finite and >= 0, in illumination\n"
        "                            units with --albedo-layer (default 0)\n"
        "  --history-clip GAMMA      atrous-recursive: clip the reprojected history of every pixel, per colour channel, to the box\n"
        "                            mean -+ GAMMA standard deviations of the current frame's neighbourhood (after the demodulation\n"
        "                            and the firefly clamp) before it is blended: when the lighting changes and the geometry does\n"
        "                            not, no ghost of the old lighting stays in the output.  GAMMA finite and >= 0; 1 is the usual value\n"
        "  --history-clip-radius R   with --history-clip: 1 | 2, a 3x3 or 5x5 neighbourhood, centre included (default 1)\n"
        "  --temporal-k K            multiframe: frames t-K..t+K of the sorted sequence instead of the reference's list\n"
        "  --animation               denoise EVERY sibling frame with temporal NLM (window +-K, default 2) instead of the mode list\n"
        "  --animation-filter F      animation mode: nlm (default: temporal NLM), or the bilateral of every frame -- bilateral\n"
        "                            (texture addressing), linear (linear addressing) or layers (guided by each frame's own\n"
        "                            RenderElements layers, 1..16 per frame, the same count for all, .png or .exr); --radius / --sigma-s / --sigma-c\n"
        "                            apply; outputs output-animation-{nonlinear-bialteral,linear-bialteral,nonlinear-bialteral-layers}-*;\n"
        "                            or nlm-layers: NLM of every frame guided by its own layers (the same layer rules as layers;\n"
        "                            --nlm-h / --search / --patch apply), outputs output-animation-nonlinear-nlm-layers-*\n"
        "                            (it ignores --temporal-k); or nlm-layers-temporal: the same over the frames t-K..t+K -- the\n"
        "                            patch distance between frame t's layer and the neighbour frame's layer, the colour from the\n"
        "                            neighbour frame (--temporal-k, default 2; frame blocks take their K halo frames and layers\n"
        "                            from the host, not with --halo rccl), outputs\n"
        "                            output-animation-nonlinear-nlm-layers-multiframe-*;\n"
        "                            or bilateral-temporal / layers-temporal: the bilateral over the frames t-K..t+K, plain or\n"
        "                            guided by each frame's layers (K = --temporal-k, default 2; --radius / --sigma-s / --sigma-c\n"
        "                            apply; halo frames and their layers from the host, not with --halo rccl), outputs\n"
        "                            output-animation-nonlinear-bialteral-multiframe-* and\n"
        "                            output-animation-nonlinear-bialteral-layers-multiframe-*;\n"
        "                            or joint / joint-temporal: the joint bilateral (one weight from all of a frame's layers,\n"
        "                            --sigma-layers) of every frame alone (joint ignores --temporal-k) or over the frames t-K..t+K\n"
        "                            (K = --temporal-k, default 2; the layer rules, frame blocks and halo of layers-temporal),\n"
        "                            outputs output-animation-nonlinear-bialteral-joint-* and\n"
        "                            output-animation-nonlinear-bialteral-joint-multiframe-*;\n"
        "                            or nlm-joint / nlm-joint-temporal: joint layer-guided NLM (one weight from all of a frame's\n"
        "                            layers, --h-layers; .png layers only) of every frame alone (nlm-joint ignores --temporal-k) or\n"
        "                            over the frames t-K..t+K (K = --temporal-k, default 2; frame blocks and halo of\n"
        "                            nlm-layers-temporal, not with --halo rccl), outputs output-animation-nonlinear-nlm-joint-* and\n"
        "                            output-animation-nonlinear-nlm-joint-multiframe-*;\n"
        "                            or atrous: the a-trous filter of every frame alone (--passes, --sigma-layers,\n"
        "                            --atrous-sigma-color; the layer rules of joint; it ignores --temporal-k, frame blocks have no\n"
        "                            halo, not with --halo rccl), outputs output-animation-nonlinear-atrous-*;\n"
        "                            or atrous-temporal: the same with pass 0 taking its taps from the frames t-K..t+K, weighed by\n"
        "                            frame t's layers against the neighbour frame's (K = --temporal-k, default 2; the later passes\n"
        "                            filter frame t's estimate; the layer rules of atrous, the frame blocks and halo of\n"
        "                            joint-temporal, not with --halo rccl), outputs output-animation-nonlinear-atrous-multiframe-*;\n"
        "                            or atrous-variance: the variance-guided a-trous filter of every frame, its variance estimated\n"
        "                            over the frames t-K..t+K (K = --temporal-k, default 2; --passes, --sigma-layers,\n"
        "                            --atrous-sigma-lum, --atrous-epsilon; the layer rules of atrous, the frame blocks and halo of\n"
        "                            joint-temporal, not with --halo rccl), outputs output-animation-nonlinear-atrous-variance-*\n"
        "                            or atrous-recursive: recursive temporal accumulation (a history of colour and luminance moments,\n"
        "                            blended as lerp(history, frame, max(1/N, alpha))), then the variance-guided passes, frame after\n"
        "                            frame (--alpha, --alpha-moments, --history-max, --feedback, --warmup, --motion-layer,\n"
        "                            --motion-scale, --albedo-layer, --albedo-floor, --firefly-rank, --firefly-radius, --firefly-gain, --firefly-floor,\n"
        "                            --history-clip, --history-clip-radius;\n"
        "                            --passes, --sigma-layers, --atrous-sigma-lum,\n"
        "                            --atrous-epsilon as atrous-variance;\n"
        "                            it ignores --temporal-k; not with --halo rccl), outputs output-animation-nonlinear-atrous-recursive-*.\n"
        "                            With --gpus N every frame block starts its history --warmup frames before its block: a sharded\n"
        "                            run equals the unsharded one bit for bit only when the warm-up reaches frame 0;\n"
        "                            or median: the median of every frame alone, weighted by its own layers or plain (--median-radius,\n"
        "                            --median-plain), output-animation-nonlinear-median-*\n"
        "                            or guided: the guided filter of every frame alone, guided by the one render element of each frame\n"
        "                            that --guide-layer names, or by the frame itself (--guided-radius, --guided-eps; it ignores\n"
        "                            --temporal-k, frame blocks have no halo, not with --halo rccl), outputs\n"
        "                            output-animation-nonlinear-guided-*\n"
        "  --gpus N                  animation mode: split the sequence into N frame blocks, one per device\n"
        "  --halo host|rccl          animation mode with --gpus N: 'host' (default) streams every block plus its K halo frames from host\n"
        "                            memory through the overlapped pipeline; 'rccl' keeps each block resident in its GPU's HBM and\n"
        "                            exchanges the halo frames GPU to GPU over RCCL/xGMI\n"
        "  --share-device            animation mode: all --gpus N blocks run on --device (a rehearsal of the N-block schedule on fewer\n"
        "                            devices; with --halo rccl it needs a stand-in for RCCL, MID_RCCL_LIBRARY: RCCL itself refuses\n"
        "                            two ranks on one device)\n"
        "  --pageable-host           the six GPU modes: decode into and read back to ordinary (not page-locked) memory; the library\n"
        "                            then moves every copy through its own pinned bounce buffers -- same files, slower copies\n"
        "  --pinned-mb M             animation mode: page-lock at most M MiB of host memory for frames in and out (default 16384);\n"
        "                            frames beyond that, or whose page-locked allocation fails, use pageable memory (a frame's\n"
        "                            layers count at their real size: 4, 8 or 16 bytes per pixel)\n"
        "  --io-threads T            animation mode: decode / encode T files at a time, one per host thread (default min(16, hardware threads))\n"
        "  --half                    .exr inputs of the GPU modes and of --animation: load the frames as RGBA16F (half float: HALF\n"
        "                            channels bit for bit), filter them as such and write HALF EXR outputs (the fp32 result rounded\n"
        "                            to nearest even).  PNG inputs and the CPU runs ignore it; not with --halo rccl.  .exr LAYERS of\n"
        "                            the bilateral modes load as RGBA16F with it as well, whatever the frames are\n"
        "  --compare TEST REFERENCE  a sub-mode that runs no filter and writes no image: how close TEST is to REFERENCE (a converged\n"
        "                            render, usually), over the pixels whose R, G and B are finite in both.  One line is printed:\n"
        "                            metrics <test> vs <reference> n <valid> invalid <k> mse <..> psnr <..> mae <..> max <..> relmse <..>\n"
        "                            ssim <..>, every number with 17 significant digits (it reads back bit for bit).  .png files load as\n"
        "                            RGBA8, .exr as RGBA32F or, with --half, as RGBA16F; the two may differ in type, not in size.\n"
        "                            With --animation TEST's siblings of its extension are paired with REFERENCE's siblings by the\n"
        "                            4-character frame id: one line per pair in sorted order, then `metrics mean over <n> frames ...`,\n"
        "                            the means of the per-frame values; a test frame with no partner, or a partner shared by two, is\n"
        "                            refused by name.  Not with --modes, --animation-filter or --gpus\n"
        "  --peak X                  with --compare: the data range PSNR and SSIM refer to, finite and > 0 (default 1; 255 for integer levels)\n"
        "  --relmse-eps X            with --compare: relMSE is the mean of d^2 / (reference^2 + X), finite and > 0 (default 0.01)\n"
        "  --no-ssim                 with --compare: the pointwise metrics only; ssim is printed as nan\n"
        "  --cpu-radius R --cpu-sigma-s S --cpu-sigma-c C   CPU path (default 10 10.0 0.2)\n"
        "  --cpu-threads A,B         thread counts of the CPU runs (default 1,8)\n"
        "  --cpu-fix-blue            use the blue channel in the CPU range distance (the reference does not)\n";
}

static bool pair_arg(const char *s, int &a, int &b) { return sscanf(s, "%d,%d", &a, &b) == 2; }

int main(int argc, char **argv)
{
    Options opt;
    bool have_image = false, modes_given = false, filter_given = false, gpus_given = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char * { if (i + 1 >= argc) { usage(); exit(EXIT_FAILURE); } return argv[++i]; };
        if (a == "-h" || a == "--help") { usage(); return EXIT_SUCCESS; }
        else if (a == "--outdir") opt.outdir = next();
        else if (a == "--device") opt.device = atoi(next());
        else if (a == "--modes") { opt.modes = next(); modes_given = true; }
        else if (a == "--compare") { opt.compare = true; opt.compare_test = next(); opt.compare_ref = next(); }
        else if (a == "--peak") {
            opt.peak = (float)atof(next());
            if (!opt.compare_other) opt.compare_other = "--peak";
            if (!(std::isfinite(opt.peak) && opt.peak > 0.f)) { std::cerr << "--peak " << opt.peak << " must be finite and > 0\n"; return EXIT_FAILURE; }
        }
        else if (a == "--relmse-eps") {
            opt.relmse_eps = (float)atof(next());
            if (!opt.compare_other) opt.compare_other = "--relmse-eps";
            if (!(std::isfinite(opt.relmse_eps) && opt.relmse_eps > 0.f)) { std::cerr << "--relmse-eps " << opt.relmse_eps << " must be finite and > 0\n"; return EXIT_FAILURE; }
        }
        else if (a == "--no-ssim") { opt.compare_ssim = false; if (!opt.compare_other) opt.compare_other = "--no-ssim"; }
        else if (a == "--guided-radius") {
            opt.guided_radius = atoi(next());
            if (!opt.guided_other) opt.guided_other = "--guided-radius";
            if (opt.guided_radius < 1 || opt.guided_radius > 16) { std::cerr << "--guided-radius " << opt.guided_radius << " is outside 1..16\n"; return EXIT_FAILURE; }
        }
        else if (a == "--guided-eps") {
            opt.guided_eps = (float)atof(next());
            if (!opt.guided_other) opt.guided_other = "--guided-eps";
            if (!(std::isfinite(opt.guided_eps) && opt.guided_eps > 0.f)) { std::cerr << "--guided-eps " << opt.guided_eps << " must be finite and > 0\n"; return EXIT_FAILURE; }
        }
        else if (a == "--median-radius") {
            opt.median_radius = atoi(next());
            if (!opt.median_other) opt.median_other = "--median-radius";
            if (opt.median_radius < 1 || opt.median_radius > 3) { std::cerr << "--median-radius " << opt.median_radius << " is outside 1..3\n"; return EXIT_FAILURE; }
        }
        else if (a == "--median-plain") { opt.median_plain = true; if (!opt.median_other) opt.median_other = "--median-plain"; }
        else if (a == "--guide-layer") { opt.guide_layer = next(); if (!opt.guided_other) opt.guided_other = "--guide-layer"; }
        else if (a == "--gpu-only") opt.run_cpu = false;
        else if (a == "--cpu-only") opt.run_gpu = false;
        else if (a == "--radius") opt.radius = atoi(next());
        else if (a == "--sigma-s") opt.sigma_s = (float)atof(next());
        else if (a == "--sigma-c") opt.sigma_c = (float)atof(next());
        else if (a == "--sigma-layers") {
            opt.sigma_layers.clear();
            const std::string s = next();
            size_t pos = 0;
            while (pos < s.size()) { size_t c = s.find(',', pos); if (c == std::string::npos) c = s.size(); opt.sigma_layers.push_back((float)atof(s.substr(pos, c - pos).c_str())); pos = c + 1; }
            if (opt.sigma_layers.empty()) { std::cerr << "--sigma-layers needs a comma list of sigmas\n"; usage(); return EXIT_FAILURE; }
        }
        else if (a == "--nlm-h") opt.nlm_h = (float)atof(next());
        else if (a == "--h-layers") {
            opt.h_layers.clear();
            const std::string s = next();
            size_t pos = 0;
            while (pos < s.size()) { size_t c = s.find(',', pos); if (c == std::string::npos) c = s.size(); opt.h_layers.push_back((float)atof(s.substr(pos, c - pos).c_str())); pos = c + 1; }
            if (opt.h_layers.empty()) { std::cerr << "--h-layers needs a comma list of values\n"; usage(); return EXIT_FAILURE; }
        }
        else if (a == "--passes") {
            opt.passes = atoi(next());
            if (opt.passes < 1 || opt.passes > 8) { std::cerr << "--passes " << opt.passes << " is outside 1..8\n"; return EXIT_FAILURE; }
        }
        else if (a == "--atrous-sigma-color") opt.atrous_sigma_color = (float)atof(next());
        else if (a == "--atrous-sigma-lum") opt.atrous_sigma_lum = (float)atof(next());
        else if (a == "--atrous-epsilon") opt.atrous_epsilon = (float)atof(next());
        else if (a == "--alpha") opt.alpha = (float)atof(next());
        else if (a == "--alpha-moments") opt.alpha_moments = (float)atof(next());
        else if (a == "--history-max") opt.history_max = (float)atof(next());
        else if (a == "--feedback") {
            opt.feedback = atoi(next());
            if (opt.feedback != 0 && opt.feedback != 1) { std::cerr << "--feedback " << opt.feedback << " is neither 0 nor 1\n"; return EXIT_FAILURE; }
        }
        else if (a == "--warmup") {
            opt.warmup = atoi(next());
            if (opt.warmup < 0) { std::cerr << "--warmup " << opt.warmup << " is negative\n"; return EXIT_FAILURE; }
        }
        else if (a == "--motion-layer") opt.motion_layer = next();
        else if (a == "--albedo-layer") opt.albedo_layer = next();
        else if (a == "--albedo-floor") { opt.albedo_floor = (float)atof(next()); opt.albedo_floor_given = true; }
        else if (a == "--firefly-rank") {
            opt.firefly_rank = atoi(next());
            if (opt.firefly_rank < 1 || opt.firefly_rank > 4) { std::cerr << "--firefly-rank " << opt.firefly_rank << " is outside 1..4\n"; return EXIT_FAILURE; }
        }
        else if (a == "--history-clip") {
            opt.history_clip_gamma = (float)atof(next());
            opt.history_clip = true;
            if (!(std::isfinite(opt.history_clip_gamma) && opt.history_clip_gamma >= 0.f)) { std::cerr << "--history-clip " << opt.history_clip_gamma << " must be finite and >= 0\n"; return EXIT_FAILURE; }
        }
        else if (a == "--history-clip-radius") {
            opt.history_clip_radius = atoi(next());
            opt.history_clip_radius_given = true;
            if (opt.history_clip_radius != 1 && opt.history_clip_radius != 2) { std::cerr << "--history-clip-radius " << opt.history_clip_radius << " is neither 1 nor 2\n"; return EXIT_FAILURE; }
        }
        else if (a == "--firefly-radius") {
            opt.firefly_radius = atoi(next());
            if (!opt.firefly_other) opt.firefly_other = "--firefly-radius";
            if (opt.firefly_radius != 1 && opt.firefly_radius != 2) { std::cerr << "--firefly-radius " << opt.firefly_radius << " is neither 1 nor 2\n"; return EXIT_FAILURE; }
        }
        else if (a == "--firefly-gain") {
            opt.firefly_gain = (float)atof(next());
            if (!opt.firefly_other) opt.firefly_other = "--firefly-gain";
            if (!(std::isfinite(opt.firefly_gain) && opt.firefly_gain > 0.f)) { std::cerr << "--firefly-gain " << opt.firefly_gain << " must be finite and > 0\n"; return EXIT_FAILURE; }
        }
        else if (a == "--firefly-floor") {
            opt.firefly_floor = (float)atof(next());
            if (!opt.firefly_other) opt.firefly_other = "--firefly-floor";
            if (!(std::isfinite(opt.firefly_floor) && opt.firefly_floor >= 0.f)) { std::cerr << "--firefly-floor " << opt.firefly_floor << " must be finite and >= 0\n"; return EXIT_FAILURE; }
        }
        else if (a == "--motion-scale") {
            if (sscanf(next(), "%f,%f", &opt.motion_sx, &opt.motion_sy) != 2) { std::cerr << "--motion-scale needs sx,sy\n"; usage(); return EXIT_FAILURE; }
        }
        else if (a == "--search") { if (!pair_arg(next(), opt.search_lo, opt.search_hi)) { usage(); return EXIT_FAILURE; } }
        else if (a == "--patch") { if (!pair_arg(next(), opt.patch_lo, opt.patch_hi)) { usage(); return EXIT_FAILURE; } }
        else if (a == "--temporal-k") opt.temporal_k = atoi(next());
        else if (a == "--animation") opt.animation = true;
        else if (a == "--animation-filter") {
            filter_given = true;
            opt.animation_filter = next();
            if (!animation_filter(opt.animation_filter)) {
                std::string names;
                for (const AnimationFilter &f : kAnimationFilters) names += std::string(names.empty() ? "" : ", ") + f.name;
                std::cerr << "unknown --animation-filter " << opt.animation_filter << " (" << names << ")\n"; usage(); return EXIT_FAILURE; }
        }
        else if (a == "--half") opt.half = true;
        else if (a == "--gpus") { opt.gpus = atoi(next()); gpus_given = true; }
        else if (a == "--share-device") opt.share_device = true;
        else if (a == "--pinned-mb") opt.pinned_mb = atol(next());
        else if (a == "--io-threads") opt.io_threads = atoi(next());
        else if (a == "--pageable-host") opt.pageable_host = true;
        else if (a == "--halo") { const std::string v = next(); if (v == "rccl") opt.halo_rccl = true; else if (v != "host") { usage(); return EXIT_FAILURE; } }
        else if (a == "--cpu-radius") opt.cpu_radius = atoi(next());
        else if (a == "--cpu-sigma-s") opt.cpu_sigma_s = (float)atof(next());
        else if (a == "--cpu-sigma-c") opt.cpu_sigma_c = (float)atof(next());
        else if (a == "--cpu-fix-blue") opt.cpu_blue_bug = false;
        else if (a == "--cpu-threads") {
            opt.cpu_threads.clear();
            std::string s = next();
            size_t pos = 0;
            while (pos < s.size()) { size_t c = s.find(',', pos); if (c == std::string::npos) c = s.size(); opt.cpu_threads.push_back(atoi(s.substr(pos, c - pos).c_str())); pos = c + 1; }
        } else if (!a.empty() && a[0] == '-') { std::cerr << "unknown option " << a << "\n"; usage(); return EXIT_FAILURE; }
        else if (!have_image) { opt.image = a; have_image = true; }
        else { usage(); return EXIT_FAILURE; }
    }
    auto listed = [&](const char *m) { return ("," + opt.modes + ",").find(std::string(",") + m + ",") != std::string::npos; };
    auto want = [&](const char *m) { return opt.modes == "all" || listed(m); };
    if ((!opt.albedo_layer.empty() || opt.albedo_floor_given) && !(opt.animation && opt.animation_filter == "atrous-recursive")) {
        std::cerr << (!opt.albedo_layer.empty() ? "--albedo-layer" : "--albedo-floor") << " applies to --animation --animation-filter atrous-recursive only\n";
        return EXIT_FAILURE;
    }
    if (opt.albedo_floor_given && opt.albedo_layer.empty()) { std::cerr << "--albedo-floor needs --albedo-layer\n"; return EXIT_FAILURE; }
    if ((opt.firefly_rank || opt.firefly_other) && !(opt.animation && opt.animation_filter == "atrous-recursive")) {
        std::cerr << (opt.firefly_rank ? "--firefly-rank" : opt.firefly_other) << " applies to --animation --animation-filter atrous-recursive only\n";
        return EXIT_FAILURE;
    }
    if (opt.firefly_other && !opt.firefly_rank) { std::cerr << opt.firefly_other << " needs --firefly-rank\n"; return EXIT_FAILURE; }
    if ((opt.history_clip || opt.history_clip_radius_given) && !(opt.animation && opt.animation_filter == "atrous-recursive")) {
        std::cerr << (opt.history_clip ? "--history-clip" : "--history-clip-radius") << " applies to --animation --animation-filter atrous-recursive only\n";
        return EXIT_FAILURE;
    }
    if (opt.history_clip_radius_given && !opt.history_clip) { std::cerr << "--history-clip-radius needs --history-clip\n"; return EXIT_FAILURE; }
    if (opt.guided_other && !(opt.animation ? opt.animation_filter == "guided" : listed("guided"))) {
        std::cerr << opt.guided_other << " applies to --modes guided and --animation --animation-filter guided only\n";
        return EXIT_FAILURE;
    }
    if (opt.median_other && !(opt.animation ? opt.animation_filter == "median" : listed("median"))) {
        std::cerr << opt.median_other << " applies to --modes median and --animation --animation-filter median only\n";
        return EXIT_FAILURE;
    }
    if (opt.compare_other && !opt.compare) { std::cerr << opt.compare_other << " applies to --compare only\n"; return EXIT_FAILURE; }
    if (opt.compare) {
        const char *with = modes_given ? "--modes" : filter_given ? "--animation-filter" : gpus_given ? "--gpus" : nullptr;
        if (with) { std::cerr << "--compare runs no filter: it cannot be combined with " << with << "\n"; return EXIT_FAILURE; }
        if (have_image) { std::cerr << "--compare takes its two files itself: the positional image " << opt.image << " has no meaning with it\n"; return EXIT_FAILURE; }
        try { run_compare(opt); }
        catch (const std::exception &e) { std::cout.flush(); std::cerr << e.what() << "\n"; return EXIT_FAILURE; }   // stdout holds `metrics` lines only
        return EXIT_SUCCESS;
    }
    if (listed("atrous-recursive")) {
        std::cerr << "--modes atrous-recursive: the recursion needs a sequence; it is an animation filter (--animation --animation-filter atrous-recursive)\n";
        return EXIT_FAILURE;
    }

    try {
        DenoiseApplication app{opt};
        auto print_time = [&] {                                                   // PRINT_TIME, src/main.cpp:1924-1927
            std::cout << FOREGROUND_COLOR << BACKGROUND_COLOR << "transfer time: " << (unsigned long long)(app.GetTransferMs() * 1e6) << "ns; "
                      << "execution time: " << (unsigned long long)(app.GetExecMs() * 1e6) << "ns\n\n" << CLEAR_COLOR;
        };
        if (!opt.animation && opt.animation_filter != "nlm") { std::cerr << "--animation-filter needs --animation\n"; return EXIT_FAILURE; }
        if (opt.animation) {
            std::cout << "######\nRunning on GPU (animation, " << animation_filter(opt.animation_filter)->banner << ")\n######\n";
            // (a failed animation run names its filter on stderr; the message itself goes where every mode's goes, below)
            try { app.RunAnimation(); }
            catch (const std::exception &) { std::cout.flush(); std::cerr << "--animation --animation-filter " << opt.animation_filter << " failed:\n"; throw; }
            print_time();
            return EXIT_SUCCESS;
        }
        if (opt.run_gpu) {
            if (want("bilateral")) { std::cout << "######\nRunning on GPU (nonlinear bialteral)\n######\n"; app.RunOnGPU(false, true, false, false, false); print_time(); }
            if (want("layers")) { std::cout << "######\nRunning on GPU (nonlinear bialteral + layers)\n######\n"; app.RunOnGPU(false, true, false, false, true); print_time(); }
            if (want("linear")) { std::cout << "######\nRunning on GPU (linear bialteral)\n######\n"; app.RunOnGPU(false, false, false, false, false); print_time(); }
            if (want("nlm")) { std::cout << "######\nRunning on GPU (nonlocal)\n######\n"; app.RunOnGPU(true, true, false, false, false); print_time(); }
            if (want("multiframe")) { std::cout << "######\nRunning on GPU (multiframe nonlocal)\n######\n"; app.RunOnGPU(true, true, true, false, false); print_time(); }
            if (want("overlap")) { std::cout << "######\nRunning on GPU (multiframe nonlocal + overlapping)\n######\n"; app.RunOnGPU(true, true, true, true, false); print_time(); }
            // (not part of `all`: the reference has no NLM with layers, and the default run writes exactly the reference's files)
            if (listed("nlm-layers")) { std::cout << "######\nRunning on GPU (nonlocal + layers)\n######\n"; app.RunOnGPU(true, true, false, false, true); print_time(); }
            if (listed("joint")) { std::cout << "######\nRunning on GPU (joint bialteral)\n######\n"; app.RunOnGPU(false, true, false, false, true, true); print_time(); }
            if (listed("nlm-joint")) { std::cout << "######\nRunning on GPU (joint nonlocal)\n######\n"; app.RunOnGPU(true, true, false, false, true, true); print_time(); }
            if (listed("atrous")) { std::cout << "######\nRunning on GPU (a-trous + layers)\n######\n"; app.RunOnGPU(false, true, false, false, true, true, 1); print_time(); }
            if (listed("guided")) { std::cout << "######\nRunning on GPU (guided filter)\n######\n"; app.RunGuided(); print_time(); }
            if (listed("median")) { std::cout << "######\nRunning on GPU (median)\n######\n"; app.RunMedian(); print_time(); }
            if (listed("atrous-variance")) { std::cout << "######\nRunning on GPU (a-trous + layers, variance-guided)\n######\n"; app.RunOnGPU(false, true, false, false, true, true, 2); print_time(); }
        }
        if (opt.run_cpu) {
            for (int threads : opt.cpu_threads) {
                const auto t0 = std::chrono::steady_clock::now();
                std::cout << "######\nRunning on CPU (" << threads << (threads == 1 ? " thread" : " threads") << " bialteral)\n######\n";
                app.RunOnCPU(opt.image, threads);
                const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                std::cout << FOREGROUND_COLOR << BACKGROUND_COLOR << "Time taken: " << sec << " sec\n\n" << CLEAR_COLOR;   // PRINT_TIME2 :1929-1933
            }
        }
    } catch (const std::exception &e) {                                         // src/main.cpp:1987-1991
        printf("%s\n", e.what());
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}
