// guided_box_sanitize.cpp -- the geometry of the guided filter's sliding box sums (csrc/guided_box.hpp, section a4o) walked on the
// host exactly as csrc/guided.hip walks it, for AddressSanitizer and UndefinedBehaviorSanitizer:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/guided_box_sanitize.cpp -o guided_box_sanitize
// (tests/test_guided_box_sanitize.py builds and runs it; nothing here touches a GPU or is loaded into Python.)
// Every image is a heap array of exactly width * height bytes and the prefix slots an array of exactly kGuidedLanes, so an index
// outside either is a sanitizer report; beyond that the walk checks, per size and radius:
//   every pixel is output by exactly one (tile, lane, row);
//   every LDS slot an output lane reads was filled in the same round;
//   every global index is inside width * height;
//   the rows inside a lane's running sum at an output row are exactly the in-image rows of its window, and the first output row of
//   a segment follows exactly 2 radius + 1 walked rows.
// The corner tiles of 16400 x 16400, 262149 x 1 and 1 x 70000 are walked without the arrays: their flat indices in size_t against
// 128-bit arithmetic.  Prints "guided_box: <checks> checks, <wrong> wrong"; exit status 1 when anything is wrong.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../image_denoising_filter_amd/csrc/guided_box.hpp"

using namespace mid;

static long long checks = 0, wrong = 0;
static void expect(bool ok, const char *what, int w, int h, int r)
{
    ++checks;
    if (!ok && ++wrong <= 20) std::printf("WRONG %s at %dx%d radius %d\n", what, w, h, r);
}

// One tile.  img / owners: width * height entries, or nullptr for the sizes too large to allocate.
static void walk_tile(int w, int h, int r, int strip, int seg, const unsigned char *img, std::vector<int> *owners)
{
    std::vector<long long> filled(kGuidedLanes, -1);            // the round that last wrote a prefix slot
    std::vector<int> n_rows(kGuidedLanes, 0);                   // rows inside each lane's running sum
    std::vector<long long> row_sum(kGuidedLanes, 0);            // and the sum of their indices
    long long round = 0;
    int walked = 0;
    bool first_out = true;
    const int y_end = guided_row_end(seg, r, h);
    for (int yy = guided_row_begin(seg, r); yy < y_end; ++yy) {
        ++walked;
        for (int t = 0; t < kGuidedLanes; ++t) {
            const int cx = guided_col(strip, r, t);
            const bool col_in = cx >= 0 && cx < w;
            if (col_in && yy >= 0 && yy < h) {
                const size_t at = guided_flat(cx, yy, w);
                expect(at < (size_t)w * (size_t)h, "entering index", w, h, r);
                expect((unsigned __int128)at == (unsigned __int128)yy * (unsigned __int128)w + (unsigned __int128)cx, "entering index value", w, h, r);
                if (img) (void)*(volatile const unsigned char *)(img + at);
                ++n_rows[t]; row_sum[t] += yy;
            }
            const int yl = guided_row_leaving(yy, r);
            if (col_in && guided_row_left(yy, seg, r) && yl >= 0 && yl < h) {
                const size_t at = guided_flat(cx, yl, w);
                expect(at < (size_t)w * (size_t)h, "leaving index", w, h, r);
                if (img) (void)*(volatile const unsigned char *)(img + at);
                --n_rows[t]; row_sum[t] -= yl;
            }
        }
        if (!guided_row_is_out(yy, seg, r)) continue;
        if (first_out) { expect(walked == 2 * r + 1, "warm-up rows", w, h, r); first_out = false; }
        ++round;
        for (int t = 0; t < kGuidedLanes; ++t) filled.at((size_t)t) = round;      // every lane stores its slot
        const int yo = guided_row_out(yy, r);
        expect(yo >= guided_seg_y0(seg) && yo < guided_seg_y1(seg, h), "output row", w, h, r);
        const int lo_row = yo - r < 0 ? 0 : yo - r, hi_row = yo + r > h - 1 ? h - 1 : yo + r;
        for (int t = 0; t < kGuidedLanes; ++t) {
            const int cx = guided_col(strip, r, t);
            if (cx >= 0 && cx < w) {
                expect(n_rows[t] == hi_row - lo_row + 1, "rows in the running sum", w, h, r);
                expect(row_sum[t] == (long long)(lo_row + hi_row) * (hi_row - lo_row + 1) / 2, "which rows are in the running sum", w, h, r);
            }
            if (!(guided_out_lane(r, t) && cx < w)) continue;
            expect(cx >= 0, "output column", w, h, r);
            const int hi = guided_slot_hi(t, r), lo = guided_slot_lo(t, r);
            expect(hi >= 0 && hi < kGuidedLanes && lo >= -1 && lo < kGuidedLanes, "slot range", w, h, r);
            expect(filled.at((size_t)hi) == round && (lo < 0 || filled.at((size_t)lo) == round), "slot filled in this round", w, h, r);
            // the slots lo + 1 .. hi are the window's columns cx - r .. cx + r
            expect(guided_col(strip, r, lo + 1) == cx - r && guided_col(strip, r, hi) == cx + r, "window columns", w, h, r);
            const size_t at = guided_flat(cx, yo, w);
            expect(at < (size_t)w * (size_t)h, "output index", w, h, r);
            expect((unsigned __int128)at == (unsigned __int128)yo * (unsigned __int128)w + (unsigned __int128)cx, "output index value", w, h, r);
            if (owners) ++(*owners)[at];
        }
    }
    expect(!first_out, "a tile with no output row", w, h, r);
}

static void walk_image(int w, int h, int r)
{
    std::vector<unsigned char> img((size_t)w * h, 1);
    std::vector<int> owners((size_t)w * h, 0);
    const int strips = guided_strips(w, r), segs = guided_segments(h);
    expect(guided_tiles(w, h, r) == (unsigned)strips * (unsigned)segs, "tile count", w, h, r);
    for (int seg = 0; seg < segs; ++seg)
        for (int strip = 0; strip < strips; ++strip) walk_tile(w, h, r, strip, seg, img.data(), &owners);
    bool one = true;
    for (int o : owners) one = one && o == 1;
    expect(one, "exactly one owner per pixel", w, h, r);
}

int main()
{
    const int radii[] = {1, 2, kGuidedMaxRadius};
    for (int r : radii) {
        for (int h = 1; h <= 12; ++h)
            for (int w = 1; w <= 12; ++w) walk_image(w, h, r);
        const int sw = guided_strip_w(r);
        const int widths[] = {63, 64, 65, sw - 1, sw, sw + 1, kGuidedLanes - 1, kGuidedLanes, kGuidedLanes + 1, 2 * sw, 2 * sw + 1};
        const int heights[] = {kGuidedPeriod - 1, kGuidedPeriod, kGuidedPeriod + 1, 2 * kGuidedPeriod, 2 * kGuidedPeriod + 1};
        for (int h : heights)
            for (int w : widths) walk_image(w, h, r);
        const int big[][2] = {{16400, 16400}, {262149, 1}, {1, 70000}};
        for (const auto &s : big) {
            const int w = s[0], h = s[1], strips = guided_strips(w, r), segs = guided_segments(h);
            for (int seg : {0, segs - 1})
                for (int strip : {0, strips - 1}) walk_tile(w, h, r, strip, seg, nullptr, nullptr);
        }
    }
    std::printf("guided_box: %lld checks, %lld wrong\n", checks, wrong);
    return wrong ? 1 : 0;
}
