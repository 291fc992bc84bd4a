// metrics_tile_sanitize.cpp -- the tile-fill geometry of the image metrics (csrc/firefly_tile.hpp at R = 5, section a4n) on the CPU,
// under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone host program, built and run by
// tests/test_metrics_tile_sanitize.py before any GPU test feeds the kernel.
//
// Over images of 1..12 x 1..12 and of 59..70 x 11..22 (every seam of the 64 x 16 tile and of its 5-texel halo), every tile of the grid:
//   * every one of the 74 x 26 places of the luminance tile is filled exactly once;
//   * every slot flagged inside indexes a table of exactly width * height texels (the read is made: ASan watches it);
//   * every in-image texel of the tile's footprint (the tile's pixels grown by 5) is read exactly once, nothing else;
//   * every pixel of the image is owned by exactly one lane of one tile, and the 4 + 10 rows of eleven taps a lane reads stay
//     inside the tile.
// Then the flat indices of the corner tiles of 16400 x 16400, 262149 x 1 and 1 x 70000 against size_t expectations, nothing allocated.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../image_denoising_filter_amd/csrc/firefly_tile.hpp"

using namespace mid;

static long wrong = 0, slots = 0;
static const int R = 5;

#define EXPECT(cond, ...) do { if (!(cond)) { if (wrong++ < 20) { std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static void sweep(int width, int height)
{
    std::vector<unsigned char> table((size_t)width * height, 1);     // exactly width * height texels, no slack
    std::vector<int> owned((size_t)width * height, 0);
    const int tx_n = firefly_tiles_x(width), ty_n = firefly_tiles_y(height), n_fill = firefly_fill_slots(R);
    const int tw = kFireflyTileW + 2 * R, th = kFireflyTileH + 2 * R;
    EXPECT(tw == 74 && th == 26 && n_fill == tw * th, "%dx%d: %d fill slots for a %dx%d tile", width, height, n_fill, tw, th);
    for (int ty = 0; ty < ty_n; ++ty)
        for (int tx = 0; tx < tx_n; ++tx) {
            std::vector<int> placed((size_t)tw * th, 0), read((size_t)width * height, 0);
            for (int f = 0; f < n_fill; ++f, ++slots) {
                const FireflySlot s = firefly_fill_slot(R, tx, ty, f, width, height);
                EXPECT(s.lds >= 0 && s.lds < tw * th, "%dx%d tile %d,%d slot %d: lds %d", width, height, tx, ty, f, s.lds);
                if (s.lds >= 0 && s.lds < tw * th) placed[s.lds]++;
                const int sx = s.lds % tw, sy = s.lds / tw;
                EXPECT(s.x == tx * kFireflyTileW + sx - R && s.y == ty * kFireflyTileH + sy - R, "%dx%d tile %d,%d slot %d: texel %d,%d at %d,%d", width,
                       height, tx, ty, f, s.x, s.y, sx, sy);
                const bool in = s.x >= 0 && s.x < width && s.y >= 0 && s.y < height;
                EXPECT(s.inside == in, "%dx%d tile %d,%d slot %d: inside %d for %d,%d", width, height, tx, ty, f, (int)s.inside, s.x, s.y);
                if (s.inside) {
                    const size_t at = firefly_flat(s.x, s.y, width);
                    wrong += table.data()[at] != 1;              // the read itself: past the table is ASan's to report
                    read[at]++;
                }
                if (f < kFireflyOwn) {                           // an own pixel: slot (R + lane, R + row), lane f % 64, row f / 64
                    EXPECT(sx == R + f % kFireflyTileW && sy == R + f / kFireflyTileW, "%dx%d slot %d is not own pixel %d,%d", width, height, f, sx, sy);
                    if (s.inside) owned[firefly_flat(s.x, s.y, width)]++;
                }
            }
            for (int i = 0; i < tw * th; ++i) EXPECT(placed[i] == 1, "%dx%d tile %d,%d: tile place %d filled %d times", width, height, tx, ty, i, placed[i]);
            for (int y = 0; y < height; ++y)
                for (int x = 0; x < width; ++x) {
                    const bool foot = x >= tx * kFireflyTileW - R && x < (tx + 1) * kFireflyTileW + R && y >= ty * kFireflyTileH - R && y < (ty + 1) * kFireflyTileH + R;
                    EXPECT(read[(size_t)y * width + x] == (foot ? 1 : 0), "%dx%d tile %d,%d: texel %d,%d read %d times", width, height, tx, ty, x, y,
                           read[(size_t)y * width + x]);
                }
        }
    for (size_t i = 0; i < owned.size(); ++i) EXPECT(owned[i] == 1, "%dx%d: pixel %zu owned %d times", width, height, i, owned[i]);
}

// What a lane of the kernel reads of the tile: rows 4 wave .. 4 wave + 13, columns lane .. lane + 10, through a tile of exactly 74 x 26.
static void tap_reads()
{
    const int tw = kFireflyTileW + 2 * R, th = kFireflyTileH + 2 * R;
    std::vector<float> tile((size_t)tw * th, 1.f);
    for (int wave = 0; wave < 4; ++wave)
        for (int lane = 0; lane < 64; ++lane) {
            const int base = (4 * wave) * tw + lane;
            for (int r = 0; r < 4 + 2 * R; ++r)
                for (int i = 0; i <= 2 * R; ++i, ++slots) wrong += tile.data()[base + r * tw + i] != 1.f;
            for (int j = 0; j < 4; ++j) {                        // pixel j's centre: the own slot of (lane, 4 wave + j)
                const FireflySlot s = firefly_fill_slot(R, 0, 0, kFireflyTileW * (4 * wave + j) + lane, 1 << 20, 1 << 10);
                EXPECT(s.lds == base + (j + R) * tw + R, "wave %d lane %d pixel %d: centre at %d, own slot at %d", wave, lane, j, base + (j + R) * tw + R, s.lds);
            }
        }
}

// The corner tiles of a frame that is never allocated: the flat index of the first and the last in-image slot of each.
static void corners(int width, int height)
{
    const int tx_n = firefly_tiles_x(width), ty_n = firefly_tiles_y(height);
    const size_t npix = (size_t)width * (size_t)height;
    for (int ty : {0, ty_n - 1})
        for (int tx : {0, tx_n - 1}) {
            size_t lo = npix, hi = 0, n_in = 0;
            for (int f = 0; f < firefly_fill_slots(R); ++f, ++slots) {
                const FireflySlot s = firefly_fill_slot(R, tx, ty, f, width, height);
                if (!s.inside) continue;
                const size_t at = firefly_flat(s.x, s.y, width);
                EXPECT(at < npix, "%dx%d tile %d,%d slot %d: flat index %zu of %zu", width, height, tx, ty, f, at, npix);
                lo = at < lo ? at : lo; hi = at > hi ? at : hi; ++n_in;
            }
            const long x0 = (long)tx * kFireflyTileW - R < 0 ? 0 : (long)tx * kFireflyTileW - R, y0 = (long)ty * kFireflyTileH - R < 0 ? 0 : (long)ty * kFireflyTileH - R;
            const long x1 = (long)(tx + 1) * kFireflyTileW + R > width ? width : (long)(tx + 1) * kFireflyTileW + R;
            const long y1 = (long)(ty + 1) * kFireflyTileH + R > height ? height : (long)(ty + 1) * kFireflyTileH + R;
            EXPECT(lo == (size_t)y0 * (size_t)width + (size_t)x0, "%dx%d tile %d,%d: first index %zu", width, height, tx, ty, lo);
            EXPECT(hi == (size_t)(y1 - 1) * (size_t)width + (size_t)(x1 - 1), "%dx%d tile %d,%d: last index %zu", width, height, tx, ty, hi);
            EXPECT(n_in == (size_t)(x1 - x0) * (size_t)(y1 - y0), "%dx%d tile %d,%d: %zu texels inside", width, height, tx, ty, n_in);
        }
}

int main()
{
    for (int h = 1; h <= 12; ++h) for (int w = 1; w <= 12; ++w) sweep(w, h);
    for (int h = 11; h <= 22; ++h) for (int w = 59; w <= 70; ++w) sweep(w, h);
    tap_reads();
    corners(16400, 16400);
    corners(262149, 1);
    corners(1, 70000);
    EXPECT(firefly_flat(16399, 16399, 16400) * 16 > ((size_t)1 << 32), "the byte offset of the last texel of 16400 x 16400");
    EXPECT(firefly_tiles_x(262149) == 4097 && firefly_tiles_y(70000) == 4375 && firefly_tiles_x(16400) == 257 && firefly_tiles_y(16400) == 1025, "tile counts");
    std::printf("slots %ld, %ld wrong\n", slots, wrong);
    return wrong ? EXIT_FAILURE : EXIT_SUCCESS;
}
