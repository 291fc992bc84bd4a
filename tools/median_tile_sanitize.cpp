// median_tile_sanitize.cpp -- the tile-fill geometry of the median filters (csrc/median_tile.hpp, section a4p) on the CPU, under
// AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone host program, built and run by tests/test_median_tile_sanitize.py
// before any GPU test feeds the kernel.
//
// Over images from 1 x 1 to one past every seam (1..8 x 1..8 and 62..66 / 126..130 x 14..18 / 30..34), radius 1, 2, 3, every tile:
//   * every fill slot f is written once into an LDS tile of exactly median_tile_slots(R) places (the write is made: ASan watches it),
//     by the thread f % 256 in its trip f / 256, and the tile's size is what median_lds_bytes accounts for at every layer count;
//   * every slot flagged inside indexes a table of exactly width * height texels (the read is made);
//   * every in-image texel of the tile's footprint (the tile's pixels grown by the radius) is read exactly once, nothing else;
//   * a lane's window reads (rows 4 wave + j .. + 2 R, columns lane .. lane + 2 R) stay inside the tile, and the centre's slot holds
//     the pixel the lane owns; every pixel of the image is owned by exactly one lane of one tile.
// Then the flat indices of the corner tiles of 16400 x 16400, 262149 x 1 and 1 x 70000 against size_t expectations, nothing allocated.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../image_denoising_filter_amd/csrc/median_tile.hpp"

using namespace mid;

static long wrong = 0, slots = 0;

#define EXPECT(cond, ...) do { if (!(cond)) { if (wrong++ < 20) { std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static void sweep(int width, int height, int R)
{
    std::vector<unsigned char> table((size_t)width * height, 1);     // exactly width * height texels, no slack
    std::vector<int> owned((size_t)width * height, 0);
    const int tx_n = median_tiles_x(width), ty_n = median_tiles_y(height), n_fill = median_tile_slots(R);
    const int tw = kMedianTileW + 2 * R, th = kMedianTileH + 2 * R;
    EXPECT(n_fill == tw * th, "%dx%d R %d: %d fill slots for a %dx%d tile", width, height, R, n_fill, tw, th);
    for (int L = 0; L <= kMedianTiledLayers; ++L)
        EXPECT(median_lds_bytes(R, L) == sizeof(float) * ((size_t)n_fill * (3 + 3 * L) + 1) && median_lds_bytes(R, L) <= 160 * 1024,
               "R %d L %d: %zu bytes of LDS", R, L, median_lds_bytes(R, L));
    for (int ty = 0; ty < ty_n; ++ty)
        for (int tx = 0; tx < tx_n; ++tx) {
            std::vector<int> tile((size_t)n_fill, 0), read((size_t)width * height, 0);      // the tile: exactly n_fill places, no slack
            std::vector<int> tex_x((size_t)n_fill, -1), tex_y((size_t)n_fill, -1);
            for (int tid = 0; tid < 256; ++tid)
                for (int f = tid; f < n_fill; f += 256, ++slots) {                            // the kernel's fill loop
                    const MedianSlot s = median_fill_slot(R, tx, ty, f, width, height);
                    tile.data()[f]++;                                                         // the store itself: past the tile is ASan's to report
                    const int sx = f % tw, sy = f / tw;
                    EXPECT(s.x == tx * kMedianTileW + sx - R && s.y == ty * kMedianTileH + sy - R, "%dx%d R %d tile %d,%d slot %d: texel %d,%d", width, height,
                           R, tx, ty, f, s.x, s.y);
                    const bool in = s.x >= 0 && s.x < width && s.y >= 0 && s.y < height;
                    EXPECT(s.inside == in, "%dx%d R %d tile %d,%d slot %d: inside %d for %d,%d", width, height, R, tx, ty, f, (int)s.inside, s.x, s.y);
                    if (s.inside) {
                        const size_t at = median_flat(s.x, s.y, width);
                        wrong += table.data()[at] != 1;                                       // the read itself
                        read[at]++;
                        tex_x[f] = s.x; tex_y[f] = s.y;
                    }
                }
            for (int i = 0; i < n_fill; ++i) EXPECT(tile[i] == 1, "%dx%d R %d tile %d,%d: slot %d written %d times", width, height, R, tx, ty, i, tile[i]);
            for (int y = 0; y < height; ++y)
                for (int x = 0; x < width; ++x) {
                    const bool foot = x >= tx * kMedianTileW - R && x < (tx + 1) * kMedianTileW + R && y >= ty * kMedianTileH - R && y < (ty + 1) * kMedianTileH + R;
                    EXPECT(read[(size_t)y * width + x] == (foot ? 1 : 0), "%dx%d R %d tile %d,%d: texel %d,%d read %d times", width, height, R, tx, ty, x, y,
                           read[(size_t)y * width + x]);
                }
            // the tap loop: thread (wave, lane), pixel j of the lane
            for (int wave = 0; wave < 4; ++wave)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j) {
                        const int row = 4 * wave + j, x = tx * kMedianTileW + lane, y = ty * kMedianTileH + row;
                        if (x >= width || y >= height) continue;
                        const int base = row * tw + lane;
                        for (int k = 0; k < (2 * R + 1) * (2 * R + 1); ++k) {
                            const int at = base + (k / (2 * R + 1)) * tw + k % (2 * R + 1);
                            wrong += tile.data()[at] != 1;                                    // the read itself
                        }
                        const int c = base + R * tw + R;
                        EXPECT(tex_x[c] == x && tex_y[c] == y, "%dx%d R %d tile %d,%d: the centre slot of pixel %d,%d holds %d,%d", width, height, R, tx, ty, x,
                               y, tex_x[c], tex_y[c]);
                        owned[median_flat(x, y, width)]++;
                    }
        }
    for (size_t i = 0; i < owned.size(); ++i) EXPECT(owned[i] == 1, "%dx%d R %d: pixel %zu owned %d times", width, height, R, i, owned[i]);
}

// The corner tiles of a frame that is never allocated: the flat index of the first and the last in-image slot of each.
static void corners(int width, int height, int R)
{
    const int tx_n = median_tiles_x(width), ty_n = median_tiles_y(height);
    const size_t npix = (size_t)width * (size_t)height;
    for (int ty : {0, ty_n - 1})
        for (int tx : {0, tx_n - 1}) {
            size_t lo = npix, hi = 0, n_in = 0;
            for (int f = 0; f < median_tile_slots(R); ++f, ++slots) {
                const MedianSlot s = median_fill_slot(R, tx, ty, f, width, height);
                if (!s.inside) continue;
                const size_t at = median_flat(s.x, s.y, width);
                EXPECT(at < npix, "%dx%d R %d tile %d,%d slot %d: flat index %zu of %zu", width, height, R, tx, ty, f, at, npix);
                lo = at < lo ? at : lo; hi = at > hi ? at : hi; ++n_in;
            }
            const long x0 = (long)tx * kMedianTileW - R < 0 ? 0 : (long)tx * kMedianTileW - R, y0 = (long)ty * kMedianTileH - R < 0 ? 0 : (long)ty * kMedianTileH - R;
            const long x1 = (long)(tx + 1) * kMedianTileW + R > width ? width : (long)(tx + 1) * kMedianTileW + R;
            const long y1 = (long)(ty + 1) * kMedianTileH + R > height ? height : (long)(ty + 1) * kMedianTileH + R;
            EXPECT(lo == (size_t)y0 * (size_t)width + (size_t)x0, "%dx%d R %d tile %d,%d: first index %zu", width, height, R, tx, ty, lo);
            EXPECT(hi == (size_t)(y1 - 1) * (size_t)width + (size_t)(x1 - 1), "%dx%d R %d tile %d,%d: last index %zu", width, height, R, tx, ty, hi);
            EXPECT(n_in == (size_t)(x1 - x0) * (size_t)(y1 - y0), "%dx%d R %d tile %d,%d: %zu texels inside", width, height, R, tx, ty, n_in);
        }
}

int main()
{
    for (int R = 1; R <= kMedianMaxRadius; ++R) {
        for (int h = 1; h <= 8; ++h) for (int w = 1; w <= 8; ++w) sweep(w, h, R);
        for (int h : {14, 15, 16, 17, 18, 30, 31, 32, 33, 34}) for (int w : {62, 63, 64, 65, 66, 126, 127, 128, 129, 130}) sweep(w, h, R);
        corners(16400, 16400, R);
        corners(262149, 1, R);
        corners(1, 70000, R);
    }
    // 16400 x 16400: the last pixel lies past 2^28 texels, its RGBA32F byte offset past 4 GiB
    EXPECT(median_flat(16399, 16399, 16400) == (size_t)268959999, "the last texel of 16400 x 16400");
    EXPECT(median_flat(16399, 16399, 16400) * 16 > ((size_t)1 << 32), "its byte offset");
    EXPECT(median_tiles_x(262149) == 4097 && median_tiles_y(1) == 1 && median_tiles_x(16400) == 257 && median_tiles_y(16400) == 1025 && median_tiles_y(70000) == 4375,
           "tile counts");
    std::printf("slots %ld, %ld wrong\n", slots, wrong);
    return wrong ? EXIT_FAILURE : EXIT_SUCCESS;
}
