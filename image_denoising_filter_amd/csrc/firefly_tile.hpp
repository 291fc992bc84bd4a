// firefly_tile.hpp -- the tile-fill geometry of the firefly clamp (include/mi_denoise.h, section a4l): which image texel a fill slot of
// a workgroup's luminance tile reads, where in the tile it lands, and whether that texel is inside the image.
// Host and device: firefly.hip's kernel calls it for every slot it fills, and tools/firefly_tile_sanitize.cpp sweeps it on the CPU
// under AddressSanitizer and UndefinedBehaviorSanitizer (it includes nothing of HIP when a plain C++ compiler reads it).
//
//   A tile covers kFireflyTileW x kFireflyTileH = 64 x 16 pixels; tile t of the frame is (t % tiles_x, t / tiles_x).  Its luminance
//   tile has (64 + 2 R) x (16 + 2 R) slots, slot (sx, sy) holding image texel (64 tile_x + sx - R, 16 tile_y + sy - R).
//   Fill slots f = 0 .. 1023 are the tile's own pixels: f = 64 row + lane, read by thread 64 (row / 4) + lane as its pixel row % 4 --
//   a lane owns four pixels of one column.  Fill slots 1024 .. are the halo: R rows above, R rows below (each 64 + 2 R wide), then
//   the 16 rows' R texels on the left, then those on the right; thread tid fills the halo slots 1024 + tid, 1024 + tid + 256, ...
//   A slot whose texel lies outside the image is not read: the kernel stores NaN there.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define MID_FIREFLY_HD __host__ __device__ __forceinline__
#else
#define MID_FIREFLY_HD inline
#endif

namespace mid {

constexpr int kFireflyTileW = 64, kFireflyTileH = 16, kFireflyOwn = kFireflyTileW * kFireflyTileH;

struct FireflySlot {
    int lds;                // index into the (64 + 2 R) x (16 + 2 R) luminance tile, row-major
    int x, y;               // the image texel; meaningful only where inside
    bool inside;
};

MID_FIREFLY_HD int firefly_tiles_x(int width) { return (width + kFireflyTileW - 1) / kFireflyTileW; }
MID_FIREFLY_HD int firefly_tiles_y(int height) { return (height + kFireflyTileH - 1) / kFireflyTileH; }
MID_FIREFLY_HD int firefly_fill_slots(int R) { return (kFireflyTileW + 2 * R) * (kFireflyTileH + 2 * R); }
MID_FIREFLY_HD size_t firefly_flat(int x, int y, int width) { return (size_t)y * (size_t)width + (size_t)x; }

// Fill slot f in [0, firefly_fill_slots(R)) of tile (tile_x, tile_y).
MID_FIREFLY_HD FireflySlot firefly_fill_slot(int R, int tile_x, int tile_y, int f, int width, int height)
{
    const int tw = kFireflyTileW + 2 * R;
    int sx, sy;
    if (f < kFireflyOwn) {                              // the tile's own pixels
        sx = R + f % kFireflyTileW; sy = R + f / kFireflyTileW;
    } else {
        int k = f - kFireflyOwn;
        if (k < R * tw) { sx = k % tw; sy = k / tw; }                                                   // above
        else if ((k -= R * tw) < R * tw) { sx = k % tw; sy = R + kFireflyTileH + k / tw; }               // below
        else if ((k -= R * tw) < R * kFireflyTileH) { sx = k % R; sy = R + k / R; }                      // left
        else { k -= R * kFireflyTileH; sx = R + kFireflyTileW + k % R; sy = R + k / R; }                 // right
    }
    FireflySlot s;
    s.lds = sy * tw + sx;
    s.x = tile_x * kFireflyTileW + sx - R;              // width * height < 2^30: no int overflows
    s.y = tile_y * kFireflyTileH + sy - R;
    s.inside = s.x >= 0 && s.x < width && s.y >= 0 && s.y < height;
    return s;
}

}  // namespace mid
