// median_tile.hpp -- the tile-fill geometry of the median filters (include/mi_denoise.h, section a4p): which image texel a fill slot
// of a workgroup's LDS tile reads, whether that texel is inside the image, and how many bytes the tile of (radius, n_layers) takes.
// Host and device: median.hip's tiled kernel calls it for every slot it fills, and tools/median_tile_sanitize.cpp sweeps it on the
// CPU under AddressSanitizer and UndefinedBehaviorSanitizer (it includes nothing of HIP when a plain C++ compiler reads it).
//
//   A tile covers kMedianTileW x kMedianTileH = 64 x 16 pixels at every (radius, n_layers); tile t of the frame is (t % tiles_x,
//   t / tiles_x).  Its LDS tile has (64 + 2 R) x (16 + 2 R) slots, row-major; fill slot f IS the LDS slot: (f % tw, f / tw) holds
//   image texel (64 tile_x + f % tw - R, 16 tile_y + f / tw - R).  Thread tid fills the slots tid, tid + 256, ...  A slot whose
//   texel lies outside the image is not read: the kernel stores NaN there (colour) and 0 (guide planes).
//   Per slot the tile holds three floats of colour and three already-scaled floats per guide layer:
//       radius  n_layers  LDS tile  bytes
//       1       0 .. 4    66 x 18   14256, 28512, 42768, 57024, 71280
//       2       0 .. 4    68 x 20   16320, 32640, 48960, 65280, 81600
//       3       0 .. 4    70 x 22   18480, 36960, 55440, 73920, 92400
//   (plus one word for the plain class's vote), all inside the 160 KB of a CU, so the tile height is 16 in every row.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define MID_MEDIAN_HD __host__ __device__ __forceinline__
#else
#define MID_MEDIAN_HD inline
#endif

namespace mid {

constexpr int kMedianTileW = 64, kMedianTileH = 16, kMedianMaxRadius = 3, kMedianTiledLayers = 4;

struct MedianSlot {
    int x, y;               // the image texel; meaningful only where inside
    bool inside;
};

MID_MEDIAN_HD int median_tiles_x(int width) { return (width + kMedianTileW - 1) / kMedianTileW; }
MID_MEDIAN_HD int median_tiles_y(int height) { return (height + kMedianTileH - 1) / kMedianTileH; }
MID_MEDIAN_HD int median_tile_slots(int R) { return (kMedianTileW + 2 * R) * (kMedianTileH + 2 * R); }
MID_MEDIAN_HD size_t median_flat(int x, int y, int width) { return (size_t)y * (size_t)width + (size_t)x; }
// floats of one tile: three colour planes, three planes per layer, and the vote word
MID_MEDIAN_HD size_t median_lds_bytes(int R, int n_layers) { return sizeof(float) * ((size_t)median_tile_slots(R) * (3 + 3 * (size_t)n_layers) + 1); }

// Fill slot f in [0, median_tile_slots(R)) of tile (tile_x, tile_y).
MID_MEDIAN_HD MedianSlot median_fill_slot(int R, int tile_x, int tile_y, int f, int width, int height)
{
    const int tw = kMedianTileW + 2 * R;
    MedianSlot s;
    s.x = tile_x * kMedianTileW + f % tw - R;           // width * height < 2^30: no int overflows
    s.y = tile_y * kMedianTileH + f / tw - R;
    s.inside = s.x >= 0 && s.x < width && s.y >= 0 && s.y < height;
    return s;
}

}  // namespace mid
