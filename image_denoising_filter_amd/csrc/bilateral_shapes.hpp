// bilateral_shapes.hpp -- what the single-frame bilateral kernels (bilateral.hip) and the kernels over neighbouring frames
// (bilateral_temporal.hip) take from one place on the host side: the exponent scales and the table of tuned radii and tile
// shapes, from which both dispatchers and both LDS sizes derive.  The device code of the two files is NOT shared: see the note
// at the head of bilateral.hip.
#pragma once
#include "common.hpp"
#include <cmath>
#include <type_traits>

namespace mid {

// The exponent scales of both argument blocks (BilArgs, BilPairArgs): ks, kc in the log2 domain, sc = sqrt(-kc) and 1/sc.
template <typename Args>
inline void bil_fill_scales(const mid_bilateral_params *p, Args &a)
{
    a.w = p->width; a.h = p->height;
    a.ks = (float)(-0.5 * 1.4426950408889634 / ((double)p->spatialSigma * (double)p->spatialSigma));
    a.kc = (float)(-0.5 * 1.4426950408889634 / ((double)p->colorSigma * (double)p->colorSigma));
    a.sc = (float)(sqrt(0.5 * 1.4426950408889634) / (double)p->colorSigma);
    a.inv_sc = (float)(1.0 / (double)a.sc);
}

// Tile shapes by A/B on MI355X (tools/ab_bil.py): the kernel is latency-sensitive, so many independent waves (P = 2 rows per
// lane, 8 waves per workgroup) beat deeper register blocking.  A radius must run the same arithmetic in every form of the
// filter (the tuned kernels add the spatial term as si + ks*j^2, the run-time one as fma(ks, j^2, si)), so this is the one list.
template <int R_, int P_, int NW_> struct BilShape { static constexpr int R = R_, P = P_, NW = NW_; };
constexpr int kBilRtP = 2, kBilRtNW = 8;                 // the run-time-radius kernels: 8 waves x 2 rows per workgroup
constexpr size_t bil_lds_bytes(int radius, int tile_h, bool split)
{
    return (size_t)(64 + 2 * radius) * (tile_h + 2 * radius) * sizeof(float4) * (split ? 2 : 1);
}
// tuned(BilShape<...>{}) for a radius of the list, other() for every other one
template <typename Tuned, typename Other>
inline int bil_for_radius(int radius, Tuned &&tuned, Other &&other)
{
    switch (radius) {
    case 4:  return tuned(BilShape<4, 2, 8>{});      // BASELINE config 1 window
    case 8:  return tuned(BilShape<8, 2, 8>{});      // BASELINE configs[1] and [3] (layer modes: also best of six shapes, profiles/r05_ab_layer_tile_shapes.txt)
    case 10: return tuned(BilShape<10, 2, 16>{});    // CPU path window, src/main.cpp:1819
    case 20: return tuned(BilShape<20, 1, 8>{});     // TEXEL_WINDOW as shipped; 80 KB tile: two workgroups per CU (or image + guide tile)
    default: return other();
    }
}

}  // namespace mid
