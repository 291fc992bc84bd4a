// reproject_taps.hpp -- the tap geometry of the recursive temporal accumulation (include/mi_denoise.h, section a4j): where pixel p of
// this frame was in the previous one, which of the four bilinear taps around that position are taken, and with which weight.
// Host and device: temporal_accumulate.hip's kernel calls it per pixel, and tools/reproject_taps_sanitize.cpp sweeps it on the CPU
// under AddressSanitizer and UndefinedBehaviorSanitizer (it includes nothing of HIP when a plain C++ compiler reads it).
//
//   ppx = (float)x + mx (one fp32 add), x0 = floorf(ppx), fx = ppx - x0 (exact); likewise y
//   taps only if ppx > -1 && ppx < width && ppy > -1 && ppy < height, compared in fp32 BEFORE any float -> int conversion: false
//   for NaN and +-Inf, and then x0 in [-1, width - 1] and y0 in [-1, height - 1] convert without overflow
//   slot 2 b + a is q = (x0 + a, y0 + b) with bw = (a ? fx : 1 - fx) * (b ? fy : 1 - fy); a slot whose q lies outside the image or
//   whose bw == 0 is NOT taken: it is never read
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MID_TAPS_HD __host__ __device__ __forceinline__
#else
#define MID_TAPS_HD inline
#endif

namespace mid {

struct ReprojectTaps {
    int x0, y0;             // top-left tap; meaningful only where a slot is taken
    float bw[4];            // slot 2 b + a: the bilinear weight of (x0 + a, y0 + b)
    bool take[4];           // the slot is inside the image and bw != 0
};

MID_TAPS_HD ReprojectTaps reproject_taps(int x, int y, float mx, float my, int width, int height)
{
    ReprojectTaps t;
    t.x0 = t.y0 = 0;
    for (int i = 0; i < 4; ++i) { t.bw[i] = 0.f; t.take[i] = false; }
    const float ppx = (float)x + mx, ppy = (float)y + my;
    if (!(ppx > -1.f && ppx < (float)width && ppy > -1.f && ppy < (float)height)) return t;
    const float fx0 = floorf(ppx), fy0 = floorf(ppy);
    const float fx = ppx - fx0, fy = ppy - fy0;
    t.x0 = (int)fx0; t.y0 = (int)fy0;       // in [-1, width - 1] x [-1, height - 1]
    const float wx[2] = {1.f - fx, fx}, wy[2] = {1.f - fy, fy};
    for (int b = 0; b < 2; ++b)
        for (int a = 0; a < 2; ++a) {
            const int qx = t.x0 + a, qy = t.y0 + b;
            const float bw = wx[a] * wy[b];
            t.bw[2 * b + a] = bw;
            t.take[2 * b + a] = qx >= 0 && qx < width && qy >= 0 && qy < height && bw != 0.f;
        }
    return t;
}

}  // namespace mid
