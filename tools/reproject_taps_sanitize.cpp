// reproject_taps_sanitize.cpp -- the tap geometry of the recursive temporal accumulation (csrc/reproject_taps.hpp) on the CPU, built
// with -fsanitize=address,undefined by tests/test_reproject_taps_sanitize.py: a sweep over every pixel of every image of 1..5 x 1..5
// texels and every pair of motions from a set that holds what a renderer can hand over by mistake -- huge, infinite and NaN vectors,
// a negative zero, and the last value above -1.  The taps are used as the kernel uses them: a table of width * height texels is
// read at every tap taken, so a tap outside the image is an AddressSanitizer report, and a float -> int conversion out of range an
// UndefinedBehaviorSanitizer one.  Checked besides: every tap taken lies inside the image, has a weight in (0, 1], and the weights
// taken sum to at most 1; integer motion inside the image takes exactly one tap of weight 1.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../image_denoising_filter_amd/csrc/reproject_taps.hpp"

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    long calls = 0, taken = 0, wrong = 0;
    for (int w = 1; w <= 5; ++w)
        for (int h = 1; h <= 5; ++h) {
            const float ms[] = {0.f, 0.25f, -0.25f, 1.f, -1.f, (float)w, -(float)w, (float)h, -(float)h, 1e9f, -1e9f, 1e30f, -1e30f,
                                inf, -inf, nan, -0.0f, -1.f + ldexpf(1.f, -24)};
            std::vector<float> table((size_t)w * h);      // exactly the image: ASan guards both ends
            for (size_t i = 0; i < table.size(); ++i) table[i] = (float)i;
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x)
                    for (float mx : ms)
                        for (float my : ms) {
                            const mid::ReprojectTaps t = mid::reproject_taps(x, y, mx, my, w, h);
                            ++calls;
                            double sum = 0.0;
                            int n = 0;
                            for (int i = 0; i < 4; ++i) {
                                if (!t.take[i]) continue;
                                const int qx = t.x0 + (i & 1), qy = t.y0 + (i >> 1);
                                const bool inside = qx >= 0 && qx < w && qy >= 0 && qy < h;
                                if (!inside || !(t.bw[i] > 0.f && t.bw[i] <= 1.f)) { ++wrong; continue; }
                                const volatile float v = table[(size_t)qy * w + qx];
                                (void)v;
                                sum += (double)t.bw[i];
                                ++n;
                            }
                            taken += n;
                            if (!(sum <= 1.0)) ++wrong;
                            const bool finite = std::isfinite(mx) && std::isfinite(my);
                            if (!finite && n != 0) ++wrong;               // NaN / Inf motion: no history
                            if (finite && std::fabs(mx) >= 1e9f && n != 0) ++wrong;
                            if (finite && mx == std::floor(mx) && my == std::floor(my)) {     // integer motion: one texel or none
                                const float sx = (float)x + mx, sy = (float)y + my;
                                const bool in = sx >= 0.f && sx < (float)w && sy >= 0.f && sy < (float)h;
                                if (n != (in ? 1 : 0)) ++wrong;
                                if (in && !(sum == 1.0 && t.take[0] && t.x0 == (int)sx && t.y0 == (int)sy)) ++wrong;
                            }
                        }
        }
    printf("reproject_taps: %ld calls, %ld taps taken, %ld wrong\n", calls, taken, wrong);
    return wrong ? 1 : 0;
}
