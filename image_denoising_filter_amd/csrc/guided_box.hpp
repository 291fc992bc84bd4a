// guided_box.hpp -- the geometry of the guided filter's sliding box sums (csrc/guided.hip; include/mi_denoise.h, section a4o),
// for the kernels and for the host program that walks it under a sanitizer (tools/guided_box_sanitize.cpp).
//
// A workgroup of kGuidedLanes threads (four waves), lanes along x, owns a TILE: a strip of guided_strip_w(r) = kGuidedLanes - 2 r
// output columns by one SEGMENT of kGuidedPeriod output rows.  Lane t holds the column guided_col(strip, r, t) = strip * strip_w - r + t
// of the image (possibly outside it: such a column sums to zero), so the lanes r .. kGuidedLanes - r - 1 are the output lanes and
// every output lane finds the 2 r + 1 columns of its window among the workgroup's lanes.  The vertical sums of a lane's column live
// in its registers and RESTART with every segment: the workgroup walks the rows guided_row_begin(seg, r) .. guided_row_end(seg, r, h) - 1,
// row yy enters the sums (when it lies inside the image), row yy - (2 r + 1) leaves them (when it entered: guided_row_left), and
// from yy = first output row + r on the row yy - r is an output row.  The first output row of a segment therefore follows exactly
// 2 r + 1 walked rows, its window, and no rounding error travels further than kGuidedPeriod + 2 r rows down a column.
// Per row the column sums cross LDS once as prefix sums along x over the kGuidedLanes lanes; an output lane's window is the
// difference of the slots guided_slot_hi(t, r) and guided_slot_lo(t, r) (-1: nothing to subtract).  All kGuidedLanes slots are
// written in every round, and an output lane reads only slots 0 .. kGuidedLanes - 1.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define GUIDED_HD __host__ __device__ __forceinline__
#else
#define GUIDED_HD inline
#endif

namespace mid {

constexpr int kGuidedLanes = 256;      // threads of a workgroup = columns it holds
constexpr int kGuidedPeriod = 32;      // output rows of a segment: the vertical sums restart after them
constexpr int kGuidedMaxRadius = 16;
constexpr unsigned kGuidedGroups = 8192;   // cap of the grid; workgroup g takes the tiles g, g + G, ...

GUIDED_HD int guided_strip_w(int r) { return kGuidedLanes - 2 * r; }
GUIDED_HD int guided_strips(int width, int r) { return (width + guided_strip_w(r) - 1) / guided_strip_w(r); }
GUIDED_HD int guided_segments(int height) { return (height + kGuidedPeriod - 1) / kGuidedPeriod; }
GUIDED_HD unsigned guided_tiles(int width, int height, int r) { return (unsigned)guided_strips(width, r) * (unsigned)guided_segments(height); }

// image column of lane t in a strip (may lie outside [0, width))
GUIDED_HD int guided_col(int strip, int r, int t) { return strip * guided_strip_w(r) - r + t; }
GUIDED_HD bool guided_out_lane(int r, int t) { return t >= r && t < kGuidedLanes - r; }
// the prefix slots whose difference is the window of output lane t
GUIDED_HD int guided_slot_hi(int t, int r) { return t + r; }
GUIDED_HD int guided_slot_lo(int t, int r) { return t - r - 1; }       // -1 for t == r: the prefix before slot 0 is zero

// rows a segment walks: [begin, end); they may lie outside the image, where nothing enters the sums
GUIDED_HD int guided_seg_y0(int seg) { return seg * kGuidedPeriod; }
GUIDED_HD int guided_seg_y1(int seg, int height) { return (seg + 1) * kGuidedPeriod < height ? (seg + 1) * kGuidedPeriod : height; }
GUIDED_HD int guided_row_begin(int seg, int r) { return guided_seg_y0(seg) - r; }
GUIDED_HD int guided_row_end(int seg, int r, int height) { return guided_seg_y1(seg, height) + r; }
// the row that leaves when row yy has entered, and whether it ever entered in this segment
GUIDED_HD int guided_row_leaving(int yy, int r) { return yy - (2 * r + 1); }
GUIDED_HD bool guided_row_left(int yy, int seg, int r) { return guided_row_leaving(yy, r) >= guided_row_begin(seg, r); }
// the output row completed by walked row yy, if any
GUIDED_HD int guided_row_out(int yy, int r) { return yy - r; }
GUIDED_HD bool guided_row_is_out(int yy, int seg, int r) { return guided_row_out(yy, r) >= guided_seg_y0(seg); }

GUIDED_HD size_t guided_flat(int x, int y, int width) { return (size_t)y * (size_t)width + (size_t)x; }

}  // namespace mid
