// image_args.hpp — what an image argument of the dense calls must satisfy (warp.hip, undistort.hip, stereo.hip, stereo_sgm.hip;
// the pixel cap also in track_lk.hip and features.hip): the pixel cap, the byte range of a strided image and the overlap test,
// the computed columns of a stereo matcher and the buffer rule of a disparity map.  A rule that can refuse returns a Check, which
// the caller turns into its own status and message (PM_REQUIRE_PASS, pm_common.hpp).  No HIP here: stereo_sgm_plan.hpp uses it
// and tests/image_args_shim.cpp builds it with the host compiler.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pm.h"

namespace pm_image {

struct Check {
    int status = PM_OK;
    const char* why = "";
};

constexpr long long MAX_PIXELS = 100000000LL;

inline Check pixel_cap(int w, int h)
{
    if (static_cast<long long>(w) * h > MAX_PIXELS) return {PM_E_UNSUPPORTED, "more than 100 000 000 pixels"};
    return {};
}

// bytes from the first element of an h x w image with `stride` elements per row to the end of its last one (h, w >= 1)
inline size_t span(int w, int h, int stride, size_t elem) { return (static_cast<size_t>(h - 1) * stride + w) * elem; }

inline bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return !(a0 + a_bytes <= b0 || b0 + b_bytes <= a0);
}

// S85 / S90: the columns whose window (`margin` columns to either side) and whose disparities dmin .. dmax stay inside both
// images, inclusive; x1 < x0: none
struct Columns {
    int x0, x1;
};
inline Columns computed_columns(bool from_right, int margin, int dmin, int dmax, int w)
{
    if (from_right) return {margin - (dmin < 0 ? dmin : 0), w - 1 - margin - (dmax > 0 ? dmax : 0)};
    return {margin + (dmax > 0 ? dmax : 0), w - 1 - margin + (dmin < 0 ? dmin : 0)};
}

// S85's buffer rule, which S90 takes over: the map overlaps neither image, the info record (may be null) none of the three
inline Check disparity_map_ranges(const void* left, const void* right, int w, int h, int lstride, int rstride, const void* disp, int dstride,
                                  const void* info)
{
    const size_t l_b = span(w, h, lstride, 1), r_b = span(w, h, rstride, 1), d_b = span(w, h, dstride, 2), i_b = sizeof(pm_stereo_info);
    if (overlap(left, l_b, disp, d_b) || overlap(right, r_b, disp, d_b)) return {PM_E_INVALID, "an input image and the disparity map overlap"};
    if (info && (overlap(info, i_b, left, l_b) || overlap(info, i_b, right, r_b) || overlap(info, i_b, disp, d_b)))
        return {PM_E_INVALID, "the info record overlaps an image or the map"};
    return {};
}

}  // namespace pm_image
