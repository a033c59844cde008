// C face of csrc/image_args.hpp (what an image argument of the dense calls must satisfy) for tests/test_image_args_cpu.py.
// Addresses travel as 64-bit integers: the rules do arithmetic on them and never follow one.
#include "image_args.hpp"

static const void* at(uint64_t a) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(a)); }

extern "C" uint64_t ia_span(int w, int h, int stride, int elem) { return pm_image::span(w, h, stride, static_cast<size_t>(elem)); }

extern "C" int ia_overlap(uint64_t a, uint64_t a_bytes, uint64_t b, uint64_t b_bytes)
{
    return pm_image::overlap(at(a), static_cast<size_t>(a_bytes), at(b), static_cast<size_t>(b_bytes)) ? 1 : 0;
}

extern "C" int ia_pixel_cap(int w, int h) { return pm_image::pixel_cap(w, h).status; }

extern "C" void ia_computed_columns(int from_right, int margin, int dmin, int dmax, int w, int* x01)
{
    const pm_image::Columns c = pm_image::computed_columns(from_right != 0, margin, dmin, dmax, w);
    x01[0] = c.x0;
    x01[1] = c.x1;
}

// the status; *why the message ("" when the ranges pass)
extern "C" int ia_disparity_map_ranges(uint64_t left, uint64_t right, int w, int h, int lstride, int rstride, uint64_t disp, int dstride, uint64_t info,
                                       const char** why)
{
    const pm_image::Check c = pm_image::disparity_map_ranges(at(left), at(right), w, h, lstride, rstride, at(disp), dstride, at(info));
    *why = c.why;
    return c.status;
}

extern "C" int ia_sizeof_info() { return static_cast<int>(sizeof(pm_stereo_info)); }
