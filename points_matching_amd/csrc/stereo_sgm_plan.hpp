// stereo_sgm_plan.hpp — host-side planning of pm_stereo_sgm[_dev] (docs/SPEC.md S89-S92): the argument checks that need no
// device, the computed rectangle of S90, the register groups per lane, the workspace and the grid of every pass.  No HIP here:
// stereo_sgm.hip launches what the plan says and tests/stereo_sgm_plan_shim.cpp builds it with the host compiler.
#pragma once
#include <cstddef>
#include <cstdint>

#include "image_args.hpp"
#include "pm.h"

namespace pm_sgm {

constexpr int CENSUS_TILE_W = 64, CENSUS_TILE_H = 4;      // output tile of a sgm_census workgroup (256 threads)
constexpr int MARGIN_X = 4, MARGIN_Y = 3;                 // the 9 x 7 census window
constexpr long long MAX_VOLUME = 1LL << 30;               // computed pixels x D: the u16 volume S stays within 2 GiB

struct Pass {
    int dx, dy;
    unsigned grid;                                        // one wave per row (dy == 0) or per start column
    int steps;
};

struct Plan {
    int status = PM_OK;
    const char* why = "";
    int from_right = 0, sgn = -1;                         // the other image's column of (x, d) is x + sgn * d
    int cx0 = 0, cx1 = -1, cy0 = 0, cy1 = -1;             // the computed rectangle, inclusive
    int wc = 0, hc = 0;                                   // its size; both 0 when there is no computed pixel
    int rows = 0;                                         // rows of a census plane: the image rows that have a census
    int nc = 1;                                           // disparities per lane, ceil(D / 64)
    size_t census_bytes = 0;                              // one plane: rows x w words of 8 bytes
    size_t s_bytes = 0;                                   // wc x hc x D sums of 2 bytes
    size_t need = 0;                                      // arena bytes: two planes and S, each on a 256-byte boundary
    unsigned census_grid_x = 0;                           // tiles of one image; the grid's y is the image
    int npass = 0;
    Pass pass[8];                                         // in launch order: the first writes S, the last picks the winner
};

inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }

inline Plan refuse(int status, const char* why)
{
    Plan q;
    q.status = status;
    q.why = why;
    return q;
}

// p is not null.  The order of the checks is pm_stereo_bm's.
inline Plan plan(int w, int h, int lstride, int rstride, int dstride, const pm_sgm_params* p)
{
    if ((p->flags & ~PM_STEREO_FROM_RIGHT) != 0) return refuse(PM_E_INVALID, "unknown flag bits");
    if (p->reserved != 0) return refuse(PM_E_INVALID, "reserved != 0");
    if (p->num_disp < 1 || p->num_disp > 256) return refuse(PM_E_INVALID, "num_disp outside [1, 256]");
    if (p->min_disp < -1024 || p->min_disp + p->num_disp - 1 > 1024) return refuse(PM_E_INVALID, "disparities outside [-1024, 1024]");
    if (p->p1 < 0 || p->p1 > p->p2 || p->p2 > 1023) return refuse(PM_E_INVALID, "need 0 <= p1 <= p2 <= 1023");
    if (p->paths != 4 && p->paths != 8) return refuse(PM_E_INVALID, "paths is neither 4 nor 8");
    if (p->uniqueness < 0 || p->uniqueness > 99) return refuse(PM_E_INVALID, "uniqueness outside [0, 99]");
    if (w < 1 || h < 1) return refuse(PM_E_INVALID, "need sizes >= 1");
    if (lstride < w || rstride < w || dstride < w) return refuse(PM_E_INVALID, "a stride below the width");
    const pm_image::Check cap = pm_image::pixel_cap(w, h);
    if (cap.status != PM_OK) return refuse(cap.status, cap.why);

    Plan q;
    const int D = p->num_disp;
    q.from_right = (p->flags & PM_STEREO_FROM_RIGHT) != 0;
    q.sgn = q.from_right ? 1 : -1;
    const pm_image::Columns cols = pm_image::computed_columns(q.from_right != 0, MARGIN_X, p->min_disp, p->min_disp + D - 1, w);
    q.cx0 = cols.x0;
    q.cx1 = cols.x1;
    q.cy0 = MARGIN_Y;
    q.cy1 = h - 1 - MARGIN_Y;
    q.rows = q.cy1 >= q.cy0 ? q.cy1 - q.cy0 + 1 : 0;
    if (q.cx1 >= q.cx0 && q.rows > 0) {
        q.wc = q.cx1 - q.cx0 + 1;
        q.hc = q.rows;
    }
    if (static_cast<long long>(q.wc) * q.hc * D > MAX_VOLUME) return refuse(PM_E_UNSUPPORTED, "computed pixels x num_disp above 2^30");
    q.nc = (D + 63) / 64;
    q.census_bytes = static_cast<size_t>(q.rows) * w * 8;
    q.s_bytes = static_cast<size_t>(q.wc) * q.hc * D * 2;
    q.need = 2 * align256(q.census_bytes) + align256(q.s_bytes) + 256;
    q.census_grid_x = static_cast<unsigned>((w + CENSUS_TILE_W - 1) / CENSUS_TILE_W) * static_cast<unsigned>((h + CENSUS_TILE_H - 1) / CENSUS_TILE_H);
    if (q.wc > 0) {
        // The sums commute, so the order is free.  A horizontal pass has only hc waves of wc steps, on a landscape frame fewer
        // and longer than any other pass: one of them goes first, where a step does not read S, and a vertical pass goes last,
        // where a step also picks the winner (1920 x 1080, D = 128, 8 paths: 4.4 ms per map, 4.8 ms with a horizontal pass last).
        static const int dirs4[4][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}};
        static const int dirs8[8][2] = {{1, 0}, {-1, 0}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1}, {0, 1}, {0, -1}};
        q.npass = p->paths;
        for (int i = 0; i < q.npass; ++i) {
            Pass& s = q.pass[i];
            s.dx = p->paths == 4 ? dirs4[i][0] : dirs8[i][0];
            s.dy = p->paths == 4 ? dirs4[i][1] : dirs8[i][1];
            s.grid = static_cast<unsigned>(s.dy == 0 ? q.hc : q.wc);
            s.steps = s.dy == 0 ? q.wc : q.hc;
        }
    }
    return q;
}

}  // namespace pm_sgm
