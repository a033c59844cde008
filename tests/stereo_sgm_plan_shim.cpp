// C face of the semi-global matcher's host-side plan (csrc/stereo_sgm_plan.hpp, SPEC S90-S91) for tests/test_sgm_cpu.py: the
// statuses that need no device, the computed rectangle, the workspace and the grids, flattened into doubles (every field is an
// int or a byte count below 2^53).
#include "stereo_sgm_plan.hpp"

// prm: min_disp, num_disp, p1, p2, paths, uniqueness, flags, reserved.  out: 12 fields, then dx, dy, grid, steps per pass (8 x 4).
extern "C" int sgm_plan_shim(int w, int h, int lstride, int rstride, int dstride, const int* prm, double* out)
{
    pm_sgm_params p;
    p.min_disp = prm[0]; p.num_disp = prm[1]; p.p1 = prm[2]; p.p2 = prm[3];
    p.paths = prm[4]; p.uniqueness = prm[5]; p.flags = prm[6]; p.reserved = prm[7];
    const pm_sgm::Plan q = pm_sgm::plan(w, h, lstride, rstride, dstride, &p);
    if (q.status != PM_OK) return q.status;
    double* o = out;
    *o++ = q.cx0; *o++ = q.cx1; *o++ = q.cy0; *o++ = q.cy1; *o++ = q.wc; *o++ = q.hc; *o++ = q.nc;
    *o++ = static_cast<double>(q.census_bytes); *o++ = static_cast<double>(q.s_bytes); *o++ = static_cast<double>(q.need);
    *o++ = q.census_grid_x; *o++ = q.npass;
    for (int i = 0; i < q.npass; ++i) {
        *o++ = q.pass[i].dx; *o++ = q.pass[i].dy; *o++ = q.pass[i].grid; *o++ = q.pass[i].steps;
    }
    return PM_OK;
}

extern "C" int sgm_plan_sizeof_params() { return static_cast<int>(sizeof(pm_sgm_params)); }
