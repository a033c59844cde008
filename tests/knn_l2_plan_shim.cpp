// C face of the L2 matcher's route planner (csrc/knn_l2_plan.hpp) for tests/test_knn_plan_cpu.py: one call flattens a
// plan into doubles (every field is an int, a bool, a float or a byte count below 2^53, so nothing is lost).
#include "knn_l2_plan.hpp"

using namespace pm_knn;

namespace {
const char* const NAMES =
    "verdict,route,want32,want16,vec,dp16,unit_hint,gen32,f16s,u8_form,u8_group,u8_int_refine,t_wide,qb_wg,nq_pad,nt_pad,"
    "g32.slots,g32.tiles_per_split,g32.rows_per_tile,g32.lid_mask,g32.eps_coef,g32.embed_coef,g32.eps_coef_gen,g32.abs_gen,"
    "g32.int_shift,"
    "g16.slots,g16.tiles_per_split,g16.rows_per_tile,g16.lid_mask,g16.eps_coef,g16.embed_coef,g16.eps_coef_gen,g16.abs_gen,"
    "g16.int_shift,"
    "splits32,splits16,lid_bits32,lid_bits16,qnorm_bytes,tnorm_bytes,c32,c16,qh,th,sdb,qfb,pkb,need,kf_tile,prep,prep_grid,"
    "prep_gen,refine8,refine_ns,refine_group,refine_km,refine_fuse,refine_vec,refine_gen";

double* put_geom(const KnnGeomPlan& g, double* o)
{
    *o++ = g.slots; *o++ = g.tiles_per_split; *o++ = g.rows_per_tile; *o++ = g.lid_mask; *o++ = g.eps_coef;
    *o++ = g.embed_coef; *o++ = g.eps_coef_gen; *o++ = g.abs_gen; *o++ = g.int_shift;
    return o;
}
}  // namespace

extern "C" const char* knn_plan_field_names() { return NAMES; }
extern "C" int knn_plan_opt_count() { return PM_OPT_COUNT_; }
extern "C" int knn_plan_u8_shift() { return U8_SHIFT; }

// req: nq, nt, dim, k, flags, n_cu, u8_rows, aligned, fuse; opts: PM_OPT_COUNT_ ints.  Returns the number of fields.
static int fields(const int* req, const int* opts, double* out)
{
    KnnL2Request r{};
    r.nq = req[0]; r.nt = req[1]; r.dim = req[2]; r.k = req[3]; r.flags = req[4]; r.n_cu = req[5];
    r.u8_rows = req[6] != 0; r.aligned = req[7] != 0; r.fuse = req[8] != 0;
    for (int i = 0; i < PM_OPT_COUNT_; ++i) r.opts[i] = opts[i];
    const KnnL2Plan p = knn_l2_plan(r);
    double* o = out;
    *o++ = p.verdict; *o++ = p.route; *o++ = p.want32; *o++ = p.want16; *o++ = p.vec; *o++ = p.dp16; *o++ = p.unit_hint;
    *o++ = p.gen32; *o++ = p.f16s; *o++ = p.u8_form; *o++ = p.u8_group; *o++ = p.u8_int_refine; *o++ = p.t_wide;
    *o++ = p.qb_wg; *o++ = p.nq_pad; *o++ = p.nt_pad;
    o = put_geom(p.g32, o);
    o = put_geom(p.g16, o);
    *o++ = p.splits32; *o++ = p.splits16; *o++ = p.lid_bits32; *o++ = p.lid_bits16;
    *o++ = static_cast<double>(p.qnorm_bytes); *o++ = static_cast<double>(p.tnorm_bytes); *o++ = static_cast<double>(p.c32);
    *o++ = static_cast<double>(p.c16); *o++ = static_cast<double>(p.qh); *o++ = static_cast<double>(p.th);
    *o++ = static_cast<double>(p.sdb); *o++ = static_cast<double>(p.qfb); *o++ = static_cast<double>(p.pkb);
    *o++ = static_cast<double>(p.need);
    *o++ = p.kf_tile; *o++ = p.prep; *o++ = p.prep_grid; *o++ = p.prep_gen; *o++ = p.refine8; *o++ = p.refine_ns;
    *o++ = p.refine_group; *o++ = p.refine_km; *o++ = p.refine_fuse; *o++ = p.refine_vec; *o++ = p.refine_gen;
    return static_cast<int>(o - out);
}

// n requests (9 ints each) with n option rows (PM_OPT_COUNT_ ints each) into n rows of fields; returns the fields per row
extern "C" int knn_plan_fields(const int* req, const int* opts, int n, double* out)
{
    int nf = 0;
    for (int i = 0; i < n; ++i) {
        nf = fields(req + 9 * static_cast<size_t>(i), opts + PM_OPT_COUNT_ * static_cast<size_t>(i), out);
        out += nf;
    }
    return nf;
}
