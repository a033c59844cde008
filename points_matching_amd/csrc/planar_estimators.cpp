// planar_estimators.cpp — the C-ABI entry points of the two planar model families of include/pm.h: the robust
// homography (RANSAC-H, ransac_h_fused.hip, refined by homography_refine.hip) and the robust affine / similarity model
// (RANSAC-A, ransac_a_fused.hip, refitted by affine_refine.hip).  Those files hold the kernels and one enqueue each;
// here are the argument checks, the staging of host arrays and one driver for every host-pointer form: upload, RANSAC
// and / or the refit on one stream, one readback into pinned memory, one synchronisation.
#include "affine_core.hpp"
#include "ransac_internal.hpp"

namespace pm_ransac {
namespace {

// The model family of a call.  Homography: 9 words, 4-point samples, refined by LM with max_iters.  Affine: 6 words,
// 3-point (PM_AFFINE_FULL) or 2-point (PM_AFFINE_PARTIAL) samples, refitted in closed form.
struct Family {
    bool affine;
    int model;                  // affine: PM_AFFINE_FULL | PM_AFFINE_PARTIAL
    int max_iters;              // homography refinement
    int words() const { return affine ? 6 : 9; }
    int min_pts() const
    {
        using namespace pm_affine;
        if (!affine) return 4;
        return model == PM_AFFINE_FULL ? Traits<FULL>::MIN_PTS : Traits<PARTIAL>::MIN_PTS;
    }
    const char* name() const { return affine ? "A" : "H"; }
};

Family homography(int max_iters) { return Family{false, 0, max_iters}; }
Family affine(int model) { return Family{true, model, 0}; }

// What a call runs: RANSAC, the refit of a model (RANSAC's winner, or the caller's), or both in that order.
enum Steps { RANSAC = 1, REFIT = 2 };

// The family's own checks, in the order every entry point runs them: model (affine), params (RANSAC), max_iters
// (homography refit).
int check_args(const Family& f, int steps, const pm_ransac_params* p)
{
    if (f.affine)
        PM_REQUIRE(f.model == PM_AFFINE_FULL || f.model == PM_AFFINE_PARTIAL, PM_E_INVALID,
                   "model must be PM_AFFINE_FULL or PM_AFFINE_PARTIAL");
    if (steps & RANSAC) {
        PM_REQUIRE(p != nullptr, PM_E_INVALID, "params is null");
        PM_REQUIRE(p->hyp_begin >= 0 && p->hyp_end > p->hyp_begin && p->hyp_end <= 0x100000000LL, PM_E_INVALID,
                   "hypothesis ids must satisfy 0 <= begin < end <= 2^32");
        PM_REQUIRE(p->hyp_end - p->hyp_begin <= 0x7FFFFFFFLL, PM_E_INVALID,
                   "a single launch takes at most 2^31 - 1 hypothesis ids: split the range");
        PM_REQUIRE(p->error_kind == PM_ERR_REPROJ, PM_E_INVALID, "error_kind must be PM_ERR_REPROJ");
    }
    if ((steps & REFIT) && !f.affine)
        PM_REQUIRE(f.max_iters >= 0 && f.max_iters <= 100, PM_E_INVALID, "max_iters must lie in [0, 100]");
    return PM_OK;
}

int enqueue_ransac(pm_ctx* ctx, const Family& f, const pm_points_view& v, const pm_ransac_params* p,
                   unsigned long long* d_key, double* d_model, uint8_t* d_mask, int mask_len, int* d_ninl)
{
    if (f.affine) return ransac_a_enqueue(ctx, f.model, v, p, d_key, d_model, d_mask, mask_len, d_ninl);
    return ransac_h_enqueue(ctx, v, p, d_key, d_model, d_mask, mask_len, d_ninl);
}

int enqueue_refine(pm_ctx* ctx, const Family& f, const pm_points_view& v, const uint8_t* d_mask, const double* d_in,
                   double* d_out, pm_h_refine_info* d_info)
{
    if (f.affine) return affine_refine_enqueue(ctx, f.model, v, d_mask, d_in, d_out, d_info);
    return homography_refine_enqueue(ctx, v, d_mask, d_in, f.max_iters, d_out, d_info);
}

// The small results of a host-pointer call, one block on the device and one in pinned memory (the mask follows the
// pinned one).  A RANSAC launch writes key, model and count; a refit reads the model and writes model and info.
struct Results {
    unsigned long long key;
    double model[9];
    int32_t count;
    pm_h_refine_info info;
};

// n correspondences as two plain device arrays: one part, no device-side count
pm_points_view one_part_view(const float* dxy1, const float* dxy2, int n)
{
    return pm_points_view{dxy1, dxy2, nullptr, 1, n, 0, 1, 0};
}

struct HostOut {
    double* model;
    uint8_t* mask;              // n bytes
    int* n_inliers;
    uint64_t* best_key;
    pm_h_refine_info* info;
};

// Driver of every host-pointer form.  RANSAC over p's ids, then (REFIT) the refit of its winner: the outputs are zeroed
// (info: status 2) before the first check.  REFIT alone: the refit of model_in on mask_in; out.model is model_in (may
// alias) and info status 1 before the first check.
int run_host(pm_ctx* ctx, const Family& f, int steps, const float* xy1, const float* xy2, int n,
             const pm_ransac_params* p, const uint8_t* mask_in, const double* model_in, const HostOut& out)
{
    const bool ransac = steps & RANSAC, refit = steps & REFIT;
    const size_t model_bytes = sizeof(double) * static_cast<size_t>(f.words());
    double in[9];
    if (ransac) {
        if (out.model) memset(out.model, 0, model_bytes);
        if (out.mask && n > 0) memset(out.mask, 0, static_cast<size_t>(n));
        if (out.n_inliers) *out.n_inliers = 0;
        if (out.best_key) *out.best_key = 0;
        if (out.info) *out.info = pm_h_refine_info{0.0, 0.0, 0, 0, 2, 0};
    } else {
        PM_REQUIRE(model_in && out.model, PM_E_INVALID, f.affine ? "null A" : "null H");
        memcpy(in, model_in, model_bytes);
        memcpy(out.model, in, model_bytes);
        if (out.info) *out.info = pm_h_refine_info{0.0, 0.0, 0, 0, 1, 0};
    }
    int rc = check_args(f, steps, p);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(n >= 0 && (n == 0 || (xy1 && xy2 && (ransac || mask_in))), PM_E_INVALID,
               ransac ? "bad point arrays" : "bad point or mask arrays");
    if (n < f.min_pts()) {
        pm::set_error("need at least %d correspondences, got %d", f.min_pts(), n);
        return PM_E_TOO_FEW;
    }
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));

    const size_t xyb = sizeof(float) * 2 * static_cast<size_t>(n);
    rc = pm::arena_reserve(ctx, 2 * pm::align_up(xyb, 256) + pm::align_up(static_cast<size_t>(n), 256) +
                                    pm::align_up(sizeof(Results), 256) +
                                    (ransac ? fused_scratch_bytes(ctx, p) + 2048 : 0));
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    float* dxy1 = static_cast<float*>(pm::arena_take(ctx, xyb));
    float* dxy2 = static_cast<float*>(pm::arena_take(ctx, xyb));
    uint8_t* dmask = static_cast<uint8_t*>(pm::arena_take(ctx, static_cast<size_t>(n)));
    Results* dres = static_cast<Results*>(pm::arena_take(ctx, sizeof(Results)));
    PM_REQUIRE(dxy1 && dxy2 && dmask && dres, PM_E_NOMEM, "scratch arena too small");
    rc = pm::pinned_reserve(ctx, sizeof(Results) + static_cast<size_t>(n));
    if (rc != PM_OK) return rc;
    Results* hres = static_cast<Results*>(ctx->pinned);
    uint8_t* hmask = reinterpret_cast<uint8_t*>(hres + 1);

    PM_HIP_CHECK(hipMemcpyAsync(dxy1, xy1, xyb, hipMemcpyHostToDevice, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(dxy2, xy2, xyb, hipMemcpyHostToDevice, ctx->stream));
    if (!ransac) {
        memcpy(hres->model, in, model_bytes);
        PM_HIP_CHECK(hipMemcpyAsync(dmask, mask_in, static_cast<size_t>(n), hipMemcpyHostToDevice, ctx->stream));
        PM_HIP_CHECK(hipMemcpyAsync(dres->model, hres->model, model_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    const pm_points_view v = one_part_view(dxy1, dxy2, n);
    if (ransac) {
        rc = enqueue_ransac(ctx, f, v, p, &dres->key, dres->model, dmask, n, &dres->count);
        if (rc != PM_OK) return rc;
    }
    if (refit) {
        rc = enqueue_refine(ctx, f, v, dmask, dres->model, dres->model, &dres->info);
        if (rc != PM_OK) return rc;
    }
    PM_HIP_CHECK(hipMemcpyAsync(hres, dres, sizeof(Results), hipMemcpyDeviceToHost, ctx->stream));
    if (ransac) PM_HIP_CHECK(hipMemcpyAsync(hmask, dmask, static_cast<size_t>(n), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    if (!ransac) {
        memcpy(out.model, hres->model, model_bytes);
        if (out.info) *out.info = hres->info;
        if (hres->info.status == 2) {
            pm::set_error("the input %s is zero (no model)", f.name());
            return PM_E_NO_MODEL;
        }
        return PM_OK;
    }
    if (out.best_key) *out.best_key = hres->key;
    if (out.info) *out.info = refit ? hres->info : pm_h_refine_info{0.0, 0.0, 0, 0, hres->key ? 1 : 2, 0};
    if (hres->key == 0ull) {
        pm::set_error("no valid model (all hypotheses degenerate)");
        return PM_E_NO_MODEL;
    }
    if (out.model) memcpy(out.model, hres->model, model_bytes);
    if (out.mask) memcpy(out.mask, hmask, static_cast<size_t>(n));
    if (out.n_inliers) *out.n_inliers = hres->count;
    return PM_OK;
}

// The model, mask and count of hypothesis id `hyp` alone: RANSAC over [hyp, hyp + 1).
int run_host_hyp(pm_ctx* ctx, const Family& f, const float* xy1, const float* xy2, int n, const pm_ransac_params* p,
                 int64_t hyp, double* model, uint8_t* mask, int* n_inliers)
{
    if (model) memset(model, 0, sizeof(double) * static_cast<size_t>(f.words()));
    if (n_inliers) *n_inliers = 0;
    PM_REQUIRE(hyp >= 0 && hyp < 0x100000000LL, PM_E_INVALID, "hypothesis id must satisfy 0 <= hyp < 2^32");
    PM_REQUIRE(p != nullptr, PM_E_INVALID, "params is null");
    pm_ransac_params q = *p;
    q.hyp_begin = hyp;
    q.hyp_end = hyp + 1;
    return run_host(ctx, f, RANSAC, xy1, xy2, n, &q, nullptr, nullptr,
                    HostOut{model, mask, n_inliers, nullptr, nullptr});
}

// The device forms' checks after the family's: the view, ctx; then the device and (RANSAC, p checked) the arena for the
// workgroup slots.
int dev_prologue(pm_ctx* ctx, const pm_points_view* view, const pm_ransac_params* p)
{
    int rc = check_view(view);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    if (!p) return PM_OK;
    rc = pm::arena_reserve(ctx, fused_scratch_bytes(ctx, p) + 1024);
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    return PM_OK;
}

int run_dev(pm_ctx* ctx, const Family& f, const pm_points_view* view, const pm_ransac_params* p, uint64_t* d_best_key,
            double* d_model, uint8_t* d_mask, int mask_len, int32_t* d_n_inliers)
{
    PM_REQUIRE(d_best_key && d_model && d_mask && d_n_inliers, PM_E_INVALID, "null argument");
    PM_REQUIRE(mask_len >= 0, PM_E_INVALID, "mask_len must be >= 0");
    int rc = check_args(f, RANSAC, p);
    if (rc != PM_OK) return rc;
    rc = dev_prologue(ctx, view, p);
    if (rc != PM_OK) return rc;
    return enqueue_ransac(ctx, f, *view, p, reinterpret_cast<unsigned long long*>(d_best_key), d_model, d_mask,
                          mask_len, d_n_inliers);
}

int refine_dev(pm_ctx* ctx, const Family& f, const pm_points_view* view, const uint8_t* d_mask, const double* d_in,
               double* d_out, pm_h_refine_info* d_info)
{
    PM_REQUIRE(d_mask && d_in && d_out, PM_E_INVALID, "null argument");
    int rc = check_args(f, REFIT, nullptr);
    if (rc != PM_OK) return rc;
    rc = dev_prologue(ctx, view, nullptr);
    if (rc != PM_OK) return rc;
    return enqueue_refine(ctx, f, *view, d_mask, d_in, d_out, d_info);
}

}  // namespace
}  // namespace pm_ransac

using namespace pm_ransac;

// ---- robust homography
extern "C" int pm_ransac_homography(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_ransac_params* p,
                                    double H[9], uint8_t* mask, int* n_inliers, uint64_t* best_key)
{
    return run_host(ctx, homography(0), RANSAC, xy1, xy2, n, p, nullptr, nullptr,
                    HostOut{H, mask, n_inliers, best_key, nullptr});
}

extern "C" int pm_ransac_homography_from_hyp(pm_ctx* ctx, const float* xy1, const float* xy2, int n,
                                             const pm_ransac_params* p, int64_t hyp, double H[9], uint8_t* mask,
                                             int* n_inliers)
{
    return run_host_hyp(ctx, homography(0), xy1, xy2, n, p, hyp, H, mask, n_inliers);
}

extern "C" int pm_ransac_homography_run_dev(pm_ctx* ctx, const pm_points_view* view, const pm_ransac_params* p,
                                            uint64_t* d_best_key, double* d_H, uint8_t* d_mask, int mask_len,
                                            int32_t* d_n_inliers)
{
    return run_dev(ctx, homography(0), view, p, d_best_key, d_H, d_mask, mask_len, d_n_inliers);
}

extern "C" int pm_homography_refine(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const uint8_t* mask,
                                    const double H_in[9], int max_iters, double H_out[9], pm_h_refine_info* info)
{
    return run_host(ctx, homography(max_iters), REFIT, xy1, xy2, n, nullptr, mask, H_in,
                    HostOut{H_out, nullptr, nullptr, nullptr, info});
}

extern "C" int pm_homography_refine_dev(pm_ctx* ctx, const pm_points_view* view, const uint8_t* d_mask,
                                        const double* d_H_in, int max_iters, double* d_H_out, pm_h_refine_info* d_info)
{
    return refine_dev(ctx, homography(max_iters), view, d_mask, d_H_in, d_H_out, d_info);
}

extern "C" int pm_ransac_homography_refined(pm_ctx* ctx, const float* xy1, const float* xy2, int n,
                                            const pm_ransac_params* p, int max_iters, double H[9], uint8_t* mask,
                                            int* n_inliers, uint64_t* best_key, pm_h_refine_info* info)
{
    return run_host(ctx, homography(max_iters), RANSAC | REFIT, xy1, xy2, n, p, nullptr, nullptr,
                    HostOut{H, mask, n_inliers, best_key, info});
}

// ---- robust affine / similarity
extern "C" int pm_ransac_affine(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n,
                                const pm_ransac_params* p, double A[6], uint8_t* mask, int* n_inliers,
                                uint64_t* best_key)
{
    return run_host(ctx, affine(model), RANSAC, xy1, xy2, n, p, nullptr, nullptr,
                    HostOut{A, mask, n_inliers, best_key, nullptr});
}

extern "C" int pm_ransac_affine_from_hyp(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n,
                                         const pm_ransac_params* p, int64_t hyp, double A[6], uint8_t* mask,
                                         int* n_inliers)
{
    return run_host_hyp(ctx, affine(model), xy1, xy2, n, p, hyp, A, mask, n_inliers);
}

extern "C" int pm_ransac_affine_run_dev(pm_ctx* ctx, int model, const pm_points_view* view, const pm_ransac_params* p,
                                        uint64_t* d_best_key, double* d_A, uint8_t* d_mask, int mask_len,
                                        int32_t* d_n_inliers)
{
    return run_dev(ctx, affine(model), view, p, d_best_key, d_A, d_mask, mask_len, d_n_inliers);
}

extern "C" int pm_affine_refine(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n, const uint8_t* mask,
                                const double A_in[6], double A_out[6], pm_h_refine_info* info)
{
    return run_host(ctx, affine(model), REFIT, xy1, xy2, n, nullptr, mask, A_in,
                    HostOut{A_out, nullptr, nullptr, nullptr, info});
}

extern "C" int pm_affine_refine_dev(pm_ctx* ctx, int model, const pm_points_view* view, const uint8_t* d_mask,
                                    const double* d_A_in, double* d_A_out, pm_h_refine_info* d_info)
{
    return refine_dev(ctx, affine(model), view, d_mask, d_A_in, d_A_out, d_info);
}

extern "C" int pm_estimate_affine(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n,
                                  const pm_ransac_params* p, int refine, double A[6], uint8_t* mask, int* n_inliers,
                                  uint64_t* best_key, pm_h_refine_info* info)
{
    return run_host(ctx, affine(model), refine ? RANSAC | REFIT : RANSAC, xy1, xy2, n, p, nullptr, nullptr,
                    HostOut{A, mask, n_inliers, best_key, info});
}
