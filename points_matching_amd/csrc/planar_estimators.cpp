// planar_estimators.cpp — the C-ABI entry points of the two planar model families of include/pm.h: the robust
// homography (RANSAC-H, ransac_h_fused.hip, refined by homography_refine.hip) and the robust affine / similarity model
// (RANSAC-A, ransac_a_fused.hip, refitted by affine_refine.hip); also the calibrated relative pose (RANSAC-E) and the
// absolute pose (RANSAC-PnP, pnp_solve.hip + ransac_p_fused.hip, refined by pnp_refine.hip).  Those files hold the
// kernels and one enqueue each; here are the argument checks, the staging of host arrays and one driver for every
// host-pointer form: upload, RANSAC and / or the refit on one stream, one readback into pinned memory, one
// synchronisation.
#include <cmath>

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

// ---- calibrated relative pose (RANSAC-E and pose recovery) ------------------------------------------------------------
// S31: K and the normalised threshold (fp32), checked before anything else of the family
int check_camera(const pm_camera* K, float thresh_px, float* thr_n)
{
    PM_REQUIRE(K != nullptr, PM_E_INVALID, "K is null");
    const bool fin = std::isfinite(K->fx) && std::isfinite(K->fy) && std::isfinite(K->cx) && std::isfinite(K->cy);
    PM_REQUIRE(fin && K->fx > 0.0 && K->fy > 0.0, PM_E_INVALID, "K needs finite values and fx, fy > 0");
    const float t = static_cast<float>(static_cast<double>(thresh_px) / (0.5 * (K->fx + K->fy)));
    PM_REQUIRE(t > 0.0f && std::isfinite(t), PM_E_INVALID, "the normalised threshold must be finite and > 0");
    *thr_n = t;
    return PM_OK;
}

int check_e_params(const pm_ransac_params* p)
{
    PM_REQUIRE(p != nullptr, PM_E_INVALID, "params is null");
    PM_REQUIRE(p->hyp_begin >= 0 && p->hyp_end > p->hyp_begin && p->hyp_end <= 0x100000000LL / 10, PM_E_INVALID,
               "sample ids must satisfy 0 <= begin < end and 10 * end <= 2^32 (model ids 10h + j)");
    PM_REQUIRE(10 * (p->hyp_end - p->hyp_begin) <= 0x7FFFFFFFLL, PM_E_INVALID,
               "a single launch takes at most (2^31 - 1) / 10 samples: split the range");
    PM_REQUIRE(p->error_kind == PM_ERR_SAMPSON, PM_E_INVALID, "error_kind must be PM_ERR_SAMPSON");
    return PM_OK;
}

// The scorer's parameters: model ids [10 begin, 10 end), the normalised threshold
pm_ransac_params model_ids(const pm_ransac_params* p, float thr_n)
{
    pm_ransac_params q = *p;
    q.hyp_begin = 10 * p->hyp_begin;
    q.hyp_end = 10 * p->hyp_end;
    q.thresh_px = thr_n;
    return q;
}

// Arena bytes of a RANSAC-E run over a view of cap_total points: normalised copy, count, candidates, scorer slots
size_t e_scratch_bytes(const pm_ctx* ctx, long long cap_total, const pm_ransac_params* p, float thr_n)
{
    const pm_ransac_params q = model_ids(p, thr_n);
    const size_t nh = static_cast<size_t>(p->hyp_end - p->hyp_begin);
    return 2 * pm::align_up(sizeof(float) * 2 * static_cast<size_t>(cap_total), 256) + 256 +
           pm::align_up(sizeof(double) * 100 * nh, 256) + fused_scratch_bytes(ctx, &q) + 1024;
}

// Solve + score on ctx->stream (the arena reserved for e_scratch_bytes; carved here).  With d_cand_out the scoring
// launch is left to the caller: *d_cand_out and *vn_out receive the candidate buffer and the normalised view.
int enqueue_essential(pm_ctx* ctx, const pm_points_view& v, const pm_camera& K, const pm_ransac_params* p, float thr_n,
                      unsigned long long* d_key, double* d_E, uint8_t* d_mask, int mask_len, int* d_ninl,
                      double** d_cand_out = nullptr, pm_points_view* vn_out = nullptr)
{
    const long long cap_total = static_cast<long long>(v.parts) * v.cap;
    const size_t nh = static_cast<size_t>(p->hyp_end - p->hyp_begin);
    float* xyn = static_cast<float*>(pm::arena_take(ctx, sizeof(float) * 4 * static_cast<size_t>(cap_total)));
    int* dn = static_cast<int*>(pm::arena_take(ctx, sizeof(int)));
    double* cand = static_cast<double*>(pm::arena_take(ctx, sizeof(double) * 100 * nh));
    PM_REQUIRE(xyn && dn && cand, PM_E_NOMEM, "scratch arena too small");
    int rc = essential_solve_enqueue(ctx, v, K, p, xyn, dn, cand);
    if (rc != PM_OK) return rc;
    const pm_points_view vn{xyn, xyn + 2 * cap_total, dn, 1, static_cast<int32_t>(cap_total), 0, 1, 0};
    if (d_cand_out) {
        *d_cand_out = cand;
        *vn_out = vn;
        return PM_OK;
    }
    const pm_ransac_params q = model_ids(p, thr_n);
    return ransac_e_enqueue(ctx, vn, &q, cand, d_key, d_E, d_mask, mask_len, d_ninl);
}

// The small results of a host-pointer call of the family (mask and points follow the pinned block)
struct EResults {
    unsigned long long key;
    double E[9];
    int32_t count;
    int32_t n_good;
    double R[9];
    double t[3];
    unsigned long long keys[10];
    double cand[100];
};

enum EStep { E_RANSAC = 1, E_POSE = 2, E_CANDIDATES = 4 };

struct EHostOut {
    double* E;                  // E_RANSAC: 9; E_CANDIDATES: 90
    uint8_t* mask;              // n bytes
    int* n_inliers;
    uint64_t* best_key;
    double* R;
    double* t;
    int* n_good;
    float* points4;             // 4 n
    int32_t* counts;            // E_CANDIDATES: 10
    int* n_models;
};

// Driver of every host-pointer form of the family: RANSAC-E (or the candidates of one sample), pose recovery (of
// RANSAC's winner on its mask, or of E_in on mask_in), one readback, one synchronisation.  Outputs are zeroed before
// the first check.
int run_e_host(pm_ctx* ctx, int steps, const float* xy1, const float* xy2, int n, const pm_camera* K,
               const pm_ransac_params* p, const double* E_in, const uint8_t* mask_in, double dist, const EHostOut& out)
{
    const bool ransac = steps & (E_RANSAC | E_CANDIDATES), pose = steps & E_POSE, cands = steps & E_CANDIDATES;
    if (out.E) memset(out.E, 0, sizeof(double) * (cands ? 90 : 9));
    if (out.mask && n > 0) memset(out.mask, 0, static_cast<size_t>(n));
    if (out.n_inliers) *out.n_inliers = 0;
    if (out.best_key) *out.best_key = 0;
    if (out.R) memset(out.R, 0, sizeof(double) * 9);
    if (out.t) memset(out.t, 0, sizeof(double) * 3);
    if (out.n_good) *out.n_good = 0;
    if (out.points4 && n > 0) memset(out.points4, 0, sizeof(float) * 4 * static_cast<size_t>(n));
    if (out.counts) for (int j = 0; j < 10; ++j) out.counts[j] = -1;
    if (out.n_models) *out.n_models = 0;
    float thr_n = 1.0f;
    int rc = PM_OK;
    if (ransac) {
        rc = check_e_params(p);
        if (rc != PM_OK) return rc;
    }
    rc = check_camera(K, ransac ? p->thresh_px : 1.0f, &thr_n);
    if (rc != PM_OK) return rc;
    if (!ransac) {
        PM_REQUIRE(E_in != nullptr, PM_E_INVALID, "null E");
    }
    if (pose) PM_REQUIRE(dist > 0.0, PM_E_INVALID, "dist must be > 0");
    if (cands) PM_REQUIRE(out.E && out.counts, PM_E_INVALID, "null E or counts");
    PM_REQUIRE(n >= 0 && (n == 0 || (xy1 && xy2)), PM_E_INVALID, "bad point arrays");
    if (n < 5) {
        pm::set_error("need at least 5 correspondences, got %d", n);
        return PM_E_TOO_FEW;
    }
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));

    const size_t xyb = sizeof(float) * 2 * static_cast<size_t>(n);
    const size_t pts = out.points4 ? sizeof(float) * 4 * static_cast<size_t>(n) : 0;
    rc = pm::arena_reserve(ctx, 2 * pm::align_up(xyb, 256) + pm::align_up(static_cast<size_t>(n), 256) + pm::align_up(pts, 256) +
                                    pm::align_up(sizeof(EResults), 256) + (ransac ? e_scratch_bytes(ctx, n, p, thr_n) : 0) + (cands ? 10 * 1024 : 0) + 1024);
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    float* dxy1 = static_cast<float*>(pm::arena_take(ctx, xyb));
    float* dxy2 = static_cast<float*>(pm::arena_take(ctx, xyb));
    uint8_t* dmask = static_cast<uint8_t*>(pm::arena_take(ctx, static_cast<size_t>(n)));
    float* dpts = pts ? static_cast<float*>(pm::arena_take(ctx, pts)) : nullptr;
    EResults* dres = static_cast<EResults*>(pm::arena_take(ctx, sizeof(EResults)));
    PM_REQUIRE(dxy1 && dxy2 && dmask && dres && (dpts || !pts), PM_E_NOMEM, "scratch arena too small");
    rc = pm::pinned_reserve(ctx, sizeof(EResults) + static_cast<size_t>(n) + pts);
    if (rc != PM_OK) return rc;
    EResults* hres = static_cast<EResults*>(ctx->pinned);
    uint8_t* hmask = reinterpret_cast<uint8_t*>(hres + 1);
    float* hpts = reinterpret_cast<float*>(hmask + n);

    PM_HIP_CHECK(hipMemcpyAsync(dxy1, xy1, xyb, hipMemcpyHostToDevice, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(dxy2, xy2, xyb, hipMemcpyHostToDevice, ctx->stream));
    if (!ransac) {
        memcpy(hres->E, E_in, sizeof(double) * 9);
        PM_HIP_CHECK(hipMemcpyAsync(dres->E, hres->E, sizeof(double) * 9, hipMemcpyHostToDevice, ctx->stream));
        if (mask_in) PM_HIP_CHECK(hipMemcpyAsync(dmask, mask_in, static_cast<size_t>(n), hipMemcpyHostToDevice, ctx->stream));
    }
    const pm_points_view v = one_part_view(dxy1, dxy2, n);
    if (cands) {
        double* dcand = nullptr;
        pm_points_view vn{};
        rc = enqueue_essential(ctx, v, *K, p, thr_n, nullptr, nullptr, nullptr, 0, nullptr, &dcand, &vn);
        if (rc != PM_OK) return rc;
        // each candidate alone: model ids [10 hyp + j, 10 hyp + j + 1); its key holds its count
        for (int j = 0; j < 10; ++j) {
            pm_ransac_params q = model_ids(p, thr_n);
            q.hyp_begin += j;
            q.hyp_end = q.hyp_begin + 1;
            rc = ransac_e_enqueue(ctx, vn, &q, dcand + 10 * j, &dres->keys[j], nullptr, dmask, 0, nullptr);
            if (rc != PM_OK) return rc;
        }
        PM_HIP_CHECK(hipMemcpyAsync(dres->cand, dcand, sizeof(double) * 100, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (ransac && !cands) {
        rc = enqueue_essential(ctx, v, *K, p, thr_n, &dres->key, dres->E, dmask, n, &dres->count);
        if (rc != PM_OK) return rc;
    }
    if (pose) {
        rc = recover_pose_enqueue(ctx, v, *K, dres->E, (ransac || mask_in) ? dmask : nullptr, dist, dres->R, dres->t, dmask, n,
                                  &dres->n_good, dpts);
        if (rc != PM_OK) return rc;
    }
    PM_HIP_CHECK(hipMemcpyAsync(hres, dres, sizeof(EResults), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(hmask, dmask, static_cast<size_t>(n), hipMemcpyDeviceToHost, ctx->stream));
    if (pts) PM_HIP_CHECK(hipMemcpyAsync(hpts, dpts, pts, hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    if (cands) {
        int nm = 0;
        for (int j = 0; j < 10; ++j) {
            if (hres->cand[10 * j + 9] == 0.0) continue;
            memcpy(out.E + 9 * j, hres->cand + 10 * j, sizeof(double) * 9);
            out.counts[j] = static_cast<int32_t>(hres->keys[j] >> 32);
            ++nm;
        }
        if (out.n_models) *out.n_models = nm;
        if (nm == 0) {
            pm::set_error("no valid candidate (degenerate sample)");
            return PM_E_NO_MODEL;
        }
        return PM_OK;
    }
    if (ransac) {
        if (out.best_key) *out.best_key = hres->key;
        if (hres->key == 0ull) {
            pm::set_error("no valid model (all samples degenerate)");
            return PM_E_NO_MODEL;
        }
        if (out.E) memcpy(out.E, hres->E, sizeof(double) * 9);
        if (out.n_inliers) *out.n_inliers = hres->count;
    }
    if (pose) {
        const bool ok = hres->t[0] != 0.0 || hres->t[1] != 0.0 || hres->t[2] != 0.0;
        if (!ok) {
            pm::set_error("E does not decompose (rank < 2 or not finite)");
            return PM_E_NO_MODEL;
        }
        if (out.R) memcpy(out.R, hres->R, sizeof(double) * 9);
        if (out.t) memcpy(out.t, hres->t, sizeof(double) * 3);
        if (out.n_good) *out.n_good = hres->n_good;
        if (out.points4) memcpy(out.points4, hpts, pts);
    }
    if (out.mask) memcpy(out.mask, hmask, static_cast<size_t>(n));
    return PM_OK;
}

// ---- absolute pose (RANSAC-PnP) -------------------------------------------------------------------------------------
// S36 and the range, kind and threshold rules of S38 / S39, in this order
int check_pnp(const pm_camera* K, const pm_ransac_params* p)
{
    PM_REQUIRE(p != nullptr, PM_E_INVALID, "params is null");
    PM_REQUIRE(p->hyp_begin >= 0 && p->hyp_end > p->hyp_begin && p->hyp_end <= 0x100000000LL / 4, PM_E_INVALID,
               "sample ids must satisfy 0 <= begin < end and 4 * end <= 2^32 (model ids 4h + j)");
    PM_REQUIRE(4 * (p->hyp_end - p->hyp_begin) <= 0x7FFFFFFFLL, PM_E_INVALID,
               "a single launch takes at most (2^31 - 1) / 4 samples: split the range");
    PM_REQUIRE(p->error_kind == PM_ERR_REPROJ, PM_E_INVALID, "error_kind must be PM_ERR_REPROJ");
    PM_REQUIRE(p->thresh_px > 0.0f && std::isfinite(p->thresh_px), PM_E_INVALID, "thresh_px must be finite and > 0");
    PM_REQUIRE(K != nullptr, PM_E_INVALID, "K is null");
    const bool fin = std::isfinite(K->fx) && std::isfinite(K->fy) && std::isfinite(K->cx) && std::isfinite(K->cy);
    PM_REQUIRE(fin && K->fx > 0.0 && K->fy > 0.0, PM_E_INVALID, "K needs finite values and fx, fy > 0");
    return PM_OK;
}

// The scorer's parameters: model ids [4 begin, 4 end)
pm_ransac_params pnp_ids(const pm_ransac_params* p)
{
    pm_ransac_params q = *p;
    q.hyp_begin = 4 * p->hyp_begin;
    q.hyp_end = 4 * p->hyp_end;
    return q;
}

// Arena bytes of a RANSAC-PnP run: candidates (80 doubles per sample), scorer slots
size_t pnp_scratch_bytes(const pm_ctx* ctx, const pm_ransac_params* p)
{
    const pm_ransac_params q = pnp_ids(p);
    return pm::align_up(sizeof(double) * 80 * static_cast<size_t>(p->hyp_end - p->hyp_begin), 256) +
           fused_scratch_bytes(ctx, &q) + 1024;
}

// Solve + score on ctx->stream (the arena reserved for pnp_scratch_bytes; carved here).  With d_cand_out the scoring
// launch is left to the caller, who receives the candidate buffer.
int enqueue_pnp(pm_ctx* ctx, const pm_points_view& v, const pm_camera& K, const pm_ransac_params* p,
                unsigned long long* d_key, double* d_Rt, uint8_t* d_mask, int mask_len, int* d_ninl,
                double** d_cand_out = nullptr)
{
    double* cand = static_cast<double*>(pm::arena_take(ctx, sizeof(double) * 80 * static_cast<size_t>(p->hyp_end - p->hyp_begin)));
    PM_REQUIRE(cand, PM_E_NOMEM, "scratch arena too small");
    int rc = pnp_solve_enqueue(ctx, v, K, p, cand);
    if (rc != PM_OK) return rc;
    if (d_cand_out) {
        *d_cand_out = cand;
        return PM_OK;
    }
    const pm_ransac_params q = pnp_ids(p);
    return ransac_p_enqueue(ctx, v, &q, cand, d_key, d_Rt, d_mask, mask_len, d_ninl);
}

// The small results of a host-pointer call (the mask follows the pinned block)
struct PResults {
    unsigned long long key;
    double Rt[12];
    int32_t count;
    int32_t pad;
    unsigned long long keys[4];
    double cand[80];
    pm_h_refine_info info;
};

enum PStep { P_RANSAC = 1, P_REFINE = 2, P_CANDIDATES = 4 };

struct PHostOut {
    double* R;                  // 9
    double* t;                  // 3
    uint8_t* mask;              // n bytes
    int* n_inliers;
    uint64_t* best_key;
    pm_h_refine_info* info;
    double* Rt;                 // P_CANDIDATES: 48
    int32_t* counts;            // P_CANDIDATES: 4
    int* n_models;
};

// Driver of the host-pointer forms: RANSAC-PnP over p's samples (P_RANSAC) and / or the S40 refinement of its winner on
// its mask or of (R_in, t_in) on mask_in (P_REFINE), or every candidate of p's one sample with its count
// (P_CANDIDATES); one readback, one synchronisation.  Outputs are zeroed before the first check (refinement alone:
// R, t = R_in, t_in and info status 1).
int run_pnp_host(pm_ctx* ctx, int steps, const float* xyz, const float* uv, int n, const pm_camera* K,
                 const pm_ransac_params* p, const uint8_t* mask_in, const double* R_in, const double* t_in, int max_iters,
                 const PHostOut& out)
{
    const bool ransac = steps & (P_RANSAC | P_CANDIDATES), refine = steps & P_REFINE, cands = steps & P_CANDIDATES;
    double in[12] = {};
    if (!ransac) {
        PM_REQUIRE(R_in && t_in && out.R && out.t, PM_E_INVALID, "null R or t");
        memcpy(in, R_in, sizeof(double) * 9);
        memcpy(in + 9, t_in, sizeof(double) * 3);
    }
    if (out.R) memcpy(out.R, in, sizeof(double) * 9);
    if (out.t) memcpy(out.t, in + 9, sizeof(double) * 3);
    if (out.mask && n > 0) memset(out.mask, 0, static_cast<size_t>(n));
    if (out.n_inliers) *out.n_inliers = 0;
    if (out.best_key) *out.best_key = 0;
    if (out.info) *out.info = pm_h_refine_info{0.0, 0.0, 0, 0, ransac ? 2 : 1, 0};
    if (out.Rt) memset(out.Rt, 0, sizeof(double) * 48);
    if (out.counts) for (int j = 0; j < 4; ++j) out.counts[j] = -1;
    if (out.n_models) *out.n_models = 0;
    int rc = ransac ? check_pnp(K, p) : PM_OK;
    if (rc != PM_OK) return rc;
    if (!ransac) {
        PM_REQUIRE(K != nullptr, PM_E_INVALID, "K is null");
        const bool fin = std::isfinite(K->fx) && std::isfinite(K->fy) && std::isfinite(K->cx) && std::isfinite(K->cy);
        PM_REQUIRE(fin && K->fx > 0.0 && K->fy > 0.0, PM_E_INVALID, "K needs finite values and fx, fy > 0");
    }
    if (refine) PM_REQUIRE(max_iters >= 0 && max_iters <= 100, PM_E_INVALID, "max_iters must lie in [0, 100]");
    if (cands) PM_REQUIRE(out.Rt && out.counts, PM_E_INVALID, "null Rt or counts");
    PM_REQUIRE(n >= 0 && (n == 0 || (xyz && uv && (ransac || mask_in))), PM_E_INVALID,
               ransac ? "bad point arrays" : "bad point or mask arrays");
    if (n < 4) {
        pm::set_error("need at least 4 correspondences, got %d", n);
        return PM_E_TOO_FEW;
    }
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));

    const size_t xb = sizeof(float) * 3 * static_cast<size_t>(n), ub = sizeof(float) * 2 * static_cast<size_t>(n);
    rc = pm::arena_reserve(ctx, pm::align_up(xb, 256) + pm::align_up(ub, 256) + pm::align_up(static_cast<size_t>(n), 256) +
                                    pm::align_up(sizeof(PResults), 256) + (ransac ? pnp_scratch_bytes(ctx, p) : 0) +
                                    (cands ? 4 * 1024 : 0));
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    float* dxyz = static_cast<float*>(pm::arena_take(ctx, xb));
    float* duv = static_cast<float*>(pm::arena_take(ctx, ub));
    uint8_t* dmask = static_cast<uint8_t*>(pm::arena_take(ctx, static_cast<size_t>(n)));
    PResults* dres = static_cast<PResults*>(pm::arena_take(ctx, sizeof(PResults)));
    PM_REQUIRE(dxyz && duv && dmask && dres, PM_E_NOMEM, "scratch arena too small");
    rc = pm::pinned_reserve(ctx, sizeof(PResults) + static_cast<size_t>(n));
    if (rc != PM_OK) return rc;
    PResults* hres = static_cast<PResults*>(ctx->pinned);
    uint8_t* hmask = reinterpret_cast<uint8_t*>(hres + 1);

    PM_HIP_CHECK(hipMemcpyAsync(dxyz, xyz, xb, hipMemcpyHostToDevice, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(duv, uv, ub, hipMemcpyHostToDevice, ctx->stream));
    if (!ransac) {
        memcpy(hres->Rt, in, sizeof in);
        PM_HIP_CHECK(hipMemcpyAsync(dres->Rt, hres->Rt, sizeof in, hipMemcpyHostToDevice, ctx->stream));
        PM_HIP_CHECK(hipMemcpyAsync(dmask, mask_in, static_cast<size_t>(n), hipMemcpyHostToDevice, ctx->stream));
    }
    const pm_points_view v{dxyz, duv, nullptr, 1, n, 0, 1, 0};
    if (cands) {
        double* dcand = nullptr;
        rc = enqueue_pnp(ctx, v, *K, p, nullptr, nullptr, nullptr, 0, nullptr, &dcand);
        if (rc != PM_OK) return rc;
        // each candidate alone: model ids [4 hyp + j, 4 hyp + j + 1); its key holds its count
        for (int j = 0; j < 4; ++j) {
            pm_ransac_params q = pnp_ids(p);
            q.hyp_begin += j;
            q.hyp_end = q.hyp_begin + 1;
            rc = ransac_p_enqueue(ctx, v, &q, dcand + 20 * j, &dres->keys[j], nullptr, dmask, 0, nullptr);
            if (rc != PM_OK) return rc;
        }
        PM_HIP_CHECK(hipMemcpyAsync(dres->cand, dcand, sizeof(double) * 80, hipMemcpyDeviceToDevice, ctx->stream));
    } else if (ransac) {
        rc = enqueue_pnp(ctx, v, *K, p, &dres->key, dres->Rt, dmask, n, &dres->count);
        if (rc != PM_OK) return rc;
    }
    if (refine) {
        rc = pnp_refine_enqueue(ctx, v, *K, dmask, dres->Rt, max_iters, dres->Rt, &dres->info);
        if (rc != PM_OK) return rc;
    }
    PM_HIP_CHECK(hipMemcpyAsync(hres, dres, sizeof(PResults), hipMemcpyDeviceToHost, ctx->stream));
    if (ransac) PM_HIP_CHECK(hipMemcpyAsync(hmask, dmask, static_cast<size_t>(n), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    if (cands) {
        int nm = 0;
        for (int j = 0; j < 4; ++j) {
            if (hres->cand[20 * j + 12] == 0.0) continue;
            memcpy(out.Rt + 12 * j, hres->cand + 20 * j, sizeof(double) * 12);
            out.counts[j] = static_cast<int32_t>(hres->keys[j] >> 32);
            ++nm;
        }
        if (out.n_models) *out.n_models = nm;
        if (nm == 0) {
            pm::set_error("no valid candidate (degenerate sample)");
            return PM_E_NO_MODEL;
        }
        return PM_OK;
    }
    if (!ransac) {
        memcpy(out.R, hres->Rt, sizeof(double) * 9);
        memcpy(out.t, hres->Rt + 9, sizeof(double) * 3);
        if (out.info) *out.info = hres->info;
        if (hres->info.status == 2) {
            pm::set_error("the input pose is zero (no model)");
            return PM_E_NO_MODEL;
        }
        return PM_OK;
    }
    if (out.best_key) *out.best_key = hres->key;
    if (out.info && refine) *out.info = hres->info;
    if (hres->key == 0ull) {
        pm::set_error("no valid model (all samples degenerate)");
        return PM_E_NO_MODEL;
    }
    if (out.R) memcpy(out.R, hres->Rt, sizeof(double) * 9);
    if (out.t) memcpy(out.t, hres->Rt + 9, sizeof(double) * 3);
    if (out.mask) memcpy(out.mask, hmask, static_cast<size_t>(n));
    if (out.n_inliers) *out.n_inliers = hres->count;
    return PM_OK;
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

// ---- calibrated relative pose
extern "C" int pm_ransac_essential(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K,
                                   const pm_ransac_params* p, double E[9], uint8_t* mask, int* n_inliers, uint64_t* best_key)
{
    EHostOut o{};
    o.E = E; o.mask = mask; o.n_inliers = n_inliers; o.best_key = best_key;
    return run_e_host(ctx, E_RANSAC, xy1, xy2, n, K, p, nullptr, nullptr, 0.0, o);
}

extern "C" int pm_ransac_essential_from_hyp(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K,
                                            const pm_ransac_params* p, int64_t hyp, double E[90], int32_t counts[10],
                                            int* n_models)
{
    EHostOut o{};
    o.E = E; o.counts = counts; o.n_models = n_models;
    if (E) memset(E, 0, sizeof(double) * 90);
    if (counts) for (int j = 0; j < 10; ++j) counts[j] = -1;
    if (n_models) *n_models = 0;
    PM_REQUIRE(hyp >= 0 && hyp < 0x100000000LL / 10, PM_E_INVALID, "sample id must satisfy 0 <= hyp and 10 * hyp + 10 <= 2^32");
    PM_REQUIRE(p != nullptr, PM_E_INVALID, "params is null");
    pm_ransac_params q = *p;
    q.hyp_begin = hyp;
    q.hyp_end = hyp + 1;
    return run_e_host(ctx, E_CANDIDATES, xy1, xy2, n, K, &q, nullptr, nullptr, 0.0, o);
}

extern "C" int pm_ransac_essential_run_dev(pm_ctx* ctx, const pm_points_view* view, const pm_camera* K,
                                           const pm_ransac_params* p, uint64_t* d_best_key, double* d_E, uint8_t* d_mask,
                                           int mask_len, int32_t* d_n_inliers)
{
    PM_REQUIRE(d_best_key && d_E && d_mask && d_n_inliers, PM_E_INVALID, "null argument");
    PM_REQUIRE(mask_len >= 0, PM_E_INVALID, "mask_len must be >= 0");
    int rc = check_e_params(p);
    if (rc != PM_OK) return rc;
    float thr_n = 1.0f;
    rc = check_camera(K, p->thresh_px, &thr_n);
    if (rc != PM_OK) return rc;
    rc = dev_prologue(ctx, view, nullptr);
    if (rc != PM_OK) return rc;
    rc = pm::arena_reserve(ctx, e_scratch_bytes(ctx, static_cast<long long>(view->parts) * view->cap, p, thr_n));
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    return enqueue_essential(ctx, *view, *K, p, thr_n, reinterpret_cast<unsigned long long*>(d_best_key), d_E, d_mask, mask_len,
                             d_n_inliers);
}

extern "C" int pm_recover_pose(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K, const double E[9],
                               const uint8_t* mask_in, double dist, double R[9], double t[3], uint8_t* mask_out, int* n_good,
                               float* points4)
{
    EHostOut o{};
    o.mask = mask_out; o.R = R; o.t = t; o.n_good = n_good; o.points4 = points4;
    return run_e_host(ctx, E_POSE, xy1, xy2, n, K, nullptr, E, mask_in, dist, o);
}

extern "C" int pm_recover_pose_dev(pm_ctx* ctx, const pm_points_view* view, const pm_camera* K, const double* d_E,
                                   const uint8_t* d_mask_in, double dist, double* d_R, double* d_t, uint8_t* d_mask_out,
                                   int32_t* d_n_good, float* d_points4)
{
    PM_REQUIRE(d_E && d_R && d_t && d_mask_out && d_n_good, PM_E_INVALID, "null argument");
    float thr_n = 1.0f;
    int rc = check_camera(K, 1.0f, &thr_n);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(dist > 0.0, PM_E_INVALID, "dist must be > 0");
    rc = dev_prologue(ctx, view, nullptr);
    if (rc != PM_OK) return rc;
    return recover_pose_enqueue(ctx, *view, *K, d_E, d_mask_in, dist, d_R, d_t, d_mask_out, view->parts * view->cap, d_n_good,
                                d_points4);
}

extern "C" int pm_estimate_pose(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K,
                                const pm_ransac_params* p, double dist, double E[9], double R[9], double t[3], uint8_t* mask,
                                int* n_inliers, int* n_good, uint64_t* best_key)
{
    EHostOut o{};
    o.E = E; o.mask = mask; o.n_inliers = n_inliers; o.best_key = best_key; o.R = R; o.t = t; o.n_good = n_good;
    return run_e_host(ctx, E_RANSAC | E_POSE, xy1, xy2, n, K, p, nullptr, nullptr, dist, o);
}

// ---- absolute pose
extern "C" int pm_ransac_pnp(pm_ctx* ctx, const float* xyz, const float* uv, int n, const pm_camera* K,
                             const pm_ransac_params* p, double R[9], double t[3], uint8_t* mask, int* n_inliers,
                             uint64_t* best_key)
{
    PHostOut o{};
    o.R = R; o.t = t; o.mask = mask; o.n_inliers = n_inliers; o.best_key = best_key;
    return run_pnp_host(ctx, P_RANSAC, xyz, uv, n, K, p, nullptr, nullptr, nullptr, 0, o);
}

extern "C" int pm_ransac_pnp_from_hyp(pm_ctx* ctx, const float* xyz, const float* uv, int n, const pm_camera* K,
                                      const pm_ransac_params* p, int64_t hyp, double Rt[48], int32_t counts[4], int* n_models)
{
    PHostOut o{};
    o.Rt = Rt; o.counts = counts; o.n_models = n_models;
    pm_ransac_params q{};
    if (p) {
        q = *p;
        q.hyp_begin = hyp;
        q.hyp_end = hyp + 1;
    }
    return run_pnp_host(ctx, P_CANDIDATES, xyz, uv, n, K, p ? &q : nullptr, nullptr, nullptr, nullptr, 0, o);
}

extern "C" int pm_ransac_pnp_run_dev(pm_ctx* ctx, const pm_pnp_view* view, const pm_camera* K, const pm_ransac_params* p,
                                     uint64_t* d_best_key, double* d_Rt, uint8_t* d_mask, int mask_len, int32_t* d_n_inliers)
{
    PM_REQUIRE(d_best_key && d_Rt && d_mask && d_n_inliers, PM_E_INVALID, "null argument");
    PM_REQUIRE(mask_len >= 0, PM_E_INVALID, "mask_len must be >= 0");
    int rc = check_pnp(K, p);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(view != nullptr && view->xyz && view->uv && view->cap >= 1, PM_E_INVALID, "need a view with points and cap >= 1");
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    rc = pm::arena_reserve(ctx, pnp_scratch_bytes(ctx, p));
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    const pm_points_view v{view->xyz, view->uv, view->count, 1, view->cap, 0, 1, 0};
    return enqueue_pnp(ctx, v, *K, p, reinterpret_cast<unsigned long long*>(d_best_key), d_Rt, d_mask, mask_len, d_n_inliers);
}

extern "C" int pm_pnp_refine(pm_ctx* ctx, const float* xyz, const float* uv, int n, const pm_camera* K, const uint8_t* mask,
                             const double R_in[9], const double t_in[3], int max_iters, double R_out[9], double t_out[3],
                             pm_h_refine_info* info)
{
    PHostOut o{};
    o.R = R_out; o.t = t_out; o.info = info;
    return run_pnp_host(ctx, P_REFINE, xyz, uv, n, K, nullptr, mask, R_in, t_in, max_iters, o);
}

extern "C" int pm_pnp_refine_dev(pm_ctx* ctx, const pm_pnp_view* view, const pm_camera* K, const uint8_t* d_mask,
                                 const double* d_Rt_in, int max_iters, double* d_Rt_out, pm_h_refine_info* d_info)
{
    PM_REQUIRE(d_mask && d_Rt_in && d_Rt_out, PM_E_INVALID, "null argument");
    PM_REQUIRE(K != nullptr, PM_E_INVALID, "K is null");
    const bool fin = std::isfinite(K->fx) && std::isfinite(K->fy) && std::isfinite(K->cx) && std::isfinite(K->cy);
    PM_REQUIRE(fin && K->fx > 0.0 && K->fy > 0.0, PM_E_INVALID, "K needs finite values and fx, fy > 0");
    PM_REQUIRE(max_iters >= 0 && max_iters <= 100, PM_E_INVALID, "max_iters must lie in [0, 100]");
    PM_REQUIRE(view != nullptr && view->xyz && view->uv && view->cap >= 1, PM_E_INVALID, "need a view with points and cap >= 1");
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    const pm_points_view v{view->xyz, view->uv, view->count, 1, view->cap, 0, 1, 0};
    return pnp_refine_enqueue(ctx, v, *K, d_mask, d_Rt_in, max_iters, d_Rt_out, d_info);
}

extern "C" int pm_solve_pnp_ransac(pm_ctx* ctx, const float* xyz, const float* uv, int n, const pm_camera* K,
                                   const pm_ransac_params* p, int max_iters, double R[9], double t[3], uint8_t* mask,
                                   int* n_inliers, uint64_t* best_key, pm_h_refine_info* info)
{
    PHostOut o{};
    o.R = R; o.t = t; o.mask = mask; o.n_inliers = n_inliers; o.best_key = best_key; o.info = info;
    return run_pnp_host(ctx, P_RANSAC | P_REFINE, xyz, uv, n, K, p, nullptr, nullptr, nullptr, max_iters, o);
}

extern "C" int pm_gather_pnp_dev(pm_ctx* ctx, const pm_match* d_matches, const int32_t* d_count, int cap, const float* d_kp_xy,
                                 int n_kp, const float* d_obj_xyz, int n_obj, float* d_uv, float* d_xyz)
{
    PM_REQUIRE(d_matches && d_kp_xy && d_obj_xyz && d_uv && d_xyz, PM_E_INVALID, "null argument");
    PM_REQUIRE(cap >= 1 && n_kp >= 0 && n_obj >= 0, PM_E_INVALID, "need cap >= 1, n_kp >= 0, n_obj >= 0");
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    return gather_pnp_enqueue(ctx, d_matches, d_count, cap, d_kp_xy, n_kp, d_obj_xyz, n_obj, d_uv, d_xyz);
}
