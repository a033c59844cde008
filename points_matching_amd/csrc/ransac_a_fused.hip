// ransac_a_fused.hip — robust 2D affine / similarity estimation in ONE launch on gfx950 (MI355X): 3- or 2-sample +
// closed-form fp64 minimal solve + forward-residual scoring of every hypothesis against every correspondence + winner +
// inlier mask (docs/SPEC.md S26-S29).  The counterparts of cv::estimateAffine2D and cv::estimateAffinePartial2D.
//
// The kernel is the default RANSAC-F launch, ransac_fused_lds (ransac_fused_kernels.hpp), with the affine policies
// AModel<FULL | PARTIAL> below, exactly as RANSAC-H uses it with HModel:
//   * a workgroup owns `hb` consecutive hypothesis ids; lane s < hb of the first wave(s) samples and solves hypothesis s
//     (fp64, S27: a few dozen operations) while the other waves load the correspondences into LDS as packed pairs;
//   * 12 waves score WHOLE hypotheses: operands by ds_read_b64, the six coefficients in SGPR pairs feeding
//     v_pk_fma_f32 (the pairs of H's u and v rows), the 14-flop S28 test, verdicts counted on the scalar unit;
//   * the last workgroup picks the winner and publishes key / A (6 doubles) / count and the mask.
#include "affine_core.hpp"
#include "ransac_fused_kernels.hpp"

namespace pm_ransac {
namespace {

using namespace pm_affine;

constexpr int RA_SYNC_WORD = 12;      // arrival ticket in ctx->sync_words (RANSAC-F uses words 0 and 2, RANSAC-H word 8)

// The affine policies of the LDS one-launch kernel (ransac_fused_kernels.hpp, ransac_fused_lds).  Models are carried
// as 9 doubles [a0 .. a5, 0, 0, 1]; the kernel publishes the first OUT_WORDS = 6.
template <int MODEL>
struct AModel {
    static constexpr int MIN_PTS = Traits<MODEL>::MIN_PTS;
    static constexpr bool SHARD_OUT = false;               // key, A, mask and count only
    static constexpr int OUT_WORDS = 6;

    // SPEC S26, S27: sample and solve hypothesis h.
    template <typename DIAG>
    static __device__ __forceinline__ bool solve(const pm_points_view& v, const int* __restrict__ offs, int n, uint64_t seed,
                                                 uint64_t h, double (&A)[9])
    {
        int idx[MIN_PTS];
        sample<MODEL>(seed, h, n, idx);
        double x1[MIN_PTS], y1[MIN_PTS], x2[MIN_PTS], y2[MIN_PTS];
#pragma unroll
        for (int i = 0; i < MIN_PTS; ++i) {
            float2 a, b;
            view_point(v, offs, idx[i], a, b);
            x1[i] = static_cast<double>(a.x); y1[i] = static_cast<double>(a.y);
            x2[i] = static_cast<double>(b.x); y2[i] = static_cast<double>(b.y);
        }
        if constexpr (MODEL == FULL) return solve3(x1, y1, x2, y2, A);
        else return solve2(x1, y1, x2, y2, A);
    }

    // SPEC S28 on two correspondences, model in SGPR pairs (the packed form of inlier_a32, same operations bit for bit).
    // u and v use exactly the coefficient pairs of RANSAC-H's u and v; the threshold check is uniform (hoisted).
    static __device__ __forceinline__ void inlier_pk(const ModelS& m, f32x2 x, f32x2 y, f32x2 xp, f32x2 yp, float thr2, bool& ia,
                                                     bool& ib)
    {
        const f32x2 u = sfma_out<0>(m.q03, x, sfma_in<0, 1>(m.q12, y));        // a0*x + (a1*y + a2)
        const f32x2 v = sfma_out<1>(m.q03, x, sfma_in<0, 1>(m.q45, y));        // a3*x + (a4*y + a5)
        const f32x2 du = u - xp, dv = v - yp;
        const f32x2 lhs = __builtin_elementwise_fma(du, du, dv * dv);
        const float t = thr_or_nan(thr2);
        ia = lhs[0] <= t;
        ib = lhs[1] <= t;
    }

    static __device__ __forceinline__ void inlier_x2(const float (&a)[9], f32x2 x, f32x2 y, f32x2 xp, f32x2 yp, float thr2,
                                                     bool& ia, bool& ib)
    {
        inlier_a32_x2(a, x, y, xp, yp, thr2, ia, ib);
    }
};

int check_model(int model)
{
    PM_REQUIRE(model == PM_AFFINE_FULL || model == PM_AFFINE_PARTIAL, PM_E_INVALID,
               "model must be PM_AFFINE_FULL or PM_AFFINE_PARTIAL");
    return PM_OK;
}

int min_pts(int model) { return model == PM_AFFINE_FULL ? Traits<FULL>::MIN_PTS : Traits<PARTIAL>::MIN_PTS; }

// Enqueue the one-launch run.  The arena must already be reserved for fused_scratch_bytes(); it is carved here.
int a_launch(pm_ctx* ctx, int model, const pm_points_view& v, const pm_ransac_params* p, unsigned long long* d_key,
             double* d_A, uint8_t* d_mask, int mask_len, int* d_ninl)
{
    const long long nh = p->hyp_end - p->hyp_begin;
    const int hb = fused_hb(ctx, nh);
    const int nwg = static_cast<int>((nh + hb - 1) / hb);
    RfSlot* slots = static_cast<RfSlot*>(pm::arena_take(ctx, sizeof(RfSlot) * static_cast<size_t>(nwg)));
    PM_REQUIRE(slots, PM_E_NOMEM, "scratch arena too small");
    int* sync = nullptr;
    int rc = sync_words(ctx, &sync);
    if (rc != PM_OK) return rc;
    RfOut out{};
    out.key = d_key; out.F = d_A; out.mask = d_mask; out.mask_len = mask_len; out.n_inliers = d_ninl;
    pm::ScopedKernelTime t(ctx, "ransac_a_fused");
    if (model == PM_AFFINE_FULL) return fused_lds_launch<AModel<FULL>, NoDiag>(ctx, v, p, nwg, hb, slots, sync + RA_SYNC_WORD, out);
    return fused_lds_launch<AModel<PARTIAL>, NoDiag>(ctx, v, p, nwg, hb, slots, sync + RA_SYNC_WORD, out);
}

// Host-pointer driver of pm_ransac_affine (range), pm_ransac_affine_from_hyp (the range [hyp, hyp + 1)) and
// pm_estimate_affine (refine != 0: the refit of affine_refine.hip follows on the same stream; one synchronisation).
int host_run_a(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n, const pm_ransac_params* p, int refine,
               double A[6], uint8_t* mask, int* n_inliers, uint64_t* best_key, pm_h_refine_info* info)
{
    if (A) for (int i = 0; i < 6; ++i) A[i] = 0.0;
    if (mask && n > 0) memset(mask, 0, static_cast<size_t>(n));
    if (n_inliers) *n_inliers = 0;
    if (best_key) *best_key = 0;
    if (info) *info = pm_h_refine_info{0.0, 0.0, 0, 0, 2, 0};
    int rc = check_model(model);
    if (rc != PM_OK) return rc;
    rc = ransac_h_check(p);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(n >= 0 && (n == 0 || (xy1 && xy2)), PM_E_INVALID, "bad point arrays");
    if (n < min_pts(model)) { pm::set_error("need at least %d correspondences, got %d", min_pts(model), n); return PM_E_TOO_FEW; }
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));

    const size_t xyb = sizeof(float) * 2 * static_cast<size_t>(n);
    const size_t need = 2 * pm::align_up(xyb, 256) + pm::align_up(static_cast<size_t>(n), 256) + 6 * 256 +
                        fused_scratch_bytes(ctx, p) + 2048;
    rc = pm::arena_reserve(ctx, need);
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    float* dxy1 = static_cast<float*>(pm::arena_take(ctx, xyb));
    float* dxy2 = static_cast<float*>(pm::arena_take(ctx, xyb));
    uint8_t* dmask = static_cast<uint8_t*>(pm::arena_take(ctx, static_cast<size_t>(n)));
    unsigned long long* dkey = static_cast<unsigned long long*>(pm::arena_take(ctx, 8));
    double* dA = static_cast<double*>(pm::arena_take(ctx, sizeof(double) * 6));
    int* dninl = static_cast<int*>(pm::arena_take(ctx, sizeof(int)));
    pm_h_refine_info* dinfo = static_cast<pm_h_refine_info*>(pm::arena_take(ctx, sizeof(pm_h_refine_info)));
    PM_REQUIRE(dxy1 && dxy2 && dmask && dkey && dA && dninl && dinfo, PM_E_NOMEM, "scratch arena too small");
    constexpr size_t HP_INFO = 64, HP_MASK = 96;    // pinned layout: key (8) | A (48) | count (4) | pad | info (32) | mask
    rc = pm::pinned_reserve(ctx, HP_MASK + static_cast<size_t>(n));
    if (rc != PM_OK) return rc;

    PM_HIP_CHECK(hipMemcpyAsync(dxy1, xy1, xyb, hipMemcpyHostToDevice, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(dxy2, xy2, xyb, hipMemcpyHostToDevice, ctx->stream));
    const pm_points_view v{dxy1, dxy2, nullptr, 1, n, 0, 1, 0};
    rc = a_launch(ctx, model, v, p, dkey, dA, dmask, n, dninl);
    if (rc != PM_OK) return rc;
    if (refine) {
        rc = affine_refine_enqueue(ctx, model, v, dmask, dA, dA, dinfo);
        if (rc != PM_OK) return rc;
    }
    char* hp = static_cast<char*>(ctx->pinned);
    unsigned long long* hkey = reinterpret_cast<unsigned long long*>(hp);
    double* hA = reinterpret_cast<double*>(hp + 8);
    int* hninl = reinterpret_cast<int*>(hp + 56);
    uint8_t* hmask = reinterpret_cast<uint8_t*>(hp + HP_MASK);
    PM_HIP_CHECK(hipMemcpyAsync(hkey, dkey, 8, hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(hA, dA, sizeof(double) * 6, hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(hninl, dninl, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (refine)
        PM_HIP_CHECK(hipMemcpyAsync(hp + HP_INFO, dinfo, sizeof(pm_h_refine_info), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(hmask, dmask, static_cast<size_t>(n), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (best_key) *best_key = *hkey;
    if (info) {
        if (refine) memcpy(info, hp + HP_INFO, sizeof(pm_h_refine_info));
        else *info = pm_h_refine_info{0.0, 0.0, 0, 0, *hkey ? 1 : 2, 0};
    }
    if (*hkey == 0ull) {
        pm::set_error("no valid model (all hypotheses degenerate)");
        return PM_E_NO_MODEL;
    }
    if (A) memcpy(A, hA, sizeof(double) * 6);
    if (mask) memcpy(mask, hmask, static_cast<size_t>(n));
    if (n_inliers) *n_inliers = *hninl;
    return PM_OK;
}

}  // namespace

// for affine_refine.hip: the model check and sample size shared by every affine entry point
int ransac_a_check_model(int model) { return check_model(model); }
int ransac_a_min_pts(int model) { return min_pts(model); }
}  // namespace pm_ransac

using namespace pm_ransac;

extern "C" int pm_ransac_affine(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n, const pm_ransac_params* p,
                                double A[6], uint8_t* mask, int* n_inliers, uint64_t* best_key)
{
    return host_run_a(ctx, model, xy1, xy2, n, p, 0, A, mask, n_inliers, best_key, nullptr);
}

extern "C" int pm_ransac_affine_from_hyp(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n,
                                         const pm_ransac_params* p, int64_t hyp, double A[6], uint8_t* mask, int* n_inliers)
{
    if (A) for (int i = 0; i < 6; ++i) A[i] = 0.0;
    if (n_inliers) *n_inliers = 0;
    PM_REQUIRE(hyp >= 0 && hyp < 0x100000000LL, PM_E_INVALID, "hypothesis id must satisfy 0 <= hyp < 2^32");
    PM_REQUIRE(p != nullptr, PM_E_INVALID, "params is null");
    pm_ransac_params q = *p;
    q.hyp_begin = hyp;
    q.hyp_end = hyp + 1;
    return host_run_a(ctx, model, xy1, xy2, n, &q, 0, A, mask, n_inliers, nullptr, nullptr);
}

extern "C" int pm_ransac_affine_run_dev(pm_ctx* ctx, int model, const pm_points_view* view, const pm_ransac_params* p,
                                        uint64_t* d_best_key, double* d_A, uint8_t* d_mask, int mask_len,
                                        int32_t* d_n_inliers)
{
    PM_REQUIRE(d_best_key && d_A && d_mask && d_n_inliers, PM_E_INVALID, "null argument");
    PM_REQUIRE(mask_len >= 0, PM_E_INVALID, "mask_len must be >= 0");
    int rc = check_model(model);
    if (rc != PM_OK) return rc;
    rc = ransac_h_check(p);
    if (rc != PM_OK) return rc;
    rc = check_view(view);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    rc = pm::arena_reserve(ctx, fused_scratch_bytes(ctx, p) + 1024);
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    return a_launch(ctx, model, *view, p, reinterpret_cast<unsigned long long*>(d_best_key), d_A, d_mask, mask_len,
                    d_n_inliers);
}

extern "C" int pm_estimate_affine(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n,
                                  const pm_ransac_params* p, int refine, double A[6], uint8_t* mask, int* n_inliers,
                                  uint64_t* best_key, pm_h_refine_info* info)
{
    return host_run_a(ctx, model, xy1, xy2, n, p, refine, A, mask, n_inliers, best_key, info);
}
