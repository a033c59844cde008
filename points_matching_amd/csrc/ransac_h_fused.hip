// ransac_h_fused.hip — RANSAC-H in ONE launch on gfx950 (MI355X): 4-sample + normalised 4-point DLT + reprojection
// scoring of every hypothesis against every correspondence + winner + inlier mask (docs/SPEC.md S19-S22).  The
// counterpart of cv::findHomography(pts1, pts2, RANSAC, thr), sibling of the findFundamentalMat call at main.cpp:95-98.
//
// The kernel is the default RANSAC-F launch, ransac_fused_lds (ransac_fused_kernels.hpp), with the homography policy
// HModel below:
//   * a workgroup owns `hb` consecutive hypothesis ids; lane s < hb of the first wave(s) samples and solves hypothesis s
//     (fp64, S20) while the other waves load the correspondences into LDS as packed pairs;
//   * 12 waves score WHOLE hypotheses (wave w: ids w, w + 12, ...): operands by ds_read_b64, model in SGPR pairs
//     feeding v_pk_fma_f32, verdicts counted on the scalar unit (s_bcnt1 of the ballot) — no atomics;
//   * each workgroup writes its best key (S22) and fp64 model to its slot and draws a ticket; the last one picks the
//     winner, publishes key / H / count and writes the mask.
#include "homography_core.hpp"
#include "ransac_fused_kernels.hpp"

namespace pm_ransac {
namespace {

using namespace pm_homog;

constexpr int RH_SYNC_WORD = 8;       // arrival ticket in ctx->sync_words (RANSAC-F uses words 0 and 2)

// The homography policy of the LDS one-launch kernel (ransac_fused_kernels.hpp, ransac_fused_lds; FModel is the
// fundamental-matrix one).
struct HModel {
    static constexpr int MIN_PTS = 4;
    static constexpr bool SHARD_OUT = false;               // key, H, mask and count only
    static constexpr int OUT_WORDS = 9;

    // SPEC S19, S20: sample and solve hypothesis h.
    template <typename DIAG>
    static __device__ __forceinline__ bool solve(const pm_points_view& v, const int* __restrict__ offs, int n, uint64_t seed,
                                                 uint64_t h, double (&H)[9])
    {
        int idx[4];
        sample4(seed, h, n, idx);
        double x1[4], y1[4], x2[4], y2[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float2 a, b;
            view_point(v, offs, idx[i], a, b);
            x1[i] = static_cast<double>(a.x); y1[i] = static_cast<double>(a.y);
            x2[i] = static_cast<double>(b.x); y2[i] = static_cast<double>(b.y);
        }
        return solve4(x1, y1, x2, y2, H);
    }

    // SPEC S21 on two correspondences, model in SGPR pairs (the packed form of inlier_h32, same operations bit for bit).
    // u, v, w use exactly the coefficient pairs of RANSAC-F's a, b, c.
    static __device__ __forceinline__ void inlier_pk(const ModelS& m, f32x2 x, f32x2 y, f32x2 xp, f32x2 yp, float thr2, bool& ia,
                                                     bool& ib)
    {
        const f32x2 u = sfma_out<0>(m.q03, x, sfma_in<0, 1>(m.q12, y));        // h0*x + (h1*y + h2)
        const f32x2 v = sfma_out<1>(m.q03, x, sfma_in<0, 1>(m.q45, y));        // h3*x + (h4*y + h5)
        const f32x2 w = sfma_out<1>(m.q36, x, sfma_in<0, 1>(m.q78, y));        // h6*x + (h7*y + h8)
        const f32x2 du = __builtin_elementwise_fma(-xp, w, u);
        const f32x2 dv = __builtin_elementwise_fma(-yp, w, v);
        const f32x2 lhs = __builtin_elementwise_fma(du, du, dv * dv);
        const f32x2 rhs = f32x2{thr2, thr2} * (w * w);
        ia = (lhs[0] <= rhs[0]) && __builtin_amdgcn_classf(rhs[0], CLASS_POS_FINITE);
        ib = (lhs[1] <= rhs[1]) && __builtin_amdgcn_classf(rhs[1], CLASS_POS_FINITE);
    }

    static __device__ __forceinline__ void inlier_x2(const float (&h)[9], f32x2 x, f32x2 y, f32x2 xp, f32x2 yp, float thr2,
                                                     bool& ia, bool& ib)
    {
        inlier_h32_x2(h, x, y, xp, yp, thr2, ia, ib);
    }
};

int check_params_h(const pm_ransac_params* p)
{
    PM_REQUIRE(p != nullptr, PM_E_INVALID, "params is null");
    PM_REQUIRE(p->hyp_begin >= 0 && p->hyp_end > p->hyp_begin && p->hyp_end <= 0x100000000LL, PM_E_INVALID,
               "hypothesis ids must satisfy 0 <= begin < end <= 2^32");
    PM_REQUIRE(p->hyp_end - p->hyp_begin <= 0x7FFFFFFFLL, PM_E_INVALID,
               "a single launch takes at most 2^31 - 1 hypothesis ids: split the range");
    PM_REQUIRE(p->error_kind == PM_ERR_REPROJ, PM_E_INVALID, "error_kind must be PM_ERR_REPROJ");
    return PM_OK;
}

// Enqueue the one-launch run.  The arena must already be reserved for fused_scratch_bytes(); it is carved here.
int h_launch(pm_ctx* ctx, const pm_points_view& v, const pm_ransac_params* p, unsigned long long* d_key, double* d_H,
             uint8_t* d_mask, int mask_len, int* d_ninl)
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
    out.key = d_key; out.F = d_H; out.mask = d_mask; out.mask_len = mask_len; out.n_inliers = d_ninl;
    pm::ScopedKernelTime t(ctx, "ransac_h_fused");
    return fused_lds_launch<HModel, NoDiag>(ctx, v, p, nwg, hb, slots, sync + RH_SYNC_WORD, out);
}

// Host-pointer driver of pm_ransac_homography (range) and pm_ransac_homography_from_hyp (the range [hyp, hyp + 1)).
int host_run_h(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_ransac_params* p, double H[9],
               uint8_t* mask, int* n_inliers, uint64_t* best_key)
{
    if (H) for (int i = 0; i < 9; ++i) H[i] = 0.0;
    if (mask && n > 0) memset(mask, 0, static_cast<size_t>(n));
    if (n_inliers) *n_inliers = 0;
    if (best_key) *best_key = 0;
    int rc = check_params_h(p);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(n >= 0 && (n == 0 || (xy1 && xy2)), PM_E_INVALID, "bad point arrays");
    if (n < 4) { pm::set_error("need at least 4 correspondences, got %d", n); return PM_E_TOO_FEW; }
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));

    const size_t xyb = sizeof(float) * 2 * static_cast<size_t>(n);
    const size_t need = 2 * pm::align_up(xyb, 256) + pm::align_up(static_cast<size_t>(n), 256) + 3 * 256 +
                        fused_scratch_bytes(ctx, p) + 2048;
    rc = pm::arena_reserve(ctx, need);
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    float* dxy1 = static_cast<float*>(pm::arena_take(ctx, xyb));
    float* dxy2 = static_cast<float*>(pm::arena_take(ctx, xyb));
    uint8_t* dmask = static_cast<uint8_t*>(pm::arena_take(ctx, static_cast<size_t>(n)));
    unsigned long long* dkey = static_cast<unsigned long long*>(pm::arena_take(ctx, 8));
    double* dH = static_cast<double*>(pm::arena_take(ctx, sizeof(double) * 9));
    int* dninl = static_cast<int*>(pm::arena_take(ctx, sizeof(int)));
    PM_REQUIRE(dxy1 && dxy2 && dmask && dkey && dH && dninl, PM_E_NOMEM, "scratch arena too small");
    constexpr size_t HP_MASK = 96;                           // pinned layout: key (8) | H (72) | count (4) | pad | mask
    rc = pm::pinned_reserve(ctx, HP_MASK + static_cast<size_t>(n));
    if (rc != PM_OK) return rc;

    PM_HIP_CHECK(hipMemcpyAsync(dxy1, xy1, xyb, hipMemcpyHostToDevice, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(dxy2, xy2, xyb, hipMemcpyHostToDevice, ctx->stream));
    const pm_points_view v{dxy1, dxy2, nullptr, 1, n, 0, 1, 0};
    rc = h_launch(ctx, v, p, dkey, dH, dmask, n, dninl);
    if (rc != PM_OK) return rc;
    char* hp = static_cast<char*>(ctx->pinned);
    unsigned long long* hkey = reinterpret_cast<unsigned long long*>(hp);
    double* hH = reinterpret_cast<double*>(hp + 8);
    int* hninl = reinterpret_cast<int*>(hp + 80);
    uint8_t* hmask = reinterpret_cast<uint8_t*>(hp + HP_MASK);
    PM_HIP_CHECK(hipMemcpyAsync(hkey, dkey, 8, hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(hH, dH, sizeof(double) * 9, hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(hninl, dninl, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(hmask, dmask, static_cast<size_t>(n), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (best_key) *best_key = *hkey;
    if (*hkey == 0ull) {
        pm::set_error("no valid model (all hypotheses degenerate)");
        return PM_E_NO_MODEL;
    }
    if (H) memcpy(H, hH, sizeof(double) * 9);
    if (mask) memcpy(mask, hmask, static_cast<size_t>(n));
    if (n_inliers) *n_inliers = *hninl;
    return PM_OK;
}

}  // namespace

// for pm_ransac_homography_refined (homography_refine.hip): RANSAC-H and the refinement on one stream, one synchronisation
int ransac_h_check(const pm_ransac_params* p) { return check_params_h(p); }
int ransac_h_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_ransac_params* p, unsigned long long* d_key,
                     double* d_H, uint8_t* d_mask, int mask_len, int* d_ninl)
{
    return h_launch(ctx, v, p, d_key, d_H, d_mask, mask_len, d_ninl);
}
}  // namespace pm_ransac

using namespace pm_ransac;

extern "C" int pm_ransac_homography(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_ransac_params* p,
                                    double H[9], uint8_t* mask, int* n_inliers, uint64_t* best_key)
{
    return host_run_h(ctx, xy1, xy2, n, p, H, mask, n_inliers, best_key);
}

extern "C" int pm_ransac_homography_from_hyp(pm_ctx* ctx, const float* xy1, const float* xy2, int n,
                                             const pm_ransac_params* p, int64_t hyp, double H[9], uint8_t* mask,
                                             int* n_inliers)
{
    if (H) for (int i = 0; i < 9; ++i) H[i] = 0.0;
    if (n_inliers) *n_inliers = 0;
    PM_REQUIRE(hyp >= 0 && hyp < 0x100000000LL, PM_E_INVALID, "hypothesis id must satisfy 0 <= hyp < 2^32");
    PM_REQUIRE(p != nullptr, PM_E_INVALID, "params is null");
    pm_ransac_params q = *p;
    q.hyp_begin = hyp;
    q.hyp_end = hyp + 1;
    return host_run_h(ctx, xy1, xy2, n, &q, H, mask, n_inliers, nullptr);
}

extern "C" int pm_ransac_homography_run_dev(pm_ctx* ctx, const pm_points_view* view, const pm_ransac_params* p,
                                            uint64_t* d_best_key, double* d_H, uint8_t* d_mask, int mask_len,
                                            int32_t* d_n_inliers)
{
    PM_REQUIRE(d_best_key && d_H && d_mask && d_n_inliers, PM_E_INVALID, "null argument");
    PM_REQUIRE(mask_len >= 0, PM_E_INVALID, "mask_len must be >= 0");
    int rc = check_params_h(p);
    if (rc != PM_OK) return rc;
    rc = check_view(view);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    rc = pm::arena_reserve(ctx, fused_scratch_bytes(ctx, p) + 1024);
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    return h_launch(ctx, *view, p, reinterpret_cast<unsigned long long*>(d_best_key), d_H, d_mask, mask_len, d_n_inliers);
}
