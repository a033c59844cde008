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

// The affine policies of the LDS one-launch kernel (ransac_fused_kernels.hpp, ransac_fused_lds).  Models are carried
// as 9 doubles [a0 .. a5, 0, 0, 1]; the kernel publishes the first OUT_WORDS = 6.
template <int MODEL>
struct AModel {
    static constexpr int MIN_PTS = Traits<MODEL>::MIN_PTS;
    static constexpr bool SHARD_OUT = false;               // key, A, mask and count only
    static constexpr int OUT_WORDS = 6;
    static constexpr bool CANDIDATES = false;
    static constexpr int SYNC_WORD = SYNC_A;
    static constexpr const char* TIMER = "ransac_a_fused";

    // SPEC S26, S27: sample and solve hypothesis h.
    template <typename DIAG>
    static __device__ __forceinline__ bool solve(const pm_points_view& v, const int* __restrict__ offs, int n, uint64_t seed,
                                                 uint64_t h, double (&A)[9])
    {
        int idx[MIN_PTS];
        sample_walk<MIN_PTS, Traits<MODEL>::STREAM>(seed, h, n, idx);
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

}  // namespace

int ransac_a_enqueue(pm_ctx* ctx, int model, const pm_points_view& v, const pm_ransac_params* p, unsigned long long* d_key,
                     double* d_A, uint8_t* d_mask, int mask_len, int* d_ninl)
{
    if (model == PM_AFFINE_FULL)
        return fused_lds_enqueue<AModel<FULL>>(ctx, v, p, d_key, d_A, d_mask, mask_len, d_ninl);
    return fused_lds_enqueue<AModel<PARTIAL>>(ctx, v, p, d_key, d_A, d_mask, mask_len, d_ninl);
}

}  // namespace pm_ransac
