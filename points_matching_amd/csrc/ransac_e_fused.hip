// ransac_e_fused.hip — the scoring launch of RANSAC-E on gfx950 (MI355X): every candidate essential matrix of the
// 5-point solve (essential_solve.hip) against every K-normalised correspondence, winner, inlier mask (docs/SPEC.md S34).
//
// The kernel is the one-launch RANSAC-F scorer, ransac_fused_lds (ransac_fused_kernels.hpp), with the policy EModel:
//   * its "hypotheses" are model ids 10h + j (S33: up to 10 candidates per sample), so a launch over samples
//     [b, e) runs over ids [10b, 10e); the key (inliers << 32) | (0xFFFFFFFF - id) then needs 10e <= 2^32;
//   * load() reads candidate id from the solve launch's buffer instead of solving (CANDIDATES = true), and a wave
//     skips the ids whose valid flag is 0 — most slots of a sample are empty;
//   * the inlier test is S8 SAMPSON, FModel<PM_ERR_SAMPSON>'s packed form, on the normalised copy with the normalised
//     threshold (S31): OpenCV's EMEstimatorCallback error [recalled].
#include "ransac_fused_kernels.hpp"

namespace pm_ransac {
namespace {

struct EModel {
    static constexpr int MIN_PTS = 5;
    static constexpr bool SHARD_OUT = false;               // key, E, mask and count only
    static constexpr int OUT_WORDS = 9;
    static constexpr bool CANDIDATES = true;
    static constexpr int SYNC_WORD = SYNC_E;
    static constexpr const char* TIMER = "ransac_e_fused";

    // candidate k of the launch (id hyp_begin + k): 9 doubles and the valid flag
    static __device__ __forceinline__ bool load(const double* __restrict__ cand, int k, double (&E)[9])
    {
        const double* c = cand + 10 * static_cast<size_t>(k);
#pragma unroll
        for (int i = 0; i < 9; ++i) E[i] = c[i];
        return c[9] != 0.0;
    }
    static __device__ __forceinline__ void inlier_pk(const ModelS& m, f32x2 x, f32x2 y, f32x2 xp, f32x2 yp, float thr2, bool& ia,
                                                     bool& ib)
    {
        FModel<PM_ERR_SAMPSON>::inlier_pk(m, x, y, xp, yp, thr2, ia, ib);
    }
    static __device__ __forceinline__ void inlier_x2(const float (&f)[9], f32x2 x, f32x2 y, f32x2 xp, f32x2 yp, float thr2,
                                                     bool& ia, bool& ib)
    {
        FModel<PM_ERR_SAMPSON>::inlier_x2(f, x, y, xp, yp, thr2, ia, ib);
    }
};

}  // namespace

int ransac_e_enqueue(pm_ctx* ctx, const pm_points_view& vn, const pm_ransac_params* q, const double* d_cand,
                     unsigned long long* d_key, double* d_E, uint8_t* d_mask, int mask_len, int* d_ninl)
{
    return fused_lds_enqueue<EModel>(ctx, vn, q, d_key, d_E, d_mask, mask_len, d_ninl, d_cand);
}

}  // namespace pm_ransac
