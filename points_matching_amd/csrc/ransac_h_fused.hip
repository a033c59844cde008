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

// The homography policy of the LDS one-launch kernel (ransac_fused_kernels.hpp, ransac_fused_lds; FModel is the
// fundamental-matrix one).
struct HModel {
    static constexpr int MIN_PTS = 4;
    static constexpr bool SHARD_OUT = false;               // key, H, mask and count only
    static constexpr int OUT_WORDS = 9;
    static constexpr bool CANDIDATES = false;
    static constexpr int SYNC_WORD = SYNC_H;
    static constexpr const char* TIMER = "ransac_h_fused";

    // SPEC S19, S20: sample and solve hypothesis h.
    template <typename DIAG>
    static __device__ __forceinline__ bool solve(const pm_points_view& v, const int* __restrict__ offs, int n, uint64_t seed,
                                                 uint64_t h, double (&H)[9])
    {
        int idx[4];
        sample_walk<4, STREAM>(seed, h, n, idx);
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

}  // namespace

int ransac_h_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_ransac_params* p, unsigned long long* d_key,
                     double* d_H, uint8_t* d_mask, int mask_len, int* d_ninl)
{
    return fused_lds_enqueue<HModel>(ctx, v, p, d_key, d_H, d_mask, mask_len, d_ninl);
}

}  // namespace pm_ransac
