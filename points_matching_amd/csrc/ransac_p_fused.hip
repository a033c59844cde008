// ransac_p_fused.hip — the scoring launch of RANSAC-PnP on gfx950 (MI355X): every candidate pose of the P3P solve
// (pnp_solve.hip) against every 2D-3D correspondence, winner, inlier mask (docs/SPEC.md S39).
//
// The kernel is the one-launch RANSAC-F scorer, ransac_fused_lds (ransac_fused_kernels.hpp), with the policy PModel:
//   * its "hypotheses" are model ids 4h + j (S38: up to 4 candidates per sample), so a launch over samples [b, e) runs
//     over ids [4b, 4e); the key (inliers << 32) | (0xFFFFFFFF - id) then needs 4e <= 2^32;
//   * its own LDS geometry (PnpGeom): a correspondence is 5 floats (X, Y, Z, u, v), so a 128-point slot holds 5 planes of
//     packed pairs (2.5 KiB) and the tile is 48 slots (120 KiB; with the 12-double models ~141 KiB of the CU's 160 KiB);
//   * load() reads candidate id from the solve launch's buffer (CANDIDATES = true): R, t for the winner and P32 =
//     (float)(K [R|t]) for the test, and a wave skips the ids whose valid flag is 0;
//   * the inlier test is S39's division-free reprojection test, the 12 entries of P32 in six SGPR pairs (the two
//     coefficients of every inner packed fma share a pair, as in FModel).
#include "pnp_core.hpp"
#include "ransac_fused_kernels.hpp"

namespace pm_ransac {
namespace {

struct PnpGeom {
    static constexpr bool OWN = true;
    static constexpr int PLANES = 5, MW = 16, FLAG = 12, WORDS = 12, MAX_SLOTS = 48;
};

__device__ __forceinline__ bool inlier1(const float (&P)[16], float x, float y, float z, float u, float v, float thr2)
{
    const float a = fmaf(P[0], x, fmaf(P[1], y, fmaf(P[2], z, P[3])));
    const float b = fmaf(P[4], x, fmaf(P[5], y, fmaf(P[6], z, P[7])));
    const float w = fmaf(P[8], x, fmaf(P[9], y, fmaf(P[10], z, P[11])));
    const float du = fmaf(-u, w, a), dv = fmaf(-v, w, b);
    const float lhs = fmaf(du, du, dv * dv), rhs = thr2 * (w * w);
    return lhs <= rhs && w > 0.0f && rhs > 0.0f && rhs < __builtin_inff();
}

// Regs, regs(), load() and mask_model() are Cand3x4's, on pnp_solve's slots: R, t for the winner, P32 for the test
struct PModel : Cand3x4<pm_pnp::SLOT_DOUBLES, pm_pnp::WORDS, pm_pnp::FLAG, pm_pnp::M32> {
    using Geom = PnpGeom;
    static constexpr int MIN_PTS = 4;
    static constexpr int OUT_WORDS = 12;
    static constexpr int SYNC_WORD = SYNC_P;
    static constexpr const char* TIMER = "ransac_p_fused";

    // points i0, i0 + 1 of the view (xy1: X Y Z, xy2: u v; NaN past n) as the 5 packed planes of one lane
    static __device__ __forceinline__ void load_pair(const pm_points_view& v, int n, int i0, f32x2* d)
    {
        const float nanv = __builtin_nanf("");
        float a[2][5];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int i = i0 + e;
            const int j = i < n ? i : (n > 0 ? n - 1 : 0);                // clamped loads, all in flight together
            const float* x = v.xy1 + 3 * static_cast<size_t>(j);
            const float2 q = *reinterpret_cast<const float2*>(v.xy2 + 2 * static_cast<size_t>(j));
            a[e][0] = x[0]; a[e][1] = x[1]; a[e][2] = x[2]; a[e][3] = q.x; a[e][4] = q.y;
            if (i >= n)
#pragma unroll
                for (int c = 0; c < 5; ++c) a[e][c] = nanv;
        }
#pragma unroll
        for (int c = 0; c < 5; ++c) d[64 * c] = f32x2{a[0][c], a[1][c]};
    }

    // SPEC S39 on two correspondences, P32 in SGPR pairs (the packed form of inlier1, same operations bit for bit)
    static __device__ __forceinline__ void inlier_pk(const Regs& m, const f32x2 (&op)[5], float thr2, bool& ia, bool& ib)
    {
        const f32x2 x = op[0], y = op[1], z = op[2], u = op[3], v = op[4];
        const f32x2 a = sfma_out<0>(m.q01, x, sfma_out<1>(m.q01, y, sfma_in<0, 1>(m.q23, z)));
        const f32x2 b = sfma_out<0>(m.q45, x, sfma_out<1>(m.q45, y, sfma_in<0, 1>(m.q67, z)));
        const f32x2 w = sfma_out<0>(m.q89, x, sfma_out<1>(m.q89, y, sfma_in<0, 1>(m.qab, z)));
        const f32x2 du = __builtin_elementwise_fma(-u, w, a), dv = __builtin_elementwise_fma(-v, w, b);
        const f32x2 lhs = __builtin_elementwise_fma(du, du, dv * dv);
        const f32x2 rhs = f32x2{thr2, thr2} * (w * w);
        ia = lhs[0] <= rhs[0] && w[0] > 0.0f && rhs[0] > 0.0f && rhs[0] < __builtin_inff();
        ib = lhs[1] <= rhs[1] && w[1] > 0.0f && rhs[1] > 0.0f && rhs[1] < __builtin_inff();
    }

    static __device__ __forceinline__ void inlier_x2(const float (&f)[16], const f32x2 (&op)[5], float thr2, bool& ia, bool& ib)
    {
        ia = inlier1(f, op[0][0], op[1][0], op[2][0], op[3][0], op[4][0], thr2);
        ib = inlier1(f, op[0][1], op[1][1], op[2][1], op[3][1], op[4][1], thr2);
    }
};

}  // namespace

int ransac_p_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_ransac_params* q, const double* d_cand,
                     unsigned long long* d_key, double* d_Rt, uint8_t* d_mask, int mask_len, int* d_ninl)
{
    return fused_lds_enqueue<PModel>(ctx, v, q, d_key, d_Rt, d_mask, mask_len, d_ninl, d_cand);
}

}  // namespace pm_ransac
