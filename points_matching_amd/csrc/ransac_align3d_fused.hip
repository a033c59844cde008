// ransac_align3d_fused.hip — the scoring launch of RANSAC over 3-D to 3-D correspondences on gfx950 (MI355X): every
// candidate transform of the triad solve (align3d_solve.hip) against every correspondence, winner, inlier mask
// (docs/SPEC.md S99, S100).
//
// The kernel is the one-launch RANSAC-F scorer, ransac_fused_lds (ransac_fused_kernels.hpp), with the policy XModel:
//   * one model per sample, so model ids are sample ids and the key (inliers << 32) | (0xFFFFFFFF - h) needs
//     hyp_end <= 2^32;
//   * its own LDS geometry (XyzGeom): a correspondence is 6 floats (x1 y1 z1 x2 y2 z2), so a 128-point slot holds 6 planes
//     of packed pairs (3 KiB) and the tile is 40 slots (120 KiB, PnP's figure; with the 13-double models ~143 KiB of the
//     CU's 160 KiB);
//   * load() reads candidate id from the solve launch's buffer (CANDIDATES = true): R, t, s for the winner and M32 =
//     (float)(s R | t) for the test, and a wave skips the ids whose valid flag is 0;
//   * the inlier test is S99's squared distance |M x1 + t - x2|^2 <= thr^2, the 12 entries of M32 in six SGPR pairs (the
//     two coefficients of every inner packed fma share a pair, as in PModel).
#include "align3d_core.hpp"
#include "ransac_fused_kernels.hpp"

namespace pm_ransac {
namespace {

struct XyzGeom {
    static constexpr bool OWN = true;
    static constexpr int PLANES = 6, MW = 16, FLAG = 12, WORDS = 13, MAX_SLOTS = 40;
};
// dynamic tile + the kernel's static arrays (s_mdl, s_m64, s_cnt, s_offs, s_wk, s_F64, s_role, s_wc) within the CU's LDS
constexpr size_t RX_LDS_DYNAMIC = static_cast<size_t>(XyzGeom::MAX_SLOTS) * XyzGeom::PLANES * 64 * sizeof(f32x2);
constexpr size_t RX_LDS_STATIC = RF_HB_MAX * (XyzGeom::MW * sizeof(float) + XyzGeom::WORDS * sizeof(double) + sizeof(int)) +
                                 (PM_MAX_PARTS + 1) * sizeof(int) + RL_WAVES * (sizeof(unsigned long long) + sizeof(int)) +
                                 XyzGeom::WORDS * sizeof(double) + sizeof(int);
static_assert(RX_LDS_DYNAMIC + RX_LDS_STATIC + 1024 < 160 * 1024, "tile + models exceed the LDS of a CU");

__device__ __forceinline__ bool inlier1(const float (&P)[16], float x, float y, float z, float u, float v, float w, float thr2)
{
    const float ra = fmaf(P[0], x, fmaf(P[1], y, fmaf(P[2], z, P[3]))) - u;
    const float rb = fmaf(P[4], x, fmaf(P[5], y, fmaf(P[6], z, P[7]))) - v;
    const float rc = fmaf(P[8], x, fmaf(P[9], y, fmaf(P[10], z, P[11]))) - w;
    const float d2 = fmaf(ra, ra, fmaf(rb, rb, rc * rc));
    return d2 <= thr2 && d2 < __builtin_inff();
}

// Regs, regs(), load() and mask_model() are Cand3x4's, on align3d_solve's slots: R, t, s for the winner, M32 for the test
struct XModel : Cand3x4<pm_align3d::SLOT_DOUBLES, pm_align3d::WORDS, pm_align3d::FLAG, pm_align3d::M32> {
    using Geom = XyzGeom;
    static constexpr int MIN_PTS = 3;
    static constexpr int OUT_WORDS = 13;
    static constexpr int SYNC_WORD = SYNC_X;
    static constexpr const char* TIMER = "ransac_align3d_fused";

    // rows i0, i0 + 1 of the view (xy1, xy2: 3 floats each; NaN past n) as the 6 packed planes of one lane
    static __device__ __forceinline__ void load_pair(const pm_points_view& v, int n, int i0, f32x2* d)
    {
        const float nanv = __builtin_nanf("");
        float a[2][6];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int i = i0 + e;
            const int j = i < n ? i : (n > 0 ? n - 1 : 0);                // clamped loads, all in flight together
            const float* x = v.xy1 + 3 * static_cast<size_t>(j);
            const float* y = v.xy2 + 3 * static_cast<size_t>(j);
            a[e][0] = x[0]; a[e][1] = x[1]; a[e][2] = x[2]; a[e][3] = y[0]; a[e][4] = y[1]; a[e][5] = y[2];
            if (i >= n)
#pragma unroll
                for (int c = 0; c < 6; ++c) a[e][c] = nanv;
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) d[64 * c] = f32x2{a[0][c], a[1][c]};
    }

    // SPEC S99 on two correspondences, M32 in SGPR pairs (the packed form of inlier1, same operations bit for bit)
    static __device__ __forceinline__ void inlier_pk(const Regs& m, const f32x2 (&op)[6], float thr2, bool& ia, bool& ib)
    {
        const f32x2 x = op[0], y = op[1], z = op[2];
        const f32x2 ra = sfma_out<0>(m.q01, x, sfma_out<1>(m.q01, y, sfma_in<0, 1>(m.q23, z))) - op[3];
        const f32x2 rb = sfma_out<0>(m.q45, x, sfma_out<1>(m.q45, y, sfma_in<0, 1>(m.q67, z))) - op[4];
        const f32x2 rc = sfma_out<0>(m.q89, x, sfma_out<1>(m.q89, y, sfma_in<0, 1>(m.qab, z))) - op[5];
        const f32x2 d2 = __builtin_elementwise_fma(ra, ra, __builtin_elementwise_fma(rb, rb, rc * rc));
        ia = d2[0] <= thr2 && d2[0] < __builtin_inff();
        ib = d2[1] <= thr2 && d2[1] < __builtin_inff();
    }

    static __device__ __forceinline__ void inlier_x2(const float (&f)[16], const f32x2 (&op)[6], float thr2, bool& ia, bool& ib)
    {
        ia = inlier1(f, op[0][0], op[1][0], op[2][0], op[3][0], op[4][0], op[5][0], thr2);
        ib = inlier1(f, op[0][1], op[1][1], op[2][1], op[3][1], op[4][1], op[5][1], thr2);
    }
};

}  // namespace

int ransac_align3d_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_ransac_params* q, const double* d_cand,
                           unsigned long long* d_key, double* d_T, uint8_t* d_mask, int mask_len, int* d_ninl)
{
    return fused_lds_enqueue<XModel>(ctx, v, q, d_key, d_T, d_mask, mask_len, d_ninl, d_cand);
}

}  // namespace pm_ransac
