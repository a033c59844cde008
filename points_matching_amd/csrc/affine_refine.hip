// affine_refine.hip — least-squares refit of a robust affine / similarity model on its inliers in ONE launch on gfx950
// (MI355X), docs/SPEC.md S30: the step cv::estimateAffine2D / estimateAffinePartial2D run after their RANSAC loop.
// Their Levenberg-Marquardt on the forward error approaches the exact minimiser [recalled]; the costs are quadratic in
// the six (four) parameters, so that minimiser is a closed-form least-squares fit.  The mask is not recomputed.
//
// One workgroup of HR_P = 512 threads, thread p owning partial p of S23's fixed reduction order (refine_reduce.hpp,
// shared with homography_refine.hip).  Three passes over the inliers, straight from global memory:
//   1. count, coordinate sums and the cost of A_in (6 sums);
//   2. the centred second moments (7 sums full, 3 partial), then the 2 x 2 cofactor solve in every thread;
//   3. the cost of the refit, which is kept only if it is not higher than A_in's.
// The launch keeps no per-call state, so the device form may be captured; the host forms (estimators.cpp)
// synchronise.
#include "affine_core.hpp"
#include "ransac_fused_kernels.hpp"
#include "refine_reduce.hpp"

namespace pm_arefine {
namespace {

using namespace pm_affine;
using pm_hrefine::HR_P;
using pm_hrefine::pass;
using pm_ransac::view_count1;
using pm_ransac::view_offsets;

constexpr double AR_DET_REL = 1e-12;     // S30: full refit only if det > AR_DET_REL * (Sxx * Syy)

// S30: squared forward residual of one correspondence under a[0..5].
__device__ __forceinline__ double cost_term(const double (&a)[6], double x, double y, double xp, double yp)
{
    const double ru = fma(a[0], x, fma(a[1], y, a[2])) - xp;
    const double rv = fma(a[3], x, fma(a[4], y, a[5])) - yp;
    return fma(ru, ru, rv * rv);
}

template <int MODEL>
__global__ __launch_bounds__(HR_P) void affine_refine(pm_points_view v, const uint8_t* mask, const double* A_in,
                                                      double* A_out, pm_h_refine_info* info)
{
    constexpr int MIN_PTS = Traits<MODEL>::MIN_PTS;
    constexpr int K2 = MODEL == FULL ? 7 : 3;
    __shared__ double s_x[pm_hrefine::HR_CH][HR_P / 2];
    __shared__ double s_red[8];
    __shared__ double s_ain[6];
    __shared__ int s_offs[PM_MAX_PARTS + 1];

    const int tid = threadIdx.x;
    int n;
    if (v.parts == 1) {
        n = view_count1(v);
    } else {
        view_offsets(v, s_offs, tid);
        n = 0;
    }
    if (tid < 6) s_ain[tid] = A_in[tid];     // read before any write: A_out may alias A_in
    __syncthreads();
    if (v.parts > 1) n = s_offs[v.parts];
    double ain[6];
    bool zero = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) { ain[i] = s_ain[i]; zero = zero && ain[i] == 0.0; }
    if (zero) {                              // S30 status 2: no model
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) A_out[i] = ain[i];
            if (info) *info = pm_h_refine_info{0.0, 0.0, 0, 0, 2, 0};
        }
        return;
    }

    // ---- pass 1: inlier count, coordinate sums, cost of A_in
    pass<6>(v, s_offs, n, mask, tid, s_x, s_red, [&](double (&a)[6], double x1, double y1, double x2, double y2) {
        a[0] = a[0] + 1.0;
        a[1] = a[1] + x1; a[2] = a[2] + y1; a[3] = a[3] + x2; a[4] = a[4] + y2;
        a[5] = a[5] + cost_term(ain, x1, y1, x2, y2);
    });
    const double nu = s_red[0], cost_in = s_red[5];
    const double cx1 = s_red[1] / nu, cy1 = s_red[2] / nu, cx2 = s_red[3] / nu, cy2 = s_red[4] / nu;

    // ---- pass 2: centred moments and the closed-form fit (every thread takes the same decisions)
    double aref[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool ok_ref = false;
    if (nu >= static_cast<double>(MIN_PTS)) {
        pass<K2>(v, s_offs, n, mask, tid, s_x, s_red, [&](double (&a)[K2], double x1, double y1, double x2, double y2) {
            const double dx = x1 - cx1, dy = y1 - cy1, ex = x2 - cx2, ey = y2 - cy2;
            if constexpr (MODEL == FULL) {
                a[0] = a[0] + dx * dx; a[1] = a[1] + dx * dy; a[2] = a[2] + dy * dy;
                a[3] = a[3] + dx * ex; a[4] = a[4] + dy * ex; a[5] = a[5] + dx * ey; a[6] = a[6] + dy * ey;
            } else {
                a[0] = a[0] + fma(dx, dx, dy * dy);
                a[1] = a[1] + fma(dx, ex, dy * ey);
                a[2] = a[2] + fma(dx, ey, -(dy * ex));
            }
        });
        if constexpr (MODEL == FULL) {
            const double sxx = s_red[0], sxy = s_red[1], syy = s_red[2];
            const double sxe = s_red[3], sye = s_red[4], sxf = s_red[5], syf = s_red[6];
            const double det = sxx * syy - sxy * sxy;
            if (det > AR_DET_REL * (sxx * syy) && det < __builtin_inf()) {
                const double idet = 1.0 / det;
                aref[0] = (sxe * syy - sye * sxy) * idet;
                aref[1] = (sxx * sye - sxy * sxe) * idet;
                aref[2] = cx2 - fma(aref[0], cx1, aref[1] * cy1);
                aref[3] = (sxf * syy - syf * sxy) * idet;
                aref[4] = (sxx * syf - sxy * sxf) * idet;
                aref[5] = cy2 - fma(aref[3], cx1, aref[4] * cy1);
                ok_ref = true;
            }
        } else {
            const double q = s_red[0];
            if (q > 0.0 && q < __builtin_inf()) {
                const double a = s_red[1] / q, b = s_red[2] / q;
                aref[0] = a; aref[1] = -b; aref[2] = cx2 - fma(a, cx1, -(b * cy1));
                aref[3] = b; aref[4] = a;  aref[5] = cy2 - fma(b, cx1, a * cy1);
                ok_ref = true;
            }
        }
    }

    // ---- pass 3: cost of the refit; kept iff cost_ref <= cost_in (NaN: no)
    double cost_out = cost_in;
    bool accepted = false;
    if (ok_ref) {
        pass<1>(v, s_offs, n, mask, tid, s_x, s_red, [&](double (&a)[1], double x1, double y1, double x2, double y2) {
            a[0] = a[0] + cost_term(aref, x1, y1, x2, y2);
        });
        const double cr = s_red[0];
        if (cr <= cost_in) { cost_out = cr; accepted = true; }
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) A_out[i] = accepted ? aref[i] : ain[i];
        if (info) *info = pm_h_refine_info{cost_in, cost_out, static_cast<int32_t>(nu), 0, accepted ? 0 : 1, 0};
    }
}

}  // namespace
}  // namespace pm_arefine

int pm_ransac::affine_refine_enqueue(pm_ctx* ctx, int model, const pm_points_view& v, const uint8_t* d_mask,
                                     const double* d_A_in, double* d_A_out, pm_h_refine_info* d_info)
{
    using namespace pm_arefine;
    pm::ScopedKernelTime t(ctx, "affine_refine");
    if (model == PM_AFFINE_FULL)
        hipLaunchKernelGGL(affine_refine<FULL>, dim3(1), dim3(HR_P), 0, ctx->stream, v, d_mask, d_A_in, d_A_out, d_info);
    else
        hipLaunchKernelGGL(affine_refine<PARTIAL>, dim3(1), dim3(HR_P), 0, ctx->stream, v, d_mask, d_A_in, d_A_out, d_info);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}
