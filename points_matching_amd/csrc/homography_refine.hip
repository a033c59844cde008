// homography_refine.hip — refinement of a robust homography on its inliers in ONE launch on gfx950 (MI355X): the
// least-squares DLT refit over all inliers (docs/SPEC.md S23) and Levenberg-Marquardt on the forward transfer error
// (S24), the two steps cv::findHomography runs after its RANSAC loop.  The mask is not recomputed (S25).
//
// One workgroup of HR_P = 512 threads (8 waves).  Thread p owns partial p of S23's fixed reduction order: it walks the
// correspondences i = p, p + 512, ... of the view straight from global memory (32 768 points are 512 KB, more than
// LDS), skips the ones the mask rejects and keeps its partial sums in fp64 registers (45 in the widest pass).  The
// stride-halving tree runs its three cross-wave steps through LDS, HR_CH accumulators at a time, and its six in-wave
// steps with cross-lane moves.  Between passes, every thread reads the sums back from LDS and takes the same control
// decisions; the Jacobi eigen-solve runs lane-parallel in wave 0, the 8 x 8 Cholesky of each LM step (S24's lm_solve_n,
// lm_core.hpp) in thread 0.
// Passes: sums + cost of H_in, centroid distances, normal matrix, cost of the refit, then the LM passes (one at the
// start point, one per iteration).
//
// The launch keeps no per-call state, so the device form may be captured; the host forms (estimators.cpp)
// synchronise.
#include "homography_core.hpp"
#include "homography_refine_core.hpp"
#include "lm_core.hpp"
#include "ransac_fused_kernels.hpp"
#include "refine_reduce.hpp"

namespace pm_hrefine {
namespace {

using pm_homog::denormalise;
using pm_ransac::scale_sign;
using pm_ransac::view_count1;
using pm_ransac::view_offsets;

__global__ __launch_bounds__(HR_P) void homography_refine(pm_points_view v, const uint8_t* mask, const double* H_in,
                                                          int max_iters, double* H_out, pm_h_refine_info* info)
{
    __shared__ double s_x[HR_CH][HR_P / 2];
    __shared__ double s_red[HR_LM];
    __shared__ double s_jtjg[44];            // J^T J and J^T r at the current LM point
    __shared__ double s_hin[9];
    __shared__ double s_hn[9];
    __shared__ double s_start[9];         // S24 start point
    __shared__ double s_h[9];             // current LM point (h[8] = 1)
    __shared__ double s_d[8];             // LM step
    __shared__ int s_jok;                 // Jacobi / Cholesky succeeded
    __shared__ int s_offs[PM_MAX_PARTS + 1];

    const int tid = threadIdx.x, lane = tid & 63;
    int n;
    if (v.parts == 1) {
        n = view_count1(v);
    } else {
        view_offsets(v, s_offs, tid);
        n = 0;
    }
    if (tid < 9) s_hin[tid] = H_in[tid];     // read before any write: H_out may alias H_in
    __syncthreads();
    if (v.parts > 1) n = s_offs[v.parts];
    double hin[9];
    bool zero = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) { hin[i] = s_hin[i]; zero = zero && hin[i] == 0.0; }
    if (zero) {                              // S25 status 2: no model
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) H_out[i] = hin[i];
            if (info) *info = pm_h_refine_info{0.0, 0.0, 0, 0, 2, 0};
        }
        return;
    }

    // ---- S23 pass 1: inlier count, coordinate sums, cost of H_in
    pass<6>(v, s_offs, n, mask, tid, s_x, s_red, [&](double (&a)[6], double x1, double y1, double x2, double y2) {
        a[0] = a[0] + 1.0;
        a[1] = a[1] + x1; a[2] = a[2] + y1; a[3] = a[3] + x2; a[4] = a[4] + y2;
        a[5] = a[5] + cost_term(hin, x1, y1, x2, y2);
    });
    const double nu = s_red[0], cost_in = s_red[5];
    const double cx1 = s_red[1] / nu, cy1 = s_red[2] / nu, cx2 = s_red[3] / nu, cy2 = s_red[4] / nu;

    // ---- S23 refit: Hartley normalisation, normal matrix, Jacobi, denormalisation
    double href[9];
    bool ok_ref = false;
    if (nu >= 4.0) {
        pass<2>(v, s_offs, n, mask, tid, s_x, s_red, [&](double (&a)[2], double x1, double y1, double x2, double y2) {
            const double dx1 = x1 - cx1, dy1 = y1 - cy1, dx2 = x2 - cx2, dy2 = y2 - cy2;
            a[0] = a[0] + sqrt(fma(dx1, dx1, dy1 * dy1));
            a[1] = a[1] + sqrt(fma(dx2, dx2, dy2 * dy2));
        });
        const double md1 = s_red[0] / nu, md2 = s_red[1] / nu;
        if (md1 > 0.0 && md1 < __builtin_inf() && md2 > 0.0 && md2 < __builtin_inf()) {
            const double s1 = 1.4142135623730951 / md1, s2 = 1.4142135623730951 / md2;
            pass<HR_NORMAL>(v, s_offs, n, mask, tid, s_x, s_red,
                            [&](double (&a)[HR_NORMAL], double x1, double y1, double x2, double y2) {
                                normal_term(a, (x1 - cx1) * s1, (y1 - cy1) * s1, (x2 - cx2) * s2, (y2 - cy2) * s2);
                            });
            if (tid < 64) {                  // wave 0
                double hk;
                const bool ok = jacobi_min_wave(s_red, lane, hk);
                if (lane < 9) s_hn[lane] = hk;
                if (lane == 0) s_jok = ok ? 1 : 0;
            }
            __syncthreads();
            if (s_jok) {
                double hn[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) hn[i] = s_hn[i];
                ok_ref = denormalise(hn, s1, -(s1 * cx1), -(s1 * cy1), s2, -(s2 * cx2), -(s2 * cy2), href);
            }
        }
    }

    // ---- S24 start point: the refit if its cost is not higher than H_in's (kept in LDS: few registers stay free
    // next to the 45 accumulators of the LM passes)
    double cost_start = cost_in;
    bool from_ref = false;
    if (ok_ref) {
        pass<1>(v, s_offs, n, mask, tid, s_x, s_red, [&](double (&a)[1], double x1, double y1, double x2, double y2) {
            a[0] = a[0] + cost_term(href, x1, y1, x2, y2);
        });
        const double cr = s_red[0];
        if (cr <= cost_in) { cost_start = cr; from_ref = true; }
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) s_start[i] = from_ref ? href[i] : s_hin[i];
    }
    __syncthreads();

    // ---- S24 LM: one pass per iteration at the trial point; the current point h and its J^T J, J^T r stay in LDS
    double cur = cost_start;
    int iters = 0;
    bool accepted = false;
    if (nu >= 4.0 && max_iters > 0 && fabs(s_start[8]) >= HR_MIN_H8) {
        {
            double h[9];
#pragma unroll
            for (int i = 0; i < 8; ++i) h[i] = s_start[i] / s_start[8];
            h[8] = 1.0;
            pass<HR_LM>(v, s_offs, n, mask, tid, s_x, s_red,
                        [&](double (&a)[HR_LM], double x1, double y1, double x2, double y2) { lm_term(a, h, x1, y1, x2, y2); });
            if (tid < 44) s_jtjg[tid] = s_red[tid];
            if (tid == 0) {
#pragma unroll
                for (int i = 0; i < 9; ++i) s_h[i] = h[i];
            }
            __syncthreads();
        }
        double lam = LM_LAMBDA0;
        for (int it = 0; it < max_iters; ++it) {
            if (tid == 0) [[clang::noinline]] s_jok = lm_solve_n<8>(s_jtjg, s_jtjg + 36, lam, s_d) ? 1 : 0;
            __syncthreads();
            if (!s_jok) break;
            double dmax = 0.0, hmax = 1.0;
            double ht[9];
#pragma unroll
            for (int i = 0; i < 8; ++i) {        // NaN propagates into dmax and stops the loop
                const double hi = s_h[i], di = s_d[i];
                if (!(fabs(di) <= dmax)) dmax = fabs(di);
                if (!(fabs(hi) <= hmax)) hmax = fabs(hi);
                ht[i] = hi + di;
            }
            ht[8] = 1.0;
            if (!(dmax > LM_STEP_TOL * hmax)) break;
            pass<HR_LM>(v, s_offs, n, mask, tid, s_x, s_red,
                        [&](double (&a)[HR_LM], double x1, double y1, double x2, double y2) { lm_term(a, ht, x1, y1, x2, y2); });
            ++iters;
            const double ct = s_red[HR_LM - 1];
            if (ct < cur) {
                cur = ct;
                lam = lam / 10.0;
                accepted = true;
                if (tid < 44) s_jtjg[tid] = s_red[tid];
                if (tid == 0) {
#pragma unroll
                    for (int i = 0; i < 9; ++i) s_h[i] = ht[i];
                }
                __syncthreads();
            } else {
                lam = lam * 10.0;
            }
        }
    }

    // ---- S25 result (thread 0)
    if (tid == 0) {
        double out[9], h[9];
        double cost_out = cost_start;
#pragma unroll
        for (int i = 0; i < 9; ++i) { out[i] = s_start[i]; h[i] = s_h[i]; }
        if (accepted) {
            if (scale_sign(h, out)) cost_out = cur;
            else accepted = false;           // out untouched: the start point
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) H_out[i] = out[i];
        if (info)
            *info = pm_h_refine_info{cost_in, cost_out, static_cast<int32_t>(nu), iters, (from_ref || accepted) ? 0 : 1, 0};
    }
}

}  // namespace
}  // namespace pm_hrefine

int pm_ransac::homography_refine_enqueue(pm_ctx* ctx, const pm_points_view& v, const uint8_t* d_mask, const double* d_H_in,
                                         int max_iters, double* d_H_out, pm_h_refine_info* d_info)
{
    using namespace pm_hrefine;
    pm::ScopedKernelTime t(ctx, "homography_refine");
    hipLaunchKernelGGL(homography_refine, dim3(1), dim3(HR_P), 0, ctx->stream, v, d_mask, d_H_in, max_iters, d_H_out, d_info);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}
