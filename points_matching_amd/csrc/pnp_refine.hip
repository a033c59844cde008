// pnp_refine.hip — refinement of an absolute pose on its inliers in ONE launch on gfx950 (MI355X): Levenberg-Marquardt
// on the squared pixel reprojection error over mask[i] != 0 (docs/SPEC.md S40), the final solvePnP(ITERATIVE) that
// cv::solvePnPRansac runs on its inliers [recalled].  The mask is not recomputed.  Also the gather of the device chain
// (pm_gather_pnp_dev): compacted matches -> (pixel, world point) rows.
//
// One workgroup of HR_P = 512 threads, built on refine_reduce.hpp as homography_refine.hip is: thread p owns partial p of
// S23's fixed reduction order and walks the correspondences i = p, p + 512, ... from global memory, keeping its 28 fp64
// partial sums (21 of J^T J, 6 of J^T r, the cost) in registers; the stride-halving tree closes every pass.  The 6 x 6
// Cholesky of each step runs in thread 0 (S24's lm_solve_n, lm_core.hpp); every thread then applies the same step (S40's
// Cayley rotation update, pose_update in lm_core.hpp: no transcendental function) and the next pass runs at the trial pose.
//
// The launch keeps no per-call state, so the device form may be captured; the host forms (estimators.cpp)
// synchronise.
#include "essential_core.hpp"
#include "lm_core.hpp"
#include "ransac_fused_kernels.hpp"
#include "refine_reduce.hpp"

namespace pm_hrefine {
namespace {

using pm_essential::Cam;
using pm_ransac::view_count1;

constexpr int PR_NJ = 21;                 // J^T J entries j <= k, row-major
constexpr int PR_LM = PR_NJ + 6 + 1;      // + J^T r + cost

struct Pt {
    double x, y, z, u, v;
};

__device__ __forceinline__ Pt point(const pm_points_view& v, int i)
{
    const float* X = v.xy1 + 3 * static_cast<size_t>(i);
    const float2 q = *reinterpret_cast<const float2*>(v.xy2 + 2 * static_cast<size_t>(i));
    return Pt{static_cast<double>(X[0]), static_cast<double>(X[1]), static_cast<double>(X[2]), static_cast<double>(q.x),
              static_cast<double>(q.y)};
}

// Y = R X, x_cam = Y + t
__device__ __forceinline__ void cam_point(const double (&Rt)[12], const Pt& p, double (&xc)[3], double (&Y)[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        Y[r] = (Rt[3 * r] * p.x + Rt[3 * r + 1] * p.y) + Rt[3 * r + 2] * p.z;
        xc[r] = Y[r] + Rt[9 + r];
    }
}

__device__ __forceinline__ double cost_term(const Cam& k, const double (&Rt)[12], const Pt& p)
{
    double xc[3], Y[3];
    cam_point(Rt, p, xc, Y);
    const double iz = 1.0 / xc[2];
    const double ru = (k.fx * (xc[0] * iz) + k.cx) - p.u;
    const double rv = (k.fy * (xc[1] * iz) + k.cy) - p.v;
    return fma(ru, ru, rv * rv);
}

// S40 step 2: the terms of one inlier at the pose Rt
__device__ __forceinline__ void lm_term(double (&a)[PR_LM], const Cam& k, const double (&Rt)[12], const Pt& p)
{
    double xc[3], Y[3];
    cam_point(Rt, p, xc, Y);
    const double iz = 1.0 / xc[2];
    const double px = xc[0] * iz, py = xc[1] * iz;
    const double ru = (k.fx * px + k.cx) - p.u;
    const double rv = (k.fy * py + k.cy) - p.v;
    const double fa = k.fx * iz, fb = k.fy * iz;
    const double ju[6] = {-((fa * px) * Y[1]), fa * Y[2] + (fa * px) * Y[0], -(fa * Y[1]), fa, 0.0, -(fa * px)};
    const double jv[6] = {-(fb * Y[2]) - (fb * py) * Y[1], (fb * py) * Y[0], fb * Y[0], 0.0, fb, -(fb * py)};
    int e = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int q = j; q < 6; ++q, ++e) a[e] = a[e] + fma(ju[j], ju[q], jv[j] * jv[q]);
#pragma unroll
    for (int j = 0; j < 6; ++j) a[PR_NJ + j] = a[PR_NJ + j] + fma(ju[j], ru, jv[j] * rv);
    a[PR_NJ + 6] = a[PR_NJ + 6] + fma(ru, ru, rv * rv);
}

// v: one-part view, xy1 = world points (3 floats each), xy2 = pixels
__global__ __launch_bounds__(HR_P) void pnp_refine(pm_points_view v, Cam k, const uint8_t* mask, const double* Rt_in,
                                                   int max_iters, double* Rt_out, pm_h_refine_info* info)
{
    __shared__ double s_x[HR_CH][HR_P / 2];
    __shared__ double s_red[PR_LM];
    __shared__ double s_jg[PR_LM];        // J^T J, J^T r at the current pose
    __shared__ double s_in[12];
    __shared__ double s_cur[12];          // current pose
    __shared__ double s_d[6];             // LM step
    __shared__ int s_ok;

    const int tid = threadIdx.x;
    const int n = view_count1(v);
    if (tid < 12) s_in[tid] = Rt_in[tid];     // read before any write: Rt_out may alias Rt_in
    __syncthreads();
    double in[12];
    bool zero = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) { in[i] = s_in[i]; zero = zero && in[i] == 0.0; }
    if (zero) {                               // S40 status 2: no model
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 12; ++i) Rt_out[i] = in[i];
            if (info) *info = pm_h_refine_info{0.0, 0.0, 0, 0, 2, 0};
        }
        return;
    }

    // ---- pass 1: inlier count and cost of the start
    {
        double acc[2] = {0.0, 0.0};
        for (int i = tid; i < n; i += HR_P) {
            if (!mask[i]) continue;
            const Pt p = point(v, i);
            acc[0] = acc[0] + 1.0;
            acc[1] = acc[1] + cost_term(k, in, p);
        }
        tree<2>(acc, tid, s_x, s_red);
    }
    const double nu = s_red[0], cost_in = s_red[1];

    double cur = cost_in;
    int iters = 0;
    bool accepted = false;
    auto lm_pass = [&](const double (&Rt)[12]) {
        double acc[PR_LM];
#pragma unroll
        for (int e = 0; e < PR_LM; ++e) acc[e] = 0.0;
        for (int i = tid; i < n; i += HR_P) {
            if (!mask[i]) continue;
            lm_term(acc, k, Rt, point(v, i));
        }
        tree<PR_LM>(acc, tid, s_x, s_red);
    };
    if (nu >= 4.0 && max_iters > 0) {
        lm_pass(in);
        if (tid < PR_LM) s_jg[tid] = s_red[tid];
        if (tid < 12) s_cur[tid] = in[tid];
        __syncthreads();
        double lam = LM_LAMBDA0;
        for (int it = 0; it < max_iters; ++it) {
            if (tid == 0) [[clang::noinline]] s_ok = lm_solve_n<6>(s_jg, s_jg + PR_NJ, lam, s_d) ? 1 : 0;
            __syncthreads();
            if (!s_ok) break;
            double dmax = 0.0, hmax = 1.0;
#pragma unroll
            for (int i = 0; i < 6; ++i)               // NaN propagates into dmax and stops the loop
                if (!(fabs(s_d[i]) <= dmax)) dmax = fabs(s_d[i]);
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (!(fabs(s_cur[9 + i]) <= hmax)) hmax = fabs(s_cur[9 + i]);
            if (!(dmax > LM_STEP_TOL * hmax)) break;
            double tr[12];
            pose_update(s_cur, s_d, tr);
            lm_pass(tr);
            ++iters;
            const double ct = s_red[PR_LM - 1];
            if (ct < cur) {
                cur = ct;
                lam = lam / 10.0;
                accepted = true;
                if (tid < PR_LM) s_jg[tid] = s_red[tid];
                if (tid < 12) s_cur[tid] = tr[tid];
                __syncthreads();
            } else {
                lam = lam * 10.0;
            }
        }
    }

    // ---- result (thread 0)
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) Rt_out[i] = accepted ? s_cur[i] : in[i];
        if (info) *info = pm_h_refine_info{cost_in, accepted ? cur : cost_in, static_cast<int32_t>(nu), iters, accepted ? 0 : 1, 0};
    }
}

// The device chain's gather: row i < n = clamp(*count, 0, cap) of the compacted match list gives
// uv[i] = kp_xy[queryIdx] and xyz[i] = obj[trainIdx]; an index out of range gives a NaN row (never an S39 inlier)
__global__ __launch_bounds__(256) void gather_pnp(const pm_match* __restrict__ m, const int32_t* __restrict__ count, int cap,
                                                  const float* __restrict__ kp_xy, int n_kp, const float* __restrict__ obj,
                                                  int n_obj, float* __restrict__ uv, float* __restrict__ xyz)
{
    int n = cap;
    if (count) { const int raw = *count; n = raw < 0 ? 0 : (raw > cap ? cap : raw); }
    const float nanv = __builtin_nanf("");
    for (int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x); i < n; i += static_cast<int>(gridDim.x) * 256) {
        const int q = m[i].queryIdx, t = m[i].trainIdx;
        float2 a = {nanv, nanv};
        if (q >= 0 && q < n_kp) a = *reinterpret_cast<const float2*>(kp_xy + 2 * static_cast<size_t>(q));
        float x = nanv, y = nanv, z = nanv;
        if (t >= 0 && t < n_obj) {
            const float* o = obj + 3 * static_cast<size_t>(t);
            x = o[0]; y = o[1]; z = o[2];
        }
        *reinterpret_cast<float2*>(uv + 2 * static_cast<size_t>(i)) = a;
        xyz[3 * static_cast<size_t>(i)] = x;
        xyz[3 * static_cast<size_t>(i) + 1] = y;
        xyz[3 * static_cast<size_t>(i) + 2] = z;
    }
}

}  // namespace
}  // namespace pm_hrefine

int pm_ransac::pnp_refine_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_camera& K, const uint8_t* d_mask,
                                  const double* d_Rt_in, int max_iters, double* d_Rt_out, pm_h_refine_info* d_info)
{
    using namespace pm_hrefine;
    pm::ScopedKernelTime t(ctx, "pnp_refine");
    hipLaunchKernelGGL(pnp_refine, dim3(1), dim3(HR_P), 0, ctx->stream, v, Cam{K.fx, K.fy, K.cx, K.cy}, d_mask, d_Rt_in,
                       max_iters, d_Rt_out, d_info);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

int pm_ransac::gather_pnp_enqueue(pm_ctx* ctx, const pm_match* d_m, const int32_t* d_count, int cap, const float* d_kp_xy,
                                  int n_kp, const float* d_obj, int n_obj, float* d_uv, float* d_xyz)
{
    using namespace pm_hrefine;
    const int nwg = (cap + 255) / 256 < 1024 ? (cap + 255) / 256 : 1024;
    pm::ScopedKernelTime t(ctx, "gather_pnp");
    hipLaunchKernelGGL(gather_pnp, dim3(nwg < 1 ? 1 : nwg), dim3(256), 0, ctx->stream, d_m, d_count, cap, d_kp_xy, n_kp, d_obj,
                       n_obj, d_uv, d_xyz);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}
