// pose_refine.hip — refinement of a calibrated relative pose (R, t) on its inliers in ONE launch on gfx950 (MI355X):
// Levenberg-Marquardt on the Sampson distance of E = [t]x R over the S31-normalised correspondences with mask[i] != 0
// (docs/SPEC.md S46-S47), over 5 parameters: a Cayley rotation step on R (S40 step 4) and a step of t in the tangent
// plane of the unit sphere.  The mask is not recomputed; the caller typically passes the pose mask of pm_recover_pose*.
//
// One workgroup of HR_P = 512 threads, built on refine_reduce.hpp as pnp_refine.hip is: thread p owns partial p of S23's
// fixed reduction order and walks the correspondences i = p, p + 512, ... of the view from global memory, keeping its 21
// fp64 partial sums (15 of J^T J, 5 of J^T r, the cost) in registers; the stride-halving tree closes every pass.  The
// 5 x 5 Cholesky and the update of each step (lm_solve_n, cayley and left_rot of lm_core.hpp) run in thread 0, which leaves
// the trial pose, its E and its tangent basis in LDS for everyone.
//
// The launch keeps no per-call state, so the device form may be captured; the host forms (estimators.cpp) synchronise.
#include "essential_core.hpp"
#include "lm_core.hpp"
#include "ransac_fused_kernels.hpp"
#include "refine_reduce.hpp"
#include "twoview_refine_core.hpp"

namespace pm_hrefine {
namespace {

using pm_essential::Cam;
using pm_ransac::view_count1;
using pm_ransac::view_offsets;

constexpr int PO_LM = 15 + 5 + 1;         // J^T J, J^T r, cost
constexpr int PO_MODEL = 27;              // R (9), t (3), E (9), b1 (3), b2 (3)

// S31: the normalised coordinate as the scorer reads it
__device__ __forceinline__ double norm31(double x, double c, double f)
{
    const float v = static_cast<float>((x - c) / f);
    return fabsf(v) <= 1048576.0f ? static_cast<double>(v) : static_cast<double>(__builtin_nanf(""));
}

// E = [t]x R
__device__ __forceinline__ void e_of(const double* R, const double* t, double* E)
{
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        E[j] = t[1] * R[6 + j] - t[2] * R[3 + j];
        E[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
        E[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
    }
}

// S47 step 2: the deterministic orthonormal basis (b1, b2) of the plane orthogonal to the unit vector t
__device__ __forceinline__ void tangent_basis(const double* t, double* b1, double* b2)
{
    int k = 0;
    double m = fabs(t[0]);
    if (fabs(t[1]) < m) { k = 1; m = fabs(t[1]); }
    if (fabs(t[2]) < m) { k = 2; }
    const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    double w[3];
    cross3u(t, e, w);
    const double inv = 1.0 / sqrt(dot3f(w, w));
#pragma unroll
    for (int i = 0; i < 3; ++i) b1[i] = w[i] * inv;
    cross3u(t, b1, b2);
}

// The model of a pass from a pose (R, t): R, t, E, b1, b2
__device__ __forceinline__ void pose_model(const double* Rt, double* mo)
{
#pragma unroll
    for (int i = 0; i < 12; ++i) mo[i] = Rt[i];
    e_of(mo, mo + 9, mo + 12);
    tangent_basis(mo + 9, mo + 21, mo + 24);
}

// S47 step 2 (thread 0): the start of LM, t_in scaled to unit norm.  false = no LM
__device__ __attribute__((noinline)) bool lm_start(const double* in, double* mo)
{
    const double tt = dot3f(in + 9, in + 9);
    if (!(tt > 0.0) || !(tt < __builtin_inf())) return false;
    const double it0 = 1.0 / sqrt(tt);
    double p[12];
#pragma unroll
    for (int i = 0; i < 9; ++i) p[i] = in[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[9 + i] = in[9 + i] * it0;
    pose_model(p, mo);
    return true;
}

// S47 step 4 (thread 0) after the solve: stop rule, trial pose and its model.  cur: the model of the current pose.
// false = stop
__device__ __attribute__((noinline)) bool lm_step(const double* cur, const double* d, double* mo)
{
    double C[9], tr[12], q[3];
    if (!(step_max<5>(d) > LM_STEP_TOL)) return false;
    cayley(d, C);
    left_rot(C, cur, tr);
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = fma(d[4], cur[24 + i], fma(d[3], cur[21 + i], cur[9 + i]));
    const double iq = 1.0 / sqrt(dot3f(q, q));
#pragma unroll
    for (int i = 0; i < 3; ++i) tr[9 + i] = q[i] * iq;
    pose_model(tr, mo);
    return true;
}

// S47 result (thread 0): E of the output pose in S33's scale and sign; zeros if its norm is not in (0, inf)
__device__ __attribute__((noinline)) void e_out_of(const double* Rt, double* E)
{
    double e[9], ss = 0.0;
    e_of(Rt, Rt + 9, e);
#pragma unroll
    for (int i = 0; i < 9; ++i) ss = fma(e[i], e[i], ss);
    const double nrm = sqrt(ss);
    const bool ok = nrm > 0.0 && nrm < __builtin_inf();
    double big = e[0];
#pragma unroll
    for (int i = 1; i < 9; ++i)
        if (fabs(e[i]) > fabs(big)) big = e[i];
    double inv = 1.0 / nrm;
    if (big < 0.0) inv = -inv;
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = ok ? e[i] * inv : 0.0;
}

struct Model {
    double R[9], t[3], E[9], b1[3], b2[3];
};

// S47 step 3: the terms of one inlier
__device__ __forceinline__ void p_lm_term(double (&acc)[PO_LM], const Cam& k, const Model& s, double x1, double y1, double x2,
                                        double y2)
{
    const double p1[3] = {norm31(x1, k.cx, k.fx), norm31(y1, k.cy, k.fy), 1.0};
    const double p2[3] = {norm31(x2, k.cx, k.fx), norm31(y2, k.cy, k.fy), 1.0};
    double Gm[9], G2[9], n[3], J[5];
    const double r = sampson_grad(s.E, p1, p2, 1.0, 1.0, Gm);
    const double* t = s.t;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        G2[j] = t[2] * Gm[3 + j] - t[1] * Gm[6 + j];
        G2[3 + j] = t[0] * Gm[6 + j] - t[2] * Gm[j];
        G2[6 + j] = t[1] * Gm[j] - t[0] * Gm[3 + j];
    }
    left_rot_grad<false>(G2, s.R, n);
    J[0] = n[0]; J[1] = n[1]; J[2] = n[2];
    left_rot_grad<false>(Gm, s.R, n);
    J[3] = dot3f(s.b1, n);
    J[4] = dot3f(s.b2, n);
    lm_sums<5>(acc, J, r);
}

__global__ __launch_bounds__(HR_P) void pose_refine(pm_points_view v, Cam k, const uint8_t* mask, const double* Rt_in,
                                                    int max_iters, double* Rt_out, double* E_out, pm_h_refine_info* info)
{
    __shared__ double s_x[HR_CH][HR_P / 2];
    __shared__ double s_red[PO_LM];
    __shared__ double s_jg[PO_LM];            // J^T J, J^T r at the current pose
    __shared__ double s_in[12];
    __shared__ double s_cur[PO_MODEL];        // current pose and its model
    __shared__ double s_tr[PO_MODEL];         // trial pose and its model
    __shared__ double s_d[5];                 // LM step
    __shared__ int s_ok;
    __shared__ int s_offs[PM_MAX_PARTS + 1];

    const int tid = threadIdx.x;
    int n;
    if (v.parts == 1) {
        n = view_count1(v);
    } else {
        view_offsets(v, s_offs, tid);
        n = 0;
    }
    if (tid < 12) s_in[tid] = Rt_in[tid];     // read before any write: Rt_out may alias Rt_in
    __syncthreads();
    if (v.parts > 1) n = s_offs[v.parts];
    double in[12];
    bool zero = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) { in[i] = s_in[i]; zero = zero && in[i] == 0.0; }
    if (zero) {                               // status 2: no model
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 12; ++i) Rt_out[i] = in[i];
            if (E_out) {
#pragma unroll
                for (int i = 0; i < 9; ++i) E_out[i] = 0.0;
            }
            if (info) *info = pm_h_refine_info{0.0, 0.0, 0, 0, 2, 0};
        }
        return;
    }
    const double fm = 0.5 * (k.fx + k.fy);
    const double f2 = fm * fm;

    // ---- S46 pass 1: inlier count and cost of the input pose
    {
        double E[9];
        e_of(in, in + 9, E);
        pass<2>(v, s_offs, n, mask, tid, s_x, s_red, [&](double (&a)[2], double x1, double y1, double x2, double y2) {
            const double p1[3] = {norm31(x1, k.cx, k.fx), norm31(y1, k.cy, k.fy), 1.0};
            const double p2[3] = {norm31(x2, k.cx, k.fx), norm31(y2, k.cy, k.fy), 1.0};
            const double r = sampson_res(E, p1, p2, 1.0, 1.0);
            a[0] = a[0] + 1.0;
            a[1] = a[1] + r * r;
        });
    }
    const double nu = s_red[0], cin = s_red[1];

    // ---- S47 LM: one pass per iteration at the trial pose; the current pose and its J^T J, J^T r stay in LDS
    auto lm_pass = [&](const double* mo) {
        Model s;
#pragma unroll
        for (int i = 0; i < 9; ++i) { s.R[i] = mo[i]; s.E[i] = mo[12 + i]; }
#pragma unroll
        for (int i = 0; i < 3; ++i) { s.t[i] = mo[9 + i]; s.b1[i] = mo[21 + i]; s.b2[i] = mo[24 + i]; }
        pass<PO_LM>(v, s_offs, n, mask, tid, s_x, s_red,
                    [&](double (&a)[PO_LM], double x1, double y1, double x2, double y2) { p_lm_term(a, k, s, x1, y1, x2, y2); });
    };
    double cur = cin;
    int iters = 0;
    bool accepted = false;
    if (tid == 0) s_ok = (nu >= 5.0 && max_iters > 0 && lm_start(s_in, s_cur)) ? 1 : 0;
    __syncthreads();
    if (s_ok) {
        lm_pass(s_cur);
        if (tid < PO_LM) s_jg[tid] = s_red[tid];
        __syncthreads();
        double lam = LM_LAMBDA0;
        for (int it = 0; it < max_iters; ++it) {
            if (tid == 0) [[clang::noinline]] s_ok = (lm_solve_n<5>(s_jg, s_jg + 15, lam, s_d) && lm_step(s_cur, s_d, s_tr)) ? 1 : 0;
            __syncthreads();
            if (!s_ok) break;
            lm_pass(s_tr);
            ++iters;
            const double ct = s_red[PO_LM - 1];
            if (ct < cur) {
                cur = ct;
                lam = lam / 10.0;
                accepted = true;
                if (tid < PO_LM) s_jg[tid] = s_red[tid];
                if (tid < PO_MODEL) s_cur[tid] = s_tr[tid];
                __syncthreads();
            } else {
                lam = lam * 10.0;
            }
        }
    }

    // ---- result (thread 0)
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) s_tr[i] = accepted ? s_cur[i] : in[i];
#pragma unroll
        for (int i = 0; i < 12; ++i) Rt_out[i] = s_tr[i];
        if (E_out) e_out_of(s_tr, E_out);
        const double cost_in = cin * f2;
        if (info)
            *info = pm_h_refine_info{cost_in, accepted ? cur * f2 : cost_in, static_cast<int32_t>(nu), iters, accepted ? 0 : 1, 0};
    }
}

}  // namespace
}  // namespace pm_hrefine

int pm_ransac::pose_refine_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_camera& K, const uint8_t* d_mask,
                                   const double* d_Rt_in, int max_iters, double* d_Rt_out, double* d_E_out,
                                   pm_h_refine_info* d_info)
{
    using namespace pm_hrefine;
    pm::ScopedKernelTime t(ctx, "pose_refine");
    hipLaunchKernelGGL(pose_refine, dim3(1), dim3(HR_P), 0, ctx->stream, v, Cam{K.fx, K.fy, K.cx, K.cy}, d_mask, d_Rt_in,
                       max_iters, d_Rt_out, d_E_out, d_info);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}
