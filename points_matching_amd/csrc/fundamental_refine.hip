// fundamental_refine.hip — refinement of a robust fundamental matrix on its inliers in ONE launch on gfx950 (MI355X): the
// Hartley-normalised least-squares 8-point refit over all inliers (docs/SPEC.md S44) and Levenberg-Marquardt on the
// Sampson distance over 7 parameters that cannot leave rank 2 (S45), the step every SfM front end runs on the host after
// cv::findFundamentalMat.  The mask is not recomputed.
//
// One workgroup of HR_P = 512 threads (8 waves), built on refine_reduce.hpp as homography_refine.hip is: thread p owns
// partial p of S23's fixed reduction order, walks the correspondences i = p, p + 512, ... of the view from global memory
// and keeps its partial sums in fp64 registers (45 in the normal-matrix pass, 36 in the LM passes).  The 9 x 9 Jacobi
// eigen-solve runs lane-parallel in wave 0 (homography_refine_core.hpp); the 3 x 3 Jacobi SVDs, the 7 x 7 Cholesky and
// the Cayley update of each LM step (lm_solve_n and cayley, lm_core.hpp) run in thread 0, which leaves the model of the
// next pass in LDS for everyone.
// Passes: sums + cost of F_in, centroid distances, normal matrix, cost of the refit, then the LM passes (one at the start
// point, one per iteration) and the cost of the LM result.
//
// The launch keeps no per-call state, so the device form may be captured; the host forms (estimators.cpp) synchronise.
#include "homography_refine_core.hpp"
#include "lm_core.hpp"
#include "ransac_fused_kernels.hpp"
#include "refine_reduce.hpp"
#include "twoview_refine_core.hpp"

namespace pm_hrefine {
namespace {

using pm_ransac::jacobi_pair;
using pm_ransac::scale_sign;
using pm_ransac::view_count1;
using pm_ransac::view_offsets;

constexpr int FR_LM = 28 + 7 + 1;         // J^T J, J^T r, cost

// S43: squared Sampson distance (px^2) of one correspondence under f
__device__ __forceinline__ double f_cost_term(const double (&f)[9], double x1, double y1, double x2, double y2)
{
    const double a = fma(f[0], x1, fma(f[1], y1, f[2]));
    const double b = fma(f[3], x1, fma(f[4], y1, f[5]));
    const double c = fma(f[6], x1, fma(f[7], y1, f[8]));
    const double num = fma(x2, a, fma(y2, b, c));
    const double at = fma(f[0], x2, fma(f[3], y2, f[6]));
    const double bt = fma(f[1], x2, fma(f[4], y2, f[7]));
    const double den = fma(a, a, fma(b, b, fma(at, at, bt * bt)));
    return (num * num) / den;
}

// S7 step 5: out = T2^T in T1 for T = [[s, 0, tx], [0, s, ty], [0, 0, 1]]
__device__ __forceinline__ void conj(const double (&in)[9], double s1, double t1x, double t1y, double s2, double t2x,
                                     double t2y, double (&out)[9])
{
    double M[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        M[i][0] = in[3 * i] * s1;
        M[i][1] = in[3 * i + 1] * s1;
        M[i][2] = fma(in[3 * i], t1x, fma(in[3 * i + 1], t1y, in[3 * i + 2]));
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        out[j] = s2 * M[0][j];
        out[3 + j] = s2 * M[1][j];
        out[6 + j] = fma(t2x, M[0][j], fma(t2y, M[1][j], M[2][j]));
    }
}

// S7 step 4 on the 9 entries g: G V = U Sigma after 6 sweeps, cn the column norms, m the smallest column
__device__ __forceinline__ int svd3(const double (&g)[9], double (&G)[3][3], double (&V)[3][3], double (&cn)[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) { G[i][j] = g[3 * i + j]; V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 6; ++sweep) {
        jacobi_pair<0, 1>(G, V);
        jacobi_pair<0, 2>(G, V);
        jacobi_pair<1, 2>(G, V);
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        double a = G[0][p] * G[0][p]; a = fma(G[1][p], G[1][p], a); a = fma(G[2][p], G[2][p], a);
        cn[p] = a;
    }
    int m = 0;
    double cm = cn[0];
    if (cn[1] < cm) { m = 1; cm = cn[1]; }
    if (cn[2] < cm) { m = 2; }
    return m;
}

// S44 steps 5-6 (thread 0): rank 2, denormalise, scale and sign.  nrm = (cx1, cy1, s1, cx2, cy2, s2)
__device__ __attribute__((noinline)) bool refit_finish(const double* gn, const double* nrm, double* out)
{
    double g[9], G[3][3], V[3][3], cn[3], Fn[9], Fd[9], Fr[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) g[i] = gn[i];
    const int m = svd3(g, G, V, cn);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int p = 0; p < 3; ++p)
            if (p == m) G[i][p] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double a = G[i][0] * V[j][0]; a = fma(G[i][1], V[j][1], a); a = fma(G[i][2], V[j][2], a);
            Fn[3 * i + j] = a;
        }
    conj(Fn, nrm[2], -(nrm[2] * nrm[0]), -(nrm[2] * nrm[1]), nrm[5], -(nrm[5] * nrm[3]), -(nrm[5] * nrm[4]), Fd);
    if (!scale_sign(Fd, Fr)) return false;
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = Fr[i];
    return true;
}

// S45 step 2 (thread 0): the LM state (u0, u1, v0, v1, sigma) of the start, in the normalised coordinates
__device__ __attribute__((noinline)) bool lm_state(const double* start, const double* nrm, double* st)
{
    double f[9], Fs[9], G[3][3], V[3][3], cn[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] = start[i];
    conj(f, 1.0 / nrm[2], nrm[0], nrm[1], 1.0 / nrm[5], nrm[3], nrm[4], Fs);
    const int m = svd3(Fs, G, V, cn);
    const int a = m == 0 ? 1 : 0, b = m == 2 ? 1 : 2;
    const double ca = m == 0 ? cn[1] : cn[0], cb = m == 2 ? cn[1] : cn[2];
    const bool sw = cb > ca;
    const int o0 = sw ? b : a, o1 = sw ? a : b;
    const double c0 = sw ? cb : ca, c1 = sw ? ca : cb;
    if (!(c1 > 0.0) || !(c0 < __builtin_inf())) return false;
    const double sa = sqrt(c0), sb = sqrt(c1);
    const double ia = 1.0 / sa, ib = 1.0 / sb;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            if (p == o0) { st[i] = G[i][p] * ia; st[6 + i] = V[i][p]; }
            if (p == o1) { st[3 + i] = G[i][p] * ib; st[9 + i] = V[i][p]; }
        }
    st[12] = sb / sa;
    return true;
}

// F = u0 v0^T + sigma u1 v1^T
__device__ __forceinline__ void f_of_state(const double* st, double* F)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) F[3 * i + j] = fma(st[i], st[6 + j], (st[12] * st[3 + i]) * st[9 + j]);
}

// The model of an LM pass from a state: F, then u1, then v1 (15 doubles)
__device__ __forceinline__ void lm_model(const double* st, double* lc)
{
    f_of_state(st, lc);
#pragma unroll
    for (int i = 0; i < 3; ++i) { lc[9 + i] = st[3 + i]; lc[12 + i] = st[9 + i]; }
}

// S45 step 4 (thread 0) after the solve: stop rule, trial state and its model.  false = stop
__device__ __attribute__((noinline)) bool lm_step(const double* st, const double* d, double* tr, double* lc)
{
    double C[9];
    if (!(step_max<7>(d) > LM_STEP_TOL)) return false;
    cayley(d, C);
    rot3(C, st, tr);
    rot3(C, st + 3, tr + 3);
    cayley(d + 3, C);
    rot3(C, st + 6, tr + 6);
    rot3(C, st + 9, tr + 9);
    tr[12] = st[12] + d[6];
    lm_model(tr, lc);
    return true;
}

// S45 result (thread 0): the accepted state back in pixels, S7 steps 5-6
__device__ __attribute__((noinline)) bool lm_result(const double* st, const double* nrm, double* out)
{
    double Fn[9], Fd[9], Fl[9];
    f_of_state(st, Fn);
    conj(Fn, nrm[2], -(nrm[2] * nrm[0]), -(nrm[2] * nrm[1]), nrm[5], -(nrm[5] * nrm[3]), -(nrm[5] * nrm[4]), Fd);
    if (!scale_sign(Fd, Fl)) return false;
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = Fl[i];
    return true;
}

// S45 step 3: the terms of one inlier at the model lc = (F, u1, v1)
__device__ __forceinline__ void f_lm_term(double (&acc)[FR_LM], const double (&F)[9], const double (&u1)[3],
                                        const double (&v1)[3], const double (&nrm)[6], double w1, double w2, double x1,
                                        double y1, double x2, double y2)
{
    const double p1[3] = {(x1 - nrm[0]) * nrm[2], (y1 - nrm[1]) * nrm[2], 1.0};
    const double p2[3] = {(x2 - nrm[3]) * nrm[5], (y2 - nrm[4]) * nrm[5], 1.0};
    double Gm[9], J[7], n[3], g[3];
    const double r = sampson_grad(F, p1, p2, w1, w2, Gm);
    left_rot_grad<false>(Gm, F, n);
    J[0] = n[0]; J[1] = n[1]; J[2] = n[2];
    left_rot_grad<true>(Gm, F, n);            // -F [e_k]x: the left rotation of F^T against Gm^T
    J[3] = n[0]; J[4] = n[1]; J[5] = n[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) g[i] = dot3f(&Gm[3 * i], v1);
    J[6] = dot3f(u1, g);
    lm_sums<7>(acc, J, r);
}

__global__ __launch_bounds__(HR_P) void fundamental_refine(pm_points_view v, const uint8_t* mask, const double* F_in,
                                                           int max_iters, double* F_out, pm_h_refine_info* info)
{
    __shared__ double s_x[HR_CH][HR_P / 2];
    __shared__ double s_red[HR_NORMAL];
    __shared__ double s_jg[FR_LM];            // J^T J and J^T r at the current LM state
    __shared__ double s_fin[9];
    __shared__ double s_gn[9];
    __shared__ double s_nrm[6];               // cx1, cy1, s1, cx2, cy2, s2
    __shared__ double s_ref[9];
    __shared__ double s_start[9];             // S45 start point
    __shared__ double s_st[13];               // current LM state
    __shared__ double s_tr[13];               // trial state
    __shared__ double s_lc[15];               // model of the next LM pass
    __shared__ double s_d[7];                 // LM step
    __shared__ double s_lm[9];                // LM result in pixels
    __shared__ int s_ok[4];                   // Jacobi, refit, LM state / step, LM result
    __shared__ int s_offs[PM_MAX_PARTS + 1];

    const int tid = threadIdx.x, lane = tid & 63;
    int n;
    if (v.parts == 1) {
        n = view_count1(v);
    } else {
        view_offsets(v, s_offs, tid);
        n = 0;
    }
    if (tid < 9) s_fin[tid] = F_in[tid];      // read before any write: F_out may alias F_in
    __syncthreads();
    if (v.parts > 1) n = s_offs[v.parts];
    double fin[9];
    bool zero = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) { fin[i] = s_fin[i]; zero = zero && fin[i] == 0.0; }
    if (zero) {                               // status 2: no model
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) F_out[i] = fin[i];
            if (info) *info = pm_h_refine_info{0.0, 0.0, 0, 0, 2, 0};
        }
        return;
    }

    // ---- S44 pass 1: inlier count, coordinate sums, cost of F_in
    pass<6>(v, s_offs, n, mask, tid, s_x, s_red, [&](double (&a)[6], double x1, double y1, double x2, double y2) {
        a[0] = a[0] + 1.0;
        a[1] = a[1] + x1; a[2] = a[2] + y1; a[3] = a[3] + x2; a[4] = a[4] + y2;
        a[5] = a[5] + f_cost_term(fin, x1, y1, x2, y2);
    });
    const double nu = s_red[0], cost_in = s_red[5];
    const double cx1 = s_red[1] / nu, cy1 = s_red[2] / nu, cx2 = s_red[3] / nu, cy2 = s_red[4] / nu;

    // ---- S44 refit: Hartley normalisation, normal matrix, Jacobi, rank 2, denormalisation
    bool norm_ok = false, ok_ref = false;
    double nrm[6] = {cx1, cy1, 0.0, cx2, cy2, 0.0};
    if (nu >= 8.0) {
        pass<2>(v, s_offs, n, mask, tid, s_x, s_red, [&](double (&a)[2], double x1, double y1, double x2, double y2) {
            const double dx1 = x1 - cx1, dy1 = y1 - cy1, dx2 = x2 - cx2, dy2 = y2 - cy2;
            a[0] = a[0] + sqrt(fma(dx1, dx1, dy1 * dy1));
            a[1] = a[1] + sqrt(fma(dx2, dx2, dy2 * dy2));
        });
        const double md1 = s_red[0] / nu, md2 = s_red[1] / nu;
        if (md1 > 0.0 && md1 < __builtin_inf() && md2 > 0.0 && md2 < __builtin_inf()) {
            norm_ok = true;
            nrm[2] = 1.4142135623730951 / md1;
            nrm[5] = 1.4142135623730951 / md2;
            if (tid < 6) s_nrm[tid] = nrm[tid];
            pass<HR_NORMAL>(v, s_offs, n, mask, tid, s_x, s_red,
                            [&](double (&a)[HR_NORMAL], double x1, double y1, double x2, double y2) {
                                const double xn = (x1 - nrm[0]) * nrm[2], yn = (y1 - nrm[1]) * nrm[2];
                                const double xq = (x2 - nrm[3]) * nrm[5], yq = (y2 - nrm[4]) * nrm[5];
                                const double r[9] = {xq * xn, xq * yn, xq, yq * xn, yq * yn, yq, xn, yn, 1.0};
                                int e = 0;
#pragma unroll
                                for (int j = 0; j < 9; ++j)
#pragma unroll
                                    for (int k = j; k < 9; ++k, ++e) a[e] = a[e] + r[j] * r[k];
                            });
            if (tid < 64) {                   // wave 0
                double gk;
                const bool ok = jacobi_min_wave(s_red, lane, gk);
                if (lane < 9) s_gn[lane] = gk;
                if (lane == 0) s_ok[0] = ok ? 1 : 0;
            }
            __syncthreads();
            if (tid == 0) s_ok[1] = (s_ok[0] && refit_finish(s_gn, s_nrm, s_ref)) ? 1 : 0;
            __syncthreads();
            ok_ref = s_ok[1] != 0;
        }
    }

    // ---- S45 step 1, start point: the refit if its cost is not higher than F_in's
    double cost_start = cost_in;
    bool from_ref = false;
    if (ok_ref) {
        double fref[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) fref[i] = s_ref[i];
        pass<1>(v, s_offs, n, mask, tid, s_x, s_red, [&](double (&a)[1], double x1, double y1, double x2, double y2) {
            a[0] = a[0] + f_cost_term(fref, x1, y1, x2, y2);
        });
        const double cr = s_red[0];
        if (cr <= cost_in) { cost_start = cr; from_ref = true; }
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) s_start[i] = from_ref ? s_ref[i] : s_fin[i];
        s_ok[2] = 0;
        if (norm_ok && max_iters > 0 && lm_state(s_start, s_nrm, s_st)) {
            lm_model(s_st, s_lc);
            s_ok[2] = 1;
        }
    }
    __syncthreads();

    // ---- S45 LM: one pass per iteration at the trial state; the current state and its J^T J, J^T r stay in LDS
    auto lm_pass = [&]() {
        double F[9], u1[3], v1[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = s_lc[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) { u1[i] = s_lc[9 + i]; v1[i] = s_lc[12 + i]; }
        const double w1 = nrm[2] * nrm[2], w2 = nrm[5] * nrm[5];
        pass<FR_LM>(v, s_offs, n, mask, tid, s_x, s_red,
                    [&](double (&a)[FR_LM], double x1, double y1, double x2, double y2) {
                        f_lm_term(a, F, u1, v1, nrm, w1, w2, x1, y1, x2, y2);
                    });
    };
    int iters = 0;
    bool accepted = false;
    if (s_ok[2]) {
        lm_pass();
        if (tid < FR_LM) s_jg[tid] = s_red[tid];
        double cur = s_red[FR_LM - 1];
        double lam = LM_LAMBDA0;
        __syncthreads();
        for (int it = 0; it < max_iters; ++it) {
            if (tid == 0) [[clang::noinline]] s_ok[2] = (lm_solve_n<7>(s_jg, s_jg + 28, lam, s_d) && lm_step(s_st, s_d, s_tr, s_lc)) ? 1 : 0;
            __syncthreads();
            if (!s_ok[2]) break;
            lm_pass();
            ++iters;
            const double ct = s_red[FR_LM - 1];
            if (ct < cur) {
                cur = ct;
                lam = lam / 10.0;
                accepted = true;
                if (tid < FR_LM) s_jg[tid] = s_red[tid];
                if (tid < 13) s_st[tid] = s_tr[tid];
                __syncthreads();
            } else {
                lam = lam * 10.0;
            }
        }
    }

    // ---- S45 result: the accepted state in pixels counts only if its pixel cost is below the start's
    double cost_out = cost_start;
    if (accepted) {
        if (tid == 0) s_ok[3] = lm_result(s_st, s_nrm, s_lm) ? 1 : 0;
        __syncthreads();
        accepted = false;
        if (s_ok[3]) {
            double fl[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) fl[i] = s_lm[i];
            pass<1>(v, s_offs, n, mask, tid, s_x, s_red, [&](double (&a)[1], double x1, double y1, double x2, double y2) {
                a[0] = a[0] + f_cost_term(fl, x1, y1, x2, y2);
            });
            const double cl = s_red[0];
            if (cl < cost_start) { cost_out = cl; accepted = true; }
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) F_out[i] = accepted ? s_lm[i] : s_start[i];
        if (info)
            *info = pm_h_refine_info{cost_in, cost_out, static_cast<int32_t>(nu), iters, (from_ref || accepted) ? 0 : 1, 0};
    }
}

}  // namespace
}  // namespace pm_hrefine

int pm_ransac::fundamental_refine_enqueue(pm_ctx* ctx, const pm_points_view& v, const uint8_t* d_mask, const double* d_F_in,
                                          int max_iters, double* d_F_out, pm_h_refine_info* d_info)
{
    using namespace pm_hrefine;
    pm::ScopedKernelTime t(ctx, "fundamental_refine");
    hipLaunchKernelGGL(fundamental_refine, dim3(1), dim3(HR_P), 0, ctx->stream, v, d_mask, d_F_in, max_iters, d_F_out, d_info);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}
