// bundle_adjust.hip — local bundle adjustment in ONE launch on gfx950 (MI355X), docs/SPEC.md S113-S117: joint
// Levenberg-Marquardt over the free poses and the points of 2 .. 8 views on the summed squared pixel error, solved through
// the Schur complement on the pose parameters.  pm_triangulate* refines the points alone and pm_pnp_refine* one pose alone;
// this call moves both at once, the step a map builder runs after it inserts a keyframe.
//
// One workgroup of HR_P = 512 threads on refine_reduce.hpp, as the five refinement kernels are: thread p owns partial p of
// S23's fixed reduction order and walks the points i = p, p + 512, ...  A point therefore belongs to one thread for the whole
// run: its fp64 position (current and trial), its used byte, its linearisation (Vp, gp, its cost, W per free view) and its
// Y = W Vp*^-1 live in the caller's workspace as records (10 doubles per point, 18 per point and free view: one address and
// constant offsets per record, where component-major arrays cost an address register pair per component and spilled), and no
// thread ever loads what another stored there — everything that crosses threads (the sums, the reduced system, the step, the
// poses) goes through LDS behind a barrier.  The linearisation visits the views in index order, one pass each: a pass adds
// that view's terms to the point blocks and, for a free view, sums the 21 + 6 pose terms through the tree, so the 27 F pose
// sums never sit in registers together.  The reduced system (6F <= 42 parameters) is summed one pair of free views at a time,
// its 36 + 6 sums in two passes of 21 partials per thread, re-reading Y and W and not the observations; its Cholesky spreads
// a column's rows over the first 6F threads (each L_ij keeps S24's ascending chain), thread 0 substitutes.  The point blocks'
// 3 x 3 factor and substitutions (lm_factor, lm_subst) and S40's pose update (pose_update) are lm_core.hpp's.
//
// The launch keeps no per-call state and allocates nothing, so the device form may be captured; the host form stages its
// rows and the workspace through pm::StagedBlock and synchronises once.
#include <cmath>

#include "essential_core.hpp"
#include "lm_core.hpp"
#include "pm_common.hpp"
#include "refine_reduce.hpp"

namespace pm_ba {
namespace {

using pm_essential::Cam;
using pm_hrefine::HR_CH;
using pm_hrefine::HR_P;
using pm_hrefine::LM_LAMBDA0;
using pm_hrefine::LM_STEP_TOL;
using pm_hrefine::group_max3;
using pm_hrefine::lm_factor;
using pm_hrefine::lm_subst;
using pm_hrefine::pose_update;
using pm_hrefine::tree;

constexpr int BA_MAXV = PM_TRI_MAX_VIEWS;
constexpr int BA_MAXF = BA_MAXV - 1;      // at least one view is held
constexpr int BA_MAXM = 6 * BA_MAXF;      // parameters of the reduced system
constexpr int BA_NU = 27;                 // per free view: U (21 entries j <= k) and gc (6)
constexpr int BA_NS = 42;                 // per pair of free views: 36 entries of Y W^T and 6 of Y gp ...
constexpr int BA_NH = BA_NS / 2;          // ... summed as two halves of three rows
constexpr int BA_PT = 10;                 // per point: Vp (6), gp (3), its cost

// The workspace in doubles, every part a multiple of 16 bytes from a 16-byte aligned base: cp = cap rounded up to even;
// X[2] (3 cp each, point i at 3 i), lin[2] ((10 + 18 Fm) cp each: point i's Vp, gp, cost at 10 i, then its W of free view f
// at 10 cp + 18 (f cp + i)), Y (18 Fm cp, as W), then the used bytes.  Fm = n_views - 1 whatever the mask.
struct Layout {
    size_t cp, X, lin, lin_size, Y, used, bytes;     // X and lin: the first of two; the second follows it
};

__host__ __device__ inline Layout layout(int n_views, int cap)
{
    Layout l;
    const size_t fm = static_cast<size_t>(n_views - 1);
    l.cp = (static_cast<size_t>(cap) + 1) & ~static_cast<size_t>(1);
    l.X = 0;
    l.lin = 6 * l.cp;
    l.lin_size = (BA_PT + 18 * fm) * l.cp;
    l.Y = l.lin + 2 * l.lin_size;
    l.used = (l.Y + 18 * fm * l.cp) * sizeof(double);
    l.bytes = 16 + l.used + ((l.cp + 15) & ~static_cast<size_t>(15));      // 16: room to align the base
    return l;
}

struct Args {
    const float* uv[BA_MAXV];
    const double* Rt[BA_MAXV];
    const int32_t* count;
    int cap, n_views;
    Cam k;
    double gate2;                         // gate_px^2; 0: no gate
    int max_iters;
    unsigned fixed_mask;
    double* Rt_out;
    float* xyz;
    uint8_t* used_out;
    char* work;
    pm_ba_info* info;
};

// S114: one observation
struct Obs {
    double e, ru, rv, ju[6], jv[6], cu[3], cv[3];
    bool depth_ok;
};

__device__ __forceinline__ void observe(const Cam& k, const double (&P)[12], const double (&X)[3], float2 pix, Obs& o)
{
    double Y[3], xc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        Y[r] = (P[3 * r] * X[0] + P[3 * r + 1] * X[1]) + P[3 * r + 2] * X[2];
        xc[r] = Y[r] + P[9 + r];
    }
    o.depth_ok = xc[2] > 0.0 && xc[2] < __builtin_inf();
    const double iz = 1.0 / xc[2];
    const double px = xc[0] * iz, py = xc[1] * iz;
    o.ru = (k.fx * px + k.cx) - static_cast<double>(pix.x);
    o.rv = (k.fy * py + k.cy) - static_cast<double>(pix.y);
    o.e = fma(o.ru, o.ru, o.rv * o.rv);
    const double fa = k.fx * iz, fb = k.fy * iz;
    const double a = fa * px, b = fb * py;
    o.ju[0] = -(a * Y[1]); o.ju[1] = fa * Y[2] + a * Y[0]; o.ju[2] = -(fa * Y[1]); o.ju[3] = fa; o.ju[4] = 0.0; o.ju[5] = -a;
    o.jv[0] = -(fb * Y[2]) - b * Y[1]; o.jv[1] = b * Y[0]; o.jv[2] = fb * Y[0]; o.jv[3] = 0.0; o.jv[4] = fb; o.jv[5] = -b;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o.cu[c] = fa * P[c] - a * P[6 + c];
        o.cv[c] = fb * P[3 + c] - b * P[6 + c];
    }
}

// The poses in LDS change only between passes, so the compiler would hoist their loads out of the point loops and hold 12
// doubles in registers through every pass (triangulate.hip's pose_fence).  This keeps each load next to its use.
__device__ __forceinline__ void lds_fence() { asm volatile("" ::: "memory"); }

__global__ __launch_bounds__(HR_P) void bundle_adjust(Args a)
{
    __shared__ double s_x[HR_CH][HR_P / 2];
    __shared__ double s_red[BA_NS];
    __shared__ double s_S[BA_MAXM * BA_MAXM];      // upper entries: the reduced system; lower and diagonal: its L
    __shared__ double s_rhs[BA_MAXM], s_y[BA_MAXM], s_d[BA_MAXM];
    __shared__ double s_U[2][BA_MAXF][BA_NU];      // U, gc of the two linearisations
    __shared__ double s_in[BA_MAXV][12], s_cur[BA_MAXV][12], s_tr[BA_MAXV][12];
    __shared__ double s_max[3][HR_P / 64];
    __shared__ const float* s_uv[BA_MAXV];
    __shared__ int s_fview[BA_MAXV], s_fidx[BA_MAXV];
    __shared__ double s_st[6];                     // the run's uniform state: see ST_*
    __shared__ int s_ok;

    const int tid = static_cast<int>(threadIdx.x);
    const int V = a.n_views;
    const Cam k = a.k;
    // every input pose is read before anything is written: Rt_out may alias the poses
#pragma unroll
    for (int v = 0; v < BA_MAXV; ++v) {
        if (v < V && tid < 12) {
            const double* p = a.Rt[v];
            const double x = p ? p[tid] : ((tid < 9 && tid % 4 == 0) ? 1.0 : 0.0);
            s_in[v][tid] = x; s_cur[v][tid] = x; s_tr[v][tid] = x;
        }
        if (tid == 0) s_uv[v] = a.uv[v];
    }
    if (tid == 0) {
        int f = 0;
        for (int v = 0; v < V; ++v) {
            s_fidx[v] = -1;
            if (!((a.fixed_mask >> v) & 1u)) { s_fidx[v] = f; s_fview[f++] = v; }
        }
    }
    __syncthreads();
    const int F = V - __popc(a.fixed_mask & ((1u << V) - 1u));
    const int M = 6 * F;

    const int n = pm::clamped_count(a.count, a.cap);
    const Layout lay = layout(V, a.cap);
    const size_t cp = lay.cp;
    char* const base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(a.work) + 15) & ~static_cast<uintptr_t>(15));
    double* const wd = reinterpret_cast<double*>(base);
    uint8_t* const wused = reinterpret_cast<uint8_t*>(base + lay.used);
    double* const Yb = wd + lay.Y;

    // ---- S113: the used set, the counts, the fp64 start
    {
        double acc[2 + BA_MAXV];
#pragma unroll
        for (int e = 0; e < 2 + BA_MAXV; ++e) acc[e] = 0.0;
        double* X0 = wd + lay.X;
        for (int i = tid; i < n; i += HR_P) {
            const float* row = a.xyz + 3 * static_cast<size_t>(i);
            const double X[3] = {static_cast<double>(row[0]), static_cast<double>(row[1]), static_cast<double>(row[2])};
            bool fin = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                X0[3 * static_cast<size_t>(i) + c] = X[c];
                fin = fin && fabs(X[c]) < __builtin_inf();
            }
            unsigned bits = 0u;
            int cnt = 0;
            for (int v = 0; v < V && fin; ++v) {
                const float2 pix = *reinterpret_cast<const float2*>(s_uv[v] + 2 * static_cast<size_t>(i));
                const float2 q = pm_essential::normalise(k, pix);
                if (!(q.x == q.x && q.y == q.y)) continue;
                double P[12];
#pragma unroll
                for (int j = 0; j < 12; ++j) P[j] = s_in[v][j];
                Obs ob;
                observe(k, P, X, pix, ob);
                if (!ob.depth_ok) continue;
                if (a.gate2 > 0.0 && !(ob.e <= a.gate2)) continue;
                bits |= 1u << v;
                ++cnt;
            }
            if (cnt < 2) bits = 0u;
            wused[i] = static_cast<uint8_t>(bits);
            if (a.used_out) a.used_out[i] = static_cast<uint8_t>(bits);
            if (bits) {
                acc[0] = acc[0] + 1.0;
                acc[1] = acc[1] + static_cast<double>(cnt);
#pragma unroll
                for (int v = 0; v < BA_MAXV; ++v) acc[2 + v] = acc[2 + v] + (((bits >> v) & 1u) ? 1.0 : 0.0);
            }
        }
        tree<2 + BA_MAXV>(acc, tid, s_x, s_red);
    }
    // The run's uniform state lives in LDS, written by thread 0 behind a barrier and read where it is used: held in
    // registers across the passes it pushed the 42-partial pass into private memory.
    enum { ST_NPOINTS, ST_NOBS, ST_COST, ST_COST_IN, ST_CUR, ST_LAM };
    int few_i = !(s_red[0] > 0.0);
    for (int f = 0; f < F; ++f) few_i |= s_red[2 + s_fview[f]] < 4.0;
    const bool few = __builtin_amdgcn_readfirstlane(few_i) != 0;
    if (tid == 0) { s_st[ST_NPOINTS] = s_red[0]; s_st[ST_NOBS] = s_red[1]; }

    // ---- S114: the linearisation of the state (sP, Xs) into Lb and Uo; returns the cost
    auto linearise = [&](const double (*sP)[12], const double* Xs, double* Lb, double (*Uo)[BA_NU]) {
        double bad = 0.0;
        for (int v = 0; v < V; ++v) {
            const int fa = s_fidx[v];
            const float* puv = s_uv[v];
            double acc[BA_NU];
#pragma unroll
            for (int e = 0; e < BA_NU; ++e) acc[e] = 0.0;
            for (int i = tid; i < n; i += HR_P) {
                const unsigned ub = wused[i];
                if (!ub) continue;
                const bool sees = ((ub >> v) & 1u) != 0u;
                if (!sees && v > 0) continue;
                double pt[BA_PT];
#pragma unroll
                for (int e = 0; e < BA_PT; ++e) pt[e] = v == 0 ? 0.0 : Lb[BA_PT * static_cast<size_t>(i) + e];
                if (sees) {
                    const double X[3] = {Xs[3 * static_cast<size_t>(i)], Xs[3 * static_cast<size_t>(i) + 1], Xs[3 * static_cast<size_t>(i) + 2]};
                    lds_fence();
                    double P[12];
#pragma unroll
                    for (int j = 0; j < 12; ++j) P[j] = sP[v][j];
                    Obs ob;
                    observe(k, P, X, *reinterpret_cast<const float2*>(puv + 2 * static_cast<size_t>(i)), ob);
                    if (!ob.depth_ok) bad = 1.0;
                    int e = 0;
#pragma unroll
                    for (int j = 0; j < 3; ++j)
#pragma unroll
                        for (int q = j; q < 3; ++q, ++e) pt[e] = pt[e] + fma(ob.cu[j], ob.cu[q], ob.cv[j] * ob.cv[q]);
#pragma unroll
                    for (int j = 0; j < 3; ++j) pt[6 + j] = pt[6 + j] + fma(ob.cu[j], ob.ru, ob.cv[j] * ob.rv);
                    pt[9] = pt[9] + ob.e;
                    if (fa >= 0) {
                        double* W = Lb + BA_PT * cp + 18 * (static_cast<size_t>(fa) * cp + i);
#pragma unroll
                        for (int j = 0; j < 6; ++j)
#pragma unroll
                            for (int c = 0; c < 3; ++c) W[3 * j + c] = fma(ob.ju[j], ob.cu[c], ob.jv[j] * ob.cv[c]);
                        e = 0;
#pragma unroll
                        for (int j = 0; j < 6; ++j)
#pragma unroll
                            for (int q = j; q < 6; ++q, ++e) acc[e] = acc[e] + fma(ob.ju[j], ob.ju[q], ob.jv[j] * ob.jv[q]);
#pragma unroll
                        for (int j = 0; j < 6; ++j) acc[21 + j] = acc[21 + j] + fma(ob.ju[j], ob.ru, ob.jv[j] * ob.rv);
                    }
                }
#pragma unroll
                for (int e = 0; e < BA_PT; ++e) Lb[BA_PT * static_cast<size_t>(i) + e] = pt[e];
            }
            if (fa >= 0) {
                tree<BA_NU>(acc, tid, s_x, s_red);
                if (tid < BA_NU) Uo[fa][tid] = s_red[tid];
            }
        }
        double acc[2] = {0.0, bad};
        for (int i = tid; i < n; i += HR_P)
            if (wused[i]) acc[0] = acc[0] + Lb[BA_PT * static_cast<size_t>(i) + 9];
        tree<2>(acc, tid, s_x, s_red);
        if (tid == 0) s_st[ST_COST] = s_red[1] > 0.0 ? __builtin_inf() : s_red[0];
        __syncthreads();                       // the cost and Uo are settled for every thread
    };

    int cl = 0, cx = 0, iters = 0, accepted = 0;  // which linearisation and which X hold the current state
    linearise(s_in, wd + lay.X, wd + lay.lin, s_U[0]);
    if (tid == 0) { s_st[ST_COST_IN] = s_st[ST_COST]; s_st[ST_CUR] = s_st[ST_COST]; s_st[ST_LAM] = LM_LAMBDA0; }
    __syncthreads();

    if (!few && a.max_iters > 0) {
        for (int it = 0; it < a.max_iters; ++it) {
            const double lam = s_st[ST_LAM];
            const double* Lc = wd + lay.lin + cl * lay.lin_size;
            const double* Xc = wd + lay.X + cx * 3 * cp;
            double* Xt = wd + lay.X + (1 - cx) * 3 * cp;
            // ---- S115 steps 1-2: the damped point blocks and Y = W Vp*^-1
            int fail = 0;
            for (int i = tid; i < n; i += HR_P) {
                const unsigned ub = wused[i];
                if (!ub) continue;
                double H[6], L[3][3];
#pragma unroll
                for (int e = 0; e < 6; ++e) H[e] = Lc[BA_PT * static_cast<size_t>(i) + e];
                if (!lm_factor<3>(H, lam, L)) { fail = 1; continue; }
                for (int f = 0; f < F; ++f) {
                    if (!((ub >> s_fview[f]) & 1u)) continue;
                    const double* W = Lc + BA_PT * cp + 18 * (static_cast<size_t>(f) * cp + i);
                    double* Y = Yb + 18 * (static_cast<size_t>(f) * cp + i);
#pragma unroll
                    for (int j = 0; j < 6; ++j) {
                        const double w[3] = {W[3 * j], W[3 * j + 1], W[3 * j + 2]};
                        double y[3];
                        lm_subst<3>(L, w, y);
#pragma unroll
                        for (int c = 0; c < 3; ++c) Y[3 * j + c] = y[c];
                    }
                }
            }
            if (__syncthreads_or(fail)) break;
            // ---- step 3: the reduced system, one pair of free views at a time
            for (int fa = 0; fa < F; ++fa)
                for (int fb = fa; fb < F; ++fb) {
                    const int va = s_fview[fa], vb = s_fview[fb];
                    const bool diag = fa == fb;
                    // rows 0-2 and rows 3-5 of the block are summed apart, 21 partials each (18 of Y W^T, 3 of Y gp): all 42 at
                    // once, with the 18 + 18 doubles of a point in flight, did not fit the 256 registers of a wave here
#pragma unroll 1
                    for (int h = 0; h < 2; ++h) {
                        double acc[BA_NH];
#pragma unroll
                        for (int e = 0; e < BA_NH; ++e) acc[e] = 0.0;
                        for (int i = tid; i < n; i += HR_P) {
                            const unsigned ub = wused[i];
                            if (!((ub >> va) & (ub >> vb) & 1u)) continue;
                            const double* Y = Yb + 18 * (static_cast<size_t>(fa) * cp + i) + 9 * h;
                            const double* W = Lc + BA_PT * cp + 18 * (static_cast<size_t>(fb) * cp + i);
                            const double* g = Lc + BA_PT * static_cast<size_t>(i) + 6;
                            double w[18];
#pragma unroll
                            for (int e = 0; e < 18; ++e) w[e] = W[e];
                            const double g0 = diag ? g[0] : 0.0, g1 = diag ? g[1] : 0.0, g2 = diag ? g[2] : 0.0;
#pragma unroll
                            for (int j = 0; j < 3; ++j) {
                                const double y0 = Y[3 * j], y1 = Y[3 * j + 1], y2 = Y[3 * j + 2];
#pragma unroll
                                for (int q = 0; q < 6; ++q)
                                    acc[6 * j + q] = acc[6 * j + q] + fma(y2, w[3 * q + 2], fma(y1, w[3 * q + 1], y0 * w[3 * q]));
                                if (diag) acc[18 + j] = acc[18 + j] + fma(y2, g2, fma(y1, g1, y0 * g0));
                            }
                        }
                        tree<BA_NH>(acc, tid, s_x, s_red);
                        if (tid < 18) {
                            const int j = 3 * h + tid / 6, q = tid % 6;
                            if (!diag) {
                                s_S[(6 * fa + j) * BA_MAXM + 6 * fb + q] = -s_red[tid];
                            } else if (j <= q) {
                                const double u = s_U[cl][fa][j * 6 - j * (j - 1) / 2 + (q - j)];
                                s_S[(6 * fa + j) * BA_MAXM + 6 * fa + q] = (j == q ? u + lam * u : u) - s_red[tid];
                            }
                        } else if (tid < BA_NH && diag) {
                            const int j = 3 * h + tid - 18;
                            s_rhs[6 * fa + j] = s_red[tid] - s_U[cl][fa][21 + j];
                        }
                    }
                }
            __syncthreads();
            // ---- step 4: Cholesky of the reduced system, row i of a column on thread i; then thread 0 substitutes
            bool stop = false;
            for (int j = 0; j < M; ++j) {
                if (tid == j) {
                    double dd = s_S[j * BA_MAXM + j];
                    for (int q = 0; q < j; ++q) dd = fma(-s_S[j * BA_MAXM + q], s_S[j * BA_MAXM + q], dd);
                    const bool ok = dd > 0.0 && dd < __builtin_inf();
                    s_ok = ok ? 1 : 0;
                    if (ok) s_S[j * BA_MAXM + j] = sqrt(dd);
                }
                __syncthreads();
                if (!s_ok) { stop = true; break; }
                if (tid > j && tid < M) {
                    double v = s_S[j * BA_MAXM + tid];
                    for (int q = 0; q < j; ++q) v = fma(-s_S[tid * BA_MAXM + q], s_S[j * BA_MAXM + q], v);
                    s_S[tid * BA_MAXM + j] = v / s_S[j * BA_MAXM + j];
                }
                __syncthreads();
            }
            if (stop) break;
            if (tid == 0) {
                for (int i = 0; i < M; ++i) {
                    double v = s_rhs[i];
                    for (int q = 0; q < i; ++q) v = fma(-s_S[i * BA_MAXM + q], s_y[q], v);
                    s_y[i] = v / s_S[i * BA_MAXM + i];
                }
                for (int i = M - 1; i >= 0; --i) {
                    double v = s_y[i];
                    for (int q = i + 1; q < M; ++q) v = fma(-s_S[q * BA_MAXM + i], s_d[q], v);
                    s_d[i] = v / s_S[i * BA_MAXM + i];
                }
            }
            __syncthreads();
            // ---- steps 5-6: the point steps, the trial points, the step test
            double dmax = 0.0, hmax = 1.0, nonfin = 0.0;
            if (tid < M) {
                const double x = fabs(s_d[tid]);
                if (!(x < __builtin_inf())) nonfin = 1.0;
                if (x > dmax) dmax = x;
            }
            if (tid < 3 * F) {
                const double x = fabs(s_cur[s_fview[tid / 3]][9 + tid % 3]);
                if (x > hmax) hmax = x;
            }
            for (int i = tid; i < n; i += HR_P) {
                const unsigned ub = wused[i];
                if (!ub) continue;
                double H[6], L[3][3], r[3], dp[3];
#pragma unroll
                for (int e = 0; e < 6; ++e) H[e] = Lc[BA_PT * static_cast<size_t>(i) + e];
                lm_factor<3>(H, lam, L);              // succeeded above on the same numbers
#pragma unroll
                for (int c = 0; c < 3; ++c) r[c] = -Lc[BA_PT * static_cast<size_t>(i) + 6 + c];
                for (int f = 0; f < F; ++f) {
                    if (!((ub >> s_fview[f]) & 1u)) continue;
                    const double* W = Lc + BA_PT * cp + 18 * (static_cast<size_t>(f) * cp + i);
#pragma unroll
                    for (int j = 0; j < 6; ++j) {
                        const double dj = s_d[6 * f + j];
#pragma unroll
                        for (int c = 0; c < 3; ++c) r[c] = fma(-W[3 * j + c], dj, r[c]);
                    }
                }
                lm_subst<3>(L, r, dp);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double xc = Xc[3 * static_cast<size_t>(i) + c];
                    const double x = fabs(dp[c]), h = fabs(xc);
                    if (!(x < __builtin_inf())) nonfin = 1.0;
                    if (x > dmax) dmax = x;
                    if (h > hmax) hmax = h;
                    Xt[3 * static_cast<size_t>(i) + c] = xc + dp[c];
                }
            }
            const auto mx = group_max3(s_max, tid, dmax, hmax, nonfin);         // of dmax, hmax, nonfin over the workgroup
            if (mx.c > 0.0 || !(mx.a > LM_STEP_TOL * mx.b)) break;
            // ---- steps 7-9: the trial poses, their linearisation, accept or reject
            if (tid < F) pose_update(s_cur[s_fview[tid]], s_d + 6 * tid, s_tr[s_fview[tid]]);
            __syncthreads();
            linearise(s_tr, Xt, wd + lay.lin + (1 - cl) * lay.lin_size, s_U[1 - cl]);
            ++iters;
            const bool better = __builtin_amdgcn_readfirstlane(static_cast<int>(s_st[ST_COST] < s_st[ST_CUR])) != 0;
            __syncthreads();                   // every thread has compared before thread 0 moves the state
            if (better) {
                ++accepted;
                cl = 1 - cl;
                cx = 1 - cx;
                if (tid < 12 * V) s_cur[tid / 12][tid % 12] = s_tr[tid / 12][tid % 12];
                if (tid == 0) { s_st[ST_CUR] = s_st[ST_COST]; s_st[ST_LAM] = s_st[ST_LAM] / 10.0; }
            } else {
                if (tid == 0) s_st[ST_LAM] = s_st[ST_LAM] * 10.0;
            }
            __syncthreads();
        }
    }

    // ---- S117: result
    if (accepted) {
        const double* Xc = wd + lay.X + cx * 3 * cp;
        for (int i = tid; i < n; i += HR_P) {
            if (!wused[i]) continue;
            float* row = a.xyz + 3 * static_cast<size_t>(i);
#pragma unroll
            for (int c = 0; c < 3; ++c) row[c] = static_cast<float>(Xc[3 * static_cast<size_t>(i) + c]);
        }
    }
    if (tid < 12 * V) {
        const int v = tid / 12, j = tid % 12;
        a.Rt_out[tid] = (accepted && s_fidx[v] >= 0) ? s_cur[v][j] : s_in[v][j];
    }
    if (tid == 0)
        *a.info = pm_ba_info{s_st[ST_COST_IN], accepted ? s_st[ST_CUR] : s_st[ST_COST_IN], static_cast<int32_t>(s_st[ST_NPOINTS]),
                             static_cast<int32_t>(s_st[ST_NOBS]), iters, accepted, few ? 2 : (accepted ? 0 : 1), 0};
}

bool camera_ok(const pm_camera* K)
{
    return std::isfinite(K->fx) && std::isfinite(K->fy) && std::isfinite(K->cx) && std::isfinite(K->cy) && K->fx > 0.0 && K->fy > 0.0;
}

// everything but the pointers of the two forms; PM_E_UNSUPPORTED comes last, after every PM_E_INVALID
int check_common(int n_views, int n, const pm_camera* K, const pm_ba_params* p)
{
    PM_REQUIRE(K != nullptr && p != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE(n_views >= 2 && n_views <= PM_TRI_MAX_VIEWS, PM_E_INVALID, "n_views outside [2, 8]");
    PM_REQUIRE(n >= 0, PM_E_INVALID, "cap or n < 0");
    PM_REQUIRE(camera_ok(K), PM_E_INVALID, "K needs finite values and fx, fy > 0");
    PM_REQUIRE(p->max_iters >= 0 && p->max_iters <= 100, PM_E_INVALID, "max_iters outside [0, 100]");
    PM_REQUIRE(std::isfinite(p->gate_px) && p->gate_px >= 0.0, PM_E_INVALID, "gate_px must be finite and >= 0");
    const uint32_t all = (1u << n_views) - 1u;
    PM_REQUIRE((p->fixed_mask & ~all) == 0, PM_E_INVALID, "fixed_mask has a bit at or above n_views");
    PM_REQUIRE((p->fixed_mask & all) != 0 && (p->fixed_mask & all) != all, PM_E_INVALID, "fixed_mask must hold a view and leave one free");
    PM_REQUIRE(p->flags == 0 && p->reserved == 0, PM_E_INVALID, "flags and reserved must be 0");
    return PM_OK;
}

}  // namespace
}  // namespace pm_ba

extern "C" size_t pm_bundle_adjust_workspace(int n_views, int cap)
{
    if (n_views < 2 || n_views > PM_TRI_MAX_VIEWS || cap < 0 || cap > PM_BA_MAX_POINTS) return 0;
    return pm_ba::layout(n_views, cap).bytes;
}

extern "C" int pm_bundle_adjust_dev(pm_ctx* ctx, const pm_tri_views* views, const pm_camera* K, const pm_ba_params* p, double* d_Rt_out,
                                    float* d_xyz, uint8_t* d_used, void* d_work, size_t work_bytes, pm_ba_info* d_info)
{
    using namespace pm_ba;
    PM_REQUIRE(views != nullptr && d_Rt_out != nullptr && d_xyz != nullptr && d_work != nullptr && d_info != nullptr, PM_E_INVALID,
               "null pointer");
    const int rc = check_common(views->n_views, views->cap, K, p);
    if (rc != PM_OK) return rc;
    Args a = {};
    for (int v = 0; v < views->n_views; ++v) {
        PM_REQUIRE(views->uv[v] != nullptr, PM_E_INVALID, "a view's uv is null");
        a.uv[v] = views->uv[v];
        a.Rt[v] = views->Rt[v];
    }
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REQUIRE(views->cap <= PM_BA_MAX_POINTS, PM_E_UNSUPPORTED, "cap above PM_BA_MAX_POINTS");
    PM_REQUIRE(work_bytes >= layout(views->n_views, views->cap).bytes, PM_E_INVALID, "work_bytes below pm_bundle_adjust_workspace()");
    a.count = views->count;
    a.cap = views->cap;
    a.n_views = views->n_views;
    a.k = Cam{K->fx, K->fy, K->cx, K->cy};
    a.gate2 = p->gate_px * p->gate_px;
    a.max_iters = p->max_iters;
    a.fixed_mask = p->fixed_mask;
    a.Rt_out = d_Rt_out; a.xyz = d_xyz; a.used_out = d_used; a.work = static_cast<char*>(d_work); a.info = d_info;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    {
        pm::ScopedKernelTime timer(ctx, "bundle_adjust");
        hipLaunchKernelGGL(bundle_adjust, dim3(1), dim3(pm_hrefine::HR_P), 0, ctx->stream, a);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_bundle_adjust(pm_ctx* ctx, const float* const* uv, const double* const* Rt, int n_views, int n, const pm_camera* K,
                                const pm_ba_params* p, double* Rt_out, float* xyz, uint8_t* used, pm_ba_info* info)
{
    using namespace pm_ba;
    PM_REQUIRE(uv != nullptr && Rt != nullptr && Rt_out != nullptr && xyz != nullptr && info != nullptr, PM_E_INVALID, "null pointer");
    const int rc = check_common(n_views, n, K, p);
    if (rc != PM_OK) return rc;
    for (int v = 0; v < n_views; ++v) PM_REQUIRE(uv[v] != nullptr, PM_E_INVALID, "a view's uv is null");
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REQUIRE(n <= PM_BA_MAX_POINTS, PM_E_UNSUPPORTED, "n above PM_BA_MAX_POINTS");
    const size_t rows = static_cast<size_t>(n), wb = layout(n_views, n).bytes;
    pm::StagedBlock b(ctx, __func__);
    size_t o_uv[PM_TRI_MAX_VIEWS], o_Rt[PM_TRI_MAX_VIEWS];
    for (int v = 0; v < n_views; ++v) { o_uv[v] = b.add(rows * 8); o_Rt[v] = b.add(Rt[v] ? 96 : 0); }
    const size_t o_out = b.add(static_cast<size_t>(n_views) * 96), o_xyz = b.add(rows * 12), o_used = b.add(used ? rows : 0);
    const size_t o_info = b.add(sizeof(pm_ba_info)), o_work = b.add(wb);
    b.alloc();
    pm_tri_views dv = {};
    for (int v = 0; v < n_views; ++v) {
        b.upload(o_uv[v], uv[v], rows * 8);
        if (Rt[v]) b.upload(o_Rt[v], Rt[v], 96);
        dv.uv[v] = b.at<const float>(o_uv[v]);
        dv.Rt[v] = Rt[v] ? b.at<const double>(o_Rt[v]) : nullptr;
    }
    b.upload(o_xyz, xyz, rows * 12);
    dv.count = nullptr;
    dv.n_views = n_views;
    dv.cap = n;
    if (b.rc == PM_OK)
        b.rc = pm_bundle_adjust_dev(ctx, &dv, K, p, b.at<double>(o_out), b.at<float>(o_xyz), used ? b.at<uint8_t>(o_used) : nullptr,
                                    b.at<void>(o_work), wb, b.at<pm_ba_info>(o_info));
    b.download(Rt_out, o_out, static_cast<size_t>(n_views) * 96);
    b.download(xyz, o_xyz, rows * 12);
    if (used) b.download(used, o_used, rows);
    b.download(info, o_info, sizeof(pm_ba_info));
    return b.sync();
}
