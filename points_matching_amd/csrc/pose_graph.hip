// pose_graph.hip — pose-graph optimisation in ONE launch on gfx950 (MI355X), docs/SPEC.md S118-S123: Levenberg-Marquardt over
// the free nodes of a graph of SE(3) or Sim(3) poses on the weighted between-residuals of its edges, each step solved by
// conjugate gradients with the nodes' damped diagonal blocks as the preconditioner.  It is the last step of a loop closer:
// pm_align3d_refine_dev leaves the measured loop transform in a row of the edge array, this call spreads the loop error over
// the keyframes, and pm_pgo_move_points* (the second kernel here) moves the map rows with the keyframes they hang on.
//
// One workgroup of HR_P = 512 threads on refine_reduce.hpp, as bundle_adjust.hip: thread p owns partial p of S23's fixed
// reduction order and walks the edges e = p, p + 512, ... and the nodes i = p, p + 512, ...  Unlike bundle adjustment, values
// in the caller's workspace cross threads here: an edge's residual and blocks are written by the edge's thread and read by the
// threads of its two nodes, q = J p goes the same way in every conjugate-gradient iteration, and the nodes' p and trial poses
// go back to the edges' threads.  Every such hand-over has a __syncthreads() between the stores and the loads (the barrier of
// a tree<K> where one follows anyway); the waves of one workgroup share one vector L1, the workspace pointers carry no
// __restrict__ and nothing of the workspace is read before the kernel first writes it, so the loads stay on the vector path.
// The records have one base address and constant offsets: per edge its residual and two blocks, per node its
// packed diagonal block and gradient, its factor and its five conjugate-gradient vectors; Jacobian rows are streamed from
// there, no block is held in registers.  The incidence lists (per node its used edges in ascending id) are built on the
// device without atomics: edges are taken 512 at a time, an edge's rank among the round's earlier edges at the same node comes
// from a scan of the round's node pairs in LDS, so the lists do not depend on the order in which waves run.
//
// The launch keeps no per-call state and allocates nothing, so the device form may be captured; the host form stages its
// rows and the workspace through pm::StagedBlock and synchronises once.
#include <cmath>

#include "lm_core.hpp"
#include "pm_common.hpp"
#include "refine_reduce.hpp"

namespace pm_pgo {
namespace {

using pm_hrefine::HR_CH;
using pm_hrefine::HR_P;
using pm_hrefine::LM_LAMBDA0;
using pm_hrefine::LM_STEP_TOL;
using pm_hrefine::group_max3;
using pm_hrefine::lm_factor;
using pm_hrefine::lm_subst;
using pm_hrefine::pose_update;
using pm_hrefine::tree;

constexpr int PS = 13;                      // doubles of a pose: R (9), t (3), s (1)

constexpr int params_of(int model) { return model == PM_PGO_SIM3 ? 7 : 6; }

// The workspace, every part from a 16-byte aligned base.  Doubles first: T[2] (13 N each), the nodes' linearisations [2]
// (node i's D then g at (TRI + P) i), their factors (TRI N, the lower triangle row-major), their vectors (5 P N: x, r, z, p,
// Ap of node i at 5 P i), the edges' linearisations [2] (edge e's r, Ja, Jb at (P + 2 P P) e), q (P E); then int32: start
// (N + 1), cursor (N), inc (2 E); then bytes: used (E), free (N).
struct Layout {
    size_t T, nlin, nlin_size, fac, vec, elin, elin_size, q, doubles;      // offsets in doubles
    size_t ints, bytes8, bytes;                                            // offsets in bytes; bytes: the whole workspace
};

__host__ __device__ inline Layout layout(int n_nodes, int cap_edges, int P)
{
    const size_t N = static_cast<size_t>(n_nodes), E = static_cast<size_t>(cap_edges), p = static_cast<size_t>(P);
    const size_t tri = p * (p + 1) / 2;
    Layout l;
    l.T = 0;
    l.nlin = 2 * PS * N;
    l.nlin_size = (tri + p) * N;
    l.fac = l.nlin + 2 * l.nlin_size;
    l.vec = l.fac + tri * N;
    l.elin = l.vec + 5 * p * N;
    l.elin_size = (p + 2 * p * p) * E;
    l.q = l.elin + 2 * l.elin_size;
    l.doubles = l.q + p * E;
    l.ints = 8 * l.doubles;
    l.bytes8 = l.ints + 4 * (2 * N + 1 + 2 * E);
    l.bytes = (16 + l.bytes8 + E + N + 15) & ~static_cast<size_t>(15);     // 16: room to align the base
    return l;
}

struct Args {
    const double* pose_in;
    const uint8_t* fixed;
    const int32_t* ab;
    const double* Z;
    const double* w;
    const int32_t* count;
    int n_nodes, cap_edges, max_iters, cg_iters;
    double cg_tol2;                         // cg_tol^2
    double* pose_out;
    uint8_t* used_out;
    char* work;
    pm_pgo_info* info;
};

__device__ __forceinline__ bool finite_all(const double* v, int n)
{
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = ok && fabs(v[i]) < __builtin_inf();
    return ok;
}

// S119: the residual and the two blocks of one edge into its record (r, Ja, Jb); true iff den > 2^-10
template <int P>
__device__ __forceinline__ bool edge_eval(const double* Ap, const double* Bp, const double* Zp, const double* wp, double* rec)
{
    double A[PS], B[PS], Z[PS];
#pragma unroll
    for (int i = 0; i < PS; ++i) { A[i] = Ap[i]; B[i] = Bp[i]; Z[i] = Zp[i]; }
    const double wr = wp[0], wt = wp[1], ws = wp[2];
    double* const r = rec;
    double* const Ja = rec + P;
    double* const Jb = rec + P + P * P;
    double RD[9], Er[9], m[3], g[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) RD[3 * i + c] = (B[3 * i] * A[3 * c] + B[3 * i + 1] * A[3 * c + 1]) + B[3 * i + 2] * A[3 * c + 2];
    const double sD = B[12] / A[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double u = (RD[3 * i] * A[9] + RD[3 * i + 1] * A[10]) + RD[3 * i + 2] * A[11];
        m[i] = sD * u;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) Er[3 * i + c] = (Z[i] * RD[c] + Z[3 + i] * RD[3 + c]) + Z[6 + i] * RD[6 + c];
    const double den = 1.0 + ((Er[0] + Er[4]) + Er[8]);
    const double id = 1.0 / den;
    g[0] = (Er[7] - Er[5]) * id; g[1] = (Er[2] - Er[6]) * id; g[2] = (Er[3] - Er[1]) * id;
#pragma unroll
    for (int e = 0; e < 2 * P * P; ++e) Ja[e] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r[k] = wr * (2.0 * g[k]);
        r[3 + k] = wt * ((B[9 + k] - m[k]) - Z[9 + k]);
    }
    if (P == 7) {
        const double sigma = sD / Z[12];
        const double is = 1.0 / sigma;
        const double c = 0.5 * (sigma + is);
        r[P - 1] = ws * (0.5 * (sigma - is));
        Ja[P * (P - 1) + P - 1] = -(ws * c);
        Jb[P * (P - 1) + P - 1] = ws * c;
    }
    // rotation rows: [g]x = (0, -g2, g1; g2, 0, -g0; -g1, g0, 0)
    const double X[9] = {0.0, -g[2], g[1], g[2], 0.0, -g[0], -g[1], g[0], 0.0};
    double Mb[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double base = (i == k ? 1.0 : 0.0) + g[i] * g[k];
            Ja[P * i + k] = -(wr * (base + X[3 * i + k]));
            Mb[3 * i + k] = base - X[3 * i + k];
        }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            Jb[P * i + k] = wr * ((Mb[3 * i] * Z[3 * k] + Mb[3 * i + 1] * Z[3 * k + 1]) + Mb[3 * i + 2] * Z[3 * k + 2]);
    // translation rows
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double q0 = wt * (sD * RD[3 * i]), q1 = wt * (sD * RD[3 * i + 1]), q2 = wt * (sD * RD[3 * i + 2]);
        double* ja = Ja + P * (3 + i);
        ja[0] = -(q1 * A[11] - q2 * A[10]);
        ja[1] = -(q2 * A[9] - q0 * A[11]);
        ja[2] = -(q0 * A[10] - q1 * A[9]);
        ja[3] = -q0; ja[4] = -q1; ja[5] = -q2;
        Jb[P * (3 + i) + 3 + i] = wt;
    }
    const double wm0 = wt * m[0], wm1 = wt * m[1], wm2 = wt * m[2];
    Jb[P * 3 + 1] = -wm2; Jb[P * 3 + 2] = wm1;
    Jb[P * 4 + 0] = wm2;  Jb[P * 4 + 2] = -wm0;
    Jb[P * 5 + 0] = -wm1; Jb[P * 5 + 1] = wm0;
    if (P == 7) {
        Ja[P * 3 + 6] = wm0; Ja[P * 4 + 6] = wm1; Ja[P * 5 + 6] = wm2;
        Jb[P * 3 + 6] = -wm0; Jb[P * 4 + 6] = -wm1; Jb[P * 5 + 6] = -wm2;
    }
    return den > 0.0009765625;
}

// t = a_0 b_0, t = fma(a_j, b_j, t)
template <int P>
__device__ __forceinline__ double dot(const double* a, const double* b)
{
    double t = a[0] * b[0];
#pragma unroll
    for (int j = 1; j < P; ++j) t = fma(a[j], b[j], t);
    return t;
}

// the packed lower triangle of a node's factor into the array lm_subst reads (its upper entries are never read)
template <int P>
__device__ __forceinline__ void load_factor(const double* f, double (&L)[P][P])
{
    int e = 0;
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int k = 0; k < P; ++k) L[i][k] = k <= i ? f[e++] : 0.0;
}

template <int P>
__global__ __launch_bounds__(HR_P) void pose_graph(Args a)
{
    constexpr int TRI = P * (P + 1) / 2;
    constexpr int NL = TRI + P;             // a node's linearisation: D, g
    constexpr int ER = P + 2 * P * P;       // an edge's linearisation: r, Ja, Jb
    enum { VX = 0, VR = P, VZ = 2 * P, VP = 3 * P, VAP = 4 * P, NV = 5 * P };

    __shared__ double s_x[HR_CH][HR_P / 2];
    __shared__ double s_red[4];
    __shared__ double s_max[3][HR_P / 64];
    __shared__ int s_ea[HR_P], s_eb[HR_P], s_scan[HR_P];
    __shared__ double s_cost;

    const int tid = static_cast<int>(threadIdx.x);
    const int N = a.n_nodes;
    const int n = pm::clamped_count(a.count, a.cap_edges);
    const Layout lay = layout(N, a.cap_edges, P);
    char* const base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(a.work) + 15) & ~static_cast<uintptr_t>(15));
    double* const wd = reinterpret_cast<double*>(base);
    int* const start = reinterpret_cast<int*>(base + lay.ints);
    int* const cursor = start + (N + 1);
    int* const inc = cursor + N;
    uint8_t* const wused = reinterpret_cast<uint8_t*>(base + lay.bytes8);
    uint8_t* const wfree = wused + a.cap_edges;
    double* const fac = wd + lay.fac;
    double* const vec = wd + lay.vec;
    double* const qv = wd + lay.q;

    // ---- every input pose is read before anything is written: pose_out may be pose_in
    for (int i = tid; i < PS * N; i += HR_P) {
        const double v = a.pose_in[i];
        wd[lay.T + i] = v;
        wd[lay.T + static_cast<size_t>(PS) * N + i] = v;
    }
    for (int i = tid; i < N; i += HR_P) cursor[i] = 0;
    __syncthreads();

    // ---- S118: the used set
    double cnt[3] = {0.0, 0.0, 0.0};        // used edges, free nodes, fixed nodes
    for (int e = tid; e < n; e += HR_P) {
        const int na = a.ab[2 * static_cast<size_t>(e)], nb = a.ab[2 * static_cast<size_t>(e) + 1];
        bool u = na >= 0 && na < N && nb >= 0 && nb < N && na != nb;
        if (u) {
            const double* A = wd + lay.T + static_cast<size_t>(PS) * na;
            const double* B = wd + lay.T + static_cast<size_t>(PS) * nb;
            const double* Ze = a.Z + static_cast<size_t>(PS) * e;
            const double* we = a.w + 3 * static_cast<size_t>(e);
            u = finite_all(Ze, PS) && finite_all(we, 3) && finite_all(A, PS) && finite_all(B, PS);
            u = u && Ze[12] > 0.0 && A[12] > 0.0 && B[12] > 0.0;
            u = u && !(a.fixed[na] && a.fixed[nb]);
            if (u) u = edge_eval<P>(A, B, Ze, we, wd + lay.elin + static_cast<size_t>(ER) * e);
        }
        wused[e] = u ? 1 : 0;
        if (a.used_out) a.used_out[e] = u ? 1 : 0;
        if (u) cnt[0] = cnt[0] + 1.0;
    }
    __syncthreads();

    // ---- the incidence lists: two sweeps over the used edges, 512 at a time.  An edge's slot at a node is the node's cursor
    // plus the number of earlier edges of the round at that node; the round's last edge at a node moves the cursor.
    auto sweep = [&](bool fill) {
        for (int e0 = 0; e0 < n; e0 += HR_P) {
            const int e = e0 + tid;
            const bool u = e < n && wused[e];
            const int na = u ? a.ab[2 * static_cast<size_t>(e)] : -1, nb = u ? a.ab[2 * static_cast<size_t>(e) + 1] : -1;
            s_ea[tid] = na;
            s_eb[tid] = nb;
            __syncthreads();
            int ra = 0, rb = 0, ca = 0, cb = 0;
            bool la = true, lb = true;
            if (u) {
                ca = cursor[na];
                cb = cursor[nb];
                const int jn = n - e0 < HR_P ? n - e0 : HR_P;
                for (int j = 0; j < jn; ++j) {
                    const int ja = s_ea[j], jb = s_eb[j];
                    const bool ma = ja == na || jb == na, mb = ja == nb || jb == nb;
                    if (j < tid) { ra += ma; rb += mb; }
                    if (j > tid) { la = la && !ma; lb = lb && !mb; }
                }
            }
            __syncthreads();                   // every cursor of the round is read before one moves
            if (u) {
                if (fill) { inc[ca + ra] = 2 * e; inc[cb + rb] = 2 * e + 1; }
                if (la) cursor[na] = ca + ra + 1;
                if (lb) cursor[nb] = cb + rb + 1;
            }
            __syncthreads();
        }
    };
    sweep(false);                             // cursor[i] = the degree of node i
    {
        const int chunk = (N + HR_P - 1) / HR_P, i0 = tid * chunk, i1 = i0 + chunk < N ? i0 + chunk : N;
        int sum = 0;
        for (int i = i0; i < i1; ++i) sum += cursor[i];
        s_scan[tid] = sum;
        __syncthreads();
        if (tid == 0) {
            int run = 0;
            for (int t = 0; t < HR_P; ++t) { const int v = s_scan[t]; s_scan[t] = run; run += v; }
            start[N] = run;
        }
        __syncthreads();
        int run = s_scan[tid];
        for (int i = i0; i < i1; ++i) {
            const int d = cursor[i];
            const bool fx = a.fixed[i] != 0;
            start[i] = run;
            cursor[i] = run;
            wfree[i] = (!fx && d > 0) ? 1 : 0;
            if (!fx && d > 0) cnt[1] = cnt[1] + 1.0;
            if (fx) cnt[2] = cnt[2] + 1.0;
            run += d;
        }
        __syncthreads();
    }
    sweep(true);
    tree<3>(cnt, tid, s_x, s_red);
    const double n_used = s_red[0], n_free = s_red[1];
    const bool few = __builtin_amdgcn_readfirstlane(static_cast<int>(!(s_red[0] > 0.0) || !(s_red[2] > 0.0))) != 0;

    // ---- S120: the linearisation at the poses Ts into the buffers of index lb; the cost goes to s_cost
    auto linearise = [&](const double* Ts, double bad, int lb) {
        double* const El = wd + lay.elin + lb * lay.elin_size;
        double* const Nl = wd + lay.nlin + lb * lay.nlin_size;
        double acc[2] = {0.0, bad};
        for (int e = tid; e < n; e += HR_P) {
            if (!wused[e]) continue;
            double* rec = El + static_cast<size_t>(ER) * e;
            const int na = a.ab[2 * static_cast<size_t>(e)], nb = a.ab[2 * static_cast<size_t>(e) + 1];
            if (!edge_eval<P>(Ts + static_cast<size_t>(PS) * na, Ts + static_cast<size_t>(PS) * nb, a.Z + static_cast<size_t>(PS) * e,
                              a.w + 3 * static_cast<size_t>(e), rec))
                acc[1] = 1.0;
            double c = 0.0;
#pragma unroll
            for (int k = 0; k < P; ++k) c = fma(rec[k], rec[k], c);
            acc[0] = acc[0] + c;
        }
        tree<2>(acc, tid, s_x, s_red);        // its barriers stand between the edges' stores and the nodes' loads
        if (tid == 0) s_cost = s_red[1] > 0.0 ? __builtin_inf() : s_red[0];
        for (int i = tid; i < N; i += HR_P) {
            if (!wfree[i]) continue;
            double D[NL];
#pragma unroll
            for (int k = 0; k < NL; ++k) D[k] = 0.0;
            const int s1 = start[i + 1];
            for (int s = start[i]; s < s1; ++s) {
                const int ent = inc[s];
                const double* rec = El + static_cast<size_t>(ER) * (ent >> 1);
                const double* J = rec + P + (ent & 1) * (P * P);
#pragma unroll 1
                for (int row = 0; row < P; ++row) {
                    double Jr[P];
#pragma unroll
                    for (int j = 0; j < P; ++j) Jr[j] = J[P * row + j];
                    const double rr = rec[row];
                    int k = 0;
#pragma unroll
                    for (int j = 0; j < P; ++j)
#pragma unroll
                        for (int c = j; c < P; ++c, ++k) D[k] = fma(Jr[j], Jr[c], D[k]);
#pragma unroll
                    for (int j = 0; j < P; ++j) D[TRI + j] = fma(Jr[j], rr, D[TRI + j]);
                }
            }
#pragma unroll
            for (int k = 0; k < NL; ++k) Nl[static_cast<size_t>(NL) * i + k] = D[k];
        }
        __syncthreads();                       // the cost is settled for every thread
    };

    int cl = 0, ct = 0, iters = 0, accepted = 0, cg_total = 0;    // which linearisation and which T hold the current state
    linearise(wd + lay.T, 0.0, 0);
    const double cost_in = s_cost;
    double cur = cost_in, lam = LM_LAMBDA0;

    if (!few && a.max_iters > 0) {
        for (int it = 0; it < a.max_iters; ++it) {
            const double* const El = wd + lay.elin + cl * lay.elin_size;
            const double* const Nl = wd + lay.nlin + cl * lay.nlin_size;
            const double* const Tc = wd + lay.T + static_cast<size_t>(ct) * PS * N;
            double* const Tt = wd + lay.T + static_cast<size_t>(1 - ct) * PS * N;
            // ---- S121 steps 1-2: the factors of the damped diagonal blocks; x = 0, r = -g, z = M^-1 r, p = z
            int fail = 0;
            double part[1] = {0.0};
            for (int i = tid; i < N; i += HR_P) {
                if (!wfree[i]) continue;
                double H[TRI], L[P][P];
#pragma unroll
                for (int k = 0; k < TRI; ++k) H[k] = Nl[static_cast<size_t>(NL) * i + k];
                if (!lm_factor<P>(H, lam, L)) { fail = 1; continue; }
                int e = 0;
#pragma unroll
                for (int r = 0; r < P; ++r)
#pragma unroll
                    for (int k = 0; k <= r; ++k) fac[static_cast<size_t>(TRI) * i + e++] = L[r][k];
                double* v = vec + static_cast<size_t>(NV) * i;
                double r[P], z[P];
#pragma unroll
                for (int j = 0; j < P; ++j) r[j] = -Nl[static_cast<size_t>(NL) * i + TRI + j];
                lm_subst<P>(L, r, z);
#pragma unroll
                for (int j = 0; j < P; ++j) { v[VX + j] = 0.0; v[VR + j] = r[j]; v[VZ + j] = z[j]; v[VP + j] = z[j]; }
                part[0] = part[0] + dot<P>(r, z);
            }
            if (__syncthreads_or(fail)) break;
            tree<1>(part, tid, s_x, s_red);   // ends in a barrier: p is settled for the edges' threads
            double rho = s_red[0];
            const double rho0 = rho;
            bool stop = false;
            for (int k = 0; k < a.cg_iters; ++k) {
                // q_e = Ja p_a + Jb p_b over the used edges; a held node adds no term
                for (int e = tid; e < n; e += HR_P) {
                    if (!wused[e]) continue;
                    const int na = a.ab[2 * static_cast<size_t>(e)], nb = a.ab[2 * static_cast<size_t>(e) + 1];
                    const bool fa = wfree[na] != 0, fb = wfree[nb] != 0;
                    const double* Ja = El + static_cast<size_t>(ER) * e + P;
                    const double* Jb = Ja + P * P;
                    double pa[P], pb[P];
#pragma unroll
                    for (int j = 0; j < P; ++j) {
                        pa[j] = fa ? vec[static_cast<size_t>(NV) * na + VP + j] : 0.0;
                        pb[j] = fb ? vec[static_cast<size_t>(NV) * nb + VP + j] : 0.0;
                    }
#pragma unroll 1
                    for (int row = 0; row < P; ++row) {
                        double v = 0.0;
                        if (fa) {
#pragma unroll
                            for (int j = 0; j < P; ++j) v = fma(Ja[P * row + j], pa[j], v);
                        }
                        if (fb) {
#pragma unroll
                            for (int j = 0; j < P; ++j) v = fma(Jb[P * row + j], pb[j], v);
                        }
                        qv[static_cast<size_t>(P) * e + row] = v;
                    }
                }
                __syncthreads();               // q crosses from the edges' threads to the nodes'
                part[0] = 0.0;
                for (int i = tid; i < N; i += HR_P) {
                    if (!wfree[i]) continue;
                    double acc[P];
#pragma unroll
                    for (int j = 0; j < P; ++j) acc[j] = 0.0;
                    const int s1 = start[i + 1];
                    for (int s = start[i]; s < s1; ++s) {
                        const int ent = inc[s];
                        const double* J = El + static_cast<size_t>(ER) * (ent >> 1) + P + (ent & 1) * (P * P);
                        const double* qe = qv + static_cast<size_t>(P) * (ent >> 1);
#pragma unroll 1
                        for (int row = 0; row < P; ++row) {
                            const double qr = qe[row];
#pragma unroll
                            for (int j = 0; j < P; ++j) acc[j] = fma(J[P * row + j], qr, acc[j]);
                        }
                    }
                    double* v = vec + static_cast<size_t>(NV) * i;
                    double pp[P];
#pragma unroll
                    for (int j = 0; j < P; ++j) {
                        pp[j] = v[VP + j];
                        acc[j] = acc[j] + (lam * Nl[static_cast<size_t>(NL) * i + j * P - j * (j - 1) / 2]) * pp[j];
                        v[VAP + j] = acc[j];
                    }
                    part[0] = part[0] + dot<P>(pp, acc);
                }
                tree<1>(part, tid, s_x, s_red);
                const double pAp = s_red[0];
                if (__builtin_amdgcn_readfirstlane(static_cast<int>(!(pAp > 0.0) || !(pAp < __builtin_inf())))) {
                    stop = k == 0;
                    break;
                }
                const double alpha = rho / pAp;
                part[0] = 0.0;
                for (int i = tid; i < N; i += HR_P) {
                    if (!wfree[i]) continue;
                    double* v = vec + static_cast<size_t>(NV) * i;
                    double L[P][P], r[P], z[P];
                    load_factor<P>(fac + static_cast<size_t>(TRI) * i, L);
#pragma unroll
                    for (int j = 0; j < P; ++j) {
                        v[VX + j] = fma(alpha, v[VP + j], v[VX + j]);
                        r[j] = fma(-alpha, v[VAP + j], v[VR + j]);
                        v[VR + j] = r[j];
                    }
                    lm_subst<P>(L, r, z);
#pragma unroll
                    for (int j = 0; j < P; ++j) v[VZ + j] = z[j];
                    part[0] = part[0] + dot<P>(r, z);
                }
                tree<1>(part, tid, s_x, s_red);
                const double rho1 = s_red[0];
                ++cg_total;
                if (__builtin_amdgcn_readfirstlane(static_cast<int>(rho1 <= a.cg_tol2 * rho0 || k + 1 == a.cg_iters))) break;
                const double beta = rho1 / rho;
                for (int i = tid; i < N; i += HR_P) {
                    if (!wfree[i]) continue;
                    double* v = vec + static_cast<size_t>(NV) * i;
#pragma unroll
                    for (int j = 0; j < P; ++j) v[VP + j] = fma(beta, v[VP + j], v[VZ + j]);
                }
                rho = rho1;
                __syncthreads();               // p crosses from the nodes' threads to the edges'
            }
            if (stop) break;
            // ---- step 5: the step test over the steps and the t of the free nodes
            double dmax = 0.0, hmax = 1.0, nonfin = 0.0;
            for (int i = tid; i < N; i += HR_P) {
                if (!wfree[i]) continue;
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    const double x = fabs(vec[static_cast<size_t>(NV) * i + VX + j]);
                    if (!(x < __builtin_inf())) nonfin = 1.0;
                    if (x > dmax) dmax = x;
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double h = fabs(Tc[static_cast<size_t>(PS) * i + 9 + c]);
                    if (h > hmax) hmax = h;
                }
            }
            const auto mx = group_max3(s_max, tid, dmax, hmax, nonfin);         // of dmax, hmax, nonfin over the workgroup
            if (__builtin_amdgcn_readfirstlane(static_cast<int>(mx.c > 0.0 || !(mx.a > LM_STEP_TOL * mx.b)))) break;
            // ---- step 6: the trial poses, their linearisation, accept or reject
            double bad = 0.0;
            for (int i = tid; i < N; i += HR_P) {
                if (!wfree[i]) continue;
                double T[PS], d[P], o[12];
#pragma unroll
                for (int j = 0; j < PS; ++j) T[j] = Tc[static_cast<size_t>(PS) * i + j];
#pragma unroll
                for (int j = 0; j < P; ++j) d[j] = vec[static_cast<size_t>(NV) * i + VX + j];
                pose_update(T, d, o);
#pragma unroll
                for (int j = 0; j < 12; ++j) Tt[static_cast<size_t>(PS) * i + j] = o[j];
                double s = T[12];
                if (P == 7) {
                    s = T[12] * (1.0 + d[P - 1]);
                    if (!(s > 0.0) || !(s < __builtin_inf())) bad = 1.0;
                }
                Tt[static_cast<size_t>(PS) * i + 12] = s;
            }
            __syncthreads();                   // the trial poses cross from the nodes' threads to the edges'
            linearise(Tt, bad, 1 - cl);
            ++iters;
            const double cost = s_cost;
            if (__builtin_amdgcn_readfirstlane(static_cast<int>(cost < cur))) {
                ++accepted;
                cur = cost;
                cl = 1 - cl;
                ct = 1 - ct;
                lam = lam / 10.0;
            } else {
                lam = lam * 10.0;
            }
            __syncthreads();                   // every thread has read the cost before the next linearisation writes it
        }
    }

    // ---- S122: result.  The current T is the input until a step is accepted, and a held node never changes in it
    {
        const double* Tc = wd + lay.T + static_cast<size_t>(ct) * PS * N;
        for (int i = tid; i < PS * N; i += HR_P) a.pose_out[i] = Tc[i];
    }
    if (tid == 0)
        *a.info = pm_pgo_info{cost_in, accepted ? cur : cost_in, static_cast<int32_t>(n_used), static_cast<int32_t>(n_free), iters,
                              accepted, cg_total, few ? 2 : (accepted ? 0 : 1)};
}

// S123: row i < n = clamp(*d_n, 0, cap) moves with its anchor node k: out = (float)(T_new,k^-1 (T_old,k X)), fp64, one
// rounding; a row with a non-finite input or result or an anchor outside [0, n_nodes) is three quiet NaNs.  out may be xyz: a
// thread reads its own row before it writes it.
__global__ __launch_bounds__(256) void pgo_move_points(const double* Told, const double* Tnew, int n_nodes, const int32_t* anchor,
                                                       const float* xyz, const int32_t* d_n, int cap, float* out)
{
    const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (i >= pm::clamped_count(d_n, cap)) return;
    const int k = anchor[i];
    const float* p = xyz + 3 * static_cast<size_t>(i);
    const double X[3] = {static_cast<double>(p[0]), static_cast<double>(p[1]), static_cast<double>(p[2])};
    bool fin = k >= 0 && k < n_nodes && finite_all(X, 3);
    double o[3] = {0.0, 0.0, 0.0};
    if (fin) {
        double A[PS], B[PS];
#pragma unroll
        for (int j = 0; j < PS; ++j) { A[j] = Told[static_cast<size_t>(PS) * k + j]; B[j] = Tnew[static_cast<size_t>(PS) * k + j]; }
        fin = finite_all(A, PS) && finite_all(B, PS);
        double v[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            v[r] = ((((A[12] * A[3 * r]) * X[0] + (A[12] * A[3 * r + 1]) * X[1]) + (A[12] * A[3 * r + 2]) * X[2]) + A[9 + r]) - B[9 + r];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[c] = ((B[c] * v[0] + B[3 + c] * v[1]) + B[6 + c] * v[2]) / B[12];
            fin = fin && fabs(o[c]) < __builtin_inf();
        }
    }
    const float nanv = __builtin_nanf("");
    float* q = out + 3 * static_cast<size_t>(i);
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = fin ? static_cast<float>(o[c]) : nanv;
}

// everything but the pointers of the two forms; PM_E_UNSUPPORTED comes last, after every PM_E_INVALID
int check_common(int n_nodes, int n_edges, const pm_pgo_params* p)
{
    PM_REQUIRE(p != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE(n_nodes >= 2, PM_E_INVALID, "n_nodes < 2");
    PM_REQUIRE(n_edges >= 0, PM_E_INVALID, "cap_edges or n_edges < 0");
    PM_REQUIRE(p->model == PM_PGO_RIGID || p->model == PM_PGO_SIM3, PM_E_INVALID, "model is not PM_PGO_*");
    PM_REQUIRE(p->max_iters >= 0 && p->max_iters <= 100, PM_E_INVALID, "max_iters outside [0, 100]");
    PM_REQUIRE(p->cg_iters >= 1 && p->cg_iters <= 1000, PM_E_INVALID, "cg_iters outside [1, 1000]");
    PM_REQUIRE(std::isfinite(p->cg_tol) && p->cg_tol >= 0.0 && p->cg_tol < 1.0, PM_E_INVALID, "cg_tol must be finite and in [0, 1)");
    PM_REQUIRE(p->flags == 0 && p->reserved == 0, PM_E_INVALID, "flags and reserved must be 0");
    return PM_OK;
}

}  // namespace
}  // namespace pm_pgo

extern "C" size_t pm_pose_graph_workspace(int n_nodes, int n_edges, int model)
{
    if (n_nodes < 2 || n_nodes > PM_PGO_MAX_NODES || n_edges < 0 || n_edges > PM_PGO_MAX_EDGES) return 0;
    if (model != PM_PGO_RIGID && model != PM_PGO_SIM3) return 0;
    return pm_pgo::layout(n_nodes, n_edges, pm_pgo::params_of(model)).bytes;
}

extern "C" int pm_pose_graph_optimize_dev(pm_ctx* ctx, const double* d_pose_in, int n_nodes, const uint8_t* d_fixed,
                                          const int32_t* d_edge_ab, const double* d_edge_Z, const double* d_edge_w,
                                          const int32_t* d_n_edges, int cap_edges, const pm_pgo_params* p, double* d_pose_out,
                                          uint8_t* d_edge_used, void* d_work, size_t work_bytes, pm_pgo_info* d_info)
{
    using namespace pm_pgo;
    PM_REQUIRE(d_pose_in != nullptr && d_fixed != nullptr && d_edge_ab != nullptr && d_edge_Z != nullptr && d_edge_w != nullptr &&
                   d_pose_out != nullptr && d_work != nullptr && d_info != nullptr,
               PM_E_INVALID, "null pointer");
    const int rc = check_common(n_nodes, cap_edges, p);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REQUIRE(n_nodes <= PM_PGO_MAX_NODES, PM_E_UNSUPPORTED, "n_nodes above PM_PGO_MAX_NODES");
    PM_REQUIRE(cap_edges <= PM_PGO_MAX_EDGES, PM_E_UNSUPPORTED, "cap_edges above PM_PGO_MAX_EDGES");
    PM_REQUIRE(work_bytes >= layout(n_nodes, cap_edges, params_of(p->model)).bytes, PM_E_INVALID,
               "work_bytes below pm_pose_graph_workspace()");
    Args a = {};
    a.pose_in = d_pose_in; a.fixed = d_fixed; a.ab = d_edge_ab; a.Z = d_edge_Z; a.w = d_edge_w; a.count = d_n_edges;
    a.n_nodes = n_nodes; a.cap_edges = cap_edges; a.max_iters = p->max_iters; a.cg_iters = p->cg_iters;
    a.cg_tol2 = p->cg_tol * p->cg_tol;
    a.pose_out = d_pose_out; a.used_out = d_edge_used; a.work = static_cast<char*>(d_work); a.info = d_info;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    {
        pm::ScopedKernelTime timer(ctx, "pose_graph");
        if (p->model == PM_PGO_SIM3)
            hipLaunchKernelGGL(pose_graph<7>, dim3(1), dim3(pm_hrefine::HR_P), 0, ctx->stream, a);
        else
            hipLaunchKernelGGL(pose_graph<6>, dim3(1), dim3(pm_hrefine::HR_P), 0, ctx->stream, a);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_pose_graph_optimize(pm_ctx* ctx, const double* pose_in, int n_nodes, const uint8_t* fixed, const int32_t* edge_ab,
                                      const double* edge_Z, const double* edge_w, int n_edges, const pm_pgo_params* p,
                                      double* pose_out, uint8_t* edge_used, pm_pgo_info* info)
{
    using namespace pm_pgo;
    PM_REQUIRE(pose_in != nullptr && fixed != nullptr && edge_ab != nullptr && edge_Z != nullptr && edge_w != nullptr &&
                   pose_out != nullptr && info != nullptr,
               PM_E_INVALID, "null pointer");
    const int rc = check_common(n_nodes, n_edges, p);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REQUIRE(n_nodes <= PM_PGO_MAX_NODES, PM_E_UNSUPPORTED, "n_nodes above PM_PGO_MAX_NODES");
    PM_REQUIRE(n_edges <= PM_PGO_MAX_EDGES, PM_E_UNSUPPORTED, "n_edges above PM_PGO_MAX_EDGES");
    const size_t N = static_cast<size_t>(n_nodes), E = static_cast<size_t>(n_edges);
    const size_t wb = layout(n_nodes, n_edges, params_of(p->model)).bytes;
    pm::StagedBlock b(ctx, __func__);
    const size_t o_pose = b.add(N * 104), o_fixed = b.add(N), o_ab = b.add(E * 8), o_Z = b.add(E * 104), o_w = b.add(E * 24);
    const size_t o_used = b.add(edge_used ? E : 0), o_info = b.add(sizeof(pm_pgo_info)), o_work = b.add(wb);
    b.alloc();
    b.upload(o_pose, pose_in, N * 104);
    b.upload(o_fixed, fixed, N);
    b.upload(o_ab, edge_ab, E * 8);
    b.upload(o_Z, edge_Z, E * 104);
    b.upload(o_w, edge_w, E * 24);
    if (b.rc == PM_OK)
        b.rc = pm_pose_graph_optimize_dev(ctx, b.at<double>(o_pose), n_nodes, b.at<uint8_t>(o_fixed), b.at<int32_t>(o_ab),
                                          b.at<double>(o_Z), b.at<double>(o_w), nullptr, n_edges, p, b.at<double>(o_pose),
                                          edge_used ? b.at<uint8_t>(o_used) : nullptr, b.at<void>(o_work), wb,
                                          b.at<pm_pgo_info>(o_info));
    b.download(pose_out, o_pose, N * 104);
    if (edge_used) b.download(edge_used, o_used, E);
    b.download(info, o_info, sizeof(pm_pgo_info));
    return b.sync();
}

extern "C" int pm_pgo_move_points_dev(pm_ctx* ctx, const double* d_pose_old, const double* d_pose_new, int n_nodes,
                                      const int32_t* d_anchor, const float* d_xyz, const int32_t* d_n, int cap, float* d_out)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REQUIRE(d_pose_old != nullptr && d_pose_new != nullptr && d_anchor != nullptr && d_xyz != nullptr && d_out != nullptr,
               PM_E_INVALID, "null pointer");
    PM_REQUIRE(n_nodes >= 0 && cap >= 0, PM_E_INVALID, "n_nodes or cap < 0");
    PM_REQUIRE(cap >= 1, PM_E_UNSUPPORTED, "cap == 0: nothing to move");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    {
        pm::ScopedKernelTime timer(ctx, "pgo_move_points");
        hipLaunchKernelGGL(pm_pgo::pgo_move_points, dim3(static_cast<unsigned>((cap + 255) / 256)), dim3(256), 0, ctx->stream,
                           d_pose_old, d_pose_new, n_nodes, d_anchor, d_xyz, d_n, cap, d_out);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_pgo_move_points(pm_ctx* ctx, const double* pose_old, const double* pose_new, int n_nodes, const int32_t* anchor,
                                  const float* xyz, int n, float* out)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REQUIRE(pose_old != nullptr && pose_new != nullptr && anchor != nullptr && xyz != nullptr && out != nullptr, PM_E_INVALID,
               "null pointer");
    PM_REQUIRE(n_nodes >= 0 && n >= 0, PM_E_INVALID, "n_nodes or n < 0");
    PM_REQUIRE(n >= 1, PM_E_UNSUPPORTED, "n == 0: nothing to move");
    const size_t pb = static_cast<size_t>(n_nodes) * 104, rows = static_cast<size_t>(n);
    pm::StagedBlock b(ctx, __func__);
    const size_t o_old = b.add(pb), o_new = b.add(pb), o_anchor = b.add(rows * 4), o_xyz = b.add(rows * 12);
    b.alloc();
    b.upload(o_old, pose_old, pb);
    b.upload(o_new, pose_new, pb);
    b.upload(o_anchor, anchor, rows * 4);
    b.upload(o_xyz, xyz, rows * 12);
    if (b.rc == PM_OK)
        b.rc = pm_pgo_move_points_dev(ctx, b.at<double>(o_old), b.at<double>(o_new), n_nodes, b.at<int32_t>(o_anchor),
                                      b.at<float>(o_xyz), nullptr, n, b.at<float>(o_xyz));
    b.download(out, o_xyz, rows * 12);
    return b.sync();
}
