// triangulate.hip — map points from 2 .. 8 posed views in ONE launch on gfx950 (MI355X), docs/SPEC.md S93-S96: the
// counterpart of cv::triangulatePoints [recalled] and of the step a map builder runs behind it — refine the point on its
// reprojection error, keep it only if it lies in front of every camera, has enough parallax and reprojects well.  The
// structure-only half of bundle adjustment; pm_pnp_refine* (pnp_refine.hip) is the motion-only half.
//
// One lane per point, grid-stride.  The kernel is instantiated per view count V: the 2V x 4 DLT system, its 4 x 4 V and
// the per-view pixels live in registers and nothing is indexed by a run-time number (a view that does not observe the
// point contributes two zero rows, which change no bit of any sum: S94).  Pixels are coalesced float2 loads from the
// view-major arrays.  The poses are wave-uniform: the workgroup copies them (and the camera centres of S96) into LDS once
// and every lane reads them from there, a broadcast read.  All arithmetic is lane-local fp64, unfused except the explicit
// fma()s, so tests/triangulate_ref.c reproduces the bits; the 3 x 3 damped Cholesky of S95 is S24's lm_solve_n (lm_core.hpp).  *d_n_good is a ballot count per wave and one integer atomic per
// wave after a hipMemsetAsync on the stream: an integer sum, so the order does not matter.
//
// The launch keeps no per-call state, so the device form may be captured; the host form stages its rows through
// pm::StagedBlock and synchronises once.
#include <cmath>

#include "essential_core.hpp"
#include "lm_core.hpp"
#include "pm_common.hpp"

namespace pm_tri {
namespace {

using pm_essential::Cam;
using pm_hrefine::LM_LAMBDA0;
using pm_hrefine::LM_STEP_TOL;
using pm_hrefine::lm_solve_n;

constexpr int TR_THREADS = 256;
constexpr int TR_MAX_WG = 2048;

struct Args {
    const float* uv[PM_TRI_MAX_VIEWS];
    const double* Rt[PM_TRI_MAX_VIEWS];
    const int32_t* count;
    int cap;
    Cam k;
    double thr2, max_cos, max_depth;
    int max_iters, use_initial;
    float* xyz;
    uint8_t* status;
    float* points4;
    float* err2;
    int32_t* n_good;
};

// The poses in LDS never change after the prologue, so the compiler would hoist their loads out of the grid-stride and the
// LM loops and hold 12 V doubles in registers throughout (scratch from V = 7 on).  This keeps each load next to its use.
__device__ __forceinline__ void pose_fence() { asm volatile("" ::: "memory"); }

// S95: the sums of one pass at X over the observing views, in index order
struct Pass {
    double H[6], g[3], cost;
    bool depth_ok;                        // every observing view has 0 < z_cam < inf
};

// sP: V poses of 12 doubles (LDS); pix: the pixels of this point; obs: bit v = view v observes it
template <int V>
__device__ __forceinline__ void lm_pass(const Cam& k, const double* sP, const float2 (&pix)[V], unsigned obs,
                                        const double (&X)[3], Pass& o)
{
#pragma unroll
    for (int e = 0; e < 6; ++e) o.H[e] = 0.0;
#pragma unroll
    for (int e = 0; e < 3; ++e) o.g[e] = 0.0;
    o.cost = 0.0;
    o.depth_ok = true;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        if (!((obs >> v) & 1u)) continue;
        const double* P = sP + 12 * v;
        double xc[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) xc[r] = ((P[3 * r] * X[0] + P[3 * r + 1] * X[1]) + P[3 * r + 2] * X[2]) + P[9 + r];
        o.depth_ok = o.depth_ok && xc[2] > 0.0 && xc[2] < __builtin_inf();
        const double iz = 1.0 / xc[2];
        const double px = xc[0] * iz, py = xc[1] * iz;
        const double ru = (k.fx * px + k.cx) - static_cast<double>(pix[v].x);
        const double rv = (k.fy * py + k.cy) - static_cast<double>(pix[v].y);
        const double fa = k.fx * iz, fb = k.fy * iz;
        const double a = fa * px, b = fb * py;
        double ju[3], jv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ju[c] = fa * P[c] - a * P[6 + c];
            jv[c] = fb * P[3 + c] - b * P[6 + c];
        }
        int e = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int q = j; q < 3; ++q, ++e) o.H[e] = o.H[e] + fma(ju[j], ju[q], jv[j] * jv[q]);
#pragma unroll
        for (int j = 0; j < 3; ++j) o.g[j] = o.g[j] + fma(ju[j], ru, jv[j] * rv);
        o.cost = o.cost + fma(ru, ru, rv * rv);
    }
    if (!o.depth_ok) o.cost = __builtin_inf();
}

template <int V>
__global__ __launch_bounds__(TR_THREADS) void triangulate_kernel(Args a)
{
    __shared__ double s_P[V * 12];        // poses: R row-major, then t
    __shared__ double s_C[V * 3];         // camera centres C = -R^T t (S96)
    const int tid = static_cast<int>(threadIdx.x);
#pragma unroll
    for (int v = 0; v < V; ++v)
        if (tid < 12) s_P[12 * v + tid] = a.Rt[v] ? a.Rt[v][tid] : ((tid < 9 && tid % 4 == 0) ? 1.0 : 0.0);
    __syncthreads();
#pragma unroll
    for (int v = 0; v < V; ++v)
        if (tid < 3) {
            const double* P = s_P + 12 * v;
            s_C[3 * v + tid] = -((P[tid] * P[9] + P[3 + tid] * P[10]) + P[6 + tid] * P[11]);
        }
    __syncthreads();

    const int n = pm::clamped_count(a.count, a.cap);
    const float nanf = __builtin_nanf("");
    int good = 0;                          // this wave's PM_TRI_OK rows (wave-uniform)
    // the bound is the same for every lane of a wave, so that all 64 reach the ballot
    for (int base = static_cast<int>(blockIdx.x) * TR_THREADS; base < n; base += static_cast<int>(gridDim.x) * TR_THREADS) {
        const int i = base + tid;
        bool ok = false;
        pose_fence();
        if (i < n) {
            // ---- S93: observations
            float2 pix[V];
            double A[2 * V][4];
            unsigned obs = 0u;
            int seen = 0;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                pix[v] = *reinterpret_cast<const float2*>(a.uv[v] + 2 * static_cast<size_t>(i));
                const float2 q = pm_essential::normalise(a.k, pix[v]);
                const bool o = q.x == q.x && q.y == q.y;
                if (o) { obs |= 1u << v; ++seen; }
                if (!a.use_initial) {
                    // ---- S94: the rows of view v (zero rows when it does not observe the point)
                    const double x = static_cast<double>(q.x), y = static_cast<double>(q.y);
                    const double* P = s_P + 12 * v;
                    const bool ident = a.Rt[v] == nullptr;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const double p0 = c < 3 ? P[c] : P[9], p1 = c < 3 ? P[3 + c] : P[10], p2 = c < 3 ? P[6 + c] : P[11];
                        const double r0 = ident ? (c == 0 ? -1.0 : (c == 2 ? x : 0.0)) : x * p2 - p0;
                        const double r1 = ident ? (c == 1 ? -1.0 : (c == 2 ? y : 0.0)) : y * p2 - p1;
                        A[2 * v][c] = o ? r0 : 0.0;
                        A[2 * v + 1][c] = o ? r1 : 0.0;
                    }
                }
            }
            int st = PM_TRI_OK;
            double X[3];
            if (a.use_initial) {
                const float* x0 = a.xyz + 3 * static_cast<size_t>(i);
#pragma unroll
                for (int c = 0; c < 3; ++c) X[c] = static_cast<double>(x0[c]);
            } else {
                double Q[4];
                pm_essential::dlt_null_vector<2 * V>(A, Q);
                if (a.points4)
                    *reinterpret_cast<float4*>(a.points4 + 4 * static_cast<size_t>(i)) =
                        float4{static_cast<float>(Q[0]), static_cast<float>(Q[1]), static_cast<float>(Q[2]), static_cast<float>(Q[3])};
#pragma unroll
                for (int c = 0; c < 3; ++c) X[c] = Q[c] / Q[3];
                if (Q[3] == 0.0) st = PM_TRI_DEGENERATE;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (!(fabs(X[c]) < __builtin_inf())) st = PM_TRI_DEGENERATE;
            if (seen < 2) st = PM_TRI_FEW_VIEWS;

            double err = 0.0;
            if (st == PM_TRI_OK) {
                // ---- S95: refinement
                Pass cur;
                lm_pass<V>(a.k, s_P, pix, obs, X, cur);
                if (cur.depth_ok && a.max_iters > 0) {
                    double lam = LM_LAMBDA0;
                    for (int it = 0; it < a.max_iters; ++it) {
                        double d[3];
                        pose_fence();
                        [[clang::always_inline]] if (!lm_solve_n<3>(cur.H, cur.g, lam, d)) break;
                        double dmax = 0.0, hmax = 1.0;
#pragma unroll
                        for (int c = 0; c < 3; ++c) {          // NaN propagates into dmax and stops the loop
                            if (!(fabs(d[c]) <= dmax)) dmax = fabs(d[c]);
                            if (!(fabs(X[c]) <= hmax)) hmax = fabs(X[c]);
                        }
                        if (!(dmax > LM_STEP_TOL * hmax)) break;
                        const double Xt[3] = {X[0] + d[0], X[1] + d[1], X[2] + d[2]};
                        Pass tr;
                        lm_pass<V>(a.k, s_P, pix, obs, Xt, tr);
                        if (tr.cost < cur.cost) {
                            cur = tr;
                            lam = lam / 10.0;
#pragma unroll
                            for (int c = 0; c < 3; ++c) X[c] = Xt[c];
                        } else {
                            lam = lam * 10.0;
                        }
                    }
                }
                // ---- S96: gates at the final point
                pose_fence();
                bool depth = true;
                double cmin = 1.0;
                double r[V][3], nn[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const double* P = s_P + 12 * v;
                    const double z = ((P[6] * X[0] + P[7] * X[1]) + P[8] * X[2]) + P[11];
                    if ((obs >> v) & 1u) {
                        depth = depth && z > 0.0 && z < a.max_depth;
                        const double iz = 1.0 / z;
                        const double xu = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[9];
                        const double xv = ((P[3] * X[0] + P[4] * X[1]) + P[5] * X[2]) + P[10];
                        const double ru = (a.k.fx * (xu * iz) + a.k.cx) - static_cast<double>(pix[v].x);
                        const double rv = (a.k.fy * (xv * iz) + a.k.cy) - static_cast<double>(pix[v].y);
                        const double e = fma(ru, ru, rv * rv);
                        if (!(e <= err)) err = e;               // a NaN propagates and fails the gate
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) r[v][c] = X[c] - s_C[3 * v + c];
                    nn[v] = fma(r[v][0], r[v][0], fma(r[v][1], r[v][1], r[v][2] * r[v][2]));
                }
                bool par = true;                               // every observing pair's cosine is a number
#pragma unroll
                for (int p = 0; p < V; ++p)
#pragma unroll
                    for (int q = p + 1; q < V; ++q) {
                        if (!((obs >> p) & (obs >> q) & 1u)) continue;
                        const double dot = fma(r[p][0], r[q][0], fma(r[p][1], r[q][1], r[p][2] * r[q][2]));
                        const double cs = dot / sqrt(nn[p] * nn[q]);
                        par = par && cs == cs;
                        if (cs < cmin) cmin = cs;
                    }
                if (!depth) st = PM_TRI_DEPTH;
                else if (a.max_cos < 1.0 && !(par && cmin < a.max_cos)) st = PM_TRI_PARALLAX;
                else if (!(err <= a.thr2)) st = PM_TRI_REPROJ;
            }
            ok = st == PM_TRI_OK;
            float* out = a.xyz + 3 * static_cast<size_t>(i);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] = ok ? static_cast<float>(X[c]) : nanf;
            a.status[i] = static_cast<uint8_t>(st);
            if (a.err2) a.err2[i] = ok ? static_cast<float>(err) : nanf;
        }
        good += __popcll(__ballot(ok));
    }
    if (a.n_good && good && (tid & 63) == 0) atomicAdd(a.n_good, good);
}

bool camera_ok(const pm_camera* K)
{
    return std::isfinite(K->fx) && std::isfinite(K->fy) && std::isfinite(K->cx) && std::isfinite(K->cy) && K->fx > 0.0 && K->fy > 0.0;
}

// everything but the pointers of the two forms
int check_common(int n_views, int n, const pm_camera* K, const pm_tri_params* p)
{
    PM_REQUIRE(K != nullptr && p != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE(n_views >= 2 && n_views <= PM_TRI_MAX_VIEWS, PM_E_INVALID, "n_views outside [2, 8]");
    PM_REQUIRE(n >= 0, PM_E_INVALID, "cap or n < 0");
    PM_REQUIRE(camera_ok(K), PM_E_INVALID, "K needs finite values and fx, fy > 0");
    PM_REQUIRE(std::isfinite(p->max_reproj_px) && p->max_reproj_px > 0.0, PM_E_INVALID, "max_reproj_px must be finite and > 0");
    PM_REQUIRE(p->max_cos_parallax > -1.0 && p->max_cos_parallax <= 1.0, PM_E_INVALID, "max_cos_parallax outside (-1, 1]");
    PM_REQUIRE(p->max_depth > 0.0, PM_E_INVALID, "max_depth must be > 0");
    PM_REQUIRE(p->max_iters >= 0 && p->max_iters <= 100, PM_E_INVALID, "max_iters outside [0, 100]");
    PM_REQUIRE((p->flags & ~PM_TRI_USE_INITIAL) == 0, PM_E_INVALID, "unknown flag bits");
    return PM_OK;
}

template <int V>
void launch(pm_ctx* ctx, const Args& a, int nwg)
{
    hipLaunchKernelGGL(triangulate_kernel<V>, dim3(static_cast<unsigned>(nwg)), dim3(TR_THREADS), 0, ctx->stream, a);
}

}  // namespace
}  // namespace pm_tri

extern "C" int pm_triangulate_dev(pm_ctx* ctx, const pm_tri_views* views, const pm_camera* K, const pm_tri_params* p, float* d_xyz,
                                  uint8_t* d_status, float* d_points4, float* d_err2, int32_t* d_n_good)
{
    using namespace pm_tri;
    PM_REQUIRE(views != nullptr && d_xyz != nullptr && d_status != nullptr, PM_E_INVALID, "null pointer");
    const int rc = check_common(views->n_views, views->cap, K, p);
    if (rc != PM_OK) return rc;
    Args a = {};
    for (int v = 0; v < views->n_views; ++v) {
        PM_REQUIRE(views->uv[v] != nullptr, PM_E_INVALID, "a view's uv is null");
        a.uv[v] = views->uv[v];
        a.Rt[v] = views->Rt[v];
    }
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    a.count = views->count;
    a.cap = views->cap;
    a.k = Cam{K->fx, K->fy, K->cx, K->cy};
    a.thr2 = p->max_reproj_px * p->max_reproj_px;
    a.max_cos = p->max_cos_parallax;
    a.max_depth = p->max_depth;
    a.max_iters = p->max_iters;
    a.use_initial = (p->flags & PM_TRI_USE_INITIAL) ? 1 : 0;
    a.xyz = d_xyz; a.status = d_status; a.points4 = a.use_initial ? nullptr : d_points4; a.err2 = d_err2; a.n_good = d_n_good;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    if (d_n_good) PM_HIP_CHECK(hipMemsetAsync(d_n_good, 0, sizeof(int32_t), ctx->stream));
    if (a.cap == 0) return PM_OK;
    const int want = (a.cap + TR_THREADS - 1) / TR_THREADS;
    const int nwg = want < TR_MAX_WG ? want : TR_MAX_WG;
    {
        pm::ScopedKernelTime timer(ctx, "triangulate");
        switch (views->n_views) {
        case 2: launch<2>(ctx, a, nwg); break;
        case 3: launch<3>(ctx, a, nwg); break;
        case 4: launch<4>(ctx, a, nwg); break;
        case 5: launch<5>(ctx, a, nwg); break;
        case 6: launch<6>(ctx, a, nwg); break;
        case 7: launch<7>(ctx, a, nwg); break;
        default: launch<8>(ctx, a, nwg); break;
        }
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_triangulate(pm_ctx* ctx, const float* const* uv, const double* const* Rt, int n_views, int n, const pm_camera* K,
                              const pm_tri_params* p, float* xyz, uint8_t* status, float* points4, float* err2, int* n_good)
{
    using namespace pm_tri;
    PM_REQUIRE(uv != nullptr && Rt != nullptr && xyz != nullptr && status != nullptr, PM_E_INVALID, "null pointer");
    const int rc = check_common(n_views, n, K, p);
    if (rc != PM_OK) return rc;
    for (int v = 0; v < n_views; ++v) PM_REQUIRE(uv[v] != nullptr, PM_E_INVALID, "a view's uv is null");
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    const bool initial = (p->flags & PM_TRI_USE_INITIAL) != 0;
    if (initial) points4 = nullptr;
    const size_t rows = static_cast<size_t>(n);
    pm::StagedBlock b(ctx, __func__);
    size_t o_uv[PM_TRI_MAX_VIEWS], o_Rt[PM_TRI_MAX_VIEWS];
    for (int v = 0; v < n_views; ++v) { o_uv[v] = b.add(rows * 8); o_Rt[v] = b.add(Rt[v] ? 96 : 0); }
    const size_t o_xyz = b.add(rows * 12), o_st = b.add(rows), o_p4 = b.add(points4 ? rows * 16 : 0), o_e2 = b.add(err2 ? rows * 4 : 0);
    const size_t o_ng = b.add(sizeof(int32_t));
    b.alloc();
    pm_tri_views dv = {};
    for (int v = 0; v < n_views; ++v) {
        b.upload(o_uv[v], uv[v], rows * 8);
        if (Rt[v]) b.upload(o_Rt[v], Rt[v], 96);
        dv.uv[v] = b.at<const float>(o_uv[v]);
        dv.Rt[v] = Rt[v] ? b.at<const double>(o_Rt[v]) : nullptr;
    }
    if (initial) b.upload(o_xyz, xyz, rows * 12);
    dv.count = nullptr;
    dv.n_views = n_views;
    dv.cap = n;
    if (b.rc == PM_OK)
        b.rc = pm_triangulate_dev(ctx, &dv, K, p, b.at<float>(o_xyz), b.at<uint8_t>(o_st), points4 ? b.at<float>(o_p4) : nullptr,
                                  err2 ? b.at<float>(o_e2) : nullptr, b.at<int32_t>(o_ng));
    b.download(xyz, o_xyz, rows * 12);
    b.download(status, o_st, rows);
    if (points4) b.download(points4, o_p4, rows * 16);
    if (err2) b.download(err2, o_e2, rows * 4);
    int32_t ng = 0;
    b.download(&ng, o_ng, sizeof(int32_t));
    const int out = b.sync();
    if (out == PM_OK && n_good) *n_good = ng;
    return out;
}
