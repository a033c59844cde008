// pnp_solve.hip — the first launch of RANSAC-PnP on gfx950 (MI355X): the P3P solve of every sample (docs/SPEC.md S37,
// S38), one launch.  Lane g samples 3 correspondences for sample hyp_begin + g and solves them on its own (fp64,
// lane-serial), writing its 4 candidate slots (R, t, valid flag, P32 = (float)(K [R|t])) to the arena for the scoring
// launch (ransac_p_fused.hip).  The kernel has launch bounds of its own (64-thread workgroups), as essential_solve has: the
// solver's state must not be paid for by the 768-thread scorer.  Its register and scratch figures are reported at build
// time (build.py).
#include "pnp_core.hpp"
#include "ransac_fused_kernels.hpp"

namespace pm_ransac {
namespace {

using namespace pm_pnp;

constexpr int PS_THREADS = 64;

// v: the correspondences as a one-part view, xy1 = world points (3 floats each), xy2 = pixels (2 floats each)
__global__ __launch_bounds__(PS_THREADS) void pnp_solve(pm_points_view v, Cam k, uint64_t seed, int64_t hyp_begin, int nh,
                                                        double* __restrict__ cand)
{
    const int g = static_cast<int>(blockIdx.x) * PS_THREADS + static_cast<int>(threadIdx.x);
    if (g >= nh) return;
    const int n = view_count1(v);
    double* out = cand + static_cast<size_t>(g) * (SLOT_DOUBLES * MAX_CAND);
    if (n < 4) {                                  // S37: 3 points cannot tell the candidates apart
        for (int j = 0; j < SLOT_DOUBLES * MAX_CAND; ++j) out[j] = 0.0;
        return;
    }
    int idx[3];
    sample_walk<3, STREAM>(seed, static_cast<uint64_t>(hyp_begin + g), n, idx);
    float X[3][3], u[3], w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float* p = v.xy1 + 3 * static_cast<size_t>(idx[i]);
        X[i][0] = p[0]; X[i][1] = p[1]; X[i][2] = p[2];
        const float2 q = *reinterpret_cast<const float2*>(v.xy2 + 2 * static_cast<size_t>(idx[i]));
        u[i] = q.x; w[i] = q.y;
    }
    p3p(k, X, u, w, out);
}

}  // namespace

int pnp_solve_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_camera& K, const pm_ransac_params* p, double* d_cand)
{
    const long long nh = p->hyp_end - p->hyp_begin;
    const int nwg = static_cast<int>((nh + PS_THREADS - 1) / PS_THREADS);
    pm::ScopedKernelTime t(ctx, "pnp_solve");
    hipLaunchKernelGGL(pnp_solve, dim3(nwg), dim3(PS_THREADS), 0, ctx->stream, v, Cam{K.fx, K.fy, K.cx, K.cy}, p->seed,
                       p->hyp_begin, static_cast<int>(nh), d_cand);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

}  // namespace pm_ransac
