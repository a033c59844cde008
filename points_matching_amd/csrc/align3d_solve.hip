// align3d_solve.hip — the first launch of RANSAC over 3-D to 3-D correspondences on gfx950 (MI355X): the minimal triad
// solve of every sample (docs/SPEC.md S97, S98), one launch.  Lane g samples 3 correspondences for sample hyp_begin + g
// and solves them on its own (fp64, lane-serial), writing its one candidate slot (R, t, s, valid flag, M32 = (float)(s R | t))
// to the arena for the scoring launch (ransac_align3d_fused.hip).  The kernel has launch bounds of its own (64-thread
// workgroups), as pnp_solve has.  Its register and scratch figures are reported at build time (build.py).
#include "align3d_core.hpp"
#include "ransac_fused_kernels.hpp"

namespace pm_ransac {
namespace {

using namespace pm_align3d;

constexpr int AS_THREADS = 64;

// v: the correspondences as a one-part view, xy1 = rows of the first frame, xy2 = of the second (3 floats each)
__global__ __launch_bounds__(AS_THREADS) void align3d_solve(pm_points_view v, int model, uint64_t seed, int64_t hyp_begin,
                                                            int nh, double* __restrict__ cand)
{
    const int g = static_cast<int>(blockIdx.x) * AS_THREADS + static_cast<int>(threadIdx.x);
    if (g >= nh) return;
    const int n = view_count1(v);
    double* out = cand + static_cast<size_t>(g) * SLOT_DOUBLES;
    if (n < 3) {
        for (int j = 0; j < SLOT_DOUBLES; ++j) out[j] = 0.0;
        return;
    }
    int idx[3];
    sample_walk<3, STREAM, STREAM_H>(seed, static_cast<uint64_t>(hyp_begin + g), n, idx);
    float a[3][3], b[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float* p = v.xy1 + 3 * static_cast<size_t>(idx[i]);
        const float* q = v.xy2 + 3 * static_cast<size_t>(idx[i]);
        a[i][0] = p[0]; a[i][1] = p[1]; a[i][2] = p[2];
        b[i][0] = q[0]; b[i][1] = q[1]; b[i][2] = q[2];
    }
    solve3(model, a, b, out);
}

}  // namespace

int align3d_solve_enqueue(pm_ctx* ctx, int model, const pm_points_view& v, const pm_ransac_params* p, double* d_cand)
{
    const long long nh = p->hyp_end - p->hyp_begin;
    const int nwg = static_cast<int>((nh + AS_THREADS - 1) / AS_THREADS);
    pm::ScopedKernelTime t(ctx, "align3d_solve");
    hipLaunchKernelGGL(align3d_solve, dim3(nwg), dim3(AS_THREADS), 0, ctx->stream, v, model, p->seed, p->hyp_begin,
                       static_cast<int>(nh), d_cand);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

}  // namespace pm_ransac
