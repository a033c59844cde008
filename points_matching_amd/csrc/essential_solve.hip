// essential_solve.hip — the first launch of RANSAC-E on gfx950 (MI355X): camera normalisation of the correspondences
// (docs/SPEC.md S31) and the 5-point solve of every sample (S32, S33), one launch.
//   * every thread takes part in the normalised copy (grid-stride over the view's device-side count): one contiguous
//     f32 array per image in the arena plus the count, the plain-array view the scorer (ransac_e_fused.hip) reads;
//   * lane g solves sample hyp_begin + g on its own (fp64, lane-serial) from the raw view, normalising its five points
//     with the same S31 arithmetic, and writes its 10 candidate slots (9 doubles + valid flag) to the arena.
// The kernel has launch bounds of its own (64-thread workgroups): the solver's state must not be paid for by the
// 768-thread scorer.  Its register and scratch figures are reported at build time (build.py) and in profiles/.
#include "essential_core.hpp"
#include "ransac_fused_kernels.hpp"

namespace pm_ransac {
namespace {

using namespace pm_essential;

constexpr int ES_THREADS = 64;

__global__ __launch_bounds__(ES_THREADS) void essential_solve(pm_points_view v, Cam k, uint64_t seed, int64_t hyp_begin, int nh,
                                                              int cap_total, float* __restrict__ xyn, int* __restrict__ n_out,
                                                              double* __restrict__ cand)
{
    __shared__ int s_offs[PM_MAX_PARTS + 1];
    const int tid = threadIdx.x;
    int n;
    if (v.parts == 1) {
        n = view_count1(v);
    } else {
        view_offsets(v, s_offs, tid);
        __syncthreads();
        n = s_offs[v.parts];
    }
    const int g = static_cast<int>(blockIdx.x) * ES_THREADS + tid;
    float2* x1n = reinterpret_cast<float2*>(xyn);
    float2* x2n = reinterpret_cast<float2*>(xyn + 2 * static_cast<size_t>(cap_total));
    for (int i = g; i < n; i += static_cast<int>(gridDim.x) * ES_THREADS) {
        float2 a, b;
        view_point(v, s_offs, i, a, b);
        x1n[i] = normalise(k, a);
        x2n[i] = normalise(k, b);
    }
    if (g == 0) *n_out = n;
    if (g >= nh) return;
    double* out = cand + static_cast<size_t>(g) * (10 * MAX_MODELS);
    if (n < 5) {
        for (int j = 0; j < 10 * MAX_MODELS; ++j) out[j] = 0.0;
        return;
    }
    int idx[5];
    sample_walk<5, STREAM>(seed, static_cast<uint64_t>(hyp_begin + g), n, idx);
    double x1[5], y1[5], x2[5], y2[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        float2 a, b;
        view_point(v, s_offs, idx[i], a, b);
        a = normalise(k, a);
        b = normalise(k, b);
        x1[i] = static_cast<double>(a.x); y1[i] = static_cast<double>(a.y);
        x2[i] = static_cast<double>(b.x); y2[i] = static_cast<double>(b.y);
    }
    solve5(x1, y1, x2, y2, out);
}

}  // namespace

int essential_solve_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_camera& K, const pm_ransac_params* p, float* d_xyn,
                            int* d_n, double* d_cand)
{
    const long long nh = p->hyp_end - p->hyp_begin;
    const long long cap_total = static_cast<long long>(v.parts) * v.cap;
    const long long copy_wgs = (cap_total < 65536 ? cap_total : 65536) / 256 + 1;     // a few points per thread
    const long long solve_wgs = (nh + ES_THREADS - 1) / ES_THREADS;
    const int nwg = static_cast<int>(solve_wgs > copy_wgs ? solve_wgs : copy_wgs);
    pm::ScopedKernelTime t(ctx, "essential_solve");
    hipLaunchKernelGGL(essential_solve, dim3(nwg), dim3(ES_THREADS), 0, ctx->stream, v, Cam{K.fx, K.fy, K.cx, K.cy}, p->seed,
                       p->hyp_begin, static_cast<int>(nh), static_cast<int>(cap_total), d_xyn, d_n, d_cand);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

}  // namespace pm_ransac
