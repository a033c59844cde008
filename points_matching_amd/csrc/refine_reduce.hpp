// refine_reduce.hpp — the fixed-order fp64 reduction of docs/SPEC.md S23 (HR_P partials, point i into partial
// i mod HR_P, stride-halving tree), run by one workgroup of HR_P threads in which thread p owns partial p.  Shared by
// the homography refinement (homography_refine.hip, S23-S25) and the affine refit (affine_refine.hip, S30): the sums do
// not depend on the grid, so the CPU restatements reproduce them bit for bit.
#pragma once
#include "ransac_fused_kernels.hpp"

namespace pm_hrefine {

constexpr int HR_P = 512;                 // S23: partials = threads of the one workgroup
constexpr int HR_CH = 16;                 // accumulators per LDS round of the cross-wave tree steps

// S23 tree over the threads' partials: for s = 256, ..., 1: part[p] += part[p + s] for p < s.  out[k] (LDS) = the sum,
// visible to every thread on return.
template <int K>
__device__ __forceinline__ void tree(double (&acc)[K], int tid, double (*s_x)[HR_P / 2], double* out)
{
#pragma unroll
    for (int c0 = 0; c0 < K; c0 += HR_CH) {
#pragma unroll
        for (int s = HR_P / 2; s >= 64; s >>= 1) {
            if (tid >= s && tid < 2 * s) {
#pragma unroll
                for (int c = 0; c < HR_CH; ++c)
                    if (c0 + c < K) s_x[c][tid - s] = acc[c0 + c];
            }
            __syncthreads();
            if (tid < s) {
#pragma unroll
                for (int c = 0; c < HR_CH; ++c)
                    if (c0 + c < K) acc[c0 + c] = acc[c0 + c] + s_x[c][tid];
            }
            __syncthreads();
        }
    }
    if (tid < 64) {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = acc[k] + __shfl_down(acc[k], s, 64);
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) out[k] = acc[k];
        }
    }
    __syncthreads();
}

// One pass: term(acc, x1, y1, x2, y2) over the inliers i = tid, tid + HR_P, ... < n, then the tree into out[0..K).
template <int K, typename Term>
__device__ __forceinline__ void pass(const pm_points_view& v, const int* offs, int n, const uint8_t* mask, int tid,
                                     double (*s_x)[HR_P / 2], double* out, Term term)
{
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int i = tid; i < n; i += HR_P) {
        if (!mask[i]) continue;
        float2 a, b;
        if (v.parts == 1) {
            a = *reinterpret_cast<const float2*>(v.xy1 + 2 * static_cast<size_t>(i));
            b = *reinterpret_cast<const float2*>(v.xy2 + 2 * static_cast<size_t>(i));
        } else {
            pm_ransac::view_point(v, offs, i, a, b);
        }
        term(acc, static_cast<double>(a.x), static_cast<double>(a.y), static_cast<double>(b.x), static_cast<double>(b.y));
    }
    tree<K>(acc, tid, s_x, out);
}

}  // namespace pm_hrefine
