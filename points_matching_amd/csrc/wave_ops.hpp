// wave_ops.hpp — the wave- and workgroup-level idioms that the kernels share: 64-lane sums, minima and maxima, the ballot
// rank, the fence of a wave-private LDS exchange, the stable selection of one 1024-thread workgroup, the rank by counting
// smaller keys and S1's combine of eight accumulators.  Device code with no kernel of its own; a wave is 64 lanes (gfx950).
// Which to reach for: a sum is the xor butterfly (there is no DPP sum here); a minimum or maximum that sits on the path of a
// one-wave-per-item loop is the DPP form, wave_min_u32 / _u64 / _f32 and wave_max_u32 / _u64, or its row stage row16_min_*
// where a 16-lane row owns the item; wave_min_u32_id is the DPP form for a value that is itself loop-carried through v_min
// (see there); wave_max_u64_xor and wave_max_f64 are butterflies for the once-per-launch picks that have always used them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pm {

#if defined(__HIPCC__)

// ---- 64-lane sums: an xor butterfly over the offsets 32 .. 1 (one ds_bpermute per step and 32 bits); every lane ends with the
// total, and all 64 lanes must be active.  The addends are integers, so the order of the butterfly is of no consequence.  One
// function per type and no deducing template: a 64-bit caller must not sum a 32-bit argument in 32 bits by accident.
// (The timed kernels that state this loop in place — ransac_score, ransac_finish, the filter prefixes of filter_gather.hip and
// knn_l2.hip, and lmeds.hip — keep it there: a function's loop is unrolled before it is inlined, the loop in place after the
// code around it has been arranged, and the two orders schedule those kernels differently.)
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += static_cast<unsigned>(__shfl_xor(static_cast<int>(v), o, 64));
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) { return static_cast<int>(wave_sum_u32(static_cast<unsigned>(v))); }
__device__ __forceinline__ long long wave_sum_i64(long long v) { return static_cast<long long>(wave_sum_u64(static_cast<unsigned long long>(v))); }

// ---- butterfly maxima; every lane ends with the maximum.  wave_max_u64_xor is NOT the DPP wave_max_u64 below: it serves the
// winner pick that runs once per launch (ransac.hip).  wave_max_f64 is an ordered compare: a NaN never wins.
__device__ __forceinline__ unsigned long long wave_max_u64_xor(unsigned long long key)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(key, o, 64);
        key = w > key ? w : key;
    }
    return key;
}
__device__ __forceinline__ double wave_max_f64(double v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double o = __shfl_xor(v, s, 64);
        v = o > v ? o : v;
    }
    return v;
}

// ---- the lanes of ONE wave exchange data through their slice of LDS.  LDS operations of a wave complete in issue order, so all
// that is needed is that the compiler keeps the order too.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- wave-wide reductions on the DPP path (all 64 lanes must be active): four v_min/v_max with a row_ror operand reduce each
// row of 16 lanes (row16_min_*: the minimum of the lane's row, in every lane of it), four v_readlane + scalar ops combine the
// rows; the result is wave-uniform.  A __shfl_xor butterfly costs six ds_bpermute round trips (two each for 64-bit values) —
// several hundred cycles per reduction in the one-wave-per-query refinements.
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned v)
{
    return static_cast<unsigned>(__builtin_amdgcn_update_dpp(static_cast<int>(v), static_cast<int>(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ unsigned row16_min_u32(unsigned v)
{
    v = min(v, dpp_u32<0x121>(v));      // row_ror:1
    v = min(v, dpp_u32<0x122>(v));      // row_ror:2
    v = min(v, dpp_u32<0x124>(v));      // row_ror:4
    v = min(v, dpp_u32<0x128>(v));      // row_ror:8
    return v;
}
// lexicographic (high word, low word): exact 64-bit minimum in two 32-bit reductions
__device__ __forceinline__ unsigned long long row16_min_u64(unsigned long long v)
{
    const unsigned hi = static_cast<unsigned>(v >> 32), lo = static_cast<unsigned>(v);
    const unsigned mh = row16_min_u32(hi);
    const unsigned ml = row16_min_u32(hi == mh ? lo : 0xFFFFFFFFu);
    return (static_cast<unsigned long long>(mh) << 32) | ml;
}
// (not row16_min_u32 plus the lane reads: stated that way the one-wave-per-query Hamming refinement and stereo_bm compile to
// different code)
__device__ __forceinline__ unsigned wave_min_u32(unsigned v)
{
    v = min(v, dpp_u32<0x121>(v));
    v = min(v, dpp_u32<0x122>(v));
    v = min(v, dpp_u32<0x124>(v));
    v = min(v, dpp_u32<0x128>(v));
    const unsigned a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const unsigned c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    return min(min(a, b), min(c, d));
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) { return ~wave_min_u32(~v); }
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
    const unsigned hi = static_cast<unsigned>(v >> 32), lo = static_cast<unsigned>(v);
    const unsigned mh = wave_min_u32(hi);
    const unsigned ml = wave_min_u32(hi == mh ? lo : 0xFFFFFFFFu);
    return (static_cast<unsigned long long>(mh) << 32) | ml;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) { return ~wave_min_u64(~v); }
// wave_min_u32 with the value that no lane reads (every row_ror lane has a source) set to the minimum's identity, so that the
// compiler folds each move into its v_min_u32: one instruction per stage instead of three.  For a value that a loop carries
// through the minimum (SGM's path step); where the two forms compile to different code a caller keeps the one it has.
__device__ __forceinline__ unsigned wave_min_u32_id(unsigned v)
{
#define PM_DPP_ID(ctrl) static_cast<unsigned>(__builtin_amdgcn_update_dpp(-1, static_cast<int>(v), ctrl, 0xF, 0xF, false))
    v = min(v, PM_DPP_ID(0x121));       // row_ror:1, 2, 4, 8
    v = min(v, PM_DPP_ID(0x122));
    v = min(v, PM_DPP_ID(0x124));
    v = min(v, PM_DPP_ID(0x128));
#undef PM_DPP_ID
    const unsigned a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const unsigned c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    return min(min(a, b), min(c, d));
}
// float minimum with fminf semantics on non-NaN data (the callers' values are finite)
__device__ __forceinline__ float wave_min_f32(float v)
{
#define PM_DPP_F(ctrl) __uint_as_float(dpp_u32<ctrl>(__float_as_uint(v)))
    v = fminf(v, PM_DPP_F(0x121));
    v = fminf(v, PM_DPP_F(0x122));
    v = fminf(v, PM_DPP_F(0x124));
    v = fminf(v, PM_DPP_F(0x128));
#undef PM_DPP_F
    const float a = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), 0));
    const float b = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), 16));
    const float c = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), 32));
    const float d = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), 48));
    return fminf(fminf(a, b), fminf(c, d));
}

// ---- ballot rank: how many lanes below `lane` have their bit set in a __ballot mask (the lane's slot in a wave's append).
// (knn_hamming_refine states it in place: next to its own 1ull << lane the function compiles to different code.)
__device__ __forceinline__ int lane_rank(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

// ---- stable selection by ONE workgroup of 1024 threads over the rows 0 .. n-1 (n the same on every thread), in chunks of 1024:
// flag(r) says whether row r < n is kept; the exclusive scan is a ballot rank inside a wave plus the 16 wave totals through
// LDS, and a running base carries the order across chunks.  move(r, d) then runs on every thread of the chunk, rows r >= n
// included (they are never kept), with d = the row's place in the output, or -1; after a barrier chunk(r0) runs on every
// thread (desc_compact's byte move, which reads what move() left in LDS); a barrier ends the round.  Thread 0 leaves the
// number of kept rows in *count.
template <class Flag, class Move, class Chunk>
__device__ __forceinline__ void select_stable_1024(int n, int32_t* count, Flag flag, Move move, Chunk chunk)
{
    __shared__ int s_wave[16];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int r0 = 0; r0 < n; r0 += 1024) {
        const int r = r0 + tid;
        const int f = r < n ? flag(r) : 0;
        const unsigned long long bal = __ballot(f);
        const int before = lane_rank(bal, lane);
        if (lane == 0) s_wave[wv] = __popcll(bal);
        __syncthreads();
        // the row's place: the kept rows of lower lanes, of lower waves, of earlier chunks.  Summed in the order in which the
        // compiler ranks the terms, so that it leaves the chain as it is: select, add, select, add, two registers.  Begun
        // with s_base it is re-associated after inlining, all sixteen selects come first and the kernel takes ten more VGPRs.
        int d = before, total = 0;
        for (int k = 0; k < 16; ++k) {
            if (k < wv) d += s_wave[k];
            total += s_wave[k];
        }
        d += s_base;
        move(r, f ? d : -1);
        __syncthreads();
        chunk(r0);
        if (tid == 0) s_base += total;
        __syncthreads();
    }
    if (tid == 0) *count = s_base;
}

// ---- rank by counting: the number of keys[0 .. n) below `mine`, by a workgroup of 256 threads that stages the keys through
// s_key[256] tile by tile.  Every thread of the workgroup must call it (barriers); n is the same on all of them.
__device__ __forceinline__ unsigned rank_below(const unsigned long long* keys, unsigned n, unsigned long long mine, unsigned long long* s_key)
{
    unsigned rank = 0;
    for (unsigned base = 0; base < n; base += 256) {
        __syncthreads();
        if (base + threadIdx.x < n) s_key[threadIdx.x] = keys[base + threadIdx.x];
        __syncthreads();
        const unsigned m = min(256u, n - base);
        for (unsigned j = 0; j < m; ++j) rank += s_key[j] < mine ? 1u : 0u;
    }
    return rank;
}

// ---- SPEC S1's combine of the eight accumulators that 8 consecutive lanes hold (lane l: accumulator l): the canonical
// association ((a0+a4) + (a1+a5)) + (a2+a6)) + (a3+a7), which makes the bits of the result.  Meaningful in lane 0 of the eight.
__device__ __forceinline__ float coop8_combine(float acc)
{
    const float s = acc + __shfl_down(acc, 4, 8);            // lanes 0..3: acc[l] + acc[l+4]
    const float s1 = __shfl_down(s, 1, 8), s2 = __shfl_down(s, 2, 8), s3 = __shfl_down(s, 3, 8);
    return ((s + s1) + s2) + s3;
}

#endif  // __HIPCC__

}  // namespace pm
