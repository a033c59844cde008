// warp_core.hpp — what warp.hip (S75-S78) and undistort.hip (S79-S83) share: the tile geometry, S77's integer bilinear sample at
// a Q5 position, the four-byte store and the count of valid pixels of a workgroup.  Device code only; one copy for both files.
#pragma once
#include <cstdint>

#include "pm_common.hpp"

namespace warp_core {

constexpr int TILE_W = 64, TILE_H = 16, PX = 4;          // output tile of a workgroup; pixels of a thread

// S77 for one pixel at the Q5 position (qx, qy): the grey value; ok = every tap of non-zero weight lies inside the source.
// A: anything with src, sw, sh, sstride, border.  Any int32 pair is a legal position: x0 + 1 <= 2^26, weights <= 1024.
template <bool REPLICATE, class A>
__device__ __forceinline__ int sample(const A& a, int qx, int qy, bool& ok)
{
    const int x0 = qx >> 5, y0 = qy >> 5, ax = qx & 31, ay = qy & 31;
    const int wx[2] = {32 - ax, ax}, wy[2] = {32 - ay, ay};
    int sum = 0;
    ok = true;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int wgt = wx[i] * wy[j];
            if (wgt == 0) continue;                                   // never read, never outside
            int xx = x0 + i, yy = y0 + j;
            const bool in = static_cast<unsigned>(xx) < static_cast<unsigned>(a.sw) && static_cast<unsigned>(yy) < static_cast<unsigned>(a.sh);
            ok = ok && in;
            int v = a.border;
            if (REPLICATE) {
                xx = min(max(xx, 0), a.sw - 1);
                yy = min(max(yy, 0), a.sh - 1);
                v = a.src[static_cast<size_t>(yy) * a.sstride + xx];
            } else if (in) {
                v = a.src[static_cast<size_t>(yy) * a.sstride + xx];
            }
            sum += wgt * v;
        }
    }
    return (sum + 512) >> 10;
}

// four bytes to p[0 .. cnt): one dword where it is aligned and whole, bytes otherwise
__device__ __forceinline__ void store4(uint8_t* p, const int v[PX], int cnt)
{
    if (cnt == PX && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        *reinterpret_cast<unsigned*>(p) = static_cast<unsigned>(v[0]) | (static_cast<unsigned>(v[1]) << 8) |
                                          (static_cast<unsigned>(v[2]) << 16) | (static_cast<unsigned>(v[3]) << 24);
    } else {
#pragma unroll
        for (int j = 0; j < PX; ++j)
            if (j < cnt) p[j] = static_cast<uint8_t>(v[j]);
    }
}

// The number of non-zero ok[] over a 256-thread workgroup: wave ballots, four wave totals through s_cnt (LDS, 4 ints), a
// barrier.  Every thread must call it; the total is meant for thread 0, which alone should read it.
__device__ __forceinline__ void block_valid_totals(const int ok[PX], int* s_cnt, int tid)
{
    int total = 0;
#pragma unroll
    for (int j = 0; j < PX; ++j) total += __popcll(__ballot(ok[j] != 0));
    if ((tid & 63) == 0) s_cnt[tid >> 6] = total;
    __syncthreads();
}
__device__ __forceinline__ int block_valid_sum(const int* s_cnt) { return (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]); }

}  // namespace warp_core
