// knn_l2_exact.hpp — the exact general kernel of the L2 matcher (any dim, k <= 16; also PM_KNN_FORCE_EXACT).  Private to
// knn_l2.hip, which holds the scheme and the launcher (anonymous namespace: no other translation unit includes this header).
#pragma once
#include "knn_l2_canonical.hpp"

namespace {

using namespace pm_knn;

constexpr int TILE_T = 64;    // train rows per LDS tile of the exact kernel
// ---------------------------------------------------------------------------------------------
// exact general kernel.  Workgroup = 4 waves = EXQ_WG queries (4 per wave); lanes ride the train
// rows of a 64-row LDS tile; K is walked in chunks of EX_KC columns so any dim fits.  Each lane
// keeps the KL smallest keys per query; k > KL takes ceil(k/KL) passes, pass p only admitting
// keys above the last one emitted by pass p-1.
// ---------------------------------------------------------------------------------------------
constexpr int EX_KC = 128;
constexpr int EX_LD = EX_KC + 4;
constexpr int EX_QPW = 4;
constexpr int EXQ_WG = 4 * EX_QPW;

template <int KL>
__global__ __launch_bounds__(256) void knn_l2_exact(const float* __restrict__ Q,
                                                    const float* __restrict__ T, int nq, int nt,
                                                    int dim, int k, pm_match* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float Ts[TILE_T * EX_LD];
    __shared__ __attribute__((aligned(16))) float Qs[EXQ_WG * EX_LD];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.x * EXQ_WG;
    const int full8 = dim / 8 * 8;              // columns covered by the 8-lane accumulators
    const int ntiles = (nt + TILE_T - 1) / TILE_T;
    const int nchunks = (dim + EX_KC - 1) / EX_KC;
    const bool vec4 = (dim & 3) == 0 && ((reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(T)) & 15) == 0;

    uint64_t floor_key[EX_QPW];                 // keys <= floor were emitted by earlier passes
    bool have_floor = false;
#pragma unroll
    for (int i = 0; i < EX_QPW; ++i) floor_key[i] = 0ull;

    for (int emitted = 0; emitted < k; emitted += KL) {
        BestN<KL> best[EX_QPW];
#pragma unroll
        for (int i = 0; i < EX_QPW; ++i) best[i].init();

        for (int tile = 0; tile < ntiles; ++tile) {
            float acc[EX_QPW][8];
            float tail[EX_QPW];
#pragma unroll
            for (int i = 0; i < EX_QPW; ++i) {
                tail[i] = 0.f;
#pragma unroll
                for (int l = 0; l < 8; ++l) acc[i][l] = 0.f;
            }
            for (int ch = 0; ch < nchunks; ++ch) {
                const int kc0 = ch * EX_KC;
                const int kw = dim - kc0 < EX_KC ? dim - kc0 : EX_KC;   // valid columns in chunk
                __syncthreads();
                if (vec4) {
                    for (int f = tid; f < TILE_T * (EX_KC / 4); f += 256) {
                        const int row = f / (EX_KC / 4), c4 = f % (EX_KC / 4);
                        int g = tile * TILE_T + row;
                        g = g < nt ? g : nt - 1;
                        f32x4 v = {0.f, 0.f, 0.f, 0.f};
                        if (4 * c4 < kw)
                            v = *reinterpret_cast<const f32x4*>(T + static_cast<size_t>(g) * dim + kc0 + 4 * c4);
                        *reinterpret_cast<f32x4*>(Ts + row * EX_LD + 4 * c4) = v;
                    }
                    for (int f = tid; f < EXQ_WG * (EX_KC / 4); f += 256) {
                        const int row = f / (EX_KC / 4), c4 = f % (EX_KC / 4);
                        int g = q0 + row;
                        g = g < nq ? g : nq - 1;
                        f32x4 v = {0.f, 0.f, 0.f, 0.f};
                        if (4 * c4 < kw)
                            v = *reinterpret_cast<const f32x4*>(Q + static_cast<size_t>(g) * dim + kc0 + 4 * c4);
                        *reinterpret_cast<f32x4*>(Qs + row * EX_LD + 4 * c4) = v;
                    }
                } else {
                    for (int f = tid; f < TILE_T * EX_KC; f += 256) {
                        const int row = f / EX_KC, c = f % EX_KC;
                        int g = tile * TILE_T + row;
                        g = g < nt ? g : nt - 1;
                        Ts[row * EX_LD + c] = c < kw ? T[static_cast<size_t>(g) * dim + kc0 + c] : 0.f;
                    }
                    for (int f = tid; f < EXQ_WG * EX_KC; f += 256) {
                        const int row = f / EX_KC, c = f % EX_KC;
                        int g = q0 + row;
                        g = g < nq ? g : nq - 1;
                        Qs[row * EX_LD + c] = c < kw ? Q[static_cast<size_t>(g) * dim + kc0 + c] : 0.f;
                    }
                }
                __syncthreads();
                // full 8-column groups of this chunk
                const int g8 = (full8 - kc0 < kw ? (full8 - kc0 > 0 ? full8 - kc0 : 0) : kw) / 8;
                const float* tr = Ts + lane * EX_LD;
                for (int gi = 0; gi < g8; ++gi) {
                    const f32x4 t0 = *reinterpret_cast<const f32x4*>(tr + 8 * gi);
                    const f32x4 t1 = *reinterpret_cast<const f32x4*>(tr + 8 * gi + 4);
#pragma unroll
                    for (int i = 0; i < EX_QPW; ++i) {
                        const float* qr = Qs + (wave * EX_QPW + i) * EX_LD + 8 * gi;
                        const f32x4 a0 = *reinterpret_cast<const f32x4*>(qr);
                        const f32x4 a1 = *reinterpret_cast<const f32x4*>(qr + 4);
#pragma unroll
                        for (int l = 0; l < 4; ++l) {
                            float x = a0[l] - t0[l];
                            float p = x * x;
                            acc[i][l] = acc[i][l] + p;
                            float y = a1[l] - t1[l];
                            float w = y * y;
                            acc[i][l + 4] = acc[i][l + 4] + w;
                        }
                    }
                }
                // scalar tail columns (dim % 8) live in the last chunk; stash them for after the
                // lane combine.  At most 7 values per query: fold them in order later.
                if (kc0 + kw == dim && full8 < dim) {
#pragma unroll
                    for (int i = 0; i < EX_QPW; ++i) {
                        // combine first (all full groups are done once the last chunk is in)
                        const float s0 = acc[i][0] + acc[i][4], s1 = acc[i][1] + acc[i][5],
                                    s2 = acc[i][2] + acc[i][6], s3 = acc[i][3] + acc[i][7];
                        float d = ((s0 + s1) + s2) + s3;
                        for (int c = full8 - kc0; c < kw; ++c) {
                            float x = Qs[(wave * EX_QPW + i) * EX_LD + c] - tr[c];
                            float p = x * x;
                            d = d + p;
                        }
                        tail[i] = d;
                    }
                }
            }
            const int j = tile * TILE_T + lane;
#pragma unroll
            for (int i = 0; i < EX_QPW; ++i) {
                float d2;
                if (full8 < dim) d2 = tail[i];
                else {
                    const float s0 = acc[i][0] + acc[i][4], s1 = acc[i][1] + acc[i][5],
                                s2 = acc[i][2] + acc[i][6], s3 = acc[i][3] + acc[i][7];
                    d2 = ((s0 + s1) + s2) + s3;
                }
                const float d = __builtin_sqrtf(d2);
                const uint64_t key = knn_key(d, j);
                if (j < nt && (!have_floor || key > floor_key[i])) best[i].insert(key, d);
            }
        }
        // merge the lanes' lists: KL rounds of wave-min
#pragma unroll
        for (int i = 0; i < EX_QPW; ++i) {
            const int q = q0 + wave * EX_QPW + i;
            for (int c = 0; c < KL; ++c) {
                const uint64_t bestk = wave_min_u64(best[i].k[0]);
                const unsigned long long owners = __ballot(best[i].k[0] == bestk);
                const int first = __ffsll(static_cast<long long>(owners)) - 1;
                const float dist = __shfl(best[i].d[0], first, 64);
                if (lane == first) best[i].pop();
                if (bestk != ~0ull) floor_key[i] = bestk;
                if (lane == 0 && q < nq && emitted + c < k) {
                    pm_match m;
                    m.queryIdx = q;
                    m.imgIdx = 0;
                    if (bestk == ~0ull) { m.trainIdx = -1; m.distance = KNN_INF; }
                    else { m.trainIdx = static_cast<int>(static_cast<uint32_t>(bestk)); m.distance = dist; }
                    out[static_cast<size_t>(q) * k + emitted + c] = m;
                }
            }
        }
        have_floor = true;
    }
}

}  // namespace
