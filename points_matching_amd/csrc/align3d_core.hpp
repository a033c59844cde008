// align3d_core.hpp — device arithmetic of 3-D to 3-D alignment (docs/SPEC.md S97 3-sample, S98 minimal triad solve, S99
// distance test): the transform between two sets of corresponding 3-D rows, x2 = s R x1 + t, rigid (s = 1) or a
// similarity.  Built with -ffp-contract=off like every unit: the only fused multiply-adds are the explicit fma() /
// fmaf() calls, so tests/align3d_ref.c (the CPU restatement) reproduces the bits.  A model is 13 doubles: R (9,
// row-major, det +1), t (3), s (1).
#pragma once
#include "pnp_core.hpp"

namespace pm_align3d {

using pm_pnp::dot3;
using pm_pnp::triad;

// S97: the 3-sample is S6's walk (sample_walk<3, STREAM, STREAM_H>) with both salts its own, n >= 3
constexpr uint64_t STREAM = 0x3C6EF372FE94F82BULL, STREAM_H = 0xA54FF53A5F1D36F1ULL;
constexpr int RIGID = PM_ALIGN3D_RIGID, SIMILARITY = PM_ALIGN3D_SIMILARITY;
constexpr int WORDS = 13;             // R (9), t (3), s (1)
constexpr int FLAG = 13;              // the valid flag (1.0 / 0.0) of a candidate slot
constexpr int M32 = 14;               // M32 = (float)(s R | t), 3 x 4 row-major, as 12 floats in doubles 14..19
// A candidate slot of the solve launch: 13 + 1 + 6 doubles = 160 B, a multiple of the 32-byte sector like pnp_core.hpp's
// slot, so no slot straddles one more sector than it must; no pad is needed.
constexpr int SLOT_DOUBLES = 20;

// S99: M32 = (float)(s R | t), row r at P[4r .. 4r + 3]
__device__ __forceinline__ void model32(const double* T, float* P)
{
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) P[4 * r + c] = static_cast<float>(T[12] * T[3 * r + c]);
        P[4 * r + 3] = static_cast<float>(T[9 + r]);
    }
}

// S98 on the 3 sampled rows a[i] (xyz1) and b[i] (xyz2): the slot out[0 .. SLOT_DOUBLES) is written in full (zero when
// the sample is invalid); returns the valid flag.
__device__ __forceinline__ bool solve3(int model, const float (&a)[3][3], const float (&b)[3][3], double* __restrict__ out)
{
    for (int j = 0; j < SLOT_DOUBLES; ++j) out[j] = 0.0;
    double A[3][3], B[3][3], T1[3][3], T2[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) { A[i][c] = static_cast<double>(a[i][c]); B[i][c] = static_cast<double>(b[i][c]); }
    if (!triad(A[0], A[1], A[2], T1) || !triad(B[0], B[1], B[2], T2)) return false;
    double T[WORDS], ma[3], mb[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) T[3 * r + c] = (T2[0][r] * T1[0][c] + T2[1][r] * T1[1][c]) + T2[2][r] * T1[2][c];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ma[c] = ((A[0][c] + A[1][c]) + A[2][c]) / 3.0;
        mb[c] = ((B[0][c] + B[1][c]) + B[2][c]) / 3.0;
    }
    double s = 1.0;
    if (model == SIMILARITY) {
        double qa = 0.0, qb = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double da[3], db[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { da[c] = A[i][c] - ma[c]; db[c] = B[i][c] - mb[c]; }
            qa = qa + dot3(da, da);
            qb = qb + dot3(db, db);
        }
        s = sqrt(qb / qa);
        if (!(s > 0.0) || !(s < __builtin_inf())) return false;
    }
    T[12] = s;
#pragma unroll
    for (int r = 0; r < 3; ++r) T[9 + r] = mb[r] - s * ((T[3 * r] * ma[0] + T[3 * r + 1] * ma[1]) + T[3 * r + 2] * ma[2]);
    bool fin = true;
#pragma unroll
    for (int i = 0; i < WORDS; ++i) fin = fin && fabs(T[i]) < __builtin_inf();
    if (!fin) return false;
#pragma unroll
    for (int i = 0; i < WORDS; ++i) out[i] = T[i];
    out[FLAG] = 1.0;
    float P[12];
    model32(T, P);
    __builtin_memcpy(out + M32, P, sizeof P);                 // 12 floats in doubles 14..19, no type punning
    return true;
}

}  // namespace pm_align3d
