// knn_l2_prep.hpp — the prep kernels of the L2 matcher: row norms (knn_l2_prep), the f16 copies of the integer, general-
// float and unit-norm forms (knn_l2_prep16 / 16g / 16u: one body of shared pieces), the centred byte copies of the u8 route
// (knn_l2_prep8 / prep8_u8) and the u8 -> f32 widening.  Private to knn_l2.hip, which holds the scheme and the launcher
// (anonymous namespace: no other translation unit includes this header).
#pragma once
#include "knn_l2_canonical.hpp"

namespace {

using namespace pm_knn;

// What the f16 and u8 prep kernels start with (knn_l2_prep, norms only, keeps its own few lines: its rows are not padded).
// One grid serves both matrices: the first `qblocks` workgroups take the query rows, the others the train rows, `rows`
// rows each; 16 lanes (`sub`) per row, thread group `grp` takes row 16 * it + grp of the block.
struct PrepRows {
    int sub, grp, row0, n;
    bool is_t;
    __device__ __forceinline__ PrepRows(int qblocks, int rows, int nq, int nt)
        : sub(threadIdx.x & 15), grp(threadIdx.x >> 4), is_t(static_cast<int>(blockIdx.x) >= qblocks)
    {
        n = is_t ? nt : nq;
        row0 = (is_t ? blockIdx.x - qblocks : blockIdx.x) * rows;
    }
    template <typename P>
    __device__ __forceinline__ P side(P q, P t) const { return is_t ? t : q; }       // this half's matrix / norms / copy
    __device__ __forceinline__ int row(int it) const { return row0 + it * 16 + grp; }
    __device__ __forceinline__ int clamped(int it) const { return row(it) < n ? row(it) : n - 1; }     // a row that can be read (n >= 1)
};

// What the f16 prep kernels that verify a premise end with: every wave leaves the OR of its threads' flag words in
// w[wave] and (MAX) the largest of their norm bits in w[4 + wave] (LDS; one loop for both: two loops cost five instruction
// lines); after the kernel's barrier thread 0 combines the words and publishes.
template <bool MAX>
__device__ __forceinline__ void prep_wave_words(unsigned bad, unsigned mx, unsigned (&w)[MAX ? 8 : 4])
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        if constexpr (MAX) mx = max(mx, static_cast<unsigned>(__shfl_xor(static_cast<int>(mx), o, 64)));
        bad |= static_cast<unsigned>(__shfl_xor(static_cast<int>(bad), o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if constexpr (MAX) w[4 + (threadIdx.x >> 6)] = mx;
        w[threadIdx.x >> 6] = bad;
    }
}

// ---------------------------------------------------------------------------------------------
// prep: squared norms of the query rows and the train rows in ONE launch (64 rows per block, 16
// lanes per row).  stats words are epoch-tagged 64-bit maxima, (epoch << 32) | payload, so a
// call never has to clear them: values left by earlier calls carry a smaller epoch and lose.
//   stats[0]: payload = float bits of the largest finite train norm
//   stats[1]: payload = 1 when any norm is not finite
// Approximate values: they only feed the coarse pass and its error bound.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void knn_l2_prep(const float* __restrict__ Q, int nq,
                                                   const float* __restrict__ T, int nt, int dim,
                                                   float* __restrict__ qnorm, float* __restrict__ tnorm,
                                                   unsigned long long* __restrict__ stats, unsigned epoch)
{
    __shared__ unsigned wmax[4];
    __shared__ unsigned wbad[4];
    const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int qblocks = (nq + 63) / 64;
    const bool is_t = static_cast<int>(blockIdx.x) >= qblocks;
    const float* x = is_t ? T : Q;
    const int n = is_t ? nt : nq;
    float* norm = is_t ? tnorm : qnorm;
    const int row0 = (is_t ? blockIdx.x - qblocks : blockIdx.x) * 64;
    unsigned mx = 0u, bad = 0u;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = row0 + it * 16 + grp;
        const int rl = row < n ? row : n - 1;
        const float* p = x + static_cast<size_t>(rl) * dim;
        float s = 0.f;
        for (int c = 4 * sub; c < dim; c += 64) {            // dim % 4 == 0 on this route
            const f32x4 v = *reinterpret_cast<const f32x4*>(p + c);
            s = fmaf(v[0], v[0], s); s = fmaf(v[1], v[1], s); s = fmaf(v[2], v[2], s); s = fmaf(v[3], v[3], s);
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
        if (sub == 0 && row < n) {
            norm[row] = s;
            if (!(s < KNN_INF)) bad = 1u;
            else if (is_t) mx = max(mx, f32_bits(s));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = max(mx, static_cast<unsigned>(__shfl_xor(static_cast<int>(mx), o, 64)));
        bad |= static_cast<unsigned>(__shfl_xor(static_cast<int>(bad), o, 64));
    }
    if ((threadIdx.x & 63) == 0) { wmax[threadIdx.x >> 6] = mx; wbad[threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mx = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
        bad = wbad[0] | wbad[1] | wbad[2] | wbad[3];
        const unsigned long long tag = static_cast<unsigned long long>(epoch) << 32;
        if (is_t) atomicMax(&stats[0], tag | mx);
        if (bad) atomicMax(&stats[1], tag | 1ull);
    }
}

// ---------------------------------------------------------------------------------------------
// f16 route: integer-valued descriptors (what OpenCV's SIFT emits: 0..255 stored as float)
//
// For integer data with dim * max|x|^2 < 2^24 every product and every partial sum of q.t is an
// integer below 2^24, so v_mfma_f32_32x32x16_f16 (f16 operands, f32 accumulate) computes the dot
// product EXACTLY at 16x the f32 matrix rate.  knn_l2_prep16 writes f16 copies of both matrices in
// rows of H_ROW = 128 data halfs (zero padded) + one 16-half chunk that carries the row seed
// through the matrix pipe:   train row : (A2, A1, A0, 0, ...),  ||t||^2 = 8192*A2 + 64*A1 + A0
//                            query row : (-4096, -32, -0.5, 0, ...)
// so the ninth k-chunk contributes exactly -||t||^2/2 and the accumulator ends as
// w = q.t - ||t||^2/2 with no VALU work.  The copies are padded to whole tiles (pad train rows
// carry A2 = 60000, i.e. w << any real row), which removes every bounds check from the kernel.
// prep16 also VERIFIES the premise on the device (integers, |x| <= 361, finite): if it fails, bit 1
// of stats[1] is raised and this route's result is not used (auto mode: the f32 kernel runs
// instead; hint mode: the refinement re-scans exactly).  Wrong data costs time, never correctness.
//
// (The coarse kernel itself lives in knn_coarse.hip.  One row group per workgroup instead of the
// 4-iteration loop below was measured slower: 11.7 vs 8.3 us at C3.)
// ---------------------------------------------------------------------------------------------
// SEEDED (round 3, hint route): rows of 128 halfs with no seed chunk; -||t||^2/2 goes to `seeds` (seed order,
// knn_shared.hpp) and starts the accumulators of the coarse kernel instead (RouteF16S).
// DP (round 3): padded data columns per row, 128 or 256 — descriptors of up to 256 dimensions (and any dim: the copies
// are zero padded, so dim % 4 != 0 only changes how the f32 rows are READ).  ALIGNED: rows read as 16-byte vectors
// (dim % 4 == 0 and 16-byte aligned base pointers), else element by element.
// Integer premise for DP columns: |x| <= floor(sqrt(2^24 / DP)) keeps every partial sum below 2^24 (361 / 255).
template <int DP>
struct F16Rows {
    static constexpr int ROWH = DP + 16;                     // halfs per row: data + the seed chunk
    static constexpr int NCB = DP / 128;                     // column blocks of 128 a lane group walks
    static constexpr float MAXABS = DP == 128 ? 361.f : 255.f;
};

// the 8 columns cb + 8*sub .. +7 of one row as floats, zero beyond dim; unconditional (clamped) loads
template <bool ALIGNED>
struct Row8 {
    f32x4 a, b;
    float e[8];
    __device__ __forceinline__ void load(const float* __restrict__ p, int c, int dim)
    {
        if constexpr (ALIGNED) {
            const int c1 = c < dim ? c : dim - 4, c2 = c + 4 < dim ? c + 4 : dim - 4;      // dim % 4 == 0, dim >= 4
            a = *reinterpret_cast<const f32x4*>(p + c1);
            b = *reinterpret_cast<const f32x4*>(p + c2);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) e[k] = p[c + k < dim ? c + k : dim - 1];
        }
    }
    __device__ __forceinline__ void get(int c, int dim, bool live, float (&v)[8]) const
    {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float x = ALIGNED ? (k < 4 ? a[k & 3] : b[k & 3]) : e[k];
            const bool in = ALIGNED ? (c + (k & ~3) < dim) : (c + k < dim);
            v[k] = (live && in) ? x : 0.f;
        }
    }
};

// ---------------------------------------------------------------------------------------------
// u8 route (round 3): u8-valued descriptors — what OpenCV's SIFT emits, 0..255 stored as float (BASELINE configs 2, 3,
// 5) — are centred to x - 128 and ranked on v_mfma_i32_32x32x32_i8: 128-byte rows (4 k-chunks instead of the f16
// route's 9), exact integer dot products, the per-row term -(||t - 128||^2 >> 1) starting the accumulators from the
// per-tile seed array (knn_shared.hpp).  Coarse squared distance of (q, t): ||q'||^2 - 2w = d2 or d2 - 1.
// knn_l2_prep8 writes the centred byte copies (padded to whole tiles, pad rows zero with the pad seed), ||q'||^2 and
// the seeds, and VERIFIES the premise (integers in [0, 255]); a wrong hint raises bit 1 of stats[1] and the refinement
// re-scans exactly, as on the f16 hint route.
// ---------------------------------------------------------------------------------------------
// Body (r6): per element one v_cvt_pk_u8_f32 (round, saturate to [0, 255], place the byte) and the premise checked by
// converting the byte back (v_cvt_f32_ubyteN) and ONE compare with the loaded value: equal exactly for the integers in
// [0, 255] (-0.0 included), unequal for NaN, +-inf, negatives, 256 and up and every non-integer, whichever way the pack
// rounded a tie.  Centring is one XOR per dword, ||x - 128||^2 one v_dot4_i32_i8 per dword (an exact integer, < 2^24, so
// float(sum) has the bits of the fmaf chain it replaces), the row sum four DPP row rotations; a wave publishes the flag
// itself, after one ballot, so clean data meet no LDS instruction and no barrier.
// Rows that FAIL the premise: their bytes, norms and seeds are saturated values and may differ from what a clamp-then-
// truncate would give.  Nothing reads them for a result (the raised epoch flag sends the refinement to the canonical
// f32 scan) and no index or address is derived from them: they only rank candidates nobody uses.
// FULL: dim == 128, no column guards.

// What both u8 prep kernels do with a row once its 16 lanes hold the centred bytes (w0, w1: bytes 8 sub .. 8 sub + 7) and
// si = ||x - 128||^2 (an exact integer: the integer refinement's row term): the byte row, the query copy in the coarse
// kernel's B-fragment order, and from the row's first lane the seeds (pad rows: the pad seed) and the norm.
__device__ __forceinline__ void prep8_row_tail(const PrepRows& a, int row, unsigned w0, unsigned w1, int si,
                                               float* __restrict__ qnorm, float* __restrict__ tnorm, uint2* __restrict__ Q8,
                                               uint2* __restrict__ T8, int* __restrict__ seeds, int t_wide, uint2* __restrict__ Qf)
{
    const bool live = row < a.n;
    a.side(Q8, T8)[static_cast<size_t>(row) * ((a.is_t && t_wide) ? U8_WIDE_ROW16 * 2 : U8_DP / 8) + a.sub] = uint2{w0, w1};
    if (!a.is_t && Qf) Qf[u8_qfrag_index2(row, a.sub)] = uint2{w0, w1};      // (the coarse kernel's B-fragment order)
    if (a.sub == 0) {
        const float s = static_cast<float>(si);
        if (a.is_t) {
            seeds[seed_pos(row)] = live ? -(si >> 1) : U8_PAD_SEED;
            if (t_wide) reinterpret_cast<int*>(T8)[u8_wide_seed_index(row)] = live ? -(si >> 1) : U8_PAD_SEED;
            if (live) tnorm[row] = s;
        } else if (live) {
            qnorm[row] = s;
        }
    }
}

template <int ITERS, bool FULL>
__global__ __launch_bounds__(256) void knn_l2_prep8(const float* __restrict__ Q, int nq, int nq_pad,
                                                    const float* __restrict__ T, int nt, int nt_pad, int dim,
                                                    float* __restrict__ qnorm, float* __restrict__ tnorm,
                                                    uint2* __restrict__ Q8, uint2* __restrict__ T8,
                                                    int* __restrict__ seeds, unsigned long long* __restrict__ stats,
                                                    unsigned epoch, int t_wide, uint2* __restrict__ Qf)
{
    const PrepRows a(nq_pad / (16 * ITERS), 16 * ITERS, nq, nt);
    const float* x = a.side(Q, T);
    const int c0 = 8 * a.sub;
    f32x4 ld[ITERS][2];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {                      // all the loads of a thread in flight together (see f16_fetch)
        const float* p = x + static_cast<size_t>(a.clamped(it)) * dim;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = (FULL || c0 + 4 * e < dim) ? c0 + 4 * e : dim - 4;
            ld[it][e] = *reinterpret_cast<const f32x4*>(p + c);
        }
    }
    bool ok = true;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int row = a.row(it);                            // < n_pad by construction
        const bool live = row < a.n;
        unsigned w[2];
        int si = 0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const f32x4 v = ld[it][e];
            unsigned u = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) u = __builtin_amdgcn_cvt_pk_u8_f32(v[b], b, u);
            bool same = true;
#pragma unroll
            for (int b = 0; b < 4; ++b) same &= static_cast<float>((u >> (8 * b)) & 0xffu) == v[b];
            const bool col = live && (FULL || c0 + 4 * e < dim);
            ok &= same || !col;
            w[e] = col ? (u ^ 0x80808080u) : 0u;              // x - 128 as signed bytes
            si = __builtin_amdgcn_sdot4(static_cast<int>(w[e]), static_cast<int>(w[e]), si, false);
        }
        si += __builtin_amdgcn_update_dpp(0, si, 0x121, 0xF, 0xF, true);       // row_ror:1, 2, 4, 8: the 16 lanes of the row
        si += __builtin_amdgcn_update_dpp(0, si, 0x122, 0xF, 0xF, true);
        si += __builtin_amdgcn_update_dpp(0, si, 0x124, 0xF, 0xF, true);
        si += __builtin_amdgcn_update_dpp(0, si, 0x128, 0xF, 0xF, true);
        prep8_row_tail(a, row, w[0], w[1], si, qnorm, tnorm, Q8, T8, seeds, t_wide, Qf);
    }
    if (__builtin_amdgcn_ballot_w64(!ok) != 0ull) {           // wave-uniform; not u8-valued: scan exactly
        if (!ok) atomicMax(&stats[1], (static_cast<unsigned long long>(epoch) << 32) | 3ull);
    }
}

// The same for u8 INPUT rows (pm_bf_knn_l2_u8: descriptors that never were floats — BASELINE config 5 streams a quarter
// of the bytes): centring is one XOR per dword, the norm one v_dot4_i32_i8 of the centred bytes with themselves, and there is
// no premise to verify.  Rows of `dim` bytes, dim % 4 == 0, dim <= 128, 4-byte aligned.
__global__ __launch_bounds__(256) void knn_l2_prep8_u8(const uint8_t* __restrict__ Q, int nq, int nq_pad,
                                                       const uint8_t* __restrict__ T, int nt, int nt_pad, int dim,
                                                       float* __restrict__ qnorm, float* __restrict__ tnorm,
                                                       uint2* __restrict__ Q8, uint2* __restrict__ T8, int* __restrict__ seeds,
                                                       int t_wide, uint2* __restrict__ Qf)
{
    const PrepRows a(nq_pad / 64, 64, nq, nt);
    const uint8_t* x = a.side(Q, T);
    const int c0 = 8 * a.sub;
    unsigned ld[4][2];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const uint8_t* p = x + static_cast<size_t>(a.clamped(it)) * dim;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = c0 + 4 * e < dim ? c0 + 4 * e : dim - 4;
            ld[it][e] = *reinterpret_cast<const unsigned*>(p + c);
        }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = a.row(it);
        const bool live = row < a.n;
        unsigned w[2];
        int si = 0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            w[e] = (live && c0 + 4 * e < dim) ? (ld[it][e] ^ 0x80808080u) : 0u;
            si = __builtin_amdgcn_sdot4(static_cast<int>(w[e]), static_cast<int>(w[e]), si, false);
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) si += __shfl_xor(si, o, 16);
        prep8_row_tail(a, row, w[0], w[1], si, qnorm, tnorm, Q8, T8, seeds, t_wide, Qf);
    }
}

// u8 rows -> f32 rows (shapes the u8 route does not take: the f32 matcher then runs on the widened copies, same bits)
__global__ __launch_bounds__(256) void knn_u8_widen(const uint8_t* __restrict__ x, size_t n, float* __restrict__ y)
{
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * 256)
        y[i] = static_cast<float>(x[i]);
}
// ---------------------------------------------------------------------------------------------
// f16 route for GENERAL floats (automatic mode, data that failed the integer premise — e.g. SURF's unit-norm
// descriptors, main.cpp:37-40): the same f16 coarse kernel on f16-ROUNDED copies, 16x the f32 matrix rate, with the
// rounding paid for by a wider refinement window (docs/SPEC.md S1c):
//     |fl16(q).fl16(t) - q.t| <= (2^-10 + 2^-22) ||q|| ||t||  <=  2^-11 (1 + 2^-12) (||q||^2 + ||t||^2)
// (every product of two f16 values is exact in the f32 accumulator).  The copies are scaled by powers of two:
//   train rows by ONE factor S_t = 2^(10 - h_t), h_t = ceil(log2 max ||t||) from the norm maximum prep16 published
//     (a query ranks train rows against each other: they need a common scale), so ||S_t t|| < 2^10;
//   query row i by its OWN factor S_i = S_t 2^j, j = clamp(h_t - h_i, -3, 7) (a query's ranking does not depend on
//     its scale): ||S_i q_i|| < 2^10 whenever its norm is within [2^-7, 2^3] of the train maximum, smaller rows lose
//     bits (their window is wide in relation to their distances: candidates, at worst re-scans), rows more than
//     8x larger than every train row are not ranked at all (NaN seed: the refinement scans them exactly).
// The seed chunk carries ||S_t t||^2 rounded to 1/16 (an integer below 2^24 in three exact f16 digits, as on the
// integer route) against query constants (-256, -2, -1/32) 2^j, so the accumulator of (i, t) ends as
// S_i S_t (q_i.t - ||t||^2 / 2) + O(2^j / 64); the refinement multiplies by 1 / (S_i S_t).  Within j in [-3, 7] every
// query constant is an exact f16 and the rows padding the last tile (A2 = A1 = 60000) stay below every real row.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int half_exp_ceil(float norm2)          // h with sqrt(norm2) < 2^h
{
    int e;
    (void)__builtin_frexpf(norm2, &e);          // norm2 = m * 2^e, 0.5 <= m < 1
    return (e + 1) >> 1;
}

__device__ __forceinline__ int train_half_exp(unsigned long long s0, unsigned epoch)
{
    const float tmax = static_cast<unsigned>(s0 >> 32) == epoch ? __uint_as_float(static_cast<unsigned>(s0)) : 0.f;
    return tmax > 0.f ? half_exp_ceil(tmax) : 10;
}

struct QueryScale {
    float sq;            // S_i
    float unscale;       // 1 / (S_i S_t)
    float qc[3];         // seed constants of the query row
    bool unranked;       // ||q_i|| > 8 max ||t||: no f16 image
};

__device__ __forceinline__ QueryScale query_scale(int ht, float qnorm2)     // the SAME function in prep16g and the refinement
{
    QueryScale g;
    const int hq = qnorm2 > 0.f ? half_exp_ceil(qnorm2) : ht;
    const int j = ht - hq;
    g.unranked = j < -3;
    const int jc = j < -3 ? -3 : (j > 7 ? 7 : j);
    g.sq = __builtin_ldexpf(1.f, 10 - ht + jc);
    g.unscale = __builtin_ldexpf(1.f, 2 * ht - 20 - jc);
    g.qc[0] = -__builtin_ldexpf(1.f, 8 + jc);
    g.qc[1] = -__builtin_ldexpf(1.f, 1 + jc);
    g.qc[2] = -__builtin_ldexpf(1.f, jc - 5);
    return g;
}

__global__ void knn_gen_off(unsigned long long* __restrict__ stats, unsigned epoch)
{
    if (threadIdx.x == 0) atomicMax(&stats[3], (static_cast<unsigned long long>(epoch) << 32) | 1ull);
}

// ---------------------------------------------------------------------------------------------
// The pieces of the three f16 prep kernels, each written once: fetch, the row pass (norm, integer premise, (scaled) f16
// store), seed chunk.  The kernels below are lists of them (addressing: PrepRows, flag publication: prep_wave_words, above).
// ---------------------------------------------------------------------------------------------
// all the loads of a thread's four rows are requested before anything is computed (unconditional, clamped
// addresses: a guarded load makes hipcc wait for each in turn — four dependent memory round trips instead of one)
template <int NCB, bool ALIGNED>
__device__ __forceinline__ void f16_fetch(Row8<ALIGNED> (&ld)[4][NCB], const float* x, const PrepRows& a, int dim)
{
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const float* p = x + static_cast<size_t>(a.clamped(it)) * dim;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) ld[it][cb].load(p, 128 * cb + 8 * a.sub, dim);
    }
}

// ONE pass over the lane's 8 * NCB columns of a fetched row (zero beyond dim; all zero unless `live`), doing what the kernel
// asks of it per element, in this order:  NORM     s = fmaf(v, v, s): the lane's part of the row's squared norm, one chain;
//                                          PREMISE  okrow &= v is an integer with |v| <= MAXABS;
//                                          STORE    the f16 copy (ROWH halfs per row): v itself (integers: exact), or SCALED
//                                                   v * sc (|v * sc| < 2^10: in range, round to nearest even).
// (One pass, not one per task: three passes over a value array cost knn_l2_prep16 11-17 instruction lines and 0.15-0.35 us.)
// A kernel names its tasks in DO; s, okrow and xh / row / sc are read only by the tasks that need them.
enum : unsigned { ROW_NORM = 1u, ROW_PREMISE = 2u, ROW_STORE = 4u, ROW_STORE_SCALED = 4u | 8u };
template <int DP, unsigned DO, int ROWH = F16Rows<DP>::ROWH, int NCB, bool ALIGNED>
__device__ __forceinline__ void f16_row_pass(const Row8<ALIGNED> (&ld)[NCB], int c0, int dim, bool live, float& s, bool& okrow,
                                             _Float16* xh, int row, float sc)
{
    constexpr bool NORM = DO & ROW_NORM, PREMISE = DO & ROW_PREMISE, STORE = DO & ROW_STORE, SCALED = DO & 8u;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        float v[8];
        ld[cb].get(128 * cb + c0, dim, live, v);
        f16x8 hv;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if constexpr (NORM) s = fmaf(v[e], v[e], s);
            if constexpr (PREMISE) okrow &= (v[e] == __builtin_rintf(v[e])) && (__builtin_fabsf(v[e]) <= F16Rows<DP>::MAXABS);
            if constexpr (STORE) hv[e] = static_cast<_Float16>(SCALED ? v[e] * sc : v[e]);
        }
        if constexpr (STORE) *reinterpret_cast<f16x8*>(xh + static_cast<size_t>(row) * ROWH + 128 * cb + c0) = hv;
    }
}

// the row's squared norm from its 16 lanes' parts
__device__ __forceinline__ float f16_row_sum(float s)
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
    return s;
}

// Seed chunk: the 16 halfs behind a row's DP data columns.  An integer tn < 2^24 travels as three exact f16 digits,
// tn = 8192 A2 + 64 A1 + A0, against the query row's three constants.
__device__ __forceinline__ void f16_seed_digits(f16x8& e0, unsigned tn)
{
    e0[0] = static_cast<_Float16>(static_cast<float>(tn >> 13));
    e0[1] = static_cast<_Float16>(static_cast<float>((tn >> 6) & 127u));
    e0[2] = static_cast<_Float16>(static_cast<float>(tn & 63u));
}

template <int DP>
__device__ __forceinline__ void f16_store_seed(_Float16* __restrict__ xh, int row, const f16x8& e0)
{
    const f16x8 e1 = {0, 0, 0, 0, 0, 0, 0, 0};
    *reinterpret_cast<f16x8*>(xh + static_cast<size_t>(row) * F16Rows<DP>::ROWH + DP) = e0;
    *reinterpret_cast<f16x8*>(xh + static_cast<size_t>(row) * F16Rows<DP>::ROWH + DP + 8) = e1;
}

// integer form: ||t||^2 itself against (-4096, -32, -0.5)
__device__ __forceinline__ f16x8 f16_seed_integer(bool is_t, bool live, float s)
{
    f16x8 e0 = {0, 0, 0, 0, 0, 0, 0, 0};
    if (is_t) {
        if (live) f16_seed_digits(e0, s < 16777216.f ? static_cast<unsigned>(s) : 0u);    // exact when eligible
        else e0[0] = static_cast<_Float16>(60000.f);                                      // pad row: w ~ -2.4e8
    } else {
        e0[0] = static_cast<_Float16>(-4096.f);
        e0[1] = static_cast<_Float16>(-32.f);
        e0[2] = static_cast<_Float16>(-0.5f);
    }
    return e0;
}

// scaled form (general floats): ||S_t t||^2 to 1/16 against the query's own constants
__device__ __forceinline__ f16x8 f16_seed_scaled(bool is_t, bool live, float norm2, float st, const QueryScale& qs)
{
    f16x8 e0 = {0, 0, 0, 0, 0, 0, 0, 0};
    if (is_t) {
        if (live) {
            // ||S_t t||^2 < 2^20, kept to 1/16: an integer below 2^24
            const float z = __builtin_rintf(norm2 * st * st * 16.f);
            f16_seed_digits(e0, z < 16777216.f ? static_cast<unsigned>(z) : 16777215u);
        } else {
            e0[0] = static_cast<_Float16>(60000.f);  // pad row: w = -1.55e7 2^j, below every real row (>= -2^20 - 2^19 2^j)
            e0[1] = static_cast<_Float16>(60000.f);
        }
    } else if (live && qs.unranked) {
        e0[0] = static_cast<_Float16>(__builtin_nanf(""));    // every value of this query is NaN: nothing is ranked
    } else {
        e0[0] = static_cast<_Float16>(qs.qc[0]);
        e0[1] = static_cast<_Float16>(qs.qc[1]);
        e0[2] = static_cast<_Float16>(qs.qc[2]);
    }
    return e0;
}

// (The scaled copy of a row — train rows by S_t, a query row by its own factor, an unranked query's row all zero — is the
// row pass with STORE and SCALED, called from the kernel: wrapped in one more helper, with or without the seed chunk,
// knn_l2_prep16u<256, true> takes 100 registers instead of 88 and loses a wave per SIMD.)

// knn_l2_prep16 (every f16 route's first pass): norms + premise + integer copies
template <bool SEEDED, int DP, bool ALIGNED>
__global__ __launch_bounds__(256) void knn_l2_prep16(const float* __restrict__ Q, int nq, int nq_pad,
                                                     const float* __restrict__ T, int nt, int nt_pad, int dim,
                                                     float* __restrict__ qnorm, float* __restrict__ tnorm,
                                                     _Float16* __restrict__ Qh, _Float16* __restrict__ Th, float* __restrict__ seeds,
                                                     unsigned long long* __restrict__ stats, unsigned epoch)
{
    typedef F16Rows<DP> G;
    constexpr int ROWH = SEEDED ? DP : G::ROWH;
    __shared__ unsigned w[8];
    const PrepRows a(nq_pad / 64, 64, nq, nt);
    const int sub = a.sub, grp = a.grp, n = a.n, row0 = a.row0;      // (copies: read through `a` in the row loop, the compiler's
    const bool is_t = a.is_t;                                        // output is longer here and costs prep16u a wave per SIMD)
    float* norm = a.side(qnorm, tnorm);
    _Float16* xh = a.side(Qh, Th);
    const int c0 = 8 * sub;
    unsigned mx = 0u, bad = 0u;
    Row8<ALIGNED> ld[4][G::NCB];
    f16_fetch(ld, a.side(Q, T), a, dim);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = row0 + it * 16 + grp;                 // < n_pad by construction
        const bool live = row < n;
        float s = 0.f;
        bool okrow = true;
        f16_row_pass<DP, ROW_NORM | ROW_PREMISE | ROW_STORE, ROWH>(ld[it], c0, dim, live, s, okrow, xh, row, 1.f);
        s = f16_row_sum(s);
        if (!okrow) bad |= 2u;
        if (sub == 0) {
            if (live) {
                norm[row] = s;
                if (!(s < KNN_INF)) bad |= 3u;
                else if (is_t) mx = max(mx, f32_bits(s));
            }
            if constexpr (SEEDED) {
                // exact when eligible (||t||^2 an integer below 2^24); rows padding the last tile sit below every real row
                if (is_t) seeds[seed_pos(row)] = live ? -0.5f * s : -1.0e30f;
            } else {
                f16_store_seed<DP>(xh, row, f16_seed_integer(is_t, live, s));
            }
        }
    }
    prep_wave_words<true>(bad, mx, w);
    __syncthreads();
    if (threadIdx.x == 0) {
        mx = max(max(w[4], w[5]), max(w[6], w[7]));
        bad = w[0] | w[1] | w[2] | w[3];
        const unsigned long long tag = static_cast<unsigned long long>(epoch) << 32;
        if (is_t) atomicMax(&stats[0], tag | mx);
        // stats[1] is a max, so the flags are published as the values 1 (non-finite), 2 (not
        // f16-eligible) or 3 (both): 3 >= 2 >= 1 keeps "not eligible" visible once any block saw it,
        // and a non-finite input is never eligible.
        if (bad) atomicMax(&stats[1], tag | static_cast<unsigned long long>(bad == 1u ? 3u : bad));
    }
}

// knn_l2_prep16g (automatic route, second pass): early-out + scaled copies from the norms knn_l2_prep16 stored
template <int DP, bool ALIGNED>
__global__ __launch_bounds__(256) void knn_l2_prep16g(const float* __restrict__ Q, int nq, int nq_pad,
                                                      const float* __restrict__ T, int nt, int nt_pad, int dim,
                                                      const float* __restrict__ qnorm, const float* __restrict__ tnorm,
                                                      _Float16* __restrict__ Qh, _Float16* __restrict__ Th,
                                                      const unsigned long long* __restrict__ stats, unsigned epoch)
{
    const unsigned long long s1 = stats[1];
    const bool flagged = static_cast<unsigned>(s1 >> 32) == epoch;
    if (!(flagged && (s1 & 2ull))) return;                  // integer-valued data: prep16's copies stand
    if (s1 & 1ull) return;                                  // a non-finite input: the refinement scans everything anyway
    const int ht = train_half_exp(stats[0], epoch);
    const float st = __builtin_ldexpf(1.f, 10 - ht);
    const PrepRows a(nq_pad / 64, 64, nq, nt);
    const float* norm = a.side(qnorm, tnorm);
    _Float16* xh = a.side(Qh, Th);
    Row8<ALIGNED> ld[4][F16Rows<DP>::NCB];
    float nrm[4];
    f16_fetch(ld, a.side(Q, T), a, dim);
#pragma unroll
    for (int it = 0; it < 4; ++it) nrm[it] = norm[a.clamped(it)];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = a.row(it);
        const QueryScale qs = query_scale(ht, nrm[it]);
        const bool zero = !(row < a.n) || (!a.is_t && qs.unranked);
        float unused = 0.f;
        bool ok = true;
        f16_row_pass<DP, ROW_STORE_SCALED>(ld[it], 8 * a.sub, dim, !zero, unused, ok, xh, row, a.is_t ? st : qs.sq);
        if (a.sub == 0) f16_store_seed<DP>(xh, row, f16_seed_scaled(a.is_t, row < a.n, nrm[it], st, qs));
    }
}

// knn_l2_prep16u: norms + bound check + scaled copies.
// The two passes above in ONE launch for data whose scale the caller states (PM_KNN_HINT_UNIT_NORM, round 3): every train
// row has ||t|| <= 1 (SURF, L2-normalised descriptors: what the reference itself matches, main.cpp:37-40).  The train
// scale then needs no norm maximum: the bound 1 IS the published maximum (stats[0]), S_t = 2^(10 - h(1)), every query row
// still gets its own power of two from its own norm, and the premise is verified here — a train row beyond the bound raises
// the non-finite flag, i.e. every query is scanned exactly (a wrong hint costs time, never a result bit).  Everything
// downstream (coarse pass, refinement, window) reads the same words as on the automatic route with the bound in place of
// the measured maximum: the window is the automatic route's whenever the largest train row really has norm 1.
template <int DP, bool ALIGNED>
__global__ __launch_bounds__(256) void knn_l2_prep16u(const float* __restrict__ Q, int nq, int nq_pad,
                                                      const float* __restrict__ T, int nt, int nt_pad, int dim,
                                                      float* __restrict__ qnorm, float* __restrict__ tnorm,
                                                      _Float16* __restrict__ Qh, _Float16* __restrict__ Th,
                                                      unsigned long long* __restrict__ stats, unsigned epoch)
{
    constexpr float BOUND2 = 1.0009765625f;                 // the stated maximum of ||t||^2: 1, with 2^-10 of slack for rows that
                                                            // were normalised in f32 (same half-exponent as 1.0)
    __shared__ unsigned wbad[4];
    const int ht = half_exp_ceil(BOUND2);
    const float st = __builtin_ldexpf(1.f, 10 - ht);
    const PrepRows a(nq_pad / 64, 64, nq, nt);
    const int sub = a.sub, grp = a.grp, n = a.n, row0 = a.row0;      // (copies: see knn_l2_prep16)
    const bool is_t = a.is_t;
    float* norm = a.side(qnorm, tnorm);
    _Float16* xh = a.side(Qh, Th);
    const int c0 = 8 * sub;
    unsigned bad = 0u;
    Row8<ALIGNED> ld[4][F16Rows<DP>::NCB];
    f16_fetch(ld, a.side(Q, T), a, dim);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = row0 + it * 16 + grp;
        const bool live = row < n;
        float s = 0.f, unused = 0.f;                        // the row's squared norm, as knn_l2_prep16 computes it
        bool ok = true;
        f16_row_pass<DP, ROW_NORM>(ld[it], c0, dim, live, s, ok, xh, row, 1.f);
        s = f16_row_sum(s);
        if (live && (!(s < KNN_INF) || (is_t && !(s <= BOUND2)))) bad = 3u;      // not finite, or beyond the stated bound
        const QueryScale qs = query_scale(ht, s);
        const float sc = is_t ? st : qs.sq;
        const bool zero = !live || (!is_t && qs.unranked);
        f16_row_pass<DP, ROW_STORE_SCALED>(ld[it], c0, dim, !zero, unused, ok, xh, row, sc);
        if (sub == 0) {
            if (live) norm[row] = s;
            f16_store_seed<DP>(xh, row, f16_seed_scaled(is_t, live, s, st, qs));
        }
    }
    prep_wave_words<false>(bad, 0u, wbad);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long tag = static_cast<unsigned long long>(epoch) << 32;
        bad = wbad[0] | wbad[1] | wbad[2] | wbad[3];
        if (blockIdx.x == 0) {
            atomicMax(&stats[0], tag | f32_bits(BOUND2));   // the "maximum" every later kernel scales and bounds with
            atomicMax(&stats[1], tag | 2ull);               // general floats (not the integer route)
        }
        if (bad) atomicMax(&stats[1], tag | 3ull);
    }
}

}  // namespace
