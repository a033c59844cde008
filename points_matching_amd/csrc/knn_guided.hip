// knn_guided.hip — guided k-NN (docs/SPEC.md S48-S49): the k nearest train rows of every query AMONG the train keypoints
// that agree with a two-view model (F: Sampson or symmetric epipolar distance, H: one-way reprojection error), one launch.
// The counterpart of the `mask` argument of cv::BFMatcher::knnMatch / of COLMAP's guided matching, with the mask never
// materialised: the gate (S8 / S21 in fp32, the RANSAC scorers' arithmetic) sits in front of the distance.
//
// One wavefront per query (64-thread workgroups, so __syncthreads() is a wave-level fence and costs no s_barrier):
//   gate phase      the lanes sweep the train keypoints, 64 per step (8 bytes each, coalesced); the per-query terms
//                   (a, b, c of S8 or u, v, w, rhs of S21) are wave-uniform and sit in scalar registers; a ballot turns
//                   the step into admitted row ids, appended in row order to a 128-entry ring in LDS.
//   distance phase  every time the ring holds GK_BATCH = 64 ids (and once more when the sweep ends) the wave evaluates
//                   exactly those rows: float rows with 8 lanes per row (lane l IS accumulator l of S1, 8 rows per pass),
//                   u8 rows (dim <= 256) and binary rows with one lane per row on integers (dot4 / popcount).  A row the
//                   gate did not admit is never read.
//   top-k           every lane keeps the KL smallest S3 keys it has seen; k 64-bit wave minima merge the 64 lists.
// The matrix cores are not used: the gate is expected to admit a few percent of the rows, and an MFMA pass would pay for
// all nq x nt pairs.  Nothing in the result depends on GK_BATCH, the ring size or the grid: a row's distance is a function
// of the two rows alone and the order is decided by the keys.
#include "pm_common.hpp"
#include "wave_ops.hpp"

namespace {

constexpr int GK_BATCH = 64;               // admitted rows per distance phase
constexpr int GK_RING = 128;               // ids in flight: < GK_BATCH left over + 64 from one step
constexpr int GK_MAX_GRID = 1 << 20;       // workgroups; more queries than this are taken in a grid-stride loop
constexpr int GK_U8_INT_MAX_DIM = 256;     // u8 rows: every partial sum of S1 is an integer below 2^24 up to here
constexpr int CLASS_POS_FINITE = 0x180;    // v_cmp_class: positive subnormal | positive normal
constexpr uint64_t GK_EMPTY = ~0ull;

__device__ __forceinline__ float uniform_f32(float v)   // wave-uniform value -> scalar register
{
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}

// SPEC S3 ordering key; NaN distances are canonicalised so they sort after +inf.
__device__ __forceinline__ uint64_t gk_key(float dist, int idx)
{
    const uint32_t b = (dist != dist) ? 0x7FC00000u : __float_as_uint(dist);
    return (static_cast<uint64_t>(b) << 32) | static_cast<uint32_t>(idx);
}

// ---- S48: the gates.  prep() holds what depends on the query alone, test() the rest, in the order of S8 / S21 ----------
template <int KIND>
struct GateF {
    float f0, f1, f3, f4, f6, f7, a, b, c, thr2;
    __device__ __forceinline__ void prep(const float (&f)[9], float x, float y, float t2)
    {
        f0 = f[0]; f1 = f[1]; f3 = f[3]; f4 = f[4]; f6 = f[6]; f7 = f[7];
        a = uniform_f32(fmaf(f[0], x, fmaf(f[1], y, f[2])));
        b = uniform_f32(fmaf(f[3], x, fmaf(f[4], y, f[5])));
        c = uniform_f32(fmaf(f[6], x, fmaf(f[7], y, f[8])));
        thr2 = t2;
    }
    __device__ __forceinline__ bool test(float xp, float yp) const
    {
        const float num = fmaf(xp, a, fmaf(yp, b, c));
        const float at = fmaf(f0, xp, fmaf(f3, yp, f6));
        const float bt = fmaf(f1, xp, fmaf(f4, yp, f7));
        const float n2 = num * num;
        if (KIND == PM_GUIDE_F_SAMPSON) {
            const float den = fmaf(a, a, fmaf(b, b, fmaf(at, at, bt * bt)));
            return n2 <= thr2 * den;
        }
        const float d2 = fmaf(a, a, b * b);
        const float d1 = fmaf(at, at, bt * bt);
        return (n2 <= thr2 * d2) && (n2 <= thr2 * d1);
    }
};

struct GateH {
    float u, v, w, rhs;
    bool rhs_ok;
    __device__ __forceinline__ void prep(const float (&h)[9], float x, float y, float t2)
    {
        u = uniform_f32(fmaf(h[0], x, fmaf(h[1], y, h[2])));
        v = uniform_f32(fmaf(h[3], x, fmaf(h[4], y, h[5])));
        w = uniform_f32(fmaf(h[6], x, fmaf(h[7], y, h[8])));
        rhs = uniform_f32(t2 * (w * w));
        rhs_ok = __builtin_amdgcn_classf(rhs, CLASS_POS_FINITE);
    }
    __device__ __forceinline__ bool test(float xp, float yp) const
    {
        const float du = fmaf(-xp, w, u);
        const float dv = fmaf(-yp, w, v);
        return (fmaf(du, du, dv * dv) <= rhs) && rhs_ok;
    }
};

template <int KIND> struct GateOf { typedef GateF<KIND> type; };
template <> struct GateOf<PM_GUIDE_H> { typedef GateH type; };

// ---- the KL smallest keys one lane has seen ----------------------------------------------------------------------------
template <int KL>
struct GkList {
    uint64_t k[KL];
    __device__ __forceinline__ void reset()
    {
#pragma unroll
        for (int i = 0; i < KL; ++i) k[i] = GK_EMPTY;
    }
    __device__ __forceinline__ void insert(uint64_t key)
    {
        if (key < k[KL - 1]) {
            k[KL - 1] = key;
#pragma unroll
            for (int i = KL - 1; i > 0; --i)
                if (k[i] < k[i - 1]) { const uint64_t t = k[i]; k[i] = k[i - 1]; k[i - 1] = t; }
        }
    }
    __device__ __forceinline__ void pop()
    {
#pragma unroll
        for (int i = 0; i + 1 < KL; ++i) k[i] = k[i + 1];
        k[KL - 1] = GK_EMPTY;
    }
};

// ---- distances ------------------------------------------------------------------------------------------------------------
// SPEC S1 by 8 consecutive lanes on rows of floats or of bytes converted to float: lane l (0..7) of the group is
// accumulator l of the canonical form (same products, same order), the combine uses the canonical association, the
// tail runs after it.  All loads of a block of 64 columns are issued before the first subtraction.  Result in lane 0.
template <class E>
__device__ __forceinline__ float gk_l2sqr_coop8(const E* __restrict__ a, const E* __restrict__ b, int dim, int l)
{
    float acc = 0.f;
    const int full8 = dim & ~7;
    int j0 = 0;
    for (; j0 + 64 <= full8; j0 += 64) {
        float av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { av[u] = static_cast<float>(a[j0 + 8 * u + l]); bv[u] = static_cast<float>(b[j0 + 8 * u + l]); }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const float t = av[u] - bv[u]; const float p = t * t; acc = acc + p; }
    }
    for (; j0 < full8; j0 += 8) {
        const float t = static_cast<float>(a[j0 + l]) - static_cast<float>(b[j0 + l]);
        const float p = t * t;
        acc = acc + p;
    }
    float d = pm::coop8_combine(acc);                        // meaningful in lane 0
    for (int j = full8; j < dim; ++j) {
        const float t = static_cast<float>(a[j]) - static_cast<float>(b[j]);
        const float p = t * t;
        d = d + p;
    }
    return d;
}

// f(query word, train word) over the nw 32-bit words of a row pair; 16-byte loads when vec16
template <class F>
__device__ __forceinline__ void gk_for_words(const uint32_t* __restrict__ q, const uint32_t* __restrict__ t, int nw, bool vec16, F f)
{
    int w = 0;
    if (vec16)
        for (; w + 4 <= nw; w += 4) {
            const uint4 a = *reinterpret_cast<const uint4*>(q + w);
            const uint4 b = *reinterpret_cast<const uint4*>(t + w);
            f(a.x, b.x); f(a.y, b.y); f(a.z, b.z); f(a.w, b.w);
        }
    for (; w < nw; ++w) f(q[w], t[w]);
}

// Descriptor policies.  LANES = lanes per admitted row; Query = what prep() derives from the query row once.
struct PolF32 {
    typedef float elem;
    static constexpr int LANES = 8;
};
struct PolU8Wide {       // u8 rows with dim > 256: S1 in float on the converted values, like the widened matcher route
    typedef uint8_t elem;
    static constexpr int LANES = 8;
};
struct PolU8 {           // u8 rows with dim <= 256: the canonical value IS the integer squared distance
    typedef uint8_t elem;
    static constexpr int LANES = 1;
    struct Query { int qq; bool words, vec16; };
    static __device__ __forceinline__ Query prep(const uint8_t* __restrict__ q, const uint8_t* T, int dim)
    {
        Query s;
        const uintptr_t both = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(T);
        s.words = (dim & 3) == 0 && (both & 3) == 0;
        s.vec16 = (dim & 15) == 0 && (both & 15) == 0;
        int qq = 0;
        for (int j = 0; j < dim; ++j) qq += static_cast<int>(q[j]) * static_cast<int>(q[j]);
        s.qq = qq;
        return s;
    }
    static __device__ __forceinline__ float dist(const Query& s, const uint8_t* __restrict__ q, const uint8_t* __restrict__ t, int dim)
    {
        int d2 = 0;
        if (s.words) {           // ||q||^2 + ||t||^2 - 2 q.t on v_dot4_u32_u8: integers below 2^25
            unsigned qt = 0, tt = 0;
            gk_for_words(reinterpret_cast<const uint32_t*>(q), reinterpret_cast<const uint32_t*>(t), dim >> 2, s.vec16,
                         [&](uint32_t a, uint32_t b) {
                             qt = __builtin_amdgcn_udot4(a, b, qt, false);
                             tt = __builtin_amdgcn_udot4(b, b, tt, false);
                         });
            d2 = s.qq + static_cast<int>(tt) - 2 * static_cast<int>(qt);
        } else {
            for (int j = 0; j < dim; ++j) {
                const int e = static_cast<int>(q[j]) - static_cast<int>(t[j]);
                d2 += e * e;
            }
        }
        return __builtin_sqrtf(static_cast<float>(d2));
    }
};
struct PolHamming {      // S2: popcount of XOR over bytes / 4 words, reported as float
    typedef uint8_t elem;
    static constexpr int LANES = 1;
    struct Query { bool vec16; };
    static __device__ __forceinline__ Query prep(const uint8_t* q, const uint8_t* T, int bytes)
    {
        Query s;
        s.vec16 = (bytes & 15) == 0 && ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(T)) & 15) == 0;
        return s;
    }
    static __device__ __forceinline__ float dist(const Query& s, const uint8_t* __restrict__ q, const uint8_t* __restrict__ t, int bytes)
    {
        int c = 0;
        gk_for_words(reinterpret_cast<const uint32_t*>(q), reinterpret_cast<const uint32_t*>(t), bytes >> 2, s.vec16,
                     [&](uint32_t a, uint32_t b) { c += __popc(a ^ b); });
        return static_cast<float>(c);
    }
};

// Distance phase over ring entries [head, head + n), n <= GK_BATCH: 8 lanes per row, 8 rows per pass.  A group beyond the
// last entry repeats the last ADMITTED row (the shuffles want whole groups) and discards the value.
template <class POL, int KL>
__device__ __forceinline__ void gk_distances8(const int* ring, unsigned head, int n, const typename POL::elem* __restrict__ qrow,
                                              const typename POL::elem* __restrict__ T, int width, int lane, GkList<KL>& best)
{
    const int g = lane >> 3, l = lane & 7;
    for (int p0 = 0; p0 < n; p0 += 8) {
        const int idx = p0 + g;
        const bool valid = idx < n;
        const int row = ring[(head + static_cast<unsigned>(valid ? idx : n - 1)) & (GK_RING - 1)];
        const float d2 = gk_l2sqr_coop8(qrow, T + static_cast<size_t>(row) * width, width, l);
        if (valid && l == 0) best.insert(gk_key(__builtin_sqrtf(d2), row));
    }
}

template <class POL, int KL>
__device__ __forceinline__ void gk_distances1(const int* ring, unsigned head, int n, const typename POL::Query& qs,
                                              const typename POL::elem* __restrict__ qrow,
                                              const typename POL::elem* __restrict__ T, int width, int lane, GkList<KL>& best)
{
    if (lane < n) {
        const int row = ring[(head + static_cast<unsigned>(lane)) & (GK_RING - 1)];
        best.insert(gk_key(POL::dist(qs, qrow, T + static_cast<size_t>(row) * width, width), row));
    }
}

template <class POL, int LANES> struct GkPhase;
template <class POL>
struct GkPhase<POL, 8> {
    struct Query {};
    static __device__ __forceinline__ Query prep(const typename POL::elem*, const typename POL::elem*, int) { return Query(); }
    template <int KL>
    static __device__ __forceinline__ void run(const int* ring, unsigned head, int n, const Query&, const typename POL::elem* qrow,
                                               const typename POL::elem* T, int width, int lane, GkList<KL>& best)
    {
        gk_distances8<POL, KL>(ring, head, n, qrow, T, width, lane, best);
    }
};
template <class POL>
struct GkPhase<POL, 1> {
    typedef typename POL::Query Query;
    static __device__ __forceinline__ Query prep(const typename POL::elem* q, const typename POL::elem* T, int width)
    {
        return POL::prep(q, T, width);
    }
    template <int KL>
    static __device__ __forceinline__ void run(const int* ring, unsigned head, int n, const Query& qs, const typename POL::elem* qrow,
                                               const typename POL::elem* T, int width, int lane, GkList<KL>& best)
    {
        gk_distances1<POL, KL>(ring, head, n, qs, qrow, T, width, lane, best);
    }
};

template <class POL, int KIND, int KL>
__global__ __launch_bounds__(64) void knn_guided(const typename POL::elem* __restrict__ Q, int nq,
                                                 const typename POL::elem* __restrict__ T, int nt, int width,
                                                 const float* __restrict__ kp1, const float* __restrict__ kp2,
                                                 const double* __restrict__ M, float tau, int k, pm_match* __restrict__ out,
                                                 int32_t* __restrict__ n_admitted)
{
    typedef GkPhase<POL, POL::LANES> Phase;
    __shared__ int ring[GK_RING];
    const int lane = threadIdx.x;

    // S48: M32 = (float)M once; a model with a non-finite entry or with nine zeros admits nothing
    float m[9];
    bool finite = true, nonzero = false;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        m[i] = uniform_f32(static_cast<float>(M[i]));
        finite = finite && (__float_as_uint(m[i]) & 0x7F800000u) != 0x7F800000u;
        nonzero = nonzero || m[i] != 0.f;
    }
    const bool model_ok = finite && nonzero;
    const float thr2 = tau * tau;

    for (int qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        const float2 p = *reinterpret_cast<const float2*>(kp1 + 2 * static_cast<size_t>(qi));
        typename GateOf<KIND>::type gate;
        gate.prep(m, p.x, p.y, thr2);
        const typename POL::elem* qrow = Q + static_cast<size_t>(qi) * width;
        const typename Phase::Query qs = Phase::prep(qrow, T, width);
        GkList<KL> best;
        best.reset();
        unsigned head = 0, tail = 0;            // ring positions; tail also counts the admitted rows

        if (model_ok) {
            for (int j0 = 0; j0 < nt; j0 += 64) {
                const int j = j0 + lane;
                bool in = false;
                if (j < nt) {
                    const float2 pp = *reinterpret_cast<const float2*>(kp2 + 2 * static_cast<size_t>(j));
                    in = gate.test(pp.x, pp.y);
                }
                const unsigned long long mask = __ballot(in);
                if (mask == 0ull) continue;                                     // wave-uniform
                if (in) ring[(tail + static_cast<unsigned>(pm::lane_rank(mask, lane))) & (GK_RING - 1)] = j;
                tail += static_cast<unsigned>(__popcll(mask));
                __syncthreads();
                if (tail - head >= static_cast<unsigned>(GK_BATCH)) {
                    Phase::template run<KL>(ring, head, GK_BATCH, qs, qrow, T, width, lane, best);
                    head += GK_BATCH;
                    __syncthreads();                                            // the ring slots are free again
                }
            }
            if (tail != head) Phase::template run<KL>(ring, head, static_cast<int>(tail - head), qs, qrow, T, width, lane, best);
            __syncthreads();
        }

        // the k smallest of the 64 lists: keys are distinct (the row id is in them), so exactly one lane pops per round
        for (int r = 0; r < k; ++r) {
            const uint64_t mine = best.k[0];
            const uint64_t mn = pm::wave_min_u64(mine);
            if (mine == mn && mn != GK_EMPTY) best.pop();
            if (lane == 0) {
                pm_match rec;
                rec.queryIdx = qi;
                rec.trainIdx = mn == GK_EMPTY ? -1 : static_cast<int>(static_cast<uint32_t>(mn));
                rec.imgIdx = 0;
                rec.distance = mn == GK_EMPTY ? __builtin_inff() : __uint_as_float(static_cast<uint32_t>(mn >> 32));
                out[static_cast<size_t>(qi) * k + r] = rec;
            }
        }
        if (n_admitted && lane == 0) n_admitted[qi] = static_cast<int32_t>(tail);
    }
}

enum { GK_F32 = 0, GK_U8 = 1, GK_HAMMING = 2 };

struct GkArgs {
    const void *q, *t;
    int nq, nt, width;
    const float *kp1, *kp2;
    int kind;
    const double* M;
    float tau;
    int k;
    pm_match* out;
    int32_t* n_admitted;
};

template <class POL, int KIND>
void gk_launch_k(pm_ctx* ctx, const GkArgs& a)
{
    typedef typename POL::elem E;
    const dim3 grid(a.nq < GK_MAX_GRID ? a.nq : GK_MAX_GRID), block(64);
    const E* q = static_cast<const E*>(a.q);
    const E* t = static_cast<const E*>(a.t);
#define PM_GK(KL_)                                                                                                           \
    hipLaunchKernelGGL((knn_guided<POL, KIND, KL_>), grid, block, 0, ctx->stream, q, a.nq, t, a.nt, a.width, a.kp1, a.kp2,  \
                       a.M, a.tau, a.k, a.out, a.n_admitted)
    if (a.k == 1) PM_GK(1);
    else if (a.k == 2) PM_GK(2);
    else PM_GK(4);
#undef PM_GK
}

template <class POL>
void gk_launch(pm_ctx* ctx, const GkArgs& a)
{
    if (a.kind == PM_GUIDE_F_SAMPSON) gk_launch_k<POL, PM_GUIDE_F_SAMPSON>(ctx, a);
    else if (a.kind == PM_GUIDE_F_SYM) gk_launch_k<POL, PM_GUIDE_F_SYM>(ctx, a);
    else gk_launch_k<POL, PM_GUIDE_H>(ctx, a);
}

int gk_run(pm_ctx* ctx, int policy, const GkArgs& a)
{
    PM_REQUIRE(ctx != nullptr && a.M != nullptr, PM_E_INVALID, "null context or model pointer");
    PM_REQUIRE(a.nq >= 0 && a.nt >= 0 && a.width >= 1, PM_E_INVALID, "need nq, nt >= 0 and a positive row width");
    PM_REQUIRE(policy != GK_HAMMING || (a.width % 4) == 0, PM_E_INVALID, "bytes must be a multiple of 4");
    PM_REQUIRE(a.k >= 1 && a.k <= 4, PM_E_INVALID, "need 1 <= k <= 4");
    PM_REQUIRE(a.kind == PM_GUIDE_F_SAMPSON || a.kind == PM_GUIDE_F_SYM || a.kind == PM_GUIDE_H, PM_E_INVALID,
               "unknown gate kind");
    PM_REQUIRE(a.nq == 0 || (a.q && a.kp1 && a.out), PM_E_INVALID, "null query / query keypoint / output pointer");
    PM_REQUIRE(a.nt == 0 || (a.t && a.kp2), PM_E_INVALID, "null train / train keypoint pointer");
    PM_REQUIRE(((reinterpret_cast<uintptr_t>(a.kp1) | reinterpret_cast<uintptr_t>(a.kp2) | reinterpret_cast<uintptr_t>(a.M)) & 7) == 0,
               PM_E_INVALID, "keypoint arrays and the model must be 8-byte aligned");
    PM_REQUIRE(policy != GK_F32 || ((reinterpret_cast<uintptr_t>(a.q) | reinterpret_cast<uintptr_t>(a.t)) & 3) == 0,
               PM_E_INVALID, "float descriptor buffers must be 4-byte aligned");
    PM_REQUIRE(policy != GK_HAMMING || ((reinterpret_cast<uintptr_t>(a.q) | reinterpret_cast<uintptr_t>(a.t)) & 3) == 0,
               PM_E_INVALID, "binary descriptor buffers must be 4-byte aligned");
    if (a.nq == 0) return PM_OK;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    pm::ScopedKernelTime timer(ctx, "knn_guided");
    if (policy == GK_F32) gk_launch<PolF32>(ctx, a);
    else if (policy == GK_HAMMING) gk_launch<PolHamming>(ctx, a);
    else if (a.width <= GK_U8_INT_MAX_DIM) gk_launch<PolU8>(ctx, a);
    else gk_launch<PolU8Wide>(ctx, a);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

}  // namespace

extern "C" int pm_bf_knn_guided_l2_f32_dev(pm_ctx* ctx, const float* d_q, int nq, const float* d_t, int nt, int dim,
                                           const float* d_kp1_xy, const float* d_kp2_xy, int kind, const double* d_M, float tau,
                                           int k, pm_match* d_out, int32_t* d_n_admitted)
{
    return gk_run(ctx, GK_F32, GkArgs{d_q, d_t, nq, nt, dim, d_kp1_xy, d_kp2_xy, kind, d_M, tau, k, d_out, d_n_admitted});
}

extern "C" int pm_bf_knn_guided_l2_u8_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int dim,
                                          const float* d_kp1_xy, const float* d_kp2_xy, int kind, const double* d_M, float tau,
                                          int k, pm_match* d_out, int32_t* d_n_admitted)
{
    return gk_run(ctx, GK_U8, GkArgs{d_q, d_t, nq, nt, dim, d_kp1_xy, d_kp2_xy, kind, d_M, tau, k, d_out, d_n_admitted});
}

extern "C" int pm_bf_knn_guided_hamming_u8_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int bytes,
                                               const float* d_kp1_xy, const float* d_kp2_xy, int kind, const double* d_M,
                                               float tau, int k, pm_match* d_out, int32_t* d_n_admitted)
{
    return gk_run(ctx, GK_HAMMING, GkArgs{d_q, d_t, nq, nt, bytes, d_kp1_xy, d_kp2_xy, kind, d_M, tau, k, d_out, d_n_admitted});
}
