// match_guided.cpp — host code around the guided k-NN kernel (knn_guided.hip): the one-call guided matching of SPEC S50
// (guided 2-NN + the fused ratio filter + gather, back to back on the context's stream) and the host conveniences that
// upload, run, download and block.  The three descriptor routes differ in the entry point they enqueue.
#include "pm_common.hpp"

namespace {

constexpr int GUIDED_MAX_NQ = 1 << 20;      // pm_filter_ratio_gather_dev: 4096 blocks of 256 rows

// knn(k, records, n_admitted): the guided k-NN of the route on the context's stream
template <class Knn>
int guided_match(pm_ctx* ctx, int nq, const float* d_kp1, const float* d_kp2, float ratio, pm_match* d_knn, pm_match* d_good,
                 float* d_xy1, float* d_xy2, int32_t* d_n_good, Knn knn)
{
    PM_REQUIRE(ctx != nullptr && d_n_good != nullptr, PM_E_INVALID, "null argument");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(nq <= GUIDED_MAX_NQ, PM_E_UNSUPPORTED, "more than 1 048 576 query rows: the compaction's limit");
    PM_REQUIRE(nq <= 0 || (d_knn && d_good), PM_E_INVALID, "null record / output pointer");
    PM_REQUIRE((d_xy1 == nullptr) == (d_xy2 == nullptr), PM_E_INVALID, "give both point outputs or none");
    int rc = knn(2, d_knn, nullptr);
    if (rc != PM_OK) return rc;
    const bool gather = d_xy1 != nullptr;
    return pm_filter_ratio_gather_dev(ctx, d_knn, nq, 2, ratio, gather ? d_kp1 : nullptr, gather ? d_kp2 : nullptr, d_good,
                                      d_xy1, d_xy2, d_n_good);
}

// Host convenience: one allocation [q | t | kp1 | kp2 | M | out | n_admitted], each block 256-byte aligned.
template <class Dev>
int guided_host(pm_ctx* ctx, const void* q, int nq, const void* t, int nt, size_t row_bytes, const float* kp1, const float* kp2,
                const double* M, int k, pm_match* out, int32_t* n_admitted, Dev dev)
{
    PM_REQUIRE(ctx != nullptr && M != nullptr, PM_E_INVALID, "null context or model");
    PM_REQUIRE(nq >= 0 && nt >= 0 && row_bytes >= 1, PM_E_INVALID, "need nq, nt >= 0 and a positive row width");
    PM_REQUIRE(k >= 1 && k <= 4, PM_E_INVALID, "need 1 <= k <= 4");
    PM_REQUIRE(nq == 0 || (q && kp1 && out), PM_E_INVALID, "null query / query keypoint / output pointer");
    PM_REQUIRE(nt == 0 || (t && kp2), PM_E_INVALID, "null train / train keypoint pointer");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t qb = static_cast<size_t>(nq) * row_bytes, tb = static_cast<size_t>(nt) * row_bytes;
    const size_t k1b = sizeof(float) * 2 * static_cast<size_t>(nq), k2b = sizeof(float) * 2 * static_cast<size_t>(nt);
    const size_t ob = sizeof(pm_match) * static_cast<size_t>(nq) * k, nb = sizeof(int32_t) * static_cast<size_t>(nq);
    pm::StagedBlock b(ctx, __func__);
    const size_t o_q = b.add(qb), o_t = b.add(tb), o_k1 = b.add(k1b), o_k2 = b.add(k2b), o_m = b.add(9 * sizeof(double));
    const size_t o_o = b.add(ob), o_n = b.add(nb);
    b.alloc();
    b.upload(o_m, M, 9 * sizeof(double));
    b.upload(o_q, q, qb);
    b.upload(o_t, t, tb);
    b.upload(o_k1, kp1, k1b);
    b.upload(o_k2, kp2, k2b);
    if (b.rc == PM_OK)
        b.rc = dev(b.at<void>(o_q), b.at<void>(o_t), b.at<float>(o_k1), b.at<float>(o_k2), b.at<double>(o_m), b.at<pm_match>(o_o),
                   b.at<int32_t>(o_n));
    b.download(out, o_o, ob);                            // nothing for nq == 0
    if (n_admitted) b.download(n_admitted, o_n, nb);
    return b.sync();
}

}  // namespace

extern "C" int pm_bf_match_guided_l2_f32_dev(pm_ctx* ctx, const float* d_q, int nq, const float* d_t, int nt, int dim,
                                             const float* d_kp1_xy, const float* d_kp2_xy, int kind, const double* d_M,
                                             float tau, float ratio, pm_match* d_knn, pm_match* d_good, float* d_xy1,
                                             float* d_xy2, int32_t* d_n_good)
{
    return guided_match(ctx, nq, d_kp1_xy, d_kp2_xy, ratio, d_knn, d_good, d_xy1, d_xy2, d_n_good,
                        [=](int k, pm_match* o, int32_t* na) {
                            return pm_bf_knn_guided_l2_f32_dev(ctx, d_q, nq, d_t, nt, dim, d_kp1_xy, d_kp2_xy, kind, d_M, tau, k, o, na);
                        });
}

extern "C" int pm_bf_match_guided_l2_u8_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int dim,
                                            const float* d_kp1_xy, const float* d_kp2_xy, int kind, const double* d_M,
                                            float tau, float ratio, pm_match* d_knn, pm_match* d_good, float* d_xy1,
                                            float* d_xy2, int32_t* d_n_good)
{
    return guided_match(ctx, nq, d_kp1_xy, d_kp2_xy, ratio, d_knn, d_good, d_xy1, d_xy2, d_n_good,
                        [=](int k, pm_match* o, int32_t* na) {
                            return pm_bf_knn_guided_l2_u8_dev(ctx, d_q, nq, d_t, nt, dim, d_kp1_xy, d_kp2_xy, kind, d_M, tau, k, o, na);
                        });
}

extern "C" int pm_bf_match_guided_hamming_u8_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int bytes,
                                                 const float* d_kp1_xy, const float* d_kp2_xy, int kind, const double* d_M,
                                                 float tau, float ratio, pm_match* d_knn, pm_match* d_good, float* d_xy1,
                                                 float* d_xy2, int32_t* d_n_good)
{
    return guided_match(ctx, nq, d_kp1_xy, d_kp2_xy, ratio, d_knn, d_good, d_xy1, d_xy2, d_n_good,
                        [=](int k, pm_match* o, int32_t* na) {
                            return pm_bf_knn_guided_hamming_u8_dev(ctx, d_q, nq, d_t, nt, bytes, d_kp1_xy, d_kp2_xy, kind, d_M, tau,
                                                                   k, o, na);
                        });
}

extern "C" int pm_bf_knn_guided_l2_f32(pm_ctx* ctx, const float* q, int nq, const float* t, int nt, int dim, const float* kp1_xy,
                                       const float* kp2_xy, int kind, const double M[9], float tau, int k, pm_match* out,
                                       int32_t* n_admitted)
{
    PM_REQUIRE(dim >= 1, PM_E_INVALID, "need dim >= 1");
    return guided_host(ctx, q, nq, t, nt, sizeof(float) * static_cast<size_t>(dim), kp1_xy, kp2_xy, M, k, out, n_admitted,
                       [=](const void* dq, const void* dt, const float* k1, const float* k2, const double* dM, pm_match* o, int32_t* na) {
                           return pm_bf_knn_guided_l2_f32_dev(ctx, static_cast<const float*>(dq), nq, static_cast<const float*>(dt), nt,
                                                              dim, k1, k2, kind, dM, tau, k, o, na);
                       });
}

extern "C" int pm_bf_knn_guided_l2_u8(pm_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int dim, const float* kp1_xy,
                                      const float* kp2_xy, int kind, const double M[9], float tau, int k, pm_match* out,
                                      int32_t* n_admitted)
{
    PM_REQUIRE(dim >= 1, PM_E_INVALID, "need dim >= 1");
    return guided_host(ctx, q, nq, t, nt, static_cast<size_t>(dim), kp1_xy, kp2_xy, M, k, out, n_admitted,
                       [=](const void* dq, const void* dt, const float* k1, const float* k2, const double* dM, pm_match* o, int32_t* na) {
                           return pm_bf_knn_guided_l2_u8_dev(ctx, static_cast<const uint8_t*>(dq), nq, static_cast<const uint8_t*>(dt),
                                                             nt, dim, k1, k2, kind, dM, tau, k, o, na);
                       });
}

extern "C" int pm_bf_knn_guided_hamming_u8(pm_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int bytes,
                                           const float* kp1_xy, const float* kp2_xy, int kind, const double M[9], float tau, int k,
                                           pm_match* out, int32_t* n_admitted)
{
    PM_REQUIRE(bytes >= 1 && (bytes % 4) == 0, PM_E_INVALID, "bytes must be a positive multiple of 4");
    return guided_host(ctx, q, nq, t, nt, static_cast<size_t>(bytes), kp1_xy, kp2_xy, M, k, out, n_admitted,
                       [=](const void* dq, const void* dt, const float* k1, const float* k2, const double* dM, pm_match* o, int32_t* na) {
                           return pm_bf_knn_guided_hamming_u8_dev(ctx, static_cast<const uint8_t*>(dq), nq,
                                                                  static_cast<const uint8_t*>(dt), nt, bytes, k1, k2, kind, dM, tau,
                                                                  k, o, na);
                       });
}
