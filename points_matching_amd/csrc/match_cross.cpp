// match_cross.cpp — one-call cross-check matching (SPEC S42): forward matcher pass, reverse matcher pass (arguments
// swapped) and the fused mutual-nearest-neighbour filter + gather (S41, filter_gather.hip), enqueued back to back on the
// context's stream.  Host code only: the three descriptor routes differ in the matcher entry point they enqueue twice.
// The reverse pass is a second full matcher run; sharing the prep copies between the passes or taking column minima in
// the coarse sweep would touch the coarse kernels and is not done here.
#include "pm_common.hpp"

namespace {

struct CrossArgs {
    int nq, nt, width;            // width: dim (L2) or bytes (Hamming)
    int cross_flags;
    float ratio;
    const float *kp1, *kp2;
    pm_match *fwd, *rev, *good;
    float *xy1, *xy2;
    int32_t* n_good;
};

int cross_validate(pm_ctx* ctx, const void* d_q, const void* d_t, const CrossArgs& a)
{
    PM_REQUIRE(ctx != nullptr && a.n_good != nullptr, PM_E_INVALID, "null argument");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(a.nq >= 0 && a.nt >= 0 && a.width >= 1, PM_E_INVALID, "need nq, nt >= 0 and a positive row width");
    PM_REQUIRE((a.cross_flags & ~(PM_CROSS_RATIO_FWD | PM_CROSS_RATIO_REV)) == 0, PM_E_INVALID, "unknown cross_flags bits");
    PM_REQUIRE(a.nq == 0 || (d_q && a.fwd && a.good), PM_E_INVALID, "null query / forward record / output pointer");
    PM_REQUIRE(a.nt == 0 || (d_t && a.rev), PM_E_INVALID, "null train / reverse record pointer");
    PM_REQUIRE((a.kp1 == nullptr) == (a.kp2 == nullptr), PM_E_INVALID, "give both keypoint arrays or none");
    PM_REQUIRE(a.kp1 == nullptr || (a.xy1 && a.xy2), PM_E_INVALID, "null point outputs");
    return PM_OK;
}

// knn(ctx, queries, n_queries, train, n_train, k, out): one matcher pass on the context's stream
template <class Knn>
int cross_enqueue(pm_ctx* ctx, const void* d_q, const void* d_t, const CrossArgs& a, Knn knn)
{
    int rc = cross_validate(ctx, d_q, d_t, a);
    if (rc != PM_OK) return rc;
    const int kf = (a.cross_flags & PM_CROSS_RATIO_FWD) ? 2 : 1, kr = (a.cross_flags & PM_CROSS_RATIO_REV) ? 2 : 1;
    rc = knn(d_q, a.nq, d_t, a.nt, kf, a.fwd, /*reverse=*/false);
    if (rc != PM_OK) return rc;
    rc = knn(d_t, a.nt, d_q, a.nq, kr, a.rev, /*reverse=*/true);
    if (rc != PM_OK) return rc;
    return pm_filter_cross_gather_dev(ctx, a.fwd, a.nq, kf, a.rev, a.nt, kr, a.cross_flags, a.ratio, a.kp1, a.kp2, a.good,
                                      a.xy1, a.xy2, a.n_good);
}

// Host convenience: upload both descriptor sets, run the device form, download the count and the survivors.
template <class Dev>
int cross_host(pm_ctx* ctx, const void* q, int nq, const void* t, int nt, size_t row_bytes, int cross_flags, pm_match* out,
               int* n_out, Dev dev)
{
    PM_REQUIRE(ctx != nullptr && n_out != nullptr, PM_E_INVALID, "null argument");
    PM_REQUIRE(nq >= 0 && nt >= 0 && row_bytes >= 1, PM_E_INVALID, "need nq, nt >= 0 and a positive row width");
    PM_REQUIRE(nq == 0 || (q && out), PM_E_INVALID, "null query/output pointer");
    PM_REQUIRE(nt == 0 || t, PM_E_INVALID, "null train pointer");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    const int kf = (cross_flags & PM_CROSS_RATIO_FWD) ? 2 : 1, kr = (cross_flags & PM_CROSS_RATIO_REV) ? 2 : 1;
    const size_t qb = static_cast<size_t>(nq) * row_bytes, tb = static_cast<size_t>(nt) * row_bytes;
    const size_t fb = sizeof(pm_match) * static_cast<size_t>(nq) * kf, rb = sizeof(pm_match) * static_cast<size_t>(nt) * kr;
    const size_t gb = sizeof(pm_match) * static_cast<size_t>(nq);
    pm::StagedBlock b(ctx, __func__);
    const size_t o_q = b.add(qb), o_t = b.add(tb), o_f = b.add(fb), o_r = b.add(rb), o_g = b.add(gb), o_n = b.add(sizeof(int32_t));
    int rc = b.alloc();
    if (rc != PM_OK) return rc;
    *n_out = 0;                                          // on every failure from here on; n once the rows have arrived
    b.upload(o_q, q, qb);
    b.upload(o_t, t, tb);
    if (b.rc == PM_OK) b.rc = dev(b.at<void>(o_q), b.at<void>(o_t), b.at<pm_match>(o_f), b.at<pm_match>(o_r), b.at<pm_match>(o_g), b.at<int32_t>(o_n));
    int32_t n = 0;
    b.download(&n, o_n, sizeof n);
    rc = b.sync();                                       // the stream is idle from here to the next download
    if (rc != PM_OK) return rc;
    if (n < 0 || n > nq) { pm::set_error("%s: survivor count %d outside [0, %d]", __func__, n, nq); return PM_E_HIP; }
    b.download(out, o_g, sizeof(pm_match) * static_cast<size_t>(n));
    rc = b.sync();
    if (rc == PM_OK) *n_out = n;
    return rc;
}

}  // namespace

extern "C" int pm_bf_match_cross_l2_f32_dev(pm_ctx* ctx, const float* d_q, int nq, const float* d_t, int nt, int dim,
                                            int knn_flags, int cross_flags, float ratio, const float* d_kp1_xy,
                                            const float* d_kp2_xy, pm_match* d_fwd, pm_match* d_rev, pm_match* d_good,
                                            float* d_xy1, float* d_xy2, int32_t* d_n_good)
{
    const CrossArgs a{nq, nt, dim, cross_flags, ratio, d_kp1_xy, d_kp2_xy, d_fwd, d_rev, d_good, d_xy1, d_xy2, d_n_good};
    return cross_enqueue(ctx, d_q, d_t, a, [=](const void* x, int nx, const void* y, int ny, int k, pm_match* o, bool reverse) {
        // PM_KNN_HINT_UNIT_NORM speaks about the train rows only: the reverse pass, whose train rows are q, goes without it
        const int flags = reverse ? (knn_flags & ~PM_KNN_HINT_UNIT_NORM) : knn_flags;
        return pm_bf_knn_l2_f32_dev(ctx, static_cast<const float*>(x), nx, static_cast<const float*>(y), ny, dim, k, flags, o);
    });
}

extern "C" int pm_bf_match_cross_l2_u8_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int dim,
                                           int cross_flags, float ratio, const float* d_kp1_xy, const float* d_kp2_xy,
                                           pm_match* d_fwd, pm_match* d_rev, pm_match* d_good, float* d_xy1, float* d_xy2,
                                           int32_t* d_n_good)
{
    const CrossArgs a{nq, nt, dim, cross_flags, ratio, d_kp1_xy, d_kp2_xy, d_fwd, d_rev, d_good, d_xy1, d_xy2, d_n_good};
    return cross_enqueue(ctx, d_q, d_t, a, [=](const void* x, int nx, const void* y, int ny, int k, pm_match* o, bool) {
        return pm_bf_knn_l2_u8_dev(ctx, static_cast<const uint8_t*>(x), nx, static_cast<const uint8_t*>(y), ny, dim, k, o);
    });
}

extern "C" int pm_bf_match_cross_hamming_u8_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt,
                                                int bytes, int cross_flags, float ratio, const float* d_kp1_xy,
                                                const float* d_kp2_xy, pm_match* d_fwd, pm_match* d_rev, pm_match* d_good,
                                                float* d_xy1, float* d_xy2, int32_t* d_n_good)
{
    const CrossArgs a{nq, nt, bytes, cross_flags, ratio, d_kp1_xy, d_kp2_xy, d_fwd, d_rev, d_good, d_xy1, d_xy2, d_n_good};
    return cross_enqueue(ctx, d_q, d_t, a, [=](const void* x, int nx, const void* y, int ny, int k, pm_match* o, bool) {
        return pm_bf_knn_hamming_u8_dev(ctx, static_cast<const uint8_t*>(x), nx, static_cast<const uint8_t*>(y), ny, bytes, k, o);
    });
}

extern "C" int pm_bf_match_cross_l2_f32(pm_ctx* ctx, const float* q, int nq, const float* t, int nt, int dim, int knn_flags,
                                        int cross_flags, float ratio, pm_match* out, int* n_out)
{
    PM_REQUIRE(dim >= 1, PM_E_INVALID, "need dim >= 1");
    return cross_host(ctx, q, nq, t, nt, sizeof(float) * static_cast<size_t>(dim), cross_flags, out, n_out,
                      [=](const void* dq, const void* dt, pm_match* f, pm_match* r, pm_match* g, int32_t* n) {
                          return pm_bf_match_cross_l2_f32_dev(ctx, static_cast<const float*>(dq), nq, static_cast<const float*>(dt),
                                                              nt, dim, knn_flags, cross_flags, ratio, nullptr, nullptr, f, r, g,
                                                              nullptr, nullptr, n);
                      });
}

extern "C" int pm_bf_match_cross_l2_u8(pm_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int dim,
                                       int cross_flags, float ratio, pm_match* out, int* n_out)
{
    PM_REQUIRE(dim >= 1, PM_E_INVALID, "need dim >= 1");
    return cross_host(ctx, q, nq, t, nt, static_cast<size_t>(dim), cross_flags, out, n_out,
                      [=](const void* dq, const void* dt, pm_match* f, pm_match* r, pm_match* g, int32_t* n) {
                          return pm_bf_match_cross_l2_u8_dev(ctx, static_cast<const uint8_t*>(dq), nq,
                                                             static_cast<const uint8_t*>(dt), nt, dim, cross_flags, ratio, nullptr,
                                                             nullptr, f, r, g, nullptr, nullptr, n);
                      });
}

extern "C" int pm_bf_match_cross_hamming_u8(pm_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int bytes,
                                            int cross_flags, float ratio, pm_match* out, int* n_out)
{
    PM_REQUIRE(bytes >= 1, PM_E_INVALID, "need bytes >= 1");
    return cross_host(ctx, q, nq, t, nt, static_cast<size_t>(bytes), cross_flags, out, n_out,
                      [=](const void* dq, const void* dt, pm_match* f, pm_match* r, pm_match* g, int32_t* n) {
                          return pm_bf_match_cross_hamming_u8_dev(ctx, static_cast<const uint8_t*>(dq), nq,
                                                                  static_cast<const uint8_t*>(dt), nt, bytes, cross_flags, ratio,
                                                                  nullptr, nullptr, f, r, g, nullptr, nullptr, n);
                      });
}
